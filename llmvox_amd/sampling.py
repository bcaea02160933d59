"""Sampling parameters of a stream (lvx_stream_sampling) and the host side of its generator.

The device draws one token per decode step from Philox4x32-10 with the counter (position, 0, 0, 0) and
the slot's 64-bit seed as the key (include/llmvox.h has the whole rule). The scheduler gives every
sentence of a stream a seed of its own, ``segment_seed``, derived with the same generator, so two
replica streams of a request and the segments of one stream draw independently, and a request's
audio is a function of (text, seed) alone.
"""
from __future__ import annotations

import math
import struct
from dataclasses import dataclass

_M32 = 0xFFFFFFFF
_MUL0, _MUL1 = 0xD2511F53, 0xCD9E8D57
_WEYL0, _WEYL1 = 0x9E3779B9, 0xBB67AE85


def philox4x32_10(counter, key):
    """Philox4x32-10: ``counter`` 4 and ``key`` 2 words of 32 bits -> 4 output words."""
    c0, c1, c2, c3 = (int(x) & _M32 for x in counter)
    k0, k1 = (int(x) & _M32 for x in key)
    for _ in range(10):
        p0, p1 = _MUL0 * c0, _MUL1 * c2
        c0, c1, c2, c3 = (p1 >> 32) ^ c1 ^ k0, p1 & _M32, (p0 >> 32) ^ c3 ^ k1, p0 & _M32
        k0, k1 = (k0 + _WEYL0) & _M32, (k1 + _WEYL1) & _M32
    return c0, c1, c2, c3


def segment_seed(seed: int, index: int, segment: int) -> int:
    """The 64-bit seed of sentence ``segment`` of the stream with replica index ``index`` of a request
    seeded ``seed``: words 0-1 of philox4x32_10((segment, index, 0, 0), (seed low, seed high))."""
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    x = philox4x32_10((segment, index, 0, 0), (seed & _M32, seed >> 32))
    return x[0] | (x[1] << 32)


@dataclass(frozen=True)
class Sampling:
    """temperature 0: greedy; top_k 0 or >= 4096: no crop; seed: 64 bits; top_p in (0, 1], 1: no nucleus crop;
    min_p in [0, 1), 0: no min-p crop; repetition_penalty > 0, 1: none, over the last repetition_window
    (1 .. 256) tokens of the sentence. Validated as the C call does (lvx_stream_sampling_ex)."""
    temperature: float
    top_k: int = 0
    seed: int = 0
    top_p: float = 1.0
    min_p: float = 0.0
    repetition_penalty: float = 1.0
    repetition_window: int = 64

    def __post_init__(self):
        t = self.temperature
        if isinstance(t, bool) or not isinstance(t, (int, float)) or not math.isfinite(t) or t < 0:
            raise ValueError(f"temperature must be finite and >= 0, got {t!r}")
        for name in ("top_k", "seed"):
            v = getattr(self, name)
            if isinstance(v, bool) or not isinstance(v, int) or v < 0:
                raise ValueError(f"{name} must be an integer >= 0, got {v!r}")
        if self.seed >> 64:
            raise ValueError("seed must fit 64 bits")
        for name in ("top_p", "min_p", "repetition_penalty"):
            v = getattr(self, name)
            if isinstance(v, bool) or not isinstance(v, (int, float)) or not math.isfinite(v):
                raise ValueError(f"{name} must be a finite number, got {v!r}")
        # (the C call sees fp32 values: a double just above 0 or just below 1 must not round onto the bound)
        def f32(v):
            try:
                return struct.unpack("f", struct.pack("f", v))[0]
            except OverflowError:
                return math.inf

        if not 0 < f32(self.top_p) <= 1:
            raise ValueError(f"top_p must be in (0, 1], got {self.top_p!r}")
        if not 0 <= f32(self.min_p) < 1:
            raise ValueError(f"min_p must be in [0, 1), got {self.min_p!r}")
        if not 0 < f32(self.repetition_penalty) < math.inf:
            raise ValueError(f"repetition_penalty must be finite and > 0, got {self.repetition_penalty!r}")
        w = self.repetition_window
        if isinstance(w, bool) or not isinstance(w, int) or not 1 <= w <= 256:
            raise ValueError(f"repetition_window must be an integer in 1 .. 256, got {w!r}")

    @property
    def extended(self) -> bool:
        """Some control beyond temperature / top_k / seed is on. ``repetition_window`` alone does not count: without
        a penalty it has no effect, so a Sampling that differs from the defaults only in the window is not
        extended and ``extra()`` is empty for it."""
        return self.top_p != 1 or self.min_p != 0 or self.repetition_penalty != 1

    def extra(self) -> dict:
        """The keywords ``Engine.set_sampling`` takes beyond (temperature, top_k, seed); empty when none is on, so
        that a stream that asks for none issues the calls it always issued."""
        if not self.extended:
            return {}
        return {"top_p": self.top_p, "min_p": self.min_p, "repetition_penalty": self.repetition_penalty,
                "repetition_window": self.repetition_window}


__all__ = ["Sampling", "philox4x32_10", "segment_seed"]

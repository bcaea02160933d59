"""Sampling parameters of a stream (lvx_stream_sampling) and the host side of its generator.

The device draws one token per decode step from Philox4x32-10 with the counter (position, 0, 0, 0) and
the slot's 64-bit seed as the key (include/llmvox.h has the whole rule). The scheduler gives every
sentence of a stream a seed of its own, ``segment_seed``, derived with the same generator, so two
replica streams of a request and the segments of one stream draw independently, and a request's
audio is a function of (text, seed) alone.
"""
from __future__ import annotations

import math
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
    """temperature 0: greedy; top_k 0 or >= 4096: no crop; seed: 64 bits. Validated as the C call does."""
    temperature: float
    top_k: int = 0
    seed: int = 0

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


__all__ = ["Sampling", "philox4x32_10", "segment_seed"]

"""Audio output formats of the service and the numpy reference of the PCM output stage's rule
(include/llmvox.h, "PCM output stage": the rates, the prototype filter, the streaming counts, the fixed
fp32 summation order and the s16le quantisation). The device stage is ``Engine.pcm_convert``; everything
here runs on the host and is what the tests and the documentation compare it with."""
from __future__ import annotations

import struct
from dataclasses import dataclass
from typing import List, Optional, Tuple

import numpy as np

BASE_RATE = 24000  # the codec's output rate
RATES = {24000: (1, 1, 0), 16000: (2, 3, 72), 8000: (1, 3, 72), 48000: (2, 1, 48)}  # rate: (L, M, N)
ENCODINGS = ("f32le", "s16le")
CONTAINERS = ("raw", "wav")
HISTORY = 160  # inputs of history a slot keeps between calls


@dataclass(frozen=True)
class AudioFormat:
    """What a stream's audio is delivered as. The default is the reference's: headerless float32 at 24 kHz."""
    sample_rate: int = BASE_RATE
    encoding: str = "f32le"
    container: str = "raw"

    def __post_init__(self):
        if isinstance(self.sample_rate, bool) or not isinstance(self.sample_rate, int) or self.sample_rate not in RATES:
            raise ValueError(f"sample_rate must be one of {sorted(RATES)}, got {self.sample_rate!r}")
        if self.encoding not in ENCODINGS:
            raise ValueError(f"encoding must be one of {ENCODINGS}, got {self.encoding!r}")
        if self.container not in CONTAINERS:
            raise ValueError(f"container must be one of {CONTAINERS}, got {self.container!r}")

    @property
    def is_default(self) -> bool:
        return self.sample_rate == BASE_RATE and self.encoding == "f32le" and self.container == "raw"

    @property
    def converts(self) -> bool:
        """The samples differ from the codec's (another rate or encoding): the stream needs the device stage."""
        return self.sample_rate != BASE_RATE or self.encoding != "f32le"

    @property
    def sample_bytes(self) -> int:
        return 2 if self.encoding == "s16le" else 4

    @property
    def dtype(self):
        return np.dtype("<i2") if self.encoding == "s16le" else np.dtype("<f4")

    @property
    def media_type(self) -> str:
        return "audio/wav" if self.container == "wav" else "application/octet-stream"


def wav_header(fmt: AudioFormat) -> bytes:
    """The 44-byte RIFF / WAVE header of a mono stream of unknown length: both sizes 0xFFFFFFFF, format
    tag 1 (integer PCM) or 3 (IEEE float)."""
    tag, nbytes = (1, 2) if fmt.encoding == "s16le" else (3, 4)
    return (b"RIFF" + struct.pack("<I", 0xFFFFFFFF) + b"WAVE" + b"fmt "
            + struct.pack("<IHHIIHH", 16, tag, 1, fmt.sample_rate, fmt.sample_rate * nbytes, nbytes, 8 * nbytes)
            + b"data" + struct.pack("<I", 0xFFFFFFFF))


# ---- the rule, in numpy ------------------------------------------------------------------------------

def design(sample_rate: int) -> Tuple[int, int, int, np.ndarray]:
    """(L, M, N, taps float64 [2 N + 1]) of a rate: the Kaiser-windowed sinc prototype in double precision
    (the library stores it as fp32: ``lvx_pcm_filter``)."""
    if sample_rate not in RATES:
        raise ValueError(f"unsupported sample rate {sample_rate}")
    L, M, _ = RATES[sample_rate]
    if sample_rate == BASE_RATE:
        return 1, 1, 0, np.ones(1)
    lo = min(1.0, L / M)
    fc = 0.5 * lo * 0.85 / L
    N = int(round(24 * L / lo))
    n = np.arange(-N, N + 1)
    return L, M, N, L * 2 * fc * np.sinc(2 * fc * n) * np.kaiser(2 * N + 1, 9.0)


def emitted_upto(sample_rate: int, T: int, final: bool) -> int:
    """Outputs of a segment emitted once T inputs are consumed (after a non-final / a final call)."""
    L, M, N = RATES[sample_rate]
    full = -((-T * L) // M)
    if final or N == 0:
        return full
    a = (T - 1) * L - N
    return 0 if a < 0 else min(a // M + 1, full)


def emitted(sample_rate: int, t0: int, n_in: int, final: bool) -> int:
    """Samples a call emits for a slot that has consumed t0 inputs of its segment (``lvx_pcm_emitted``)."""
    return emitted_upto(sample_rate, t0 + n_in, final) - emitted_upto(sample_rate, t0, False)


def resample_ref(x, sample_rate: int, taps=None, m0: int = 0, m1: Optional[int] = None, dtype=np.float32) -> np.ndarray:
    """Outputs m0 .. m1 - 1 (default: all ceil(T L / M)) of the segment x[0 .. T) at ``sample_rate``.
    dtype float32: the rule's fixed order (inputs ascending, a rounded product and a rounded sum per tap, no
    fused multiply-add), bit for bit what the device computes with the same fp32 taps. dtype float64: the
    same sums in double (with the fp32 taps' values): the yardstick of the device's accumulation error."""
    L, M, N = RATES[sample_rate]
    x = np.asarray(x, dtype=np.float32)
    T = x.shape[-1]
    if taps is None:
        taps = design(sample_rate)[3].astype(np.float32)
    h = np.asarray(taps, dtype=np.float32).astype(dtype)
    if m1 is None:
        m1 = -((-T * L) // M)
    m = np.arange(m0, m1, dtype=np.int64)
    y = np.zeros(x.shape[:-1] + (m.size,), dtype=dtype)
    if N == 0:
        y[...] = x[..., m0:m1]
        return y
    pad = 2 * N // L + 2
    xp = np.zeros(x.shape[:-1] + (T + 2 * pad + int(m.size and (m[-1] * M + N) // L + 1),), dtype=dtype)
    xp[..., pad:pad + T] = x
    for p in range(L):  # the outputs whose m M is congruent to p mod L share their tap indices
        sel = np.nonzero((m * M) % L == p)[0]
        if not sel.size:
            continue
        mm = m[sel] * M
        ilo = -((-(mm - N)) // L)  # ceil((m M - N) / L)
        t = int(mm[0] - ilo[0] * L)  # the first tap index, the same for every output of the phase
        acc = np.zeros(x.shape[:-1] + (sel.size,), dtype=dtype)
        k = 0
        while t >= -N:
            acc = acc + xp[..., ilo + k + pad] * h[t + N]
            t -= L
            k += 1
        y[..., sel] = acc
    return y


def quantize_s16(v) -> np.ndarray:
    """q = rint(clamp(v * 32768, -32768, 32767)), half to even, NaN -> 0 (exact in fp32)."""
    v = np.asarray(v, dtype=np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        s = np.clip(v * np.float32(32768.0), np.float32(-32768.0), np.float32(32767.0))
        return np.where(np.isnan(v), np.float32(0), np.rint(s)).astype(np.int16)


def encode_ref(y, fmt: AudioFormat) -> np.ndarray:
    return quantize_s16(y) if fmt.encoding == "s16le" else np.asarray(y, dtype=np.float32)


def convert_ref(x, fmt: AudioFormat, taps=None) -> np.ndarray:
    """A whole segment x (float32 at 24 kHz) in the format's rate and encoding (int16 or float32 array)."""
    return encode_ref(resample_ref(x, fmt.sample_rate, taps), fmt)


class StreamRef:
    """The streaming form of the rule for one slot, on the host: ``push(x, final)`` returns the samples the
    call emits (``lvx_pcm_convert`` for one row). Keeps the whole segment; for tests and stand-in engines."""

    def __init__(self, fmt: AudioFormat, taps=None):
        self.fmt, self.taps = fmt, taps
        self.seg: List[np.ndarray] = []
        self.t0 = 0

    def reset(self):
        self.seg, self.t0 = [], 0

    def push(self, x, final: bool) -> np.ndarray:
        x = np.asarray(x, dtype=np.float32).reshape(-1)
        rate = self.fmt.sample_rate
        m0 = emitted_upto(rate, self.t0, False)
        m1 = emitted_upto(rate, self.t0 + x.size, final)
        self.seg.append(x)
        self.t0 += x.size
        whole = np.concatenate(self.seg) if self.seg else np.zeros(0, np.float32)
        y = encode_ref(resample_ref(whole, rate, self.taps, m0, m1), self.fmt)
        if final:
            self.reset()
        return y


__all__ = ["AudioFormat", "wav_header", "design", "emitted", "emitted_upto", "resample_ref", "quantize_s16",
           "convert_ref", "StreamRef", "RATES", "ENCODINGS", "CONTAINERS", "BASE_RATE", "HISTORY"]

"""Audio output formats of the service and the numpy reference of the PCM output stage's rule
(include/llmvox.h, "PCM output stage": the rates, the prototype filter, the streaming counts, the fixed
fp32 summation order and the s16le quantisation). The device stage is ``Engine.pcm_convert``; everything
here runs on the host and is what the tests and the documentation compare it with. The speaking-rate
control ("PCM time stretch" in the same header: WSOLA on the 24 kHz rows, before the resampler) is stated
here too: ``stretch_ref``. So is the pitch control ("PCM pitch shift": the integer plan that turns a speed and a
pitch into a stretch and a resampling ratio L / M, and the resampler of that ratio, between the stretch and the
rate conversion): ``pitch_plan``, ``ratio_ref``. And the join of a sentence's dumps ("PCM dump join": a held-back
frame crossfaded with the next dump's rendering of it, in front of the other three): ``join_ref``. And the volume
control ("PCM level": a gain and a feed-forward peak limiter, between the ratio and the rate conversion):
``level_ref``. And the formant control ("PCM formant": the integer plan of the envelope correction Fn / Fd and a
short-time Fourier correction of the spectral envelope, between the ratio and the level): ``formant_plan``,
``formant_ref``. And the G.711 encodings ("PCM G.711": the s16 quantisation companded to 8-bit mu-law or A-law, integer
arithmetic only): ``g711_encode``, ``g711_decode``. And the FLAC output ("PCM FLAC": the s16 samples cut into frames of
40 ms, each a CONSTANT, FIXED or VERBATIM subframe, integer arithmetic only): ``flac_subframe``, ``flac_frame``,
``flac_encode_ref``, and ``FlacMux``, which finishes the device's subframes into frames on the delivery path. And the
pause control ("PCM pause": the encoded samples cut into slots of 10 ms, each marked silent or not on the device, and
the host's rule that trims, caps and spaces sentences by whole blocks): ``pause_slots_ref``, ``pause_ref``, ``PauseMux``.
And the watermark ("PCM mark": the formant stage's transform under a keyed table of signs, between the formant and the
level, and the blind detector of delivered audio): ``mark_table``, ``mark_ref``, ``mark_detect``."""
from __future__ import annotations

import struct
from dataclasses import dataclass, field
from math import gcd
from typing import List, Optional, Tuple

import numpy as np

BASE_RATE = 24000  # the codec's output rate
RATES = {24000: (1, 1, 0), 16000: (2, 3, 72), 8000: (1, 3, 72), 48000: (2, 1, 48)}  # rate: (L, M, N)
ENCODINGS = ("f32le", "s16le", "ulaw", "alaw")  # the sample encodings: what lvx_pcm_convert writes, one dtype each
FORMAT_ENCODINGS = ENCODINGS + ("flac",)  # what a format may name: those, and the FLAC stream made behind s16le
G711_LAWS = ("ulaw", "alaw")  # the 8-bit companded encodings (LVX_PCM_ULAW, LVX_PCM_ALAW)
_SAMPLE_DTYPE = {"f32le": np.dtype("<f4"), "s16le": np.dtype("<i2"), "ulaw": np.dtype("u1"), "alaw": np.dtype("u1"),
                 "flac": np.dtype("u1")}  # (flac: the bytes of the device's slots, then of the stream)
_G711_TAG = {"ulaw": 7, "alaw": 6}   # WAVE format tags, the values of LVX_PCM_ULAW / LVX_PCM_ALAW
_G711_SILENCE = {"ulaw": 0xFF, "alaw": 0xD5}  # the codes of q = 0
CONTAINERS = ("raw", "wav")
FRAME_MS = (10, 20, 30, 40, 60)  # the fixed frame durations a request may ask its byte stream to be cut into
HISTORY = 160  # inputs of history a slot keeps between calls
SPEED_MIN, SPEED_MAX = 50, 200  # speed_pct of a stream (100: no stretch)
STRETCH_H = 240         # output hop of the time stretch (10 ms)
STRETCH_D = 240         # its search radius
STRETCH_C = 480         # its correlation length
STRETCH_HISTORY = 1280  # inputs of history a slot keeps between stretch calls
PITCH_MIN, PITCH_MAX = 50, 200  # pitch_pct of a stream (100: no shift)
RATIO_MAX = 200         # L and M of a ratio the resampler takes: 1 .. 200, coprime, M <= 4 L and L <= 4 M
RATIO_HISTORY = 256     # inputs of history a slot keeps between ratio calls
JOIN_HOLD = 320         # samples the dump join holds back and crossfades (LVX_JOIN_HOLD): one codec frame
JOIN_CONTEXT = 16       # the most context frames a joined dump is decoded with (LVX_JOIN_CONTEXT)
VOLUME_MIN, VOLUME_MAX = 0, 400  # volume_pct of a stream (100: no level stage)
LEVEL_A = 120           # the limiter's attack half-window in samples (LVX_LEVEL_A): 5 ms
LEVEL_R = 1200          # its hold (LVX_LEVEL_R): 50 ms
LEVEL_CEIL = np.float32(0.8912509)  # its ceiling c (LVX_LEVEL_CEIL): -1 dBFS
LEVEL_HISTORY = 1600    # inputs of history a slot keeps between level calls
FORMANT_MIN, FORMANT_MAX = 50, 200  # formant_pct of a stream (None: the formants follow the pitch, no stage)
FORMANT_N = 1024        # the formant stage's frame length (LVX_FORMANT_N)
FORMANT_H = 256         # its hop (LVX_FORMANT_H)
FORMANT_K = 12          # its smoothing half-width in bins (LVX_FORMANT_K)
FORMANT_EPS = np.float32(1e-10)  # the floor added to both envelope values
FORMANT_G2_MIN, FORMANT_G2_MAX = np.float32(1.0 / 256.0), np.float32(256.0)  # the clamp on the squared gain: +-24 dB
FORMANT_MAX_TERM = 40000  # Fn and Fd of a correction ratio the stage takes: 1 .. 40000, coprime, within 1/2 .. 2
FORMANT_HISTORY = 1792  # inputs of history a slot keeps between formant calls (7 H)
MARK_K0 = 24            # the watermark's first marked bin (LVX_MARK_K0): 562.5 Hz
MARK_BW = 5             # bins of a sub-band (LVX_MARK_BW)
MARK_U = 24             # sub-bands (LVX_MARK_U): the band ends below bin 144, 3375 Hz
MARK_PAIRS = MARK_U // 2  # pair m is the sub-bands (2 m, 2 m + 1)
MARK_Q = 4              # frames of a block (LVX_MARK_Q)
MARK_P = 64             # blocks of a period (LVX_MARK_P): 2.73 s
MARK_STRENGTH_MIN, MARK_STRENGTH_MAX = 1, 3  # a = 2^-(7 - strength): 1/64, 1/32, 1/16
FLAC_MAX_K = 14         # the largest Rice parameter the FLAC stage chooses (the escape code is never used)
PAUSE_THRESH = 103      # a sample louder than this on the 16-bit scale makes its block active (LVX_PAUSE_THRESH): -50 dBFS
PAUSE_LEAD = 2          # silent blocks kept in front of a sentence's first active one (LVX_PAUSE_LEAD): 20 ms of onset
PAUSE_TRAIL = 5         # silent blocks kept behind its last active one (LVX_PAUSE_TRAIL): 50 ms of decay
PAUSE_MS_MAX = 2000     # the largest pause_ms and max_pause_ms
MAX_PAUSE_MS_MIN = 100  # the smallest max_pause_ms: C >= 10 blocks, so the kept head of a capped run covers the trail


def pitch_plan(speed_pct: int, pitch_pct: int) -> Tuple[int, int, int]:
    """(stretch_pct, L, M) of a stream's speed and pitch, all integers (``lvx_pcm_pitch_plan``): the PCM is
    time-stretched at stretch_pct = speed 100 / pitch rounded half up, then resampled by L / M =
    stretch_pct / speed_pct in lowest terms (output count over input count). The duration is that of speed_pct,
    the pitch is multiplied by M / L. ValueError: either outside [50, 200], or a stretch_pct outside."""
    for name, v in (("speed_pct", speed_pct), ("pitch_pct", pitch_pct)):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not 50 <= v <= 200:
            raise ValueError(f"{name} must be an integer in [50, 200], got {v!r}")
    speed_pct, pitch_pct = int(speed_pct), int(pitch_pct)
    stretch = (200 * speed_pct + pitch_pct) // (2 * pitch_pct)
    if not SPEED_MIN <= stretch <= SPEED_MAX:
        raise ValueError(f"speed_pct {speed_pct} with pitch_pct {pitch_pct} needs a time stretch of {stretch} percent, "
                         f"outside [{SPEED_MIN}, {SPEED_MAX}]")
    g = gcd(stretch, speed_pct)
    return stretch, stretch // g, speed_pct // g


def _check_formant_pct(formant_pct) -> int:
    if isinstance(formant_pct, bool) or not isinstance(formant_pct, (int, np.integer)) \
            or not FORMANT_MIN <= formant_pct <= FORMANT_MAX:
        raise ValueError(f"formant_pct must be an integer in [{FORMANT_MIN}, {FORMANT_MAX}], got {formant_pct!r}")
    return int(formant_pct)


def formant_plan(speed_pct: int, pitch_pct: int, formant_pct: int) -> Tuple[int, int]:
    """(Fn, Fd) of a stream's speed, pitch and formant, all integers (``lvx_pcm_formant_plan``): behind the
    resampling by L / M of ``pitch_plan`` the spectral envelope sits at M / L times the model's; to leave it at
    formant_pct / 100 the formant stage corrects by rho = (100 M) / (formant_pct L), in lowest terms Fn / Fd.
    1 / 1: no stage. ValueError: a percentage outside [50, 200], a pair ``pitch_plan`` rejects, or a rho outside
    1/2 .. 2."""
    _, L, M = pitch_plan(speed_pct, pitch_pct)
    formant_pct = _check_formant_pct(formant_pct)
    n, d = 100 * M, formant_pct * L
    g = gcd(n, d)
    Fn, Fd = n // g, d // g
    if Fd > 2 * Fn or Fn > 2 * Fd:
        raise ValueError(f"speed_pct {speed_pct}, pitch_pct {pitch_pct} and formant_pct {formant_pct} need an envelope "
                         f"correction of {Fn} / {Fd}, outside 1/2 .. 2")
    return Fn, Fd


@dataclass(frozen=True)
class AudioFormat:
    """What a stream's audio is delivered as. The default is the reference's: headerless float32 at 24 kHz."""
    sample_rate: int = BASE_RATE
    encoding: str = "f32le"
    container: str = "raw"
    speed_pct: int = 100  # speaking rate in percent (pitch-preserving time stretch of the PCM; 100: none)
    pitch_pct: int = 100  # pitch in percent (a stretch and a resampling of the PCM, ``pitch_plan``; 100: none)
    join: bool = False    # click-free dump joins: context frames and a crossfade at every dump boundary (``join_ref``)
    volume_pct: int = 100  # volume in percent (a gain and a peak limiter on the PCM, ``level_ref``; 100: none)
    # where the formants sit, in percent of the model's own (``formant_ref`` behind the resampling; None: they follow
    # the pitch, no stage)
    formant_pct: Optional[int] = None
    # the pacing (``pause_ref``): the silence between two sentences in ms, their edges trimmed (None: as rendered), and
    # the longest silence inside a sentence in ms (None: as rendered)
    pause_ms: Optional[int] = None
    max_pause_ms: Optional[int] = None
    # the watermark (``mark_ref`` behind the formant stage, in front of the level stage; None: no mark, no stage): its
    # 64-bit key, which no header, error text or info endpoint repeats, its payload byte and its strength
    mark_key: Optional[int] = field(default=None, repr=False)
    mark_id: int = 0
    mark_strength: int = 2

    def __post_init__(self):
        if isinstance(self.sample_rate, bool) or not isinstance(self.sample_rate, int) or self.sample_rate not in RATES:
            raise ValueError(f"sample_rate must be one of {sorted(RATES)}, got {self.sample_rate!r}")
        if self.encoding not in FORMAT_ENCODINGS:
            raise ValueError(f"encoding must be one of {FORMAT_ENCODINGS}, got {self.encoding!r}")
        if self.container not in CONTAINERS:
            raise ValueError(f"container must be one of {CONTAINERS}, got {self.container!r}")
        if self.encoding == "flac" and self.container != "raw":
            raise ValueError("encoding 'flac' is its own container: container must be 'raw', got 'wav'")
        if isinstance(self.speed_pct, bool) or not isinstance(self.speed_pct, int) \
                or not SPEED_MIN <= self.speed_pct <= SPEED_MAX:
            raise ValueError(f"speed_pct must be an integer in [{SPEED_MIN}, {SPEED_MAX}], got {self.speed_pct!r}")
        if isinstance(self.pitch_pct, bool) or not isinstance(self.pitch_pct, int) \
                or not PITCH_MIN <= self.pitch_pct <= PITCH_MAX:
            raise ValueError(f"pitch_pct must be an integer in [{PITCH_MIN}, {PITCH_MAX}], got {self.pitch_pct!r}")
        pitch_plan(self.speed_pct, self.pitch_pct)  # (the two together: the stretch they need must exist)
        if not isinstance(self.join, bool):
            raise ValueError(f"join must be true or false, got {self.join!r}")
        if isinstance(self.volume_pct, bool) or not isinstance(self.volume_pct, int) \
                or not VOLUME_MIN <= self.volume_pct <= VOLUME_MAX:
            raise ValueError(f"volume_pct must be an integer in [{VOLUME_MIN}, {VOLUME_MAX}], got {self.volume_pct!r}")
        if self.formant_pct is not None:
            formant_plan(self.speed_pct, self.pitch_pct, self.formant_pct)  # (the three together: the ratio must exist)
        for name, v, lo in (("pause_ms", self.pause_ms, 0), ("max_pause_ms", self.max_pause_ms, MAX_PAUSE_MS_MIN)):
            if v is not None and (isinstance(v, bool) or not isinstance(v, int) or not lo <= v <= PAUSE_MS_MAX or v % 10):
                raise ValueError(f"{name} must be an integer multiple of 10 in [{lo}, {PAUSE_MS_MAX}] or null, got {v!r}")
        if self.mark_key is not None or self.mark_id != 0 or self.mark_strength != 2:
            _check_mark(0 if self.mark_key is None else self.mark_key, self.mark_id, self.mark_strength)
        if self.pauses and self.encoding == "flac":
            raise ValueError("pause_ms / max_pause_ms with encoding 'flac': its frames are cut on the device, per "
                             "sentence, before the host could trim")

    @property
    def pauses(self) -> bool:
        """The format names a pause or a longest pause: the stream's rows pass the pause stage (``pause_slots_ref``)
        and its body ``PauseMux``."""
        return self.pause_ms is not None or self.max_pause_ms is not None

    @property
    def marks(self) -> bool:
        """The format names a watermark key: the stream's rows pass the mark stage (``mark_ref``)."""
        return self.mark_key is not None

    @property
    def is_default(self) -> bool:
        return (self.sample_rate == BASE_RATE and self.encoding == "f32le" and self.container == "raw"
                and self.speed_pct == 100 and self.pitch_pct == 100 and not self.join and self.volume_pct == 100
                and self.formant_pct is None and self.mark_key is None)

    @property
    def converts(self) -> bool:
        """The samples differ from the codec's (another rate, encoding, speed, pitch, volume or formant, or joined
        dumps): the stream needs the device stage."""
        return (self.sample_rate != BASE_RATE or self.encoding != "f32le" or self.speed_pct != 100
                or self.pitch_pct != 100 or self.join or self.volume_pct != 100 or self.formant != (1, 1)
                or self.pauses or self.marks)

    @property
    def stretch_pct(self) -> int:
        """What the time stretch runs at (``pitch_plan``): speed_pct itself without a pitch."""
        return pitch_plan(self.speed_pct, self.pitch_pct)[0]

    @property
    def ratio(self) -> Tuple[int, int]:
        """(L, M) of the resampling behind the stretch (``pitch_plan``): (1, 1) without a pitch."""
        return pitch_plan(self.speed_pct, self.pitch_pct)[1:]

    @property
    def formant(self) -> Tuple[int, int]:
        """(Fn, Fd) of the envelope correction behind the resampling (``formant_plan``): (1, 1) without a formant, and
        where the named formant is where the pitch has put the envelope anyway."""
        if self.formant_pct is None:
            return 1, 1
        return formant_plan(self.speed_pct, self.pitch_pct, self.formant_pct)

    @property
    def formant_moved(self) -> float:
        """The factor by which the spectral envelope moves against the model's own voice: formant_pct / 100 where the
        format names one, the realised pitch ratio M / L where it does not."""
        if self.formant_pct is not None:
            return self.formant_pct / 100.0
        L, M = self.ratio
        return M / L

    @property
    def sample_bytes(self) -> int:
        return _SAMPLE_DTYPE[self.encoding].itemsize

    @property
    def dtype(self):
        return _SAMPLE_DTYPE[self.encoding]

    @property
    def media_type(self) -> str:
        if self.encoding == "flac":
            return "audio/flac"
        return "audio/wav" if self.container == "wav" else "application/octet-stream"


def wav_header(fmt: AudioFormat) -> bytes:
    """The 44-byte RIFF / WAVE header of a mono stream of unknown length: both sizes 0xFFFFFFFF, format
    tag 1 (integer PCM) or 3 (IEEE float). G.711 (tag 7 mu-law, 6 A-law) takes the 58-byte form the WAVE
    specification asks of a non-PCM tag: an 18-byte fmt chunk (cbSize 0) and a fact chunk, its sample count
    unknown too (0xFFFFFFFF)."""
    if fmt.encoding in G711_LAWS:
        return (b"RIFF" + struct.pack("<I", 0xFFFFFFFF) + b"WAVE" + b"fmt "
                + struct.pack("<IHHIIHHH", 18, _G711_TAG[fmt.encoding], 1, fmt.sample_rate, fmt.sample_rate, 1, 8, 0)
                + b"fact" + struct.pack("<II", 4, 0xFFFFFFFF) + b"data" + struct.pack("<I", 0xFFFFFFFF))
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
    N, h = ratio_design(L, M)
    return L, M, N, h


def _check_ratio(L: int, M: int):
    if not (1 <= L <= RATIO_MAX and 1 <= M <= RATIO_MAX and M <= 4 * L and L <= 4 * M and gcd(L, M) == 1):
        raise ValueError(f"L / M must be coprime, each in 1 .. {RATIO_MAX}, with M <= 4 L and L <= 4 M, got {L} / {M}")


def ratio_design(L: int, M: int) -> Tuple[int, np.ndarray]:
    """(N, taps float64 [2 N + 1]) of the ratio L / M, the one design of the fixed rates and of the pitch
    control's ratios (the library stores it as fp32: ``lvx_pcm_ratio_filter``). 1 / 1 is the identity: N = 0
    and the tap 1."""
    _check_ratio(L, M)
    if L == M:
        return 0, np.ones(1)
    lo = min(1.0, L / M)
    fc = 0.5 * lo * 0.85 / L
    N = int(round(24 * L / lo))  # 24 max(L, M)
    n = np.arange(-N, N + 1)
    return N, L * 2 * fc * np.sinc(2 * fc * n) * np.kaiser(2 * N + 1, 9.0)


def _ratio_N(L: int, M: int) -> int:
    return 0 if L == M else 24 * max(L, M)


def ratio_emitted_upto(L: int, M: int, T: int, final: bool) -> int:
    """Outputs of a segment resampled by L / M emitted once T inputs are consumed (after a non-final / a
    final call)."""
    N = _ratio_N(L, M)
    full = -((-T * L) // M)
    if final or N == 0:
        return full
    a = (T - 1) * L - N
    return 0 if a < 0 else min(a // M + 1, full)


def ratio_emitted(L: int, M: int, t0: int, n_in: int, final: bool) -> int:
    """Samples a ratio call emits for a slot that has consumed t0 inputs of its segment
    (``lvx_pcm_ratio_emitted``)."""
    return ratio_emitted_upto(L, M, t0 + n_in, final) - ratio_emitted_upto(L, M, t0, False)


def emitted_upto(sample_rate: int, T: int, final: bool) -> int:
    """Outputs of a segment emitted once T inputs are consumed (after a non-final / a final call)."""
    L, M, _ = RATES[sample_rate]
    return ratio_emitted_upto(L, M, T, final)


def emitted(sample_rate: int, t0: int, n_in: int, final: bool) -> int:
    """Samples a call emits for a slot that has consumed t0 inputs of its segment (``lvx_pcm_emitted``)."""
    return emitted_upto(sample_rate, t0 + n_in, final) - emitted_upto(sample_rate, t0, False)


def resample_ref(x, sample_rate: int, taps=None, m0: int = 0, m1: Optional[int] = None, dtype=np.float32) -> np.ndarray:
    """Outputs m0 .. m1 - 1 (default: all ceil(T L / M)) of the segment x[0 .. T) at ``sample_rate``.
    dtype float32: the rule's fixed order (inputs ascending, a rounded product and a rounded sum per tap, no
    fused multiply-add), bit for bit what the device computes with the same fp32 taps. dtype float64: the
    same sums in double (with the fp32 taps' values): the yardstick of the device's accumulation error."""
    L, M, _ = RATES[sample_rate]
    return ratio_ref(x, L, M, taps, m0, m1, dtype)


def ratio_ref(x, L: int, M: int, taps=None, m0: int = 0, m1: Optional[int] = None, dtype=np.float32) -> np.ndarray:
    """``resample_ref`` for any ratio L / M the resampler takes (output count over input count): outputs
    m0 .. m1 - 1 (default: all ceil(T L / M)) of the segment x[0 .. T), in the rule's fixed fp32 order (the
    device's bits, ``lvx_pcm_ratio``, with the same fp32 taps) or, dtype float64, the same sums in double."""
    _check_ratio(L, M)
    N = _ratio_N(L, M)
    x = np.asarray(x, dtype=np.float32)
    T = x.shape[-1]
    if taps is None:
        taps = ratio_design(L, M)[1].astype(np.float32)
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


# ---- the G.711 rule (include/llmvox.h, "PCM G.711"), in numpy: integers only ---------------------------

def _bit_length7(t) -> np.ndarray:
    """The bit length of t, an int32 array in 0 .. 127."""
    n = np.zeros_like(t)
    for k in range(7):
        n += (t >> k) > 0
    return n


def _check_law(law: str):
    if law not in G711_LAWS:
        raise ValueError(f"law must be one of {G711_LAWS}, got {law!r}")


def g711_encode(q, law: str) -> np.ndarray:
    """The 8-bit codes (uint8) of the s16 samples q at ``law`` ("ulaw" / "alaw"): the ITU-T G.191 STL form, a
    negative q taken in one's complement (``lvx_pcm_g711_encode``; the device's epilogue after ``quantize_s16``)."""
    _check_law(law)
    q = np.asarray(q)
    if q.dtype.kind not in "iu" or (q.size and (q.min() < -32768 or q.max() > 32767)):
        raise ValueError("q must hold integers in -32768 .. 32767")
    q = q.astype(np.int32)
    sign = np.where(q >= 0, 0x80, 0).astype(np.int32)
    m = np.where(q >= 0, q, ~q)
    if law == "ulaw":
        a = np.minimum((m >> 2) + 33, 0x1FFF)
        seg = 1 + _bit_length7(a >> 6)
        return (((8 - seg) << 4) | (0xF - ((a >> seg) & 0xF)) | sign).astype(np.uint8)
    x = m >> 4
    e = _bit_length7(x >> 4)  # 0: x <= 15, the linear segment; else the loop's e
    x = np.where(e > 0, (x >> np.maximum(e - 1, 0)) - 16 + (e << 4), x)
    return ((x | sign) ^ 0x55).astype(np.uint8)


def g711_decode(codes, law: str) -> np.ndarray:
    """The s16 samples (int16) of the 8-bit codes at ``law`` (``lvx_pcm_g711_decode``): host only, what a client
    does with the stream."""
    _check_law(law)
    c = np.asarray(codes)
    if c.dtype.kind not in "iu" or (c.size and (c.min() < 0 or c.max() > 255)):
        raise ValueError("codes must hold integers in 0 .. 255")
    c = c.astype(np.int32)
    if law == "ulaw":
        m = ~c & 0xFF
        e = (m >> 4) & 7
        step = 4 << (e + 1)
        lin = (0x80 << e) + step * (m & 0xF) + step // 2 - 132
        return np.where(c < 0x80, -lin, lin).astype(np.int16)
    i = c ^ 0x55
    e = (i & 0x7F) >> 4
    m = (((i & 0xF) + np.where(e > 0, 16, 0)) << 4) + 8
    m = np.where(e > 1, m << np.maximum(e - 1, 0), m)
    return np.where(i & 0x80, m, -m).astype(np.int16)


def silence_byte(fmt) -> int:
    """The byte a stream of ``fmt`` (an AudioFormat or an encoding's name) is padded with: the G.711 code of
    q = 0 (0xFF mu-law, 0xD5 A-law); 0 for the PCM encodings, whose zero sample is zero bytes."""
    return _G711_SILENCE.get(getattr(fmt, "encoding", fmt), 0)


def frame_ms_of(v) -> Optional[int]:
    """A request's frame duration: None (today's chunking) or one of FRAME_MS, an integer; ValueError for anything
    else, a bool and a float included."""
    if v is None:
        return None
    if isinstance(v, bool) or not isinstance(v, int) or v not in FRAME_MS:
        raise ValueError(f"frame_ms must be one of {FRAME_MS} or null, got {v!r}")
    return v


def frame_bytes(fmt: AudioFormat, frame_ms: int) -> int:
    """Bytes of one frame of ``frame_ms`` milliseconds of ``fmt``: a whole number at every rate and duration."""
    return fmt.sample_rate * frame_ms_of(frame_ms) // 1000 * fmt.sample_bytes


def frame_chunks(chunks, fmt: AudioFormat, frame_ms: int):
    """The byte chunks of a stream of ``fmt`` re-cut on the host into whole frames of ``frame_ms`` milliseconds:
    every chunk yielded is a multiple of ``frame_bytes``; what a chunk leaves over waits for the next one; at the
    end the last partial frame is filled with the encoding's silence (``silence_byte``). The concatenation is the
    input's, then that fill."""
    size, rest = frame_bytes(fmt, frame_ms), b""
    for c in chunks:
        rest += c
        n = len(rest) // size * size
        if n:
            yield rest[:n]
            rest = rest[n:]
    if rest:
        yield rest + bytes([silence_byte(fmt)]) * (size - len(rest))


def encode_ref(y, fmt: AudioFormat) -> np.ndarray:
    if fmt.encoding == "flac":  # a whole sentence: every frame's slot, as the device writes them
        q = quantize_s16(y)
        return flac_slots_ref(q, fmt.sample_rate, 0, flac_frames_upto(fmt.sample_rate, q.size, True))
    if fmt.encoding in G711_LAWS:
        return g711_encode(quantize_s16(y), fmt.encoding)
    return quantize_s16(y) if fmt.encoding == "s16le" else np.asarray(y, dtype=np.float32)


# ---- the FLAC rule (include/llmvox.h, "PCM FLAC"), in numpy: integers only -----------------------------

_FLAC_RATE_CODE = {8000: 4, 16000: 5, 24000: 7, 48000: 10}


def flac_block(sample_rate: int) -> int:
    """BS = sample_rate / 25: the samples of a whole frame, 40 ms (``lvx_pcm_flac_block``)."""
    if sample_rate not in RATES:
        raise ValueError(f"unsupported sample rate {sample_rate}")
    return sample_rate // 25


def flac_slot_bytes(sample_rate: int) -> int:
    """Bytes of one slot of the device's output (LVX_FLAC_SLOT): the 8-byte record and the longest subframe of the
    rate, 1 + 2 (BS + 15) bytes, rounded up to 16."""
    return (8 + 1 + 2 * (flac_block(sample_rate) + 15) + 15) // 16 * 16


def flac_frames_upto(sample_rate: int, T: int, final: bool) -> int:
    """Frames of a segment emitted once T inputs are consumed: after a non-final call the whole frames
    max(0, floor((T - 16) / BS)); a final call adds the frame of the remaining samples."""
    k = max(0, (T - 16) // flac_block(sample_rate))
    return k + (1 if final and T > 0 else 0)


def flac_emitted(sample_rate: int, t0: int, n_in: int, final: bool) -> int:
    """Frames a FLAC call emits for a slot that has consumed t0 inputs of its segment (``lvx_pcm_flac_emitted``)."""
    if t0 < 0 or n_in < 0:
        raise ValueError("t0 and n_in must be >= 0")
    return flac_frames_upto(sample_rate, t0 + n_in, final) - flac_frames_upto(sample_rate, t0, False)


def flac_frames_of(T: int, sample_rate: int) -> List[int]:
    """The block sizes of a sentence of T samples: k = max(0, floor((T - 16) / BS)) frames of BS, then one frame of
    the remaining T - k BS (16 .. BS + 15 samples, fewer only for a sentence shorter than 16); none for T = 0."""
    bs = flac_block(sample_rate)
    if T <= 0:
        return []
    k = max(0, (T - 16) // bs)
    return [bs] * k + [T - k * bs]


def _flac_s16(x) -> np.ndarray:
    x = np.asarray(x)
    if x.dtype.kind not in "iu" or (x.size and (x.min() < -32768 or x.max() > 32767)):
        raise ValueError("the samples must be integers in -32768 .. 32767")
    return x.astype(np.int64).reshape(-1)


def _flac_put(bits: np.ndarray, pos, length: int, val):
    """The low ``length`` bits of val (arrays or scalars) at bit positions pos, MSB first."""
    pos, val = np.asarray(pos, dtype=np.int64), np.asarray(val, dtype=np.int64)
    for t in range(length):
        bits[pos + t] = (val >> (length - 1 - t)) & 1


def flac_subframe(x) -> bytes:
    """The subframe of the frame x[0 .. n), n >= 1 int16 samples, by the header's rule (``lvx_flac_subframe``; the
    device's ``pcm_flac_kernel``): CONSTANT, else FIXED of the order with the least error sum, its residuals Rice-coded
    in partitions, else VERBATIM where that is not smaller."""
    x = _flac_s16(x)
    n = x.size
    if n < 1:
        raise ValueError("a frame has at least one sample")
    if np.all(x == x[0]):
        return bytes([0x00]) + struct.pack(">H", int(x[0]) & 0xFFFF)
    diffs = [x]
    for _ in range(4):  # r_p[i] for i >= p (the entries in front hold differences with x[-1 ..] = 0 and are not used)
        diffs.append(np.diff(diffs[-1], prepend=0))
    E = [int(np.abs(d[4:]).sum()) for d in diffs]
    p = int(np.argmin(E))  # (the first of the least: the smallest p)
    r = diffs[p][p:]
    u = np.where(r >= 0, 2 * r, -2 * r - 1)
    P = 0
    while P < 3 and n % (2 << P) == 0:
        P += 1
    while P > 0 and (n >> P) < 16:
        P -= 1
    psize = n >> P
    parts, start = [], 0
    for j in range(1 << P):
        cnt = psize - (p if j == 0 else 0)
        uj = u[start:start + cnt]
        cost = [int(((uj >> k) + 1 + k).sum()) for k in range(FLAC_MAX_K + 1)]
        k = int(np.argmin(cost))  # (the smallest k at a tie)
        parts.append((k, uj, cost[k]))
        start += cnt
    total = 8 + 16 * p + 2 + 4 + sum(4 + c for _, _, c in parts)
    if total >= 8 + 16 * n:
        return bytes([0x02]) + (x & 0xFFFF).astype(">u2").tobytes()
    bits = np.zeros((total + 7) // 8 * 8, dtype=np.uint8)
    _flac_put(bits, 0, 8, (8 | p) << 1)
    _flac_put(bits, 8 + 16 * np.arange(p), 16, x[:p] & 0xFFFF)
    pos = 8 + 16 * p
    _flac_put(bits, pos, 6, P)  # the coding method 00, then P in 4 bits
    pos += 6
    for k, uj, c in parts:
        _flac_put(bits, pos, 4, k)
        pos += 4
        q = uj >> k
        ends = pos + np.cumsum(q + 1 + k)  # a sample's bits end here: q zeros, the one, k low bits
        bits[ends - k - 1] = 1
        _flac_put(bits, ends - k, k, uj & ((1 << k) - 1))
        pos += c
    assert pos == total
    return np.packbits(bits).tobytes()


def _crc_table(poly: int, width: int) -> List[int]:
    top, mask, table = 1 << (width - 1), (1 << width) - 1, []
    for i in range(256):
        c = i << (width - 8)
        for _ in range(8):
            c = ((c << 1) ^ poly) & mask if c & top else (c << 1) & mask
        table.append(c)
    return table


_CRC8, _CRC16 = _crc_table(0x07, 8), _crc_table(0x8005, 16)


def flac_crc8(data: bytes) -> int:
    """CRC-8 of a frame header: polynomial 0x07, initial value 0 (0xF4 over b"123456789")."""
    c = 0
    for b in data:
        c = _CRC8[c ^ b]
    return c


def flac_crc16(data: bytes) -> int:
    """CRC-16 of a frame: polynomial 0x8005, initial value 0, not reflected (0xFEE8 over b"123456789")."""
    c = 0
    for b in data:
        c = ((c << 8) & 0xFFFF) ^ _CRC16[(c >> 8) ^ b]
    return c


def _flac_utf8(v: int) -> bytes:
    """The sample number in FLAC's UTF-8-like coding: 1 .. 7 bytes for a number below 2^36."""
    if not 0 <= v < 1 << 36:
        raise ValueError(f"sample number {v} is outside [0, 2^36)")
    if v < 0x80:
        return bytes([v])
    n = 2
    while n < 7 and v >= 1 << (5 * n + 1):
        n += 1
    first = ((0xFF00 >> n) & 0xFF) | (v >> (6 * (n - 1)) if n < 7 else 0)
    return bytes([first] + [0x80 | ((v >> (6 * (n - 1 - i))) & 0x3F) for i in range(1, n)])


def flac_finish_ref(sample_rate: int, n: int, body: bytes, sample_no: int) -> bytes:
    """A frame from its subframe: the header (sync 0xFFF9, block size code 0111, the rate's code, 0x08, the first
    sample's number, n - 1 in 16 bits, the CRC-8), the subframe, the CRC-16 (``lvx_flac_finish`` for one slot)."""
    flac_block(sample_rate)
    if sample_no + n > 1 << 36:
        raise ValueError("the sample number passes 2^36")
    head = bytes([0xFF, 0xF9, 0x70 | _FLAC_RATE_CODE[sample_rate], 0x08]) + _flac_utf8(sample_no) + struct.pack(">H", n - 1)
    frame = head + bytes([flac_crc8(head)]) + body
    return frame + struct.pack(">H", flac_crc16(frame))


def flac_frame(x, sample_rate: int, sample_no: int) -> bytes:
    """The frame of the samples x at ``sample_rate`` whose first sample has the number ``sample_no``: at most
    2 n + 17 bytes."""
    x = _flac_s16(x)
    return flac_finish_ref(sample_rate, x.size, flac_subframe(x), sample_no)


def flac_stream_header(sample_rate: int) -> bytes:
    """"fLaC" and the one STREAMINFO block, 42 bytes (``lvx_flac_stream_header``): min blocksize 16, max blocksize
    BS + 15, mono, 16 bits; the frame sizes, the total sample count and the MD5 are 0 (unknown)."""
    bs = flac_block(sample_rate)
    info = struct.pack(">HH", 16, bs + 15) + bytes(6) + struct.pack(">Q", (sample_rate << 44) | (15 << 36)) + bytes(16)
    return b"fLaC" + bytes([0x80, 0, 0, 34]) + info


def flac_encode_ref(q, sample_rate: int, sample_no: int = 0, header: bool = True) -> bytes:
    """One sentence q (int16 samples at ``sample_rate``) as FLAC: the stream header (``header``), then the frames of
    ``flac_frames_of``, the first at ``sample_no``. What the device's slots give once ``lvx_flac_finish`` has run."""
    q = _flac_s16(q)
    out, at = [flac_stream_header(sample_rate)] if header else [], 0
    for n in flac_frames_of(q.size, sample_rate):
        out.append(flac_frame(q[at:at + n], sample_rate, sample_no + at))
        at += n
    return b"".join(out)


def flac_slots_ref(q, sample_rate: int, j0: int, j1: int) -> np.ndarray:
    """Frames j0 .. j1 - 1 of the sentence q as the device writes them (``lvx_pcm_flac``): slots of
    ``flac_slot_bytes``, each the record {u16 n, u16 body_bytes, u32 0}, the subframe, zeros (uint8)."""
    q = _flac_s16(q)
    bs, size = flac_block(sample_rate), flac_slot_bytes(sample_rate)
    sizes = flac_frames_of(q.size, sample_rate)
    out = np.zeros((j1 - j0) * size, dtype=np.uint8)
    for j in range(j0, j1):
        body = flac_subframe(q[j * bs:j * bs + sizes[j]])
        rec = struct.pack("<HHI", sizes[j], len(body), 0) + body
        out[(j - j0) * size:(j - j0) * size + len(rec)] = np.frombuffer(rec, dtype=np.uint8)
    return out


class FlacMux:
    """The host end of a FLAC stream: ``header()`` is the stream header; ``push(blob)`` turns the slots one call of
    the device stage delivered (bytes or uint8, whole slots of ``flac_slot_bytes``) into frames with the running
    sample number, through the library's ``lvx_flac_finish``. The one place that knows the speaking order."""

    def __init__(self, sample_rate: int):
        self.sample_rate, self.slot = sample_rate, flac_slot_bytes(sample_rate)
        self.sample_no = 0

    def header(self) -> bytes:
        return flac_stream_header(self.sample_rate)

    def push(self, blob) -> bytes:
        import ctypes

        from . import _lib
        blob = blob.tobytes() if isinstance(blob, np.ndarray) else bytes(blob)
        if len(blob) % self.slot:
            raise ValueError(f"{len(blob)} bytes are no whole slots of {self.slot}")
        frames = len(blob) // self.slot
        if not frames:
            return b""
        cap = frames * self.slot + 16 * frames  # (a frame is at most its subframe and 16 bytes)
        out = ctypes.create_string_buffer(cap)
        no = ctypes.c_ulonglong(self.sample_no)
        n = _lib.load().lvx_flac_finish(self.sample_rate, blob, frames, ctypes.byref(no), out, cap)
        if n < 0:
            raise _lib.error_for(int(n))
        self.sample_no = int(no.value)
        return out.raw[:n]


# ---- the pause rule (include/llmvox.h, "PCM pause"), in numpy: bytes copied, integers compared -----------

def pause_block(sample_rate: int) -> int:
    """bl = sample_rate / 100: the samples of a block, 10 ms."""
    if sample_rate not in RATES:
        raise ValueError(f"unsupported sample rate {sample_rate}")
    return sample_rate // 100


def pause_slot_bytes(fmt: AudioFormat) -> int:
    """Bytes of one slot of the device's output (LVX_PAUSE_SLOT, ``lvx_pcm_pause_slot``): the 8-byte record and a whole
    block of the format's samples."""
    return 8 + pause_block(fmt.sample_rate) * fmt.sample_bytes


def pause_blocks_upto(sample_rate: int, T: int, final: bool) -> int:
    """Blocks of a sentence emitted once T samples are consumed: after a non-final call the complete ones that at
    least one more sample follows, after a final call all ceil(T / bl)."""
    bl = pause_block(sample_rate)
    return 0 if T <= 0 else -(-T // bl) if final else (T - 1) // bl


def pause_emitted(sample_rate: int, t0: int, n_in: int, final: bool) -> int:
    """Blocks a pause call emits for a slot that has consumed t0 inputs of its segment (``lvx_pcm_pause_emitted``)."""
    if t0 < 0 or n_in < 0:
        raise ValueError("t0 and n_in must be >= 0")
    return pause_blocks_upto(sample_rate, t0 + n_in, final) - pause_blocks_upto(sample_rate, t0, False)


def pause_loud(y, fmt) -> np.ndarray:
    """Per encoded sample of y (the dtype of ``fmt``, an AudioFormat or an encoding's name): louder than PAUSE_THRESH
    on the 16-bit scale. s16le: |q| > 103 (in 32 bits); f32le: |v| > 103 / 32768, a NaN counting as loud; G.711: the
    s16le test on the decoded sample."""
    enc = getattr(fmt, "encoding", fmt)
    y = np.asarray(y, dtype=_SAMPLE_DTYPE[enc])
    if enc == "f32le":
        return ~(np.abs(y) <= np.float32(PAUSE_THRESH / 32768.0))
    q = g711_decode(y, enc) if enc in G711_LAWS else y
    return np.abs(q.astype(np.int32)) > PAUSE_THRESH


def pause_slots_ref(y, fmt: AudioFormat, j0: int, j1: int) -> np.ndarray:
    """Blocks j0 .. j1 - 1 of the finished sentence y (encoded samples of ``fmt``) as the device writes them
    (``lvx_pcm_pause``, ``lvx_pause_slots``): slots of ``pause_slot_bytes``, each the record {u16 n, u8 active, u8 last,
    u32 0} and the block's n samples, the encoding's silence up to bl (uint8)."""
    y = np.ascontiguousarray(y, dtype=fmt.dtype).reshape(-1)
    bl, size, bps = pause_block(fmt.sample_rate), pause_slot_bytes(fmt), fmt.sample_bytes
    blocks = pause_blocks_upto(fmt.sample_rate, y.size, True)
    if not 0 <= j0 <= j1 <= blocks:
        raise ValueError(f"blocks {j0} .. {j1} outside the sentence's {blocks}")
    raw, loud = y.view(np.uint8), pause_loud(y, fmt)
    out = np.full((j1 - j0) * size, silence_byte(fmt), dtype=np.uint8)
    for j in range(j0, j1):
        n, at = min(bl, y.size - j * bl), (j - j0) * size
        rec = struct.pack("<HBBI", n, int(loud[j * bl:j * bl + n].any()), int(j == blocks - 1), 0)
        out[at:at + 8] = np.frombuffer(rec, dtype=np.uint8)
        out[at + 8:at + 8 + n * bps] = raw[j * bl * bps:(j * bl + n) * bps]
    return out


def _pause_blocks(fmt: AudioFormat) -> Tuple[Optional[int], Optional[int]]:
    """(P, C) of a format in blocks: the gap between sentences and the longest run inside one (None: not named)."""
    if not fmt.pauses:
        raise ValueError("the format names neither pause_ms nor max_pause_ms")
    return (None if fmt.pause_ms is None else fmt.pause_ms // 10,
            None if fmt.max_pause_ms is None else fmt.max_pause_ms // 10)


def pause_ref(sentences, fmt: AudioFormat) -> bytes:
    """The body of a request whose finished sentences are ``sentences`` (encoded samples of ``fmt`` each, in speaking
    order), in one shot. P = pause_ms / 10 blocks, C = max_pause_ms / 10 blocks or none. With P: a sentence without an
    active block delivers nothing and takes part in no gap; any other delivers its blocks from max(first active -
    PAUSE_LEAD, 0) through min(last active + PAUSE_TRAIL, its last block), and between two delivering sentences come
    exactly P blocks of the encoding's silence. Without P (only max_pause_ms named) every sentence delivers all its
    blocks and no gap is inserted. With C, of the blocks a sentence delivers, a run of r > C silent ones between two
    active ones keeps its first C - 2 and its last 2. The sentence's last block is delivered with its n samples only.
    No crossfade: both sides of every cut are blocks whose peak is at most PAUSE_THRESH, -50 dBFS."""
    P, C = _pause_blocks(fmt)
    bl, bps = pause_block(fmt.sample_rate), fmt.sample_bytes
    gap = bytes([silence_byte(fmt)]) * (bl * bps)
    out, spoke = [], False
    for y in sentences:
        y = np.ascontiguousarray(y, dtype=fmt.dtype).reshape(-1)
        K = pause_blocks_upto(fmt.sample_rate, y.size, True)
        loud = pause_loud(y, fmt)
        active = [bool(loud[j * bl:(j + 1) * bl].any()) for j in range(K)]
        on = [j for j in range(K) if active[j]]
        if P is not None and not on:
            continue
        keep = set(range(K)) if P is None else set(range(max(on[0] - PAUSE_LEAD, 0), min(on[-1] + PAUSE_TRAIL, K - 1) + 1))
        if C is not None:
            for a, b in zip(on, on[1:]):  # the run a + 1 .. b - 1 between two active blocks
                if b - a - 1 > C:
                    keep -= set(range(a + 1 + C - 2, b - 2))
        if not keep:
            continue
        if P is not None and spoke:
            out.append(gap * P)
        spoke = True
        raw = y.view(np.uint8)
        out.extend(raw[j * bl * bps:(j + 1) * bl * bps].tobytes() for j in sorted(keep))
    return b"".join(out)


class PauseMux:
    """The host end of a pausing stream: ``push(blob)`` takes the slots one call of the device stage delivered (bytes
    or uint8, whole slots of ``pause_slot_bytes``, the request's sentences in speaking order) and returns the bytes that
    may leave now; the concatenation over a request is ``pause_ref`` of its sentences, however the pushes and the
    device calls were cut. An active block leaves at once, behind the silent blocks kept in front of it; the first
    PAUSE_TRAIL silent blocks behind an active one (the first C - 2 where no edge is trimmed) leave at once; further
    silent blocks wait until an active block or the sentence's last one decides their fate; the gap is emitted in
    front of the next delivering sentence's first block. Only silence ever waits: at most C blocks of it where the rule
    lets the middle of a long run go (a trimmed format with max_pause_ms), a sentence's silence otherwise."""

    def __init__(self, fmt: AudioFormat):
        self.P, self.C = _pause_blocks(fmt)
        self.fmt, self.slot = fmt, pause_slot_bytes(fmt)
        self.bps = fmt.sample_bytes
        self.gap = bytes([silence_byte(fmt)]) * (pause_block(fmt.sample_rate) * self.bps)
        self.spoke = False  # some sentence of the request has delivered
        self._sentence()

    def _sentence(self):
        self.seen = False          # the sentence has had an active block
        self.run = 0               # silent blocks since its last active one
        self.held: List[bytes] = []  # silent blocks that wait

    def push(self, blob) -> bytes:
        blob = blob.tobytes() if isinstance(blob, np.ndarray) else bytes(blob)
        if len(blob) % self.slot:
            raise ValueError(f"{len(blob)} bytes are no whole slots of {self.slot}")
        out: List[bytes] = []
        for at in range(0, len(blob), self.slot):
            n, active, last, zero = struct.unpack_from("<HBBI", blob, at)
            if not 1 <= n <= (self.slot - 8) // self.bps or active > 1 or last > 1 or zero or (n * self.bps != self.slot - 8 and not last):
                raise ValueError("a record that is none of the pause stage's")
            # (the sentence's last block: its n samples only)
            self._block(blob[at + 8:at + 8 + (n * self.bps if last else self.slot - 8)], bool(active), bool(last), out)
        return b"".join(out)

    def _block(self, payload: bytes, active: bool, last: bool, out: List[bytes]):
        P, C = self.P, self.C
        at_once = PAUSE_TRAIL if P is not None else C - 2  # silent blocks behind an active one that never wait
        if active:
            if not self.seen and P is not None and self.spoke:
                out.append(self.gap * P)
            if P is None and self.run > C:  # (the run's first C - 2 have left; a trimmed format pruned as it went)
                self.held = self.held[-2:]
            out.extend(self.held)
            out.append(payload)
            self.held, self.run, self.seen, self.spoke = [], 0, True, True
        elif not self.seen:  # in front of the first active block: the last PAUSE_LEAD wait, or nothing is trimmed
            if P is None:
                out.append(payload)
                self.spoke = True
            else:
                self.held = (self.held + [payload])[-PAUSE_LEAD:]
        else:
            self.run += 1
            if self.run <= at_once:
                out.append(payload)
            else:
                self.held.append(payload)
                if P is not None and C is not None and len(self.held) > C - 2 - at_once + 2:
                    del self.held[C - 2 - at_once]  # (neither of the run's first C - 2 nor of its last 2)
        if last:
            if P is None:  # no edge is trimmed: a run that no active block follows is kept whole
                out.extend(self.held)
            self._sentence()


# ---- the time stretch's rule (include/llmvox.h, "PCM time stretch"), in numpy -------------------------

def stretch_window() -> Tuple[np.ndarray, np.ndarray]:
    """(wr, wf) float32 [H]: the rising half-Hann window and its complement, built in double, each rounded
    once (the library's own: ``lvx_pcm_stretch_window``)."""
    n = np.arange(STRETCH_H, dtype=np.float64)
    wr = 0.5 - 0.5 * np.cos(np.pi * (n + 0.5) / STRETCH_H)
    return wr.astype(np.float32), (1.0 - wr).astype(np.float32)


def _stretch_a(j: int, speed_pct: int) -> int:
    return (j * STRETCH_H * speed_pct) // 100


def _stretch_need(j: int, speed_pct: int) -> int:
    """Inputs of the segment hop j reads (the exclusive upper end of what its search and output touch)."""
    if j == 0:
        return 2 * STRETCH_H
    return max(_stretch_a(j, speed_pct) + STRETCH_D + 2 * STRETCH_H,
               _stretch_a(j - 1, speed_pct) + STRETCH_D + 3 * STRETCH_H)


def _stretch_hops(speed_pct: int, T: int) -> int:
    """How many hops j have need_j <= T (need_j does not decrease with j)."""
    n = max(0, (T - 3 * STRETCH_H) * 100 // (STRETCH_H * speed_pct)) + 2
    while n > 0 and _stretch_need(n - 1, speed_pct) > T:
        n -= 1
    while _stretch_need(n, speed_pct) <= T:
        n += 1
    return n


def stretch_emitted_upto(speed_pct: int, T: int, final: bool) -> int:
    """Samples of a segment the stretch has emitted once T inputs are consumed (after a non-final / a final
    call). speed_pct 100 is no stretch: T."""
    if speed_pct == 100:
        return T
    if final:
        return -((-T * 100) // speed_pct)
    return STRETCH_H * _stretch_hops(speed_pct, T)


def stretch_emitted(speed_pct: int, t0: int, n_in: int, final: bool) -> int:
    """Samples a stretch call emits for a slot that has consumed t0 inputs of its segment
    (``lvx_pcm_stretch_emitted``)."""
    return stretch_emitted_upto(speed_pct, t0 + n_in, final) - stretch_emitted_upto(speed_pct, t0, False)


def _stretch_run(x, speed_pct: int, wr, wf, j0: int, j1: int, p_prev: int, force_d0: bool = False):
    """Hops j0 .. j1 - 1 of the segment x[0 .. T) (zero outside), continuing from p_{j0 - 1} = p_prev:
    (samples float32 [(j1 - j0) H], d int32 [j1 - j0], p_{j1 - 1}). Every product, sum and quotient is an fp32
    operation in the rule's order: the bits the device computes."""
    H, D, C = STRETCH_H, STRETCH_D, STRETCH_C
    x = np.asarray(x, dtype=np.float32).reshape(-1)
    lo = D + H  # the lowest input a hop reads is a_1 - D >= -D
    hi = _stretch_need(max(j1 - 1, 0), speed_pct) + H
    xp = np.zeros(lo + max(x.size, hi), dtype=np.float32)
    xp[lo:lo + x.size] = x
    y = np.zeros((j1 - j0) * H, dtype=np.float32)
    ds = np.zeros(j1 - j0, dtype=np.int32)
    eps = np.float32(1e-9)
    zero = np.zeros((2 * D + 1, 1), dtype=np.float32)
    for j in range(j0, j1):
        a = _stretch_a(j, speed_pct)
        e = p_prev + H
        d = 0
        if j >= 1 and not force_d0:
            span = xp[lo + a - D:lo + a + D + C]  # the candidates' inputs: 2 D + C of them
            tmpl = xp[lo + e:lo + e + C]
            cand = np.lib.stride_tricks.sliding_window_view(span, C)  # [2 D + 1, C]
            with np.errstate(invalid="ignore", over="ignore", under="ignore", divide="ignore"):
                # acc = 0, then acc = fl(acc + fl(product)) for k ascending: what an fp32 accumulate does
                corr = np.add.accumulate(np.concatenate([zero, cand * tmpl], axis=1), axis=1, dtype=np.float32)[:, -1]
                en = np.add.accumulate(np.concatenate([zero, cand * cand], axis=1), axis=1, dtype=np.float32)[:, -1]
                score = (corr * np.abs(corr)) / (en + eps)
            score = np.where(np.isnan(score), np.float32(-np.inf), score)
            best = np.nonzero(score == score.max())[0].astype(np.int64) - D
            d = int(best[np.lexsort((best, np.abs(best)))[0]])  # the smallest |d|; of +-d the negative one
        p = a + d
        with np.errstate(invalid="ignore", over="ignore", under="ignore"):
            y[(j - j0) * H:(j - j0 + 1) * H] = xp[lo + e:lo + e + H] * wf + xp[lo + p:lo + p + H] * wr
        ds[j - j0] = d
        p_prev = p
    return y, ds, p_prev


def stretch_ref(x, speed_pct: int, windows=None, force_d0: bool = False) -> Tuple[np.ndarray, np.ndarray]:
    """A whole segment x (float32 at 24 kHz) time-stretched to ceil(T 100 / speed_pct) samples: (samples
    float32, the chosen d_j of every hop int32). ``windows``: (wr, wf) fp32 tables (default: built here; the
    device tests pass the library's). ``force_d0``: plain overlap-add at the nominal positions (every
    d_j = 0), the yardstick of what the search buys. speed_pct 100: x itself and no hops."""
    x = np.asarray(x, dtype=np.float32).reshape(-1)
    if speed_pct == 100:
        return x.copy(), np.zeros(0, dtype=np.int32)
    wr, wf = windows if windows is not None else stretch_window()
    total = stretch_emitted_upto(speed_pct, x.size, True)
    hops = -(-total // STRETCH_H)
    y, ds, _ = _stretch_run(x, speed_pct, np.asarray(wr, np.float32), np.asarray(wf, np.float32), 0, hops,
                            -STRETCH_H, force_d0)
    return y[:total], ds


# ---- the dump join's rule (include/llmvox.h, "PCM dump join"), in numpy --------------------------------

def join_window() -> Tuple[np.ndarray, np.ndarray]:
    """(wr, wf) float32 [320]: the crossfade's rising half-Hann window and its complement, built in double,
    each rounded once (the library's own: ``lvx_pcm_join_window``)."""
    n = np.arange(JOIN_HOLD, dtype=np.float64)
    wr = 0.5 - 0.5 * np.cos(np.pi * (n + 0.5) / JOIN_HOLD)
    return wr.astype(np.float32), (1.0 - wr).astype(np.float32)


def join_emitted(open: bool, ctx_frames: int, n_in: int, final: bool) -> int:
    """Samples a join call of n_in samples, the first 320 ctx_frames of them context, emits for a slot whose
    segment is open or closed (``lvx_pcm_join_emitted``). ValueError for a call the rule does not admit."""
    c = ctx_frames
    bad = n_in < 0 or n_in % JOIN_HOLD or not 0 <= c <= JOIN_CONTEXT
    if not bad and n_in == 0:
        bad = not final or c != 0
    elif not bad:
        bad = JOIN_HOLD * c >= n_in or (c > 0 and not open)
    if bad:
        raise ValueError(f"not a join call: n_in {n_in}, ctx_frames {c}, final {bool(final)}, "
                         f"{'open' if open else 'closed'} segment")
    if n_in == 0:
        return JOIN_HOLD if open else 0
    return (JOIN_HOLD if open else 0) + n_in - JOIN_HOLD * c - (0 if final else JOIN_HOLD)


def _join_step(tail: Optional[np.ndarray], r: np.ndarray, c: int, final: bool, wr, wf):
    """One call of the rule for a slot whose tail is ``tail`` (None: closed): (samples emitted float32, the
    slot's next tail or None). Head, body, state, in the header's order; every product and the sum of the
    crossfade an fp32 operation."""
    n_out = join_emitted(tail is not None, c, r.size, final)
    s = JOIN_HOLD * c
    parts = []
    if tail is not None:
        if c >= 1:
            with np.errstate(invalid="ignore", over="ignore", under="ignore"):
                parts.append(tail * wf + r[s - JOIN_HOLD:s] * wr)
        else:
            parts.append(tail)
    if r.size:
        parts.append(r[s:] if final else r[s:r.size - JOIN_HOLD])
    out = np.concatenate(parts).astype(np.float32) if parts else np.zeros(0, dtype=np.float32)
    assert out.size == n_out
    return out, (None if final else r[r.size - JOIN_HOLD:].copy())


def join_ref(rows, ctx_frames, windows=None) -> List[np.ndarray]:
    """The rule over the calls of one sentence: ``rows[k]`` (float32, 320 (c_k + Lb_k) samples) is the codec's
    rendering of call k's ``ctx_frames[k]`` context frames followed by its new frames; the last call is the
    final one (an empty last row: a flush). Returns what each call emits; concatenated, 320 samples per frame
    of the sentence. ``windows``: (wr, wf) fp32 tables (default: built here; the device tests pass the
    library's). The bits the device computes (``lvx_pcm_join``)."""
    wr, wf = windows if windows is not None else join_window()
    wr, wf = np.asarray(wr, dtype=np.float32), np.asarray(wf, dtype=np.float32)
    if len(rows) != len(ctx_frames):
        raise ValueError("one ctx_frames per row")
    out, tail = [], None
    for k, (r, c) in enumerate(zip(rows, ctx_frames)):
        y, tail = _join_step(tail, np.asarray(r, dtype=np.float32).reshape(-1), int(c), k == len(rows) - 1, wr, wf)
        out.append(y)
    return out


# ---- the volume control's rule (include/llmvox.h, "PCM level"), in numpy --------------------------------

def _check_volume(volume_pct) -> int:
    if isinstance(volume_pct, bool) or not isinstance(volume_pct, (int, np.integer)) \
            or not VOLUME_MIN <= volume_pct <= VOLUME_MAX:
        raise ValueError(f"volume_pct must be an integer in [{VOLUME_MIN}, {VOLUME_MAX}], got {volume_pct!r}")
    return int(volume_pct)


def level_window() -> np.ndarray:
    """w float32 [2 A + 1]: the limiter's smoothing window w[k] = (0.5 + 0.5 cos(pi k / (A + 1))) / (A + 1),
    k = -A .. A, built in double, each tap rounded once (the library's own: ``lvx_pcm_level_window``)."""
    k = np.arange(-LEVEL_A, LEVEL_A + 1, dtype=np.float64)
    return ((0.5 + 0.5 * np.cos(np.pi * k / (LEVEL_A + 1))) / (LEVEL_A + 1)).astype(np.float32)


def level_emitted_upto(volume_pct: int, T: int, final: bool) -> int:
    """Samples of a segment the level stage has emitted once T inputs are consumed (after a non-final / a
    final call): the last 2 A wait for their right-hand inputs. volume_pct 100 is no stage: T."""
    if volume_pct == 100 or final:
        return T
    return max(0, T - 2 * LEVEL_A)


def level_emitted(volume_pct: int, t0: int, n_in: int, final: bool) -> int:
    """Samples a level call emits for a slot that has consumed t0 inputs of its segment
    (``lvx_pcm_level_emitted``)."""
    _check_volume(volume_pct)
    if t0 < 0 or n_in < 0:
        raise ValueError("t0 and n_in must be >= 0")
    return level_emitted_upto(volume_pct, t0 + n_in, final) - level_emitted_upto(volume_pct, t0, False)


def level_ref(x, volume_pct: int, window=None, n0: int = 0, n1: Optional[int] = None) -> Tuple[np.ndarray, np.ndarray]:
    """Outputs n0 .. n1 - 1 (default: all T) of the segment x[0 .. T) (float32 at 24 kHz, zero outside) at
    ``volume_pct``: (samples float32, the gains g[n] float32). The gain G = volume_pct / 100, then the
    feed-forward limiter, every product, quotient and sum an fp32 operation in the rule's order (the 241-term
    sum k ascending, no fused multiply-add): the bits the device computes (``lvx_pcm_level``) with the same
    fp32 window. ``window``: the fp32 table (default: built here; the device tests pass the library's).
    volume_pct 100 is evaluated like any other (the service never sends such a stream here)."""
    pct = _check_volume(volume_pct)
    A, R, c = LEVEL_A, LEVEL_R, LEVEL_CEIL
    x = np.asarray(x, dtype=np.float32)
    T = x.shape[-1]
    if n1 is None:
        n1 = T
    n = max(0, n1 - n0)
    w = level_window() if window is None else np.asarray(window, dtype=np.float32)
    if w.shape != (2 * A + 1,):
        raise ValueError(f"the window has {2 * A + 1} taps")
    lead = x.shape[:-1]
    if n == 0:
        return np.zeros(lead + (0,), dtype=np.float32), np.zeros(lead + (0,), dtype=np.float32)
    lo, hi = n0 - 2 * A - R, n1 + 2 * A  # r over [n0 - A - R, hi) is what the outputs read; the rest is slack
    xs = np.zeros(lead + (hi - lo,), dtype=np.float32)
    a, b = max(lo, 0), min(hi, T)
    if b > a:
        xs[..., a - lo:b - lo] = x[..., a:b]
    G = np.float32(pct / 100.0)
    one = np.float32(1.0)
    with np.errstate(invalid="ignore", over="ignore", under="ignore", divide="ignore"):
        v = G * xs
        av = np.abs(v)
        r = np.where(av > c, c / np.where(av > c, av, one), one).astype(np.float32)
        # m[i] = min r[i - R .. i + A] for i in [n0 - A, n1 + A): the window that starts at r's index i - R - lo
        m = np.lib.stride_tricks.sliding_window_view(r[..., A:], R + A + 1, axis=-1).min(axis=-1)
        d = one - m  # [n + 2 A]: d[j] is the segment's d[n0 - A + j]
        acc = np.zeros(lead + (n,), dtype=np.float32)
        for k in range(2 * A + 1):  # k ascending: acc = fl(acc + fl(d[n + k] w[k]))
            acc = acc + d[..., k:k + n] * w[k]
        s = one - acc
        rn = r[..., 2 * A + R:2 * A + R + n]
        g = np.maximum(np.float32(0.0), np.minimum(s, rn)).astype(np.float32)
        y = (v[..., 2 * A + R:2 * A + R + n] * g).astype(np.float32)
    return y, g


# ---- the formant control's rule (include/llmvox.h, "PCM formant"), in numpy -----------------------------

def _check_formant(Fn: int, Fd: int):
    if not (1 <= Fn <= FORMANT_MAX_TERM and 1 <= Fd <= FORMANT_MAX_TERM and Fd <= 2 * Fn and Fn <= 2 * Fd
            and gcd(Fn, Fd) == 1):
        raise ValueError(f"Fn / Fd must be coprime, each in 1 .. {FORMANT_MAX_TERM}, with Fd <= 2 Fn and Fn <= 2 Fd, "
                         f"got {Fn} / {Fd}")


def formant_tables() -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """(w float32 [1024], c float32 [25], tw float32 [1024]): the formant stage's window w[n] = 0.5 - 0.5 cos(2 pi
    (n + 0.5) / N), its smoothing taps c[d] = (0.5 + 0.5 cos(pi d / (K + 1))) / (K + 1), d = -K .. K, and the
    twiddles exp(-2 pi i k / N), k < N / 2 (tw[:512] the real parts cos(2 pi k / N), tw[512:] the imaginary parts
    -sin(2 pi k / N)), built in double, each entry rounded once (the library's own: ``lvx_pcm_formant_tables``)."""
    N, K = FORMANT_N, FORMANT_K
    n = np.arange(N, dtype=np.float64)
    w = 0.5 - 0.5 * np.cos(2.0 * np.pi * (n + 0.5) / N)
    d = np.arange(-K, K + 1, dtype=np.float64)
    c = (0.5 + 0.5 * np.cos(np.pi * d / (K + 1))) / (K + 1)
    k = np.arange(N // 2, dtype=np.float64)
    tw = np.concatenate([np.cos(2.0 * np.pi * k / N), -np.sin(2.0 * np.pi * k / N)])
    return w.astype(np.float32), c.astype(np.float32), tw.astype(np.float32)


def formant_emitted_upto(T: int, final: bool) -> int:
    """Samples of a segment the formant stage has emitted once T inputs are consumed (after a non-final / a final
    call): a hop block waits for the four frames that cover it, so the last 768 .. 1023 wait for more input."""
    if final:
        return T
    return max(0, (T // FORMANT_H - 3) * FORMANT_H)


def formant_emitted(t0: int, n_in: int, final: bool) -> int:
    """Samples a formant call emits for a slot that has consumed t0 inputs of its segment
    (``lvx_pcm_formant_emitted``)."""
    if t0 < 0 or n_in < 0:
        raise ValueError("t0 and n_in must be >= 0")
    return formant_emitted_upto(t0 + n_in, final) - formant_emitted_upto(t0, False)


_FORMANT_REV = np.array([int(format(n, "010b")[::-1], 2) for n in range(FORMANT_N)], dtype=np.int64)


def _formant_dft(re: np.ndarray, im: np.ndarray, tr: np.ndarray, ti: np.ndarray) -> Tuple[np.ndarray, np.ndarray]:
    """The rule's DFT_N of float32 [..., N] (natural order in and out) with the twiddles tr + ti i: radix 2, decimation
    in time, ten stages of whole-array float32 operations, each product and each sum rounded on its own."""
    N = FORMANT_N
    lead = re.shape[:-1]
    re, im = re[..., _FORMANT_REV], im[..., _FORMANT_REV]
    h = 1
    while h < N:
        wr, wi = tr[::N // (2 * h)], ti[::N // (2 * h)]  # the h twiddles of the stage
        a, b = re.reshape(lead + (N // (2 * h), 2, h)), im.reshape(lead + (N // (2 * h), 2, h))
        ur, ui, vr, vi = a[..., 0, :], b[..., 0, :], a[..., 1, :], b[..., 1, :]
        pr = vr * wr - vi * wi
        pi = vr * wi + vi * wr
        re = np.stack([ur + pr, ur - pr], axis=-2).reshape(lead + (N,))
        im = np.stack([ui + pi, ui - pi], axis=-2).reshape(lead + (N,))
        h *= 2
    return re, im


def _formant_stft(x: np.ndarray, j0: int, j1: int, tables, gains) -> Tuple[np.ndarray, np.ndarray]:
    """Frames j0 .. j1 - 1 of the segment x[..., T) by the rule's steps 1, 7 and 8 around ``gains(re, im)``, which
    turns the bins 0 .. N / 2 of the frames' spectra into their gains (the formant rule's steps 2 to 6, the mark
    rule's table): (y float32 [..., j1 - j0, N], the gains G float32 [..., j1 - j0, N / 2 + 1])."""
    N, H = FORMANT_N, FORMANT_H
    w, _, tw = tables
    tr, ti = tw[:N // 2], tw[N // 2:]
    T = x.shape[-1]
    lo, hi = (j0 - 3) * H, (j1 + 3) * H  # frame j covers [(j - 3) H, (j + 1) H); the rest is slack
    xs = np.zeros(x.shape[:-1] + (hi - lo,), dtype=np.float32)
    a, b = max(lo, 0), min(hi, T)
    if b > a:
        xs[..., a - lo:b - lo] = x[..., a:b]
    fr = np.lib.stride_tricks.sliding_window_view(xs, N, axis=-1)[..., ::H, :][..., :j1 - j0, :]
    with np.errstate(invalid="ignore", over="ignore", under="ignore", divide="ignore"):
        re, im = _formant_dft(w * fr, np.zeros(fr.shape, dtype=np.float32), tr, ti)  # 1.
        re, im = re[..., :N // 2 + 1], im[..., :N // 2 + 1]
        G = gains(re, im)
        yr, yi = G * re, G * im  # 7.
        yr = np.concatenate([yr, yr[..., N // 2 - 1:0:-1]], axis=-1)
        yi = np.concatenate([yi, -yi[..., N // 2 - 1:0:-1]], axis=-1)
        back = _formant_dft(yr, yi, tr, -ti)[0]
        y = w * (np.float32(2.0 ** -10) * back)  # 8.
    return y.astype(np.float32), G


def _formant_sum(y: np.ndarray, nb: int) -> np.ndarray:
    """The output sum of nb hop blocks from the frames y [..., nb + 3, N] that cover them, in ascending j:
    fl(s (((y_b + y_b+1) + y_b+2) + y_b+3)), float32 [..., nb H]."""
    H = FORMANT_H
    acc = y[..., 0:nb, 3 * H:]
    for q in (1, 2, 3):
        acc = acc + y[..., q:q + nb, (3 - q) * H:(4 - q) * H]
    out = np.float32(2.0 / 3.0) * acc
    return out.reshape(y.shape[:-2] + (nb * H,))


def _formant_frames(x: np.ndarray, Fn: int, Fd: int, j0: int, j1: int, tables) -> Tuple[np.ndarray, np.ndarray]:
    """Frames j0 .. j1 - 1 of the segment x[..., T) by the rule's eight steps: (y float32 [..., j1 - j0, N], the
    gains G float32 [..., j1 - j0, N / 2 + 1])."""
    N, K = FORMANT_N, FORMANT_K
    c = tables[1]

    def gains(re, im):
        P = re * re + im * im  # 2.
        at = np.abs(np.arange(-K, N // 2 + 1 + K))
        Pe = P[..., np.where(at > N // 2, N - at, at)]  # 3.
        E = np.zeros(P.shape, dtype=np.float32)
        for d in range(2 * K + 1):  # 4. d ascending: acc = fl(acc + fl(c[d] P[k + d]))
            E = E + c[d] * Pe[..., d:d + N // 2 + 1]
        kn = np.arange(N // 2 + 1, dtype=np.int64) * Fn  # 5.
        i = kn // Fd
        f = (kn % Fd).astype(np.float32) / np.float32(Fd)
        i0 = np.minimum(i, N // 2 - 1)
        e0 = E[..., i0]
        Es = np.where(i >= N // 2, E[..., N // 2:], e0 + f * (E[..., i0 + 1] - e0))
        G2 = np.minimum(np.maximum((Es + FORMANT_EPS) / (E + FORMANT_EPS), FORMANT_G2_MIN), FORMANT_G2_MAX)  # 6.
        return np.sqrt(G2).astype(np.float32)

    return _formant_stft(x, j0, j1, tables, gains)


def formant_gains(x, Fn: int, Fd: int, tables=None) -> np.ndarray:
    """The gains G[j, k] float32 [..., ceil(T / H) + 3, 513] every frame of the segment x applies to its bins."""
    _check_formant(Fn, Fd)
    x = np.asarray(x, dtype=np.float32)
    tables = formant_tables() if tables is None else tuple(np.asarray(t, dtype=np.float32) for t in tables)
    return _formant_frames(x, Fn, Fd, 0, -(-x.shape[-1] // FORMANT_H) + 3, tables)[1]


def formant_ref(x, Fn: int, Fd: int, tables=None, n0: int = 0, n1: Optional[int] = None) -> np.ndarray:
    """Outputs n0 .. n1 - 1 (default: all T; n0 a multiple of H) of the segment x[0 .. T) (float32 at 24 kHz, zero
    outside) with its spectral envelope moved by Fd / Fn (the envelope of the output at bin k is that of the input at
    k Fn / Fd): frames of 1024 at a hop of 256, in each the smoothed power spectrum looked up at k Fn / Fd over
    itself, the square root of that as a gain on the bins, and the overlap-add of the four frames that cover a hop,
    every operation fp32 in the rule's order (the transform's factorisation included): the bits the device computes
    (``lvx_pcm_formant``) with the same fp32 tables. ``tables``: (w, c, tw) (default: built here; the device tests pass
    the library's). 1 / 1 is evaluated like any other (the service never sends such a stream here). The bit identity
    is for finite input: a NaN or an infinity spreads through its frames' transforms, and there the device may differ
    (which NaN an operation returns is the processor's; the device's min and max drop a NaN, numpy's keep it)."""
    _check_formant(Fn, Fd)
    H = FORMANT_H
    x = np.asarray(x, dtype=np.float32)
    T = x.shape[-1]
    if n1 is None:
        n1 = T
    if n0 % H:
        raise ValueError("n0 must be a multiple of the hop")
    if n1 <= n0:
        return np.zeros(x.shape[:-1] + (0,), dtype=np.float32)
    tables = formant_tables() if tables is None else tuple(np.asarray(t, dtype=np.float32) for t in tables)
    b0, b1 = n0 // H, -(-n1 // H)  # the hop blocks of the outputs; block b is covered by the frames b .. b + 3
    y = _formant_frames(x, Fn, Fd, b0, b1 + 3, tables)[0]
    return _formant_sum(y, b1 - b0)[..., :n1 - n0].astype(np.float32)


# ---- the watermark's rule (include/llmvox.h, "PCM mark"), in numpy, and its detector --------------------

_MASK64 = (1 << 64) - 1


def _check_mark(key, mark_id, strength):
    # (no message repeats the key)
    if isinstance(key, bool) or not isinstance(key, (int, np.integer)) or not 0 <= int(key) <= _MASK64:
        raise ValueError("mark_key must be an integer in 0 .. 2^64 - 1")
    if isinstance(mark_id, bool) or not isinstance(mark_id, (int, np.integer)) or not 0 <= mark_id <= 255:
        raise ValueError(f"mark_id must be an integer in [0, 255], got {mark_id!r}")
    if isinstance(strength, bool) or not isinstance(strength, (int, np.integer)) \
            or not MARK_STRENGTH_MIN <= strength <= MARK_STRENGTH_MAX:
        raise ValueError(f"mark_strength must be an integer in [{MARK_STRENGTH_MIN}, {MARK_STRENGTH_MAX}], "
                         f"got {strength!r}")


def mark_table(key: int, mark_id: int = 0) -> np.ndarray:
    """uint16 [64]: the watermark's sign table (``lvx_pcm_mark_table``), integers only. Bit m of word p is
    c(p, m) XOR bit ((12 p + m) mod 8) of ``mark_id``, c the top bit of output number 12 p + m of SplitMix64 started
    at ``key``. A set bit: pair m of block p has g- on its even sub-band and g+ on its odd one; clear: the opposite."""
    _check_mark(key, mark_id, MARK_STRENGTH_MIN)
    state, words = int(key), np.zeros(MARK_P, dtype=np.uint16)
    for p in range(MARK_P):
        word = 0
        for m in range(MARK_PAIRS):
            state = (state + 0x9E3779B97F4A7C15) & _MASK64
            z = state
            z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & _MASK64
            z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & _MASK64
            z ^= z >> 31
            word |= ((z >> 63) ^ ((int(mark_id) >> ((MARK_PAIRS * p + m) % 8)) & 1)) << m
        words[p] = word
    return words


def mark_emitted_upto(T: int, final: bool) -> int:
    """Samples of a segment the mark stage has emitted once T inputs are consumed: the formant stage's count."""
    return formant_emitted_upto(T, final)


def mark_emitted(t0: int, n_in: int, final: bool) -> int:
    """Samples a mark call emits for a slot that has consumed t0 inputs of its segment (``lvx_pcm_mark_emitted``)."""
    return formant_emitted(t0, n_in, final)


def mark_gains(words, strength: int, j0: int, j1: int) -> np.ndarray:
    """The gains G[j, k] float32 [j1 - j0, 513] of the frames j0 .. j1 - 1 under the sign table ``words``: 1 outside
    the band, inside the pair's g+ = 1 + a or g- = 1 - a from word (j div Q) mod P, a = 2^-(7 - strength)."""
    a = np.float32(2.0 ** -(7 - int(strength)))
    gp, gm = np.float32(1.0) + a, np.float32(1.0) - a
    words = np.asarray(words, dtype=np.uint16).astype(np.int64)
    word = words[(np.arange(j0, j1) // MARK_Q) % MARK_P]  # [frames]
    u = np.arange(MARK_U)
    bit = (word[:, None] >> (u // 2)[None, :]) & 1  # [frames, U]
    g = np.where(bit == (u % 2)[None, :], gp, gm).astype(np.float32)  # a set bit: g- on the even, g+ on the odd
    G = np.ones((j1 - j0, FORMANT_N // 2 + 1), dtype=np.float32)
    G[:, MARK_K0:MARK_K0 + MARK_U * MARK_BW] = np.repeat(g, MARK_BW, axis=1)
    return G


def mark_ref(x, key: int, mark_id: int = 0, strength: int = 2, tables=None, n0: int = 0, n1: Optional[int] = None,
             words=None) -> np.ndarray:
    """Outputs n0 .. n1 - 1 (default: all T; n0 a multiple of H) of the segment x[0 .. T) (float32 at 24 kHz, zero
    outside) under the watermark of (key, mark_id, strength): the formant stage's frames, transform and output sum
    (``formant_ref``), the gain of a bin a lookup in ``mark_table``, every operation fp32 in the rule's order: the bits
    the device computes (``lvx_pcm_mark``) with the same fp32 tables. ``tables``: the formant stage's (w, c, tw)
    (default: built here); ``words``: the sign table (default: built here; the device tests pass the library's)."""
    _check_mark(key, mark_id, strength)
    H = FORMANT_H
    x = np.asarray(x, dtype=np.float32)
    T = x.shape[-1]
    if n1 is None:
        n1 = T
    if n0 % H:
        raise ValueError("n0 must be a multiple of the hop")
    if n1 <= n0:
        return np.zeros(x.shape[:-1] + (0,), dtype=np.float32)
    tables = formant_tables() if tables is None else tuple(np.asarray(t, dtype=np.float32) for t in tables)
    words = mark_table(key, mark_id) if words is None else np.asarray(words, dtype=np.uint16)
    b0, b1 = n0 // H, -(-n1 // H)  # the hop blocks of the outputs; block b is covered by the frames b .. b + 3
    G = mark_gains(words, strength, b0, b1 + 3)
    y = _formant_stft(x, b0, b1 + 3, tables, lambda re, im: G)[0]
    return _formant_sum(y, b1 - b0)[..., :n1 - n0].astype(np.float32)


_MARK_TO_BASE = {8000: (3, 1), 16000: (3, 2), 24000: (1, 1), 48000: (1, 2)}  # (L, M) that bring a rate to 24 kHz
MARK_DETECT_STEP = 64      # the detector's hop and the step of its sample offsets
MARK_DETECT_MIN = 8.0      # detected: S >= 8 (P(S >= 8) <= 2^8 P(N(0, 1) >= 8) per candidate under no mark)


def _mark_search(z: np.ndarray, signs: np.ndarray) -> Tuple[float, np.ndarray, int]:
    """The detector's search over one stretch of 24 kHz audio z (float64): (S, z_b [8], offset) of the best of the
    16 sample offsets x 64 block phases. ``signs``: +-1 [P, 12] from the key alone."""
    N, H, Q, P, U, BW, K0, step = FORMANT_N, FORMANT_H, MARK_Q, MARK_P, MARK_U, MARK_BW, MARK_K0, MARK_DETECT_STEP
    w = 0.5 - 0.5 * np.cos(2.0 * np.pi * (np.arange(N) + 0.5) / N)
    zp = np.concatenate([np.zeros(3 * H), z, np.zeros(N)])
    n_fr = (zp.size - N) // step
    best = (-1.0, np.zeros(8), 0)
    if n_fr <= 0:
        return best
    fr = np.lib.stride_tricks.sliding_window_view(zp, N)[::step][:n_fr]
    X = np.fft.rfft(w * fr, axis=-1)[:, K0:K0 + U * BW]
    Pw = (X.real ** 2 + X.imag ** 2).reshape(n_fr, U, BW).sum(-1)  # the power of every sub-band at every hop
    per, bits = H // step, (MARK_PAIRS * np.arange(P)[:, None] + np.arange(MARK_PAIRS)[None, :]) % 8
    for off in range(0, Q * H, step):  # where a block starts, in samples
        o = off // step
        nb = (n_fr - o - 3 * per) // (Q * per)
        if nb < 3:
            continue
        i1 = o + (np.arange(nb) * Q + 1) * per  # the block's two middle frames
        L = np.log(Pw[i1] + Pw[i1 + per] + 1e-12)
        D = L[:, 0::2] - L[:, 1::2]  # even sub-band over odd, per pair
        d = D[1:-1] - 0.5 * (D[:-2] + D[2:])  # against the neighbouring blocks: the speech's own envelope cancels
        sd = 1.48 * np.median(np.abs(d))
        d = np.clip(d, -2.0 * sd, 2.0 * sd)
        d2 = d * d
        for ph in range(P):  # which block of the period the first one is
            q = (np.arange(1, nb - 1) + ph) % P
            c, ii = d * signs[q], bits[q]
            num = np.array([c[ii == b].sum() for b in range(8)])
            den = np.sqrt(np.array([d2[ii == b].sum() for b in range(8)]))
            zb = num / np.maximum(den, 1e-30)
            S = float(np.abs(zb).sum() / np.sqrt(8.0))
            if S > best[0]:
                best = (S, zb, off)
    return best


def mark_detect(x, sample_rate: int, key: int, window_s: Optional[float] = None) -> Tuple[float, bool, int, int]:
    """The watermark's blind detector: (S, detected, id, offset) of the audio x (float samples at ``sample_rate``, one
    of the service's four) under ``key``. x is brought to 24 kHz (``ratio_ref`` by 3/1, 3/2, 1/1 or 1/2); the powers
    of the 24 sub-bands are taken at a hop of 64; for every candidate alignment (16 sample offsets x 64 block phases)
    each block gives D[m] = log power of pair m's even sub-band minus its odd one's from the block's two middle
    frames, d = D_q - (D_{q-1} + D_{q+1}) / 2 clipped at twice its robust spread, and every payload bit b
    z_b = sum(d sign) / sqrt(sum d^2) over its chips, the signs from the key alone; S = sum |z_b| / sqrt(8). The best
    candidate is reported; ``id`` from the signs of its z_b; ``detected`` is S >= 8; ``offset`` the sample (at 24 kHz)
    at which its blocks start, plus the window's start. ``window_s``: search windows of that many seconds at half that
    step instead of the whole signal and report the best (every sentence of a request restarts the pattern)."""
    _check_mark(key, 0, MARK_STRENGTH_MIN)
    if sample_rate not in _MARK_TO_BASE:
        raise ValueError(f"sample_rate must be one of {sorted(_MARK_TO_BASE)}, got {sample_rate!r}")
    x = np.asarray(x, dtype=np.float32).reshape(-1)
    L, M = _MARK_TO_BASE[sample_rate]
    z = (ratio_ref(x, L, M) if L != M else x).astype(np.float64)
    signs = 1.0 - 2.0 * ((mark_table(key, 0).astype(np.int64)[:, None] >> np.arange(MARK_PAIRS)[None, :]) & 1)
    if window_s is None:
        starts, n = [0], max(z.size, 1)
    else:
        n = int(round(window_s * BASE_RATE))
        if n < 8 * MARK_Q * FORMANT_H:
            raise ValueError(f"window_s must cover at least 8 blocks ({8 * MARK_Q * FORMANT_H / BASE_RATE:.3f} s)")
        starts = list(range(0, max(z.size - n, 0) + 1, max(n // 2, 1)))
    best = (-1.0, np.zeros(8), 0)
    for s0 in starts:
        S, zb, off = _mark_search(z[s0:s0 + n], signs)
        if S > best[0]:
            best = (S, zb, s0 + off)
    S, zb, off = best
    mark_id = int(sum(1 << b for b in range(8) if zb[b] < 0))
    return max(S, 0.0), bool(S >= MARK_DETECT_MIN), mark_id, int(off)


def convert_ref(x, fmt: AudioFormat, taps=None, windows=None, ratio_taps=None, level_win=None,
                formant_tabs=None) -> np.ndarray:
    """A whole segment x (float32 at 24 kHz) at the format's speed, pitch, volume, rate and encoding (a float32,
    int16 or uint8 array): stretched at the plan's stretch_pct, resampled by its L / M, its envelope corrected by
    the plan's Fn / Fd, watermarked where it names a key, levelled at its volume_pct, then resampled to the rate and encoded. ``ratio_taps``: the fp32
    table of the format's ratio (default: designed here); ``level_win``: the level stage's fp32 window (default:
    built here); ``formant_tabs``: the formant stage's fp32 tables (default: built here)."""
    stretch, (L, M), (Fn, Fd) = fmt.stretch_pct, fmt.ratio, fmt.formant
    if stretch != 100:
        x = stretch_ref(x, stretch, windows)[0]
    if L != M:
        x = ratio_ref(x, L, M, ratio_taps)
    if Fn != Fd:
        x = formant_ref(x, Fn, Fd, formant_tabs)
    if fmt.marks:
        x = mark_ref(x, fmt.mark_key, fmt.mark_id, fmt.mark_strength, formant_tabs)
    if fmt.volume_pct != 100:
        x = level_ref(x, fmt.volume_pct, level_win)[0]
    return encode_ref(resample_ref(x, fmt.sample_rate, taps), fmt)


class StreamRef:
    """The streaming form of the rule for one slot, on the host: ``push(x, final)`` returns the samples the
    call emits (``Engine.pcm_convert`` for one row: ``lvx_pcm_join`` when the format joins its dumps, then
    ``lvx_pcm_stretch`` when the plan has a stretch, then ``lvx_pcm_ratio`` when it has a ratio, then
    ``lvx_pcm_formant`` when it has an envelope correction, then ``lvx_pcm_mark`` when it names a watermark key, then ``lvx_pcm_level`` when it has a volume, then
    ``lvx_pcm_convert`` and, a FLAC format, ``lvx_pcm_flac`` behind it as s16le: the slots of the frames the call
    emits; a pausing format, ``lvx_pcm_pause`` last: the slots of the blocks the call emits). ``ctx_frames``: the context frames in front of x (a joined format only). Keeps the whole segment; for
    tests and stand-in engines. ``last_d``: the d_j of the hops the last push emitted."""

    def __init__(self, fmt: AudioFormat, taps=None, windows=None, ratio_taps=None, join_windows=None, level_win=None,
                 formant_tabs=None):
        self.fmt, self.taps, self.ratio_taps = fmt, taps, ratio_taps
        self.Fn, self.Fd = fmt.formant
        if self.Fn != self.Fd or fmt.marks:
            tabs = formant_tables() if formant_tabs is None else formant_tabs
            self.formant_tabs = tuple(np.asarray(t, dtype=np.float32) for t in tabs)
        if fmt.marks:
            self.mark_words = mark_table(fmt.mark_key, fmt.mark_id)
        if fmt.volume_pct != 100:
            self.level_win = level_window() if level_win is None else np.asarray(level_win, dtype=np.float32)
        if fmt.join:
            wr, wf = join_windows if join_windows is not None else join_window()
            self.join_windows = (np.asarray(wr, dtype=np.float32), np.asarray(wf, dtype=np.float32))
        self.stretch_pct, (self.L, self.M) = fmt.stretch_pct, fmt.ratio
        if self.stretch_pct != 100:
            wr, wf = windows if windows is not None else stretch_window()
            self.windows = (np.asarray(wr, dtype=np.float32), np.asarray(wf, dtype=np.float32))
        self.last_d = np.zeros(0, dtype=np.int32)
        self.reset()

    def reset(self):
        self.seg: List[np.ndarray] = []
        self.t0 = 0
        self.raw: List[np.ndarray] = []  # the stretch's view: the segment's input, its count, hops and p_{j-1}
        self.raw_t0, self.hops, self.p_prev = 0, 0, -STRETCH_H
        self.mid: List[np.ndarray] = []  # the ratio resampler's view: the stretched segment and its count
        self.mid_t0 = 0
        self.join_tail: Optional[np.ndarray] = None  # the join's view: the held-back frame (None: closed)
        self.fmn: List[np.ndarray] = []  # the formant stage's view: the resampled segment and its count
        self.fmn_t0 = 0
        self.mrk: List[np.ndarray] = []  # the mark stage's view: the segment in front of it and its count
        self.mrk_t0 = 0
        self.lvl: List[np.ndarray] = []  # the level stage's view: the resampled segment and its count
        self.lvl_t0 = 0
        self.fq: List[np.ndarray] = []  # the FLAC stage's view: the segment's s16 samples and their count
        self.fq_t0 = 0
        self.pq: List[np.ndarray] = []  # the pause stage's view: the segment's encoded samples and their count
        self.pq_t0 = 0

    def _ratio(self, x, final: bool) -> np.ndarray:
        m0 = ratio_emitted_upto(self.L, self.M, self.mid_t0, False)
        m1 = ratio_emitted_upto(self.L, self.M, self.mid_t0 + x.size, final)
        self.mid.append(x)
        self.mid_t0 += x.size
        return ratio_ref(np.concatenate(self.mid), self.L, self.M, self.ratio_taps, m0, m1)

    def _formant(self, x, final: bool) -> np.ndarray:
        n0 = formant_emitted_upto(self.fmn_t0, False)
        n1 = formant_emitted_upto(self.fmn_t0 + x.size, final)
        self.fmn.append(x)
        self.fmn_t0 += x.size
        return formant_ref(np.concatenate(self.fmn), self.Fn, self.Fd, self.formant_tabs, n0, n1)

    def _mark(self, x, final: bool) -> np.ndarray:
        n0 = mark_emitted_upto(self.mrk_t0, False)
        n1 = mark_emitted_upto(self.mrk_t0 + x.size, final)
        self.mrk.append(x)
        self.mrk_t0 += x.size
        return mark_ref(np.concatenate(self.mrk), self.fmt.mark_key, self.fmt.mark_id, self.fmt.mark_strength,
                        self.formant_tabs, n0, n1, self.mark_words)

    def _level(self, x, final: bool) -> np.ndarray:
        pct = self.fmt.volume_pct
        n0 = level_emitted_upto(pct, self.lvl_t0, False)
        n1 = level_emitted_upto(pct, self.lvl_t0 + x.size, final)
        self.lvl.append(x)
        self.lvl_t0 += x.size
        return level_ref(np.concatenate(self.lvl), pct, self.level_win, n0, n1)[0]

    def _stretch(self, x, final: bool) -> np.ndarray:
        pct = self.stretch_pct
        self.raw.append(x)
        self.raw_t0 += x.size
        m0 = self.hops * STRETCH_H
        m1 = stretch_emitted_upto(pct, self.raw_t0, final)
        j1 = -(-m1 // STRETCH_H)
        whole = np.concatenate(self.raw)
        y, self.last_d, self.p_prev = _stretch_run(whole, pct, self.windows[0], self.windows[1], self.hops, j1,
                                                   self.p_prev)
        self.hops = j1
        return y[:max(0, m1 - m0)]

    def push(self, x, final: bool, ctx_frames: int = 0) -> np.ndarray:
        x = np.asarray(x, dtype=np.float32).reshape(-1)
        if self.fmt.join:
            x, self.join_tail = _join_step(self.join_tail, x, int(ctx_frames), bool(final), *self.join_windows)
        elif ctx_frames:
            raise ValueError("ctx_frames without a joined format")
        if self.stretch_pct != 100:
            x = self._stretch(x, final)
        if self.L != self.M:
            x = self._ratio(x, final)
        if self.Fn != self.Fd:
            x = self._formant(x, final)
        if self.fmt.marks:
            x = self._mark(x, final)
        if self.fmt.volume_pct != 100:
            x = self._level(x, final)
        rate = self.fmt.sample_rate
        m0 = emitted_upto(rate, self.t0, False)
        m1 = emitted_upto(rate, self.t0 + x.size, final)
        self.seg.append(x)
        self.t0 += x.size
        whole = np.concatenate(self.seg) if self.seg else np.zeros(0, np.float32)
        y = resample_ref(whole, rate, self.taps, m0, m1)
        if self.fmt.encoding == "flac":  # the sixth stage: the s16le samples cut into frames, whole slots out
            q = quantize_s16(y)
            j0 = flac_frames_upto(rate, self.fq_t0, False)
            j1 = flac_frames_upto(rate, self.fq_t0 + q.size, final)
            self.fq.append(q)
            self.fq_t0 += q.size
            # (a frame that is whole now reads the same samples in the sentence as it stands as in the finished one)
            y = flac_slots_ref(np.concatenate(self.fq), rate, j0, j1) if j1 > j0 else np.zeros(0, np.uint8)
        else:
            y = encode_ref(y, self.fmt)
        if self.fmt.pauses:  # the last stage: the encoded samples cut into blocks of 10 ms, whole slots out
            j0 = pause_blocks_upto(rate, self.pq_t0, False)
            j1 = pause_blocks_upto(rate, self.pq_t0 + y.size, final)
            self.pq.append(y)
            self.pq_t0 += y.size
            # (a block that leaves now holds the same samples in the sentence as it stands as in the finished one,
            # and the sentence's last block leaves only with the final call)
            y = pause_slots_ref(np.concatenate(self.pq), self.fmt, j0, j1) if j1 > j0 else np.zeros(0, np.uint8)
        if final:
            self.reset()
        return y


__all__ = ["AudioFormat", "wav_header", "design", "emitted", "emitted_upto", "resample_ref", "quantize_s16",
           "convert_ref", "StreamRef", "RATES", "ENCODINGS", "FORMAT_ENCODINGS", "G711_LAWS", "g711_encode", "g711_decode", "silence_byte",
           "FRAME_MS", "frame_ms_of", "frame_bytes", "frame_chunks", "CONTAINERS",
           "flac_block", "flac_slot_bytes", "flac_frames_upto", "flac_emitted", "flac_frames_of", "flac_subframe",
           "flac_frame", "flac_finish_ref", "flac_stream_header", "flac_encode_ref", "flac_slots_ref", "flac_crc8",
           "flac_crc16", "FlacMux", "FLAC_MAX_K", "BASE_RATE", "HISTORY",
           "pause_block", "pause_slot_bytes", "pause_blocks_upto", "pause_emitted", "pause_loud", "pause_slots_ref",
           "pause_ref", "PauseMux", "PAUSE_THRESH", "PAUSE_LEAD", "PAUSE_TRAIL", "PAUSE_MS_MAX", "MAX_PAUSE_MS_MIN",
           "stretch_window", "stretch_ref", "stretch_emitted", "stretch_emitted_upto", "SPEED_MIN", "SPEED_MAX",
           "STRETCH_H", "STRETCH_D", "STRETCH_C", "STRETCH_HISTORY", "pitch_plan", "ratio_design", "ratio_emitted",
           "ratio_emitted_upto", "ratio_ref", "PITCH_MIN", "PITCH_MAX", "RATIO_MAX", "RATIO_HISTORY",
           "join_window", "join_emitted", "join_ref", "JOIN_HOLD", "JOIN_CONTEXT",
           "level_window", "level_emitted", "level_emitted_upto", "level_ref", "VOLUME_MIN", "VOLUME_MAX",
           "LEVEL_A", "LEVEL_R", "LEVEL_CEIL", "LEVEL_HISTORY",
           "formant_plan", "formant_tables", "formant_emitted", "formant_emitted_upto", "formant_ref", "formant_gains",
           "FORMANT_MIN", "FORMANT_MAX", "FORMANT_N", "FORMANT_H", "FORMANT_K", "FORMANT_EPS", "FORMANT_MAX_TERM",
           "FORMANT_HISTORY",
           "mark_table", "mark_emitted", "mark_emitted_upto", "mark_gains", "mark_ref", "mark_detect", "MARK_K0", "MARK_BW",
           "MARK_U", "MARK_PAIRS", "MARK_Q", "MARK_P", "MARK_STRENGTH_MIN", "MARK_STRENGTH_MAX", "MARK_DETECT_MIN"]

"""Constructed speech for the watermark tests: a synthetic vowel with resonances at 700, 1,200 and 2,600 Hz under a
four-per-second syllable envelope, and the delivery chains a marked sentence leaves the service by, each brought back to
float samples at its own rate as a receiver would hold them."""
import numpy as np

from llmvox_amd import audio as A

KEY = 0x5EEDC0DEF00DFACE   # the key of the tests
OTHER_KEY = 0x0123456789ABCDEF
ID = 0xA5                  # the payload of the tests
SECONDS = 3
CROP = 5037                # "an arbitrary leading crop": samples at 24 kHz, no multiple of anything in the rule

# every delivery chain: (name, rate, encoding)
CHAINS = [("f32le-24k", 24000, "f32le"), ("s16le-8k", 8000, "s16le"), ("s16le-16k", 16000, "s16le"),
          ("s16le-48k", 48000, "s16le"), ("ulaw-8k", 8000, "ulaw"), ("alaw-8k", 8000, "alaw"), ("flac-24k", 24000, "flac")]


def vowel(seconds=SECONDS, seed=3, rate=24000):
    """float32 [seconds * rate]: 31 harmonics of a wandering 120 Hz under three resonances, a syllable envelope of four
    a second that never quite closes, a noise floor of 3e-4; peak 0.25."""
    T = int(seconds * rate)
    rng = np.random.default_rng(seed)
    t = np.arange(T) / rate
    f0 = 120.0 * (1 + 0.05 * np.sin(2 * np.pi * 2.3 * t) + 0.1 * np.sin(2 * np.pi * 0.4 * t))
    ph = 2 * np.pi * np.cumsum(f0) / rate
    x = np.zeros(T)
    for h in range(1, 32):
        f = h * 120.0
        amp = sum(g / (1 + ((f - fc) / bw) ** 2) for fc, bw, g in ((700, 130, 1.0), (1200, 150, 0.6), (2600, 200, 0.35)))
        x += amp * np.sin(h * ph + 0.7 * h)
    env = 0.05 + 0.95 * np.sin(np.pi * np.minimum(1.0, (t * 4.0) % 1.0 / 0.8)) ** 2
    return (0.25 * env * x / np.abs(x).max() + rng.normal(0, 3e-4, T)).astype(np.float32)


def delivered(y, rate, encoding, crop=0):
    """The sentence y (float32 at 24 kHz) as a receiver of (rate, encoding) holds it: float32 samples at ``rate``, the
    first ``crop`` samples (counted at 24 kHz) cut off. FLAC goes through the stream's bytes and tests/flac_decode.py."""
    from flac_decode import decode
    if encoding == "flac":
        blob = A.flac_encode_ref(A.quantize_s16(A.resample_ref(y, rate)), rate)
        v = decode(blob)[0].astype(np.float32) / np.float32(32768.0)
    else:
        q = A.convert_ref(y, A.AudioFormat(rate, encoding))
        if encoding in A.G711_LAWS:
            q = A.g711_decode(q, encoding)
        v = q if encoding == "f32le" else q.astype(np.float32) / np.float32(32768.0)
    return np.asarray(v, dtype=np.float32)[crop * rate // 24000:]

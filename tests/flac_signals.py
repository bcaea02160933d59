"""The int16 test signals of the FLAC tests (CPU, host program's twin, GPU): chosen so that the numpy rule alone shows
every subframe kind. ``signal(kind, T, rate)`` is deterministic."""
import numpy as np

KINDS = ("silence", "constant", "sines", "noise", "alternating", "ramp", "hiss", "walk", "smooth", "voiced")
RATES = (8000, 16000, 24000, 48000)


def lengths(rate):
    """The sentence lengths around every frame cut of a rate."""
    bs = rate // 25
    return [1, 15, 16, 17, bs - 1, bs, bs + 15, bs + 16, bs + 17, 2 * bs + 15, 2 * bs + 16, 3 * bs + 7]


def voiced(T, rate, seed=7):
    """Eleven harmonics of a wobbling 110 Hz under a syllable envelope, plus a little noise: a stand-in for speech."""
    rng = np.random.default_rng(seed)
    t = np.arange(T) / rate
    f0 = 110.0 * (1.0 + 0.04 * np.sin(2 * np.pi * 3.1 * t))
    phase = 2 * np.pi * np.cumsum(f0) / rate
    x = sum(np.sin(h * phase + 0.7 * h) / h for h in range(1, 12))
    env = 0.15 + 0.85 * np.sin(np.pi * np.minimum(1.0, (t * 4.0) % 1.0 / 0.8)) ** 2  # four syllables a second
    y = 9000.0 * env * x / 2.0 + rng.normal(0.0, 12.0, T)
    return np.clip(np.rint(y), -32768, 32767).astype(np.int16)


def signal(kind, T, rate=24000, seed=1):
    rng = np.random.default_rng([seed, T, KINDS.index(kind)])
    t = np.arange(T, dtype=np.int64)
    if kind == "silence":
        x = np.zeros(T)
    elif kind == "constant":
        x = np.full(T, -7)
    elif kind == "sines":  # two sines plus +-20 of integer noise
        x = np.rint(9000 * np.sin(0.031 * t) + 4000 * np.sin(0.27 * t + 1.0)) + rng.integers(-20, 21, T)
    elif kind == "noise":  # full scale, uniform: VERBATIM
        x = rng.integers(-32768, 32768, T)
    elif kind == "alternating":
        x = np.where(t % 2 == 0, 32767, -32768)
    elif kind == "ramp":
        x = (5 * t) % 30000 - 15000
    elif kind == "hiss":  # white: order 0
        x = rng.integers(-300, 301, T)
    elif kind == "walk":  # its first difference is white: order 1
        x = 2000 + np.cumsum(rng.integers(-40, 41, T)) % 9000
    elif kind == "smooth":  # third difference +-1 in long runs, so the fourth is 0 but at the turns: order 4
        m = 12
        half = np.concatenate([np.ones(m), -np.ones(2 * m), np.ones(m)])
        d3 = np.tile(np.concatenate([half, -half]), T // (8 * m) + 1)[:T]
        x = np.cumsum(np.cumsum(np.cumsum(d3)))
    else:
        return voiced(T, rate)
    x = np.asarray(x, dtype=np.int64)
    assert x.size == T and (T == 0 or (x.min() >= -32768 and x.max() <= 32767)), kind
    return x.astype(np.int16)

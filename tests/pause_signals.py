"""Constructed sentences for the pause tests: encoded samples of a format whose 10 ms blocks are silent or active by a
given pattern, every block's content different from every other's, and the request the PauseMux tests speak."""
import numpy as np

from llmvox_amd import audio as A

C_MS = 100  # the max_pause_ms of the tests: C = 10 blocks
C = C_MS // 10


def encode(q, fmt):
    """int16 samples as the format's encoded samples (f32le: q / 32768, exact)."""
    q = np.asarray(q, dtype=np.int16)
    if fmt.encoding == "f32le":
        return (q.astype(np.float32) / np.float32(32768.0)).astype(np.float32)
    return A.g711_encode(q, fmt.encoding) if fmt.encoding in A.G711_LAWS else q


def sentence(fmt, pattern, rng, tail=None):
    """A sentence of len(pattern) blocks, block j active iff pattern[j]; ``tail``: the samples of its last block
    (default: a whole one). A silent block is noise of at most 60 on the 16-bit scale, an active one has a few samples
    of 2,000 .. 30,000 in it, the first of them anywhere in the block."""
    bl = A.pause_block(fmt.sample_rate)
    q = rng.integers(-60, 61, len(pattern) * bl).astype(np.int16)
    for j, on in enumerate(pattern):
        if on:
            at = j * bl + rng.integers(0, bl, 3)
            q[at] = rng.integers(2000, 30000, 3) * rng.choice([-1, 1], 3)
    if tail is not None:
        keep = (len(pattern) - 1) * bl + tail
        if pattern[-1]:  # (the cut block stays active)
            q[keep - 1] = 12345
        q = q[:keep]
    y = encode(q, fmt)
    marks = [bool(A.pause_loud(y[j * bl:(j + 1) * bl], fmt).any()) for j in range(len(pattern))]
    assert marks == [bool(p) for p in pattern]
    return y


def request(fmt, seed=0):
    """The sentences of one request: leading silence of 0, 1, 2, 3 and 40 blocks; trailing silence of 0, 4, 5, 6 and
    60; interior runs of C - 1, C and C + 1; an all-silent sentence first, in the middle and last; a one-sample
    sentence (a loud one and a silent one); a last block of 7 samples."""
    rng = np.random.default_rng(seed)
    s = lambda pattern, tail=None: sentence(fmt, pattern, rng, tail)
    return [s([0] * 4),
            s([1] + [0] * (C - 1) + [1]),
            s([0, 1] + [0] * C + [1] + [0] * 4),
            s([0, 0, 1] + [0] * (C + 1) + [1, 1] + [0] * 5),
            s([0] * 9),
            s([0] * 3 + [1] + [0] * 6, tail=7),
            s([1], tail=1),
            s([0] * 40 + [1, 0, 1] + [0] * 60),
            s([0], tail=1),
            s([1, 1], tail=3),
            s([0] * 3)]


def slots_of(sentences, fmt):
    """The request's slots as the device writes them, one blob a sentence."""
    return [A.pause_slots_ref(y, fmt, 0, A.pause_blocks_upto(fmt.sample_rate, y.size, True)).tobytes() for y in sentences]


def pushed(blob, fmt, cut):
    """The slots of ``blob`` through one PauseMux in pushes of ``cut`` slots (None: one push)."""
    mux, size = A.PauseMux(fmt), A.pause_slot_bytes(fmt)
    step = len(blob) if cut is None else cut * size
    return b"".join(mux.push(blob[at:at + step]) for at in range(0, len(blob), max(step, 1)))

"""The pause rule on the host (llmvox_amd/audio.py, "PCM pause" of include/llmvox.h), CPU only: the slots of
``pause_slots_ref`` (layout, counts, the mark at the threshold's edges in all four encodings), ``PauseMux`` against the
one-shot ``pause_ref`` on constructed sentences however the pushes and the device calls are cut, the rule's three
consequences asserted on the bytes themselves, and the new ``AudioFormat`` fields."""
import struct

import numpy as np
import pytest

import pause_signals as PS
from llmvox_amd import audio as A

RATES = (8000, 16000, 24000, 48000)
FMTS = [A.AudioFormat(r, e, pause_ms=0) for r in RATES for e in A.ENCODINGS]
MUX_FMTS = [A.AudioFormat(8000, "s16le", pause_ms=150, max_pause_ms=PS.C_MS), A.AudioFormat(24000, "f32le", pause_ms=0),
            A.AudioFormat(8000, "ulaw", max_pause_ms=PS.C_MS), A.AudioFormat(16000, "alaw", pause_ms=30, max_pause_ms=PS.C_MS),
            A.AudioFormat(48000, "s16le", "wav", pause_ms=2000)]
_id = lambda f: f"{f.sample_rate}-{f.encoding}-{f.pause_ms}-{f.max_pause_ms}"


def _lengths(bl):
    return [1, bl - 1, bl, bl + 1, 2 * bl, 3 * bl + 7]


def _records(blob, fmt):
    size = A.pause_slot_bytes(fmt)
    assert len(blob) % size == 0
    return [struct.unpack_from("<HBBI", blob, at) for at in range(0, len(blob), size)]


@pytest.mark.parametrize("fmt", FMTS, ids=_id)
def test_slots_layout_and_counts(fmt):
    bl, bps, size = fmt.sample_rate // 100, fmt.sample_bytes, A.pause_slot_bytes(fmt)
    assert size == 8 + bl * bps and size % 8 == 0
    rng = np.random.default_rng(bl + bps)
    for T in _lengths(bl):
        pattern = list(rng.integers(0, 2, -(-T // bl)))
        y = PS.sentence(fmt, pattern, rng, tail=T - (len(pattern) - 1) * bl)
        assert y.size == T
        K = A.pause_blocks_upto(fmt.sample_rate, T, True)
        assert K == -(-T // bl) and A.pause_blocks_upto(fmt.sample_rate, T, False) == (T - 1) // bl
        blob = A.pause_slots_ref(y, fmt, 0, K).tobytes()
        raw = y.view(np.uint8).tobytes()
        for j, (n, active, last, zero) in enumerate(_records(blob, fmt)):
            assert n == min(bl, T - j * bl) and active == pattern[j] and last == (j == K - 1) and zero == 0
            payload = blob[j * size + 8:(j + 1) * size]
            assert payload[:n * bps] == raw[j * bl * bps:(j * bl + n) * bps]
            assert payload[n * bps:] == bytes([A.silence_byte(fmt)]) * ((bl - n) * bps)
        # any range of blocks is that part of the whole; the calls' counts add up to it, the last block with the final
        assert A.pause_slots_ref(y, fmt, 1, K).tobytes() == blob[size:] if K > 1 else True
        for step in (1, 17, bl + 16):
            got, t0 = 0, 0
            while t0 < T:
                n_in = min(step, T - t0)
                got += A.pause_emitted(fmt.sample_rate, t0, n_in, t0 + n_in == T)
                assert t0 + n_in == T or got < -(-(t0 + n_in) // bl)  # (never the block that may still be the last)
                t0 += n_in
            assert got == K
    assert A.pause_blocks_upto(fmt.sample_rate, 0, True) == 0 and A.pause_emitted(fmt.sample_rate, 0, 0, True) == 0


def _mark(samples, fmt):
    """The active byte of the one-block sentence ``samples`` (already encoded)."""
    return _records(A.pause_slots_ref(samples, fmt, 0, 1).tobytes(), fmt)[0][1]


def test_threshold_edges():
    s16, f32 = A.AudioFormat(8000, "s16le", pause_ms=0), A.AudioFormat(8000, "f32le", pause_ms=0)
    for q, want in ((103, 0), (-103, 0), (104, 1), (-104, 1), (-32768, 1), (32767, 1), (0, 0)):
        assert _mark(np.array([0, q, 0], np.int16), s16) == want, q
    t = np.float32(103 / 32768)
    assert float(t) == 0.003143310546875
    up = np.nextafter(t, np.float32(1))
    for v, want in ((t, 0), (-t, 0), (up, 1), (-up, 1), (np.float32("nan"), 1), (np.float32("inf"), 1), (np.float32(0), 0)):
        assert _mark(np.array([0, v], np.float32), f32) == want, v
    for law, below, silence in (("ulaw", 96, 0xFF), ("alaw", 88, 0xD5)):
        fmt = A.AudioFormat(8000, law, pause_ms=0)
        lin = A.g711_decode(np.arange(256, dtype=np.uint8), law).astype(np.int32)
        mags = np.unique(np.abs(lin))
        assert mags[mags <= 103].max() == below and mags[mags > 103].min() == 104  # the magnitudes nearest the threshold
        for c in range(256):
            assert _mark(np.array([c], np.uint8), fmt) == int(abs(int(lin[c])) > 103), (law, c)
        assert {int(abs(lin[c])) for c in range(256) if abs(lin[c]) in (below, 104)} == {below, 104}
        assert A.silence_byte(fmt) == silence and _mark(np.array([silence] * 5, np.uint8), fmt) == 0
    assert int(A.g711_decode(np.array([0xD5], np.uint8), "alaw")[0]) == 8
    # the mark is a property of the encoded samples: 103.4 / 32768 is loud as f32le and silent as s16le
    v = np.array([103.4 / 32768], np.float32)
    assert _mark(v, f32) == 1 and _mark(A.quantize_s16(v), s16) == 0


def _cut_slots(y, fmt, step):
    """The sentence's slots as calls of ``step`` samples emit them (the last one final), concatenated."""
    parts, t0 = [], 0
    while True:
        n_in = min(step, y.size - t0)
        final = t0 + n_in == y.size
        j0 = A.pause_blocks_upto(fmt.sample_rate, t0, False)
        j1 = A.pause_blocks_upto(fmt.sample_rate, t0 + n_in, final)
        # (a call sees the sentence only as far as it has come)
        parts.append(A.pause_slots_ref(y[:t0 + n_in] if not final else y, fmt, j0, j1).tobytes())
        t0 += n_in
        if final:
            return b"".join(parts)


@pytest.mark.parametrize("fmt", MUX_FMTS, ids=_id)
def test_mux_is_the_one_shot_rule_however_it_is_cut(fmt):
    sentences = PS.request(fmt, seed=fmt.sample_rate)
    want = A.pause_ref(sentences, fmt)
    whole = b"".join(PS.slots_of(sentences, fmt))
    for cut in (1, 3, None):
        assert PS.pushed(whole, fmt, cut) == want, cut
    bl = fmt.sample_rate // 100
    for step in (1, 17, bl + 16):  # and however the device calls were cut: the slots are the same slots
        assert b"".join(_cut_slots(y, fmt, step) for y in sentences) == whole, step
    with pytest.raises(ValueError):
        A.PauseMux(fmt).push(whole[:-1])
    with pytest.raises(ValueError):
        A.PauseMux(fmt).push(b"\0" * A.pause_slot_bytes(fmt))  # n = 0: no record of the stage


def _active_blocks(y, fmt):
    bl = fmt.sample_rate // 100
    K = A.pause_blocks_upto(fmt.sample_rate, y.size, True)
    return [j for j in range(K) if A.pause_loud(y[j * bl:(j + 1) * bl], fmt).any()]


@pytest.mark.parametrize("fmt", [f for f in MUX_FMTS if f.pause_ms is not None], ids=_id)
def test_consequences_on_the_bytes(fmt):
    sentences = PS.request(fmt, seed=3)
    out = PS.pushed(b"".join(PS.slots_of(sentences, fmt)), fmt, 3)
    bl, bps, P = fmt.sample_rate // 100, fmt.sample_bytes, fmt.pause_ms // 10
    at, found = 0, []  # every active block, bit for bit and in order: [(sentence, block, where it starts, where it ends)]
    for k, y in enumerate(sentences):
        raw = y.view(np.uint8).tobytes()
        for j in _active_blocks(y, fmt):
            block = raw[j * bl * bps:(j + 1) * bl * bps]
            at = out.index(block, at)
            found.append((k, j, at, at + len(block)))
            at += len(block)
    assert len(found) == sum(len(_active_blocks(y, fmt)) for y in sentences) > 10
    gaps = 0
    for (k0, j0, _, end), (k1, j1, start, _) in zip(found, found[1:]):
        if k0 == k1:
            continue
        between = (start - end) // bps  # samples between one sentence's last active block and the next one's first
        a, b = sentences[k0], sentences[k1]
        trail = max(0, a.size - (j0 + 1) * bl)  # samples of silence behind the last active block; in front of the first: j1 bl
        assert between <= (A.PAUSE_TRAIL + P + A.PAUSE_LEAD) * bl
        assert between == (min(trail, A.PAUSE_TRAIL * bl) + P * bl + min(j1, A.PAUSE_LEAD) * bl)
        if trail >= A.PAUSE_TRAIL * bl and j1 >= A.PAUSE_LEAD:
            assert between == (A.PAUSE_TRAIL + P + A.PAUSE_LEAD) * bl
            gaps += 1
        assert out[end + min(trail, A.PAUSE_TRAIL * bl) * bps:start - min(j1, A.PAUSE_LEAD) * bl * bps] == \
            bytes([A.silence_byte(fmt)]) * (P * bl * bps)  # the inserted gap is the encoding's silence
    assert gaps >= 1
    # nothing before the first delivering sentence's kept onset, nothing behind the last one's kept decay
    first, last = found[0], found[-1]
    assert first[2] == min(first[1], A.PAUSE_LEAD) * bl * bps
    assert len(out) - last[3] == min(max(0, sentences[last[0]].size - (last[1] + 1) * bl), A.PAUSE_TRAIL * bl) * bps


def test_cap_keeps_the_head_and_the_tail_of_a_long_run():
    fmt = A.AudioFormat(8000, "s16le", max_pause_ms=PS.C_MS)
    rng = np.random.default_rng(9)
    for r, kept in ((PS.C - 1, PS.C - 1), (PS.C, PS.C), (PS.C + 1, PS.C), (PS.C + 30, PS.C)):
        y = PS.sentence(fmt, [0] * 50 + [1] + [0] * r + [1] + [0] * 70, rng)
        out = PS.pushed(PS.slots_of([y], fmt)[0], fmt, 1)
        assert out == A.pause_ref([y], fmt) and len(out) == (50 + 1 + kept + 1 + 70) * 160  # no edge is trimmed
        run = y[51 * 80:(51 + r) * 80].tobytes()
        if r > PS.C:
            assert out[51 * 160:(51 + kept) * 160] == run[:(PS.C - 2) * 160] + run[-2 * 160:]
        trimmed = A.AudioFormat(8000, "s16le", pause_ms=0, max_pause_ms=PS.C_MS)
        assert len(A.pause_ref([y], trimmed)) == (2 + 1 + kept + 1 + 5) * 160
    assert A.pause_ref([PS.sentence(fmt, [0] * 200, rng)], fmt) != b""  # an all-silent sentence stays where no edge is trimmed


def test_audio_format_fields():
    d = A.AudioFormat()
    assert d.pause_ms is None and d.max_pause_ms is None and not d.pauses and d.is_default and not d.converts
    assert A.AudioFormat(16000, "s16le", "wav", 125, 100, True, 250, 110) == \
        A.AudioFormat(16000, "s16le", "wav", 125, 100, True, 250, 110, None, None)  # the older fields keep their places
    f = A.AudioFormat(pause_ms=150)
    assert f.pauses and f.converts and f.pause_ms == 150 and f.max_pause_ms is None
    assert A.AudioFormat(max_pause_ms=400).pauses and A.AudioFormat(pause_ms=0).pauses
    for ok in (0, 10, 150, 2000):
        A.AudioFormat(pause_ms=ok)
    for ok in (100, 110, 2000):
        A.AudioFormat(max_pause_ms=ok)
    for bad in (-10, 5, 15, 2010, True, False, 20.0, "20", 1.5):
        with pytest.raises(ValueError, match="pause_ms"):
            A.AudioFormat(pause_ms=bad)
    for bad in (0, 90, 105, 2010, True, 100.0, "100"):
        with pytest.raises(ValueError, match="max_pause_ms"):
            A.AudioFormat(max_pause_ms=bad)
    for kw in (dict(pause_ms=100), dict(max_pause_ms=100)):
        with pytest.raises(ValueError, match="flac"):
            A.AudioFormat(8000, "flac", **kw)
    A.AudioFormat(8000, "flac")
    with pytest.raises(ValueError):
        A.PauseMux(A.AudioFormat(8000, "s16le"))

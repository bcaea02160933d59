"""The watermark on the host (CPU): the sign table (``audio.mark_table`` against ``lvx_pcm_mark_table`` on a sweep of keys
and ids, a digest of it pinned), the streaming counts, the independence of the rule from how a sentence is cut
(``StreamRef`` against the one-shot ``mark_ref``), silence, the bins outside the band, the argument errors, and what the
mark is for: ``audio.mark_detect`` finds it, and reads its payload, in a 3 s synthetic vowel through every delivery chain
of the service, with and without a leading crop, and finds none in the same audio unmarked or under another key.

Measured on this test's vowel (the figures the assertions below keep a margin to):
  marked, strength 2: S = 10.46 .. 11.95 over the 14 chains (the lowest: 8 kHz A-law, cropped), the id exact in all;
  unmarked: S <= 4.20; marked under another key: S <= 4.21 (each the maximum of a search over 1,024 candidates);
  rms(marked - unmarked) / rms(signal): -37.75 dB, -31.73 dB, -25.71 dB at strengths 1, 2, 3."""
import ctypes
import hashlib

import numpy as np
import pytest

import mark_signals as MS
from llmvox_amd import audio as A

H = A.FORMANT_H
KEY, ID = MS.KEY, MS.ID
TS = (1, 255, 256, 257, 1025, 7 * 256 + 5, 3000)
CUTS = (1, 255, 256, 257, 1791)
# the margins of the detection test: a marked chain scores at least 8 + 2, a null at most 8 - 2 (measured: above)
S_MARKED_MIN, S_NULL_MAX = 10.0, 6.0


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _signal(T, seed=5):
    rng = np.random.default_rng(seed)
    t = np.arange(T, dtype=np.float64)
    tone = 0.1 * sum(np.sin(2 * np.pi * h * t / 113 + h) / h for h in range(1, 16))
    return (tone * np.linspace(0.3, 1.0, T) + rng.standard_normal(T) * 0.01).astype(np.float32)


# ---- the table --------------------------------------------------------------------------------------------------

def test_the_table_is_its_definition_and_the_librarys():
    from llmvox_amd import _lib
    lib = _lib.load()
    got = np.zeros(64, dtype=np.uint16)
    p = got.ctypes.data_as(ctypes.c_void_p)
    rng = np.random.default_rng(1)
    keys = [0, 1, KEY, MS.OTHER_KEY, (1 << 63), (1 << 64) - 1] + [int(k) for k in rng.integers(0, 1 << 63, 10)]
    for key in keys:
        base = A.mark_table(key, 0)
        for mark_id in (0, 1, 2, 0x5A, ID, 255):
            assert lib.lvx_pcm_mark_table(key, mark_id, p, 64) == _lib.LVX_OK
            want = A.mark_table(key, mark_id)
            assert want.dtype == np.uint16 and want.shape == (64,) and np.array_equal(got, want), (key, mark_id)
            assert not (want >> 12).any()
            # the payload is an XOR on the key's own signs: bit (12 p + m) mod 8 of the id
            flip = (want ^ base).astype(np.int64)
            for pp in range(64):
                for m in range(12):
                    assert (flip[pp] >> m) & 1 == (mark_id >> ((12 * pp + m) % 8)) & 1
    assert lib.lvx_pcm_mark_table(KEY, 256, p, 64) == _lib.LVX_E_ARG and lib.lvx_pcm_mark_table(KEY, 0, p, 63) == _lib.LVX_E_ARG
    # SplitMix64 from state 0: its first output is 0xE220A8397B1DCDAF, top bit set; no payload: bit 0 of word 0 is set
    assert int(A.mark_table(0, 0)[0]) & 1 == 1
    # pinned: the table of the tests' key and id, and of key 0
    assert hashlib.sha256(A.mark_table(KEY, ID).astype("<u2").tobytes()).hexdigest() == \
        "2e7bb89e15878b9ea35d9977e2bbbb3a4ecc2dc8c7b267ba7cd17db1a0999118"
    assert hashlib.sha256(A.mark_table(0, 0).astype("<u2").tobytes()).hexdigest() == \
        "e541ab26030540d1fce917d6454107464b955b673a4d6c6de37f5d9319aa839a"
    # about half the signs are set, and two keys share about half of them
    a = np.unpackbits(A.mark_table(KEY, 0).view(np.uint8))
    b = np.unpackbits(A.mark_table(MS.OTHER_KEY, 0).view(np.uint8))
    assert 320 < a.sum() < 448 and 320 < (a ^ b).sum() < 448


def test_the_gains_are_the_tables():
    words = A.mark_table(KEY, ID)
    for strength, a in ((1, 1 / 64), (2, 1 / 32), (3, 1 / 16)):
        G = A.mark_gains(words, strength, 0, 4 * 64 + 8)
        assert G.shape == (264, 513) and G.dtype == np.float32
        assert (G[:, :24] == 1).all() and (G[:, 144:] == 1).all()
        assert set(np.unique(G[:, 24:144]).tolist()) == {1 - a, 1 + a}
        for j in (0, 3, 4, 255, 256, 263):  # word (j div 4) mod 64
            w = int(words[(j // 4) % 64])
            for m in range(12):
                even, odd = G[j, 24 + 10 * m:29 + 10 * m], G[j, 29 + 10 * m:34 + 10 * m]
                assert (even == (1 - a if (w >> m) & 1 else 1 + a)).all() and (odd == (1 + a if (w >> m) & 1 else 1 - a)).all()
        assert np.array_equal(G[:4], G[256:260])  # the period: 64 blocks of 4 frames


# ---- the counts -------------------------------------------------------------------------------------------------

def test_counts_add_up_over_any_cutting():
    from llmvox_amd import _lib
    lib = _lib.load()
    rng = np.random.default_rng(2)
    for T in (1, 255, 256, 257, 767, 768, 769, 1024, 3000, 50000):
        for _ in range(10):
            t0, total = 0, 0
            while t0 < T:
                n = int(min(T - t0, rng.integers(1, 1500)))
                final = t0 + n == T
                m = A.mark_emitted(t0, n, final)
                assert m == lib.lvx_pcm_mark_emitted(t0, n, int(final)) == A.formant_emitted(t0, n, final)
                total += m
                t0 += n
                if not final:  # held back: everything below 3 H inputs, then 768 .. 1023
                    assert total == 0 if t0 < 3 * H else 768 <= t0 - total <= 1023
            assert total == T
    assert A.mark_emitted(0, 0, True) == 0 and lib.lvx_pcm_mark_emitted(-1, 0, 0) < 0 and lib.lvx_pcm_mark_emitted(0, -1, 0) < 0
    with pytest.raises(ValueError):
        A.mark_emitted(-1, 5, False)


# ---- independence of the cuts -----------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def one_shot():
    x = _signal(max(TS))
    out = {T: A.mark_ref(x[:T], KEY, ID, 2) for T in TS}
    for y in out.values():
        y.setflags(write=False)
    return x, out


@pytest.mark.parametrize("T", TS)
def test_streamref_in_any_cutting_gives_the_one_shot_bits(one_shot, T):
    x, want = one_shot
    fmt = A.AudioFormat(mark_key=KEY, mark_id=ID)  # the mark stage alone
    assert fmt.marks and fmt.converts and fmt.ratio == (1, 1) and fmt.formant == (1, 1)
    for cut in CUTS:
        ref = A.StreamRef(fmt)
        parts = [ref.push(x[a:min(a + cut, T)], a + cut >= T) for a in range(0, T, cut)]
        got = np.concatenate(parts)
        assert got.shape == want[T].shape == (T,) and np.array_equal(_bits(got), _bits(want[T])), (T, cut)
    ref = A.StreamRef(fmt)  # a flush-only final call behind the samples
    got = np.concatenate([ref.push(x[:T], False), ref.push(x[:0], True)])
    assert np.array_equal(_bits(got), _bits(want[T]))
    assert np.array_equal(_bits(ref.push(x[:T], True)), _bits(want[T]))  # and the next sentence starts the pattern again


def test_the_whole_chain_in_cuts_is_convert_ref():
    fmt = A.AudioFormat(16000, "s16le", "raw", 100, 125, False, 200, 100, mark_key=KEY, mark_id=ID, mark_strength=3)
    x = _signal(6400, seed=8)
    want = A.convert_ref(x, fmt)
    ref = A.StreamRef(fmt)
    got = np.concatenate([ref.push(x[a:a + 1600], a + 1600 >= x.size) for a in range(0, x.size, 1600)])
    assert want.dtype == np.int16 and np.array_equal(got, want)
    assert not np.array_equal(want, A.convert_ref(x, A.AudioFormat(16000, "s16le", "raw", 100, 125, False, 200, 100)))
    # the mark sits behind the formant stage and in front of the level stage
    mid = A.formant_ref(A.ratio_ref(A.stretch_ref(x, 80)[0], 4, 5), 5, 4)
    mid = A.level_ref(A.mark_ref(mid, KEY, ID, 3), 200)[0]
    assert np.array_equal(want, A.encode_ref(A.resample_ref(mid, 16000), fmt))
    # and the limiter's ceiling holds behind it
    loud = A.convert_ref(x * np.float32(8.0), A.AudioFormat(volume_pct=400, mark_key=KEY, mark_strength=3))
    assert float(np.abs(loud).max()) <= float(A.LEVEL_CEIL) * (1 + 2.0 ** -22)  # (the level stage's own bound: two roundings)


# ---- silence, and the bins outside the band ---------------------------------------------------------------------

def test_silence_in_silence_out():
    for strength in (1, 2, 3):
        y = A.mark_ref(np.zeros(2000, dtype=np.float32), KEY, ID, strength)
        assert y.shape == (2000,) and not _bits(y).any()
    x = _signal(3000)
    x[700:1900] = 0.0  # silence inside a sentence: the frames wholly inside it stay exactly silent
    y = A.mark_ref(x, KEY, ID, 3)
    assert np.isfinite(y).all() and not y[700 + 768:1900 - 768].any()


def test_bins_outside_the_band_reconstruct():
    """Two tones of a whole number of periods in a frame, at bins 10 and 300, below and above the band: away from the
    sentence's edges no marked bin holds anything and the output is the input to fp32 rounding, the bound of the
    formant stage's flat-envelope case. The same tones moved into the band do change."""
    n = np.arange(8192)
    outside = (0.2 * np.sin(2 * np.pi * 10 * n / 1024) + 0.1 * np.sin(2 * np.pi * 300 * n / 1024 + 1)).astype(np.float32)
    y = A.mark_ref(outside, KEY, ID, 3)
    assert float(np.abs(y - outside)[1024:-1024].max()) < 1e-5
    inside = (0.2 * np.sin(2 * np.pi * 30 * n / 1024) + 0.1 * np.sin(2 * np.pi * 100 * n / 1024 + 1)).astype(np.float32)
    y = A.mark_ref(inside, KEY, ID, 3)
    assert float(np.abs(y - inside)[1024:-1024].max()) > 1e-3
    # the difference of any marked signal from its input lies inside the band
    x = _signal(8192)
    d = (A.mark_ref(x, KEY, ID, 3) - x).astype(np.float64)[1024:-1024]
    D = np.abs(np.fft.rfft(d * np.hanning(d.size))) ** 2
    k = np.arange(D.size) * 1024.0 / d.size  # in bins of the rule's frame
    assert D[(k > 22) & (k < 146)].sum() > 0.999 * D.sum()


def test_argument_errors():
    x = _signal(600)
    for key, mark_id, strength in ((-1, 0, 2), (1 << 64, 0, 2), (True, 0, 2), (1.5, 0, 2), ("1", 0, 2), (KEY, -1, 2), (KEY, 256, 2),
                                   (KEY, True, 2), (KEY, 1.0, 2), (KEY, 0, 0), (KEY, 0, 4), (KEY, 0, True), (KEY, 0, 2.0)):
        with pytest.raises(ValueError) as ei:
            A.mark_ref(x, key, mark_id, strength)
        assert str(KEY) not in str(ei.value)
        if key is not True:  # (the format's own checks; a bool key is refused by both)
            with pytest.raises(ValueError) as ei:
                A.AudioFormat(mark_key=key, mark_id=mark_id, mark_strength=strength)
            assert str(KEY) not in str(ei.value)
    with pytest.raises(ValueError):
        A.AudioFormat(mark_key=True)
    with pytest.raises(ValueError):
        A.AudioFormat(mark_id=300)  # (checked with or without a key)
    with pytest.raises(ValueError):
        A.mark_ref(x, KEY, ID, 2, None, 100, 600)  # n0 inside a hop
    assert A.mark_ref(x, KEY, ID, 2, None, 256, 256).shape == (0,)
    assert A.mark_ref(np.stack([x, x]), KEY, ID).shape == (2, 600)
    with pytest.raises(ValueError):
        A.mark_detect(x, 44100, KEY)
    with pytest.raises(ValueError):
        A.mark_detect(x, 24000, -1)
    with pytest.raises(ValueError):
        A.mark_detect(x, 24000, KEY, window_s=0.1)
    S, found, _, _ = A.mark_detect(np.zeros(100, np.float32), 24000, KEY)  # too short to hold three blocks: nothing
    assert S == 0.0 and not found
    # the key is in no header and in no repr
    fmt = A.AudioFormat(8000, "ulaw", "wav", mark_key=KEY)
    assert A.wav_header(fmt) == A.wav_header(A.AudioFormat(8000, "ulaw", "wav")) and str(KEY) not in repr(fmt)


# ---- it does what it is for -------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def vowel():
    x = MS.vowel()
    y = A.mark_ref(x, KEY, ID, 2)
    x.setflags(write=False)
    y.setflags(write=False)
    return x, y


@pytest.mark.parametrize("crop", (0, MS.CROP), ids=["whole", "cropped"])
@pytest.mark.parametrize("name,rate,encoding", MS.CHAINS, ids=[c[0] for c in MS.CHAINS])
def test_the_mark_survives_every_delivery_chain(vowel, name, rate, encoding, crop):
    x, y = vowel
    got = MS.delivered(y, rate, encoding, crop)
    S, found, mark_id, offset = A.mark_detect(got, rate, KEY)
    print(f"{name} crop {crop}: marked S = {S:.2f}, id {mark_id:#x}, offset {offset}")
    assert found and mark_id == ID and S >= S_MARKED_MIN, (name, crop, S, mark_id)
    # where the blocks start, modulo a block: the score changes slowly with the alignment (a frame is 1,024 samples
    # under a Hann window), so the best candidate lies within two steps of the true one, not always on the nearest
    miss = (offset - (-crop)) % 1024
    assert min(miss, 1024 - miss) <= 2 * 64, (name, crop, offset)
    S0, found0, _, _ = A.mark_detect(MS.delivered(x, rate, encoding, crop), rate, KEY)
    S1, found1, _, _ = A.mark_detect(got, rate, MS.OTHER_KEY)
    print(f"{name} crop {crop}: unmarked S = {S0:.2f}, marked under another key S = {S1:.2f}")
    assert not found0 and not found1 and max(S0, S1) <= S_NULL_MAX, (name, crop, S0, S1)


def test_strengths_and_windows(vowel):
    x, _ = vowel
    xs = x.astype(np.float64)
    rel = {}
    for strength in (1, 2, 3):
        y = A.mark_ref(x, KEY, ID, strength)
        rel[strength] = 10 * np.log10(((y - xs) ** 2).sum() / (xs ** 2).sum())
        print(f"strength {strength}: rms(marked - unmarked) / rms(signal) = {rel[strength]:.2f} dB")
        assert float(np.abs(y).max()) <= 1.07 * float(np.abs(x).max())  # (g+ <= 1 + 1/16)
    # a step of the strength doubles a: 6.02 dB each; the difference stays below a times the signal
    assert abs(rel[2] - rel[1] - 6.02) < 0.05 and abs(rel[3] - rel[2] - 6.02) < 0.05
    assert rel[1] < 20 * np.log10(1 / 64) and rel[2] < 20 * np.log10(1 / 32) and rel[3] < 20 * np.log10(1 / 16)
    S3, found, mark_id, _ = A.mark_detect(A.mark_ref(x, KEY, 0x3C, 3), 24000, KEY)
    print(f"strength 3: S = {S3:.2f}")
    assert found and mark_id == 0x3C and S3 >= S_MARKED_MIN
    # two sentences of a request, each restarting the pattern, behind half a second of unmarked audio: windows find it
    y = A.mark_ref(x, KEY, ID, 2)
    body = np.concatenate([x[:12000], y, y[:48000]])
    S, found, mark_id, offset = A.mark_detect(body, 24000, KEY, window_s=3.0)
    print(f"windows of 3 s over two sentences: S = {S:.2f}, offset {offset}")
    assert found and mark_id == ID and S >= 8.0

"""The dump join's rule on the host (include/llmvox.h, "PCM dump join"; llmvox_amd/audio.py: join_ref): the
windows, the counts, the two identities (a sentence delivers 320 samples per frame; a one-dump sentence is
the codec's row), the library's host functions against the numpy ones, and, with the oracle codec, that the
joined seams lie nearer the one-shot rendering of the sentence than the plain ones (a test of the rule on
synthetic weights, not a claim about a trained checkpoint's sound)."""
import ctypes
import itertools

import numpy as np
import pytest

from llmvox_amd import audio as A

H = A.JOIN_HOLD


def test_format_field():
    assert A.AudioFormat().join is False and A.AudioFormat().is_default and not A.AudioFormat().converts
    f = A.AudioFormat(join=True)
    assert f.converts and not f.is_default and f == A.AudioFormat(24000, "f32le", "raw", 100, 100, True)
    for bad in (1, 0, "true", None):
        with pytest.raises(ValueError):
            A.AudioFormat(join=bad)


def test_windows_against_their_formula():
    wr, wf = A.join_window()
    assert wr.dtype == wf.dtype == np.float32 and wr.size == wf.size == H == 320
    n = np.arange(320, dtype=np.float64)
    r = 0.5 - 0.5 * np.cos(np.pi * (n + 0.5) / 320)
    assert np.array_equal(wr, r.astype(np.float32)) and np.array_equal(wf, (1.0 - r).astype(np.float32))
    assert np.all(np.diff(wr) > 0) and 0 < wr[0] < 1e-4 and np.allclose(wr + wf, 1.0, atol=1e-7)
    assert np.array_equal(wr, wf[::-1])  # (the half-sample offset makes the pair symmetric)


def _cuts(T, k):
    """Every cut of T frames into exactly k dumps of >= 1 frame."""
    for bars in itertools.combinations(range(1, T), k - 1):
        yield [b - a for a, b in zip((0,) + bars, bars + (T,))]


def _rows(x, cut, ctx):
    """The calls of a sentence whose frames are rendered the same in every call: rows of x, context in front."""
    rows, at = [], 0
    for L, c in zip(cut, ctx):
        rows.append(x[(at - c) * H:(at + L) * H])
        at += L
    return rows


def test_emitted_against_join_ref_lengths_and_the_total():
    rng = np.random.default_rng(1)
    n_cuts = 0
    for T in range(1, 41):
        x = rng.standard_normal(T * H).astype(np.float32)
        for k in range(1, min(4, T) + 1):
            cuts = list(_cuts(T, k))
            if len(cuts) > 12:  # (every cut of the short sentences, a sample of the long ones')
                cuts = [cuts[i] for i in rng.choice(len(cuts), 12, replace=False)]
            for cut in cuts:
                done = np.cumsum([0] + cut[:-1])
                ctx = [int(min(A.JOIN_CONTEXT, d, rng.integers(0, 18))) for d in done]
                out = A.join_ref(_rows(x, cut, ctx), ctx)
                for j, (L, c, y) in enumerate(zip(cut, ctx, out)):
                    assert y.size == A.join_emitted(j > 0, c, (c + L) * H, j == k - 1)
                assert sum(y.size for y in out) == 320 * T
                n_cuts += 1
    assert n_cuts > 1000


def test_every_cut_of_T_frames_into_up_to_4_dumps_totals_320_T():
    """The counts of every cut (the samples themselves, and that the counts are join_ref's: the test above)."""
    for T in range(1, 41):
        for k in range(1, min(4, T) + 1):
            for cut in _cuts(T, k):
                total, done = 0, 0
                for j, L in enumerate(cut):
                    c = min(A.JOIN_CONTEXT, done)
                    total += A.join_emitted(j > 0, c, (c + L) * H, j == k - 1)
                    done += L
                assert total == 320 * T, cut
    x = np.arange(12 * H, dtype=np.float32)
    for k in range(1, 5):  # (with a flush in place of a final dump: the same total)
        for cut in _cuts(12, k):
            ctx = [0] + [1] * (k - 1)
            out = A.join_ref(_rows(x, cut, ctx) + [x[:0]], ctx + [0])
            assert sum(y.size for y in out) == 320 * 12


def test_counts_table():
    for Lb in (1, 2, 7):
        n = Lb * H
        assert A.join_emitted(False, 0, n, False) == n - 320
        assert A.join_emitted(True, 0, n, False) == n
        assert A.join_emitted(True, 3, n + 3 * H, False) == n
        assert A.join_emitted(True, 0, n, True) == n + 320
        assert A.join_emitted(True, 16, n + 16 * H, True) == n + 320
        assert A.join_emitted(False, 0, n, True) == n
    assert A.join_emitted(True, 0, 0, True) == 320 and A.join_emitted(False, 0, 0, True) == 0


BAD_CALLS = [(False, 0, 321, False), (True, 0, -320, False), (True, 17, 18 * 320, False), (True, -1, 640, False),
             (True, 2, 640, False), (True, 3, 640, True), (False, 1, 640, False), (False, 0, 0, False),
             (True, 0, 0, False), (True, 1, 0, True)]


@pytest.mark.parametrize("call", BAD_CALLS)
def test_calls_the_rule_does_not_admit(call):
    with pytest.raises(ValueError):
        A.join_emitted(*call)


def test_one_dump_sentence_is_its_row_bit_for_bit():
    x = np.random.default_rng(2).standard_normal(5 * H).astype(np.float32)
    x[:4] = [0.0, -0.0, 1e30, 1e-40]
    (y,) = A.join_ref([x], [0])
    assert np.array_equal(y.view(np.int32), x.view(np.int32))
    ref = A.StreamRef(A.AudioFormat(join=True))
    assert np.array_equal(ref.push(x, True).view(np.int32), x.view(np.int32))


def test_a_seam_without_context_is_concatenation():
    rng = np.random.default_rng(3)
    rows = [rng.standard_normal(L * H).astype(np.float32) for L in (1, 4, 2, 3)]
    out = A.join_ref(rows, [0, 0, 0, 0])
    assert [y.size for y in out] == [0, 4 * H, 2 * H, 4 * H]
    assert np.array_equal(np.concatenate(out).view(np.int32), np.concatenate(rows).view(np.int32))
    # a flush as the last call
    out = A.join_ref(rows + [np.zeros(0, np.float32)], [0] * 5)
    assert out[-1].size == 320 and np.array_equal(np.concatenate(out), np.concatenate(rows))


def test_the_crossfade_is_two_rounded_products_and_a_rounded_sum():
    rng = np.random.default_rng(4)
    a, b = rng.standard_normal(3 * H).astype(np.float32), rng.standard_normal(4 * H).astype(np.float32)
    wr, wf = A.join_window()
    out = A.join_ref([a, b], [0, 2])
    assert np.array_equal(out[0], a[:2 * H])
    want = np.empty(H, np.float32)
    for n in range(H):
        want[n] = np.float32(np.float32(a[2 * H + n] * wf[n]) + np.float32(b[H + n] * wr[n]))
    assert np.array_equal(out[1][:H], want) and np.array_equal(out[1][H:], b[2 * H:])
    # StreamRef is the same rule, call by call; join and then the other stages
    ref = A.StreamRef(A.AudioFormat(join=True))
    assert np.array_equal(ref.push(a, False), out[0]) and np.array_equal(ref.push(b, True, ctx_frames=2), out[1])
    fmt = A.AudioFormat(16000, "s16le", speed_pct=130, join=True)
    ref, rest = A.StreamRef(fmt), A.StreamRef(A.AudioFormat(16000, "s16le", speed_pct=130))
    got = np.concatenate([ref.push(a, False), ref.push(b, True, ctx_frames=2)])
    assert np.array_equal(got, np.concatenate([rest.push(out[0], False), rest.push(out[1], True)]))
    with pytest.raises(ValueError):
        A.StreamRef(A.AudioFormat(16000)).push(b, True, ctx_frames=2)


def test_host_functions_of_the_library():
    from llmvox_amd import _lib
    lib = _lib.load()
    wr, wf = np.zeros(320, np.float32), np.zeros(320, np.float32)
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
    assert lib.lvx_pcm_join_window(p(wr), p(wf), 320) == 0
    assert np.array_equal(wr, A.join_window()[0]) and np.array_equal(wf, A.join_window()[1])
    assert lib.lvx_pcm_join_window(p(wr), p(wf), 319) == _lib.LVX_E_ARG
    assert lib.lvx_pcm_join_window(None, p(wf), 320) == _lib.LVX_E_ARG
    for open_ in (False, True):
        for c in range(-1, 19):
            for frames in range(0, 20):
                for final in (False, True):
                    try:
                        want = A.join_emitted(open_, c, frames * 320, final)
                    except ValueError:
                        want = _lib.LVX_E_ARG
                    assert lib.lvx_pcm_join_emitted(int(open_), c, frames * 320, int(final)) == want
    for call in BAD_CALLS:
        assert lib.lvx_pcm_join_emitted(int(call[0]), call[1], call[2], int(call[3])) == _lib.LVX_E_ARG


def test_joined_seams_are_nearer_the_one_shot_rendering_with_the_oracle_codec():
    """Synthetic weights, 137 random codes cut 10 / 30 / 90 / 7, windows of +-640 samples round each seam: the
    RMS deviation from the one-shot decode of the sentence is strictly smaller joined than plain at each of
    the three seams. A test of the rule, not a quality claim: the synthetic codec emits noise-like audio."""
    import torch
    from llmvox_amd import weights as LW
    from oracle import reference_cpu as R
    _, cw, _ = LW.synthetic_all(1234)
    Wc = R.to_torch(cw)
    codes = np.random.default_rng(0).integers(0, 4096, 137)
    cut = [10, 30, 90, 7]

    def dec(toks):
        with torch.no_grad():
            return R.decode_codes(Wc, torch.tensor([list(toks)])).numpy()[0].astype(np.float32)

    whole = dec(codes)
    rows, plain, ctx, at = [], [], [], 0
    for L in cut:
        c = min(A.JOIN_CONTEXT, at)
        rows.append(dec(codes[at - c:at + L]))
        plain.append(dec(codes[at:at + L]))
        ctx.append(c)
        at += L
    joined = np.concatenate(A.join_ref(rows, ctx))
    plain = np.concatenate(plain)
    assert joined.size == plain.size == whole.size == 137 * 320
    for seam in np.cumsum(cut[:-1]) * 320:
        w = slice(seam - 640, seam + 640)
        rms_j = float(np.sqrt(np.mean((joined[w].astype(np.float64) - whole[w]) ** 2)))
        rms_p = float(np.sqrt(np.mean((plain[w].astype(np.float64) - whole[w]) ** 2)))
        print(f"seam {seam}: plain {rms_p:.4f} joined {rms_j:.4f}")
        assert rms_j < rms_p

"""The formant control on the host (CPU): the integer plan (``audio.formant_plan``, and ``lvx_pcm_formant_plan`` against it
on a sweep), the streaming counts (``audio.formant_emitted``, ``lvx_pcm_formant_emitted``), the independence of the rule
(``audio.formant_ref``, include/llmvox.h "PCM formant") of how a sentence is cut into calls, through ``StreamRef``, silence
and the range of the gains, and what the stage is for: on synthetic vowels whose formants a resampling has moved, the
harmonic amplitudes come back towards those of the vowel at the same f0 with its formants in place."""
import ctypes
from fractions import Fraction
from math import gcd

import numpy as np
import pytest

from llmvox_amd import audio as A

TS = (1, 255, 256, 257, 767, 768, 769, 1024, 3000)
CUTS = (1, 255, 256, 257, 1041)
H = A.FORMANT_H


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _signal(T, seed=5):
    """Four harmonics of a 150-sample period under a ramp, and noise: never silent, never periodic in the hop."""
    rng = np.random.default_rng(seed)
    t = np.arange(T, dtype=np.float64)
    tone = 0.1 * sum(np.sin(2 * np.pi * h * t / 150.0 + h) / h for h in range(1, 5))
    return (tone * np.linspace(0.5, 1.0, T) + 0.02 * rng.standard_normal(T)).astype(np.float32)


# ---- the plan -------------------------------------------------------------------------------------------------

def _triples():
    for speed in (50, 77, 100, 130, 200):
        for pitch in (50, 80, 90, 100, 110, 125, 150, 200):
            for formant in (50, 67, 80, 90, 100, 111, 125, 150, 199, 200):
                yield speed, pitch, formant


def test_plan_is_rho_in_lowest_terms_or_raises():
    valid = invalid = 0
    for speed, pitch, formant in _triples():
        try:
            _, L, M = A.pitch_plan(speed, pitch)
        except ValueError:
            with pytest.raises(ValueError):
                A.formant_plan(speed, pitch, formant)
            invalid += 1
            continue
        rho = Fraction(100 * M, formant * L)
        if Fraction(1, 2) <= rho <= 2:
            Fn, Fd = A.formant_plan(speed, pitch, formant)
            assert gcd(Fn, Fd) == 1 and Fraction(Fn, Fd) == rho and Fd <= 2 * Fn and Fn <= 2 * Fd
            assert 1 <= Fn <= A.FORMANT_MAX_TERM and 1 <= Fd <= A.FORMANT_MAX_TERM
            assert A.AudioFormat(speed_pct=speed, pitch_pct=pitch, formant_pct=formant).formant == (Fn, Fd)
            valid += 1
        else:
            with pytest.raises(ValueError, match="outside 1/2 .. 2"):
                A.formant_plan(speed, pitch, formant)
            with pytest.raises(ValueError):
                A.AudioFormat(speed_pct=speed, pitch_pct=pitch, formant_pct=formant)
            invalid += 1
    assert valid > 100 and invalid > 50
    assert A.formant_plan(100, 125, 100) == (5, 4) and A.formant_plan(100, 100, 90) == (10, 9)
    assert A.formant_plan(100, 80, 100) == (4, 5)
    with pytest.raises(ValueError):
        A.formant_plan(100, 200, 50)  # pitch 2.0 with formant 0.5: rho = 4
    for bad in (49, 201, True, 100.0, "100", None):
        with pytest.raises(ValueError):
            A.formant_plan(100, 100, bad)


def test_a_formant_at_the_realised_pitch_is_the_identity():
    n = 0
    for speed in (50, 80, 100, 120, 200):
        for pitch in range(50, 201):
            try:
                _, L, M = A.pitch_plan(speed, pitch)
            except ValueError:
                continue
            if (100 * M) % L == 0 and 50 <= 100 * M // L <= 200:
                fmt = A.AudioFormat(speed_pct=speed, pitch_pct=pitch, formant_pct=100 * M // L)
                assert fmt.formant == (1, 1)
                assert fmt.converts == A.AudioFormat(speed_pct=speed, pitch_pct=pitch).converts
                n += 1
    assert n >= 30


def test_the_c_plan_agrees_on_a_sweep():
    from llmvox_amd import _lib
    lib = _lib.load()
    for speed in (48, 50, 100, 133, 200, 201):
        for pitch in (49, 50, 75, 100, 125, 160, 200, 202):
            for formant in range(48, 203, 7):
                Fn, Fd = ctypes.c_int(-1), ctypes.c_int(-1)
                rc = lib.lvx_pcm_formant_plan(speed, pitch, formant, ctypes.byref(Fn), ctypes.byref(Fd))
                try:
                    want = A.formant_plan(speed, pitch, formant)
                except ValueError:
                    assert rc == _lib.LVX_E_ARG and (Fn.value, Fd.value) == (-1, -1), (speed, pitch, formant)
                else:
                    assert rc == _lib.LVX_OK and (Fn.value, Fd.value) == want, (speed, pitch, formant)
    assert lib.lvx_pcm_formant_plan(100, 125, 100, None, None) == _lib.LVX_OK  # (every output is optional)


def test_the_format_field():
    fmt = A.AudioFormat(24000, "f32le", "raw", 100, 100, False, 100)  # (positional construction stays valid)
    assert fmt.formant_pct is None and fmt.formant == (1, 1) and fmt.is_default and not fmt.converts
    assert fmt.formant_moved == 1.0
    f = A.AudioFormat(formant_pct=90)
    assert not f.is_default and f.converts and f.formant == (10, 9) and f.formant_moved == 0.9
    f = A.AudioFormat(formant_pct=100)  # named, but where the envelope already is: no stage
    assert not f.is_default and not f.converts and f.formant == (1, 1)
    f = A.AudioFormat(pitch_pct=125)
    assert f.formant == (1, 1) and f.formant_moved == 1.25
    f = A.AudioFormat(pitch_pct=125, formant_pct=100)
    assert f.formant == (5, 4) and f.formant_moved == 1.0 and f.converts
    for bad in (49, 201, True, 1.0, "100"):
        with pytest.raises(ValueError):
            A.AudioFormat(formant_pct=bad)


# ---- the counts -----------------------------------------------------------------------------------------------

def test_counts_add_up_over_any_cutting_and_emit_only_complete_frames():
    from llmvox_amd import _lib
    lib = _lib.load()
    rng = np.random.default_rng(3)
    for T in TS + (5000,):
        for cut in CUTS + (None,):
            t0 = total = 0
            while t0 < T:
                n = min(T - t0, cut if cut else int(rng.integers(1, 900)))
                final = t0 + n == T
                m = A.formant_emitted(t0, n, final)
                assert m == lib.lvx_pcm_formant_emitted(t0, n, int(final))
                total += m
                t0 += n
                if not final:
                    # the last emitted hop block's last frame, block + 3, covers [block H, (block + 4) H): all consumed
                    assert total % H == 0 and (total == 0 or (total // H - 1 + 4) * H <= t0)
                    assert 0 <= t0 - total <= 4 * H - 1
            assert total == T
    assert A.formant_emitted_upto(1023, False) == 0 and A.formant_emitted_upto(1024, False) == 256
    assert A.formant_emitted(0, 0, True) == 0 and lib.lvx_pcm_formant_emitted(-1, 0, 0) < 0
    assert lib.lvx_pcm_formant_emitted(0, -1, 0) < 0
    with pytest.raises(ValueError):
        A.formant_emitted(-1, 1, False)


# ---- independence of the cuts ---------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def one_shot():
    x = _signal(max(TS))
    out = {T: A.formant_ref(x[:T], 5, 4) for T in TS}
    for y in out.values():
        y.setflags(write=False)
    return x, out


@pytest.mark.parametrize("T", TS)
def test_streamref_in_any_cutting_gives_the_one_shot_bits(one_shot, T):
    x, want = one_shot
    fmt = A.AudioFormat(formant_pct=80)  # the formant stage alone: no stretch, no resampling in front of it
    assert fmt.ratio == (1, 1) and fmt.stretch_pct == 100 and fmt.formant == (5, 4)
    for cut in CUTS:
        ref = A.StreamRef(fmt)
        parts = [ref.push(x[a:min(a + cut, T)], a + cut >= T) for a in range(0, T, cut)]
        got = np.concatenate(parts)
        assert got.shape == want[T].shape == (T,) and np.array_equal(_bits(got), _bits(want[T])), (T, cut)


def test_the_whole_chain_in_cuts_is_convert_ref():
    fmt = A.AudioFormat(16000, "s16le", "raw", 100, 125, False, 200, 100)
    x = _signal(6400, seed=8)
    want = A.convert_ref(x, fmt)
    ref = A.StreamRef(fmt)
    got = np.concatenate([ref.push(x[a:a + 1600], a + 1600 >= x.size) for a in range(0, x.size, 1600)])
    assert want.dtype == np.int16 and np.array_equal(got, want)
    assert not np.array_equal(want, A.convert_ref(x, A.AudioFormat(16000, "s16le", "raw", 100, 125, False, 200)))


# ---- silence and headroom ---------------------------------------------------------------------------------------

def test_silence_in_silence_out():
    for Fn, Fd in ((3, 2), (1, 2), (199, 200)):
        y = A.formant_ref(np.zeros(2000, dtype=np.float32), Fn, Fd)
        assert y.shape == (2000,) and not np.isnan(y).any() and not y.any()
        g = A.formant_gains(np.zeros(2000, dtype=np.float32), Fn, Fd)
        assert np.array_equal(g, np.ones_like(g))  # (e / e: exactly 1)
    x = _signal(3000)
    x[700:1900] = 0.0  # silence inside a sentence: whole frames of zeros between others
    y = A.formant_ref(x, 2, 3)
    assert np.isfinite(y).all()


def test_the_gain_stays_within_24_db():
    rng = np.random.default_rng(11)
    t = np.arange(4000)
    tone = (0.5 * np.sin(2 * np.pi * t * 1000.0 / 24000)).astype(np.float32)  # one line: the steepest envelope there is
    click = np.zeros(4000, dtype=np.float32)
    click[[5, 2000, 3999]] = 1.0
    for x in (tone, click, (rng.standard_normal(4000) * 0.2).astype(np.float32), _signal(4000)):
        for Fn, Fd in ((2, 1), (1, 2), (3, 2), (2, 3), (199, 200)):
            g = A.formant_gains(x, Fn, Fd)
            assert g.shape == (-(-4000 // H) + 3, 513) and g.dtype == np.float32
            assert float(g.min()) >= 1.0 / 16.0 and float(g.max()) <= 16.0
    assert float(A.formant_gains(tone, 2, 1).max()) == 16.0 and float(A.formant_gains(tone, 2, 1).min()) == 1.0 / 16.0


def test_perfect_reconstruction_where_the_envelope_is_flat():
    """White noise has a flat envelope, so the gains stay near 1 and the overlap-add gives the input back but for the
    gains' ripple; an impulse's spectrum is exactly flat in every frame, and the output is the input to fp32 rounding."""
    x = np.zeros(3000, dtype=np.float32)
    x[1500] = 0.5
    y = A.formant_ref(x, 3, 2)
    assert float(np.abs(y - x).max()) < 1e-5


def test_argument_errors():
    x = _signal(600)
    for Fn, Fd in ((2, 4), (0, 1), (1, 3), (3, 1), (40001, 40000), (-1, 1)):
        with pytest.raises(ValueError):
            A.formant_ref(x, Fn, Fd)
    with pytest.raises(ValueError):
        A.formant_ref(x, 3, 2, None, 100, 600)  # n0 inside a hop
    assert A.formant_ref(x, 3, 2, None, 256, 256).shape == (0,)
    assert A.formant_ref(np.stack([x, x]), 3, 2).shape == (2, 600)


# ---- it does what it is for -------------------------------------------------------------------------------------

G, BW, FORMANTS = (1.0, 0.5, 0.25), (90.0, 110.0, 170.0), (700.0, 1200.0, 2600.0)
F0S = (90, 110, 150, 180, 240, 300)
RATIOS = (Fraction(3, 2), Fraction(5, 4), Fraction(11, 10), Fraction(9, 10), Fraction(4, 5), Fraction(2, 3), Fraction(2),
          Fraction(1, 2))


def vowel(f0, formants, n=24000):
    """One second at 24 kHz: the harmonics k f0 below 11 kHz, amplitude sum_i g_i / sqrt(1 + ((f - F_i) / (b_i / 2))^2),
    phase 0.3 k, the peak normalised to 0.3 (float64)."""
    t = np.arange(n) / 24000.0
    k = np.arange(1, int(11000 / f0) + 2)
    k = k[k * f0 < 11000]
    f = k * f0
    amp = sum(g / np.sqrt(1 + ((f - F) / (b / 2)) ** 2) for g, F, b in zip(G, formants, BW))
    x = (amp[:, None] * np.cos(2 * np.pi * f[:, None] * t[None, :] + 0.3 * k[:, None])).sum(0)
    return x * (0.3 / np.abs(x).max())


def harmonics(x, f0):
    """The amplitudes of the harmonics below 4 kHz from a Hann window of 8,192 samples from sample 4,000, each the
    maximum within f0 / 3, the set normalised to its own rms."""
    S = np.abs(np.fft.rfft(np.asarray(x, dtype=np.float64)[4000:4000 + 8192] * np.hanning(8192)))
    fr = np.arange(S.size) * 24000.0 / 8192
    a = np.array([S[np.abs(fr - k * f0) <= f0 / 3].max() for k in range(1, int(4000 / f0) + 2) if k * f0 < 4000])
    return a / np.sqrt((a ** 2).mean())


def distance(a, b):
    return float(np.sqrt(((20 * np.log10(a / b)) ** 2).mean()))


def test_the_stage_moves_the_envelope_back():
    """Each case: a vowel at f0 r with its formants at r F (what a resampling by r makes of the vowel at f0), through the
    stage at rho = r, against the vowel at f0 r with its formants at F. The rms difference of the harmonic amplitudes in
    dB: every case strictly below its untreated figure, the grid's mean at most half of the untreated mean.
    Measured with the fp32 rule: untreated mean 5.94 dB (3.19 .. 9.12), the stage's output mean 2.44 dB, worst 4.31 dB,
    never above 0.783 of its own case's untreated figure."""
    untreated, treated = [], []
    for f0 in F0S:
        for r in RATIOS:
            fp = f0 * float(r)
            target = harmonics(vowel(fp, FORMANTS), fp)
            xin = vowel(fp, [float(r) * F for F in FORMANTS])
            y = A.formant_ref(xin.astype(np.float32), r.numerator, r.denominator)
            u, s = distance(harmonics(xin, fp), target), distance(harmonics(y, fp), target)
            print(f"f0 {f0} r {r}: untreated {u:.2f} dB, stage {s:.2f} dB")
            assert s < u, (f0, r, s, u)
            untreated.append(u)
            treated.append(s)
    um, sm = float(np.mean(untreated)), float(np.mean(treated))
    worst = max(s / u for s, u in zip(treated, untreated))
    print(f"untreated mean {um:.2f} dB ({min(untreated):.2f} .. {max(untreated):.2f}), stage mean {sm:.2f} dB, "
          f"worst {max(treated):.2f} dB, worst share {worst:.3f}")
    assert sm <= 0.5 * um


def test_the_whole_chain_measured():
    """A measurement, not a condition: ``convert_ref`` at pitch 1.25 and 0.8 with formant 1.0 on the unshifted vowel,
    against that vowel synthesised at the realised f0. It only has to run and give finite figures; they are in the
    README."""
    for pitch in (125, 80):
        fmt = A.AudioFormat(pitch_pct=pitch, formant_pct=100)
        plain = A.AudioFormat(pitch_pct=pitch)
        L, M = fmt.ratio
        for f0 in (110, 180):
            x = vowel(f0, FORMANTS, 36000).astype(np.float32)
            fp = f0 * M / L
            target = harmonics(vowel(fp, FORMANTS), fp)
            with_stage = distance(harmonics(A.convert_ref(x, fmt), fp), target)
            without = distance(harmonics(A.convert_ref(x, plain), fp), target)
            print(f"pitch {pitch / 100} f0 {f0}: chain without the stage {without:.2f} dB, with it {with_stage:.2f} dB")
            assert np.isfinite(with_stage) and np.isfinite(without)

"""CPU reference of the extended sampled select (include/llmvox.h, lvx_stream_sampling_ex; numpy only), built
on tests/sampling_ref.py: repetition penalty, temperature, top-k, the integer nucleus, min-p, then the draw.

``rule`` restates steps 1-5 of the header. The penalty, the division by T, top-k and min-p are exact fp32 / order
statements, so numpy gives the device's bits. The nucleus is an integer comparison over q[i] = floor(w[i] 2^24),
but w is the DEVICE's fp32 exp; here it is a float64 exp of the same fp32 difference z - zmax, so single q may
differ by a unit or two (w 2^24 straddling an integer, a few ulp of exp): about 2^-22 of Aq and of Sq. A candidate
whose |Aq 2^24 - P Sq| <= 2^-16 P Sq is therefore called ``near``: it (and every token of the same z) may fall on
either side, and a row with a near candidate has an undetermined nucleus. 2^-16 is sampling_ref's EPS, ~60 x the
error above. The share of undetermined rows is capped per case (UNDETERMINED_CAP), so the allowance cannot hide a
wrong kernel.

Every crop is a threshold on z, so a device's kept set is {i : z[i] >= low} with ``low`` the lowest kept z that
lvx_sample_kept reports. ``Tally.add`` checks that set against the reference: every kept token that is not near
is in it, and nothing else but near candidates; on a determined row that is equality. The token is then checked
against the draw over the device's own kept set, with sampling_ref's acceptable-set rule.
"""
import numpy as np

from tests import sampling_ref as SR

VOCAB = SR.VOCAB
EPS = SR.EPS
UNDETERMINED_CAP = 0.08
ONE24 = 1 << 24


def p24(top_p):
    """P = round(top_p 2^24) of the fp32 top_p, clamped to [1, 2^24]; 2^24: the nucleus is off."""
    return int(min(max(np.floor(np.float64(np.float32(top_p)) * ONE24 + 0.5), 1), ONE24))


def lnminp(min_p):
    """(float)log((double)min_p) of the fp32 min_p; -inf for 0: the crop is off."""
    with np.errstate(divide="ignore"):
        return np.float32(np.log(np.float64(np.float32(min_p))))


def window_set(history, p, W, hist_from=0):
    """The distinct tokens decided at positions max(hist_from, p - W) .. p - 1 (``history`` indexed by position)."""
    lo = max(int(hist_from), p - int(W))
    return sorted({int(history[i]) for i in range(lo, p)})


def penalised(logits, R, window):
    """Step 1: l'[i] = l[i] > 0 ? l[i] / R : l[i] * R for i in the window set (fp32 IEEE)."""
    l = np.array(logits, dtype=np.float32)
    if len(window) and np.float32(R) != np.float32(1):
        idx = np.asarray(sorted(set(int(t) for t in window)))
        v, r = l[idx], np.float32(R)
        l[idx] = np.where(v > 0, v / r, v * r).astype(np.float32)
    return l


class Rule:
    """z fp32 [V]; kept: the reference's kept set; near: candidates of the nucleus within the allowance (either
    side is acceptable); determined: no near candidate; n_pen: distinct penalised tokens (0 with R = 1: the
    phase is skipped)."""

    def __init__(self, z, kept, near, n_pen):
        self.z, self.kept, self.near, self.n_pen = z, kept, near, n_pen
        self.determined = not near.any()


def rule(logits, T, k=0, top_p=1.0, min_p=0.0, R=1.0, window=()):
    lp = penalised(logits, R, window)
    n_pen = len(set(int(t) for t in window)) if np.float32(R) != np.float32(1) else 0
    z = SR.scaled(lp, T)
    zmax = z.max()
    kept = SR.kept_set(lp, T, k)
    d = (z - zmax).astype(np.float32)  # fl(z - zmax), what exp and min-p see
    near = np.zeros(z.size, dtype=bool)
    P = p24(top_p)
    if P < ONE24:
        w = np.where(kept, np.exp(d.astype(np.float64)), 0.0)
        q = np.floor(w * ONE24).astype(np.int64)
        Sq = int(q.sum())
        vals, inv = np.unique(z, return_inverse=True)  # ascending; -0 and +0 are one value
        mass = np.zeros(vals.size, dtype=np.int64)
        np.add.at(mass, inv, q)
        above = (Sq - np.cumsum(mass))[inv]  # Aq(z[i]): the mass strictly above
        lhs, rhs = above << 24, P * Sq       # < 2^61
        near = kept & (np.abs(lhs - rhs) <= (rhs >> 16))
        kept = kept & (lhs < rhs)
    ok = d >= lnminp(min_p)
    return Rule(z, kept & ok, near & ok, n_pen)


def draw_check(z, kept, seed, pos):
    """sampling_ref.check's draw over a given kept set of z -> (reference token, sorted acceptable tokens)."""
    z = z.astype(np.float64)
    w = np.where(kept, np.exp(z - z[kept].max()), 0.0)
    cdf = np.cumsum(w) / w.sum()
    u = SR.draw(seed, pos)
    lo = np.concatenate(([0.0], cdf[:-1]))
    over = np.nonzero(cdf > u)[0]
    ref = int(over[0]) if len(over) else int(np.nonzero(kept)[0][-1])
    ok = kept & (lo - EPS <= u) & (u <= cdf + EPS)
    return ref, sorted(set(np.nonzero(ok)[0].tolist()) | {ref})


def check(logits, T, k, seed, pos, top_p=1.0, min_p=0.0, R=1.0, window=()):
    """-> (reference token, sorted acceptable tokens, whether the kept set is determined), over the reference's
    kept set."""
    r = rule(logits, T, k, top_p, min_p, R, window)
    ref, acc = draw_check(r.z, r.kept, seed, pos)
    return ref, acc, r.determined


class Tally(SR.Tally):
    """sampling_ref.Tally for the extended rule; also checks lvx_sample_kept's record and counts the rows with
    an undetermined nucleus."""

    def __init__(self):
        super().__init__()
        self.undetermined = 0

    def add(self, token, record, logits, T, k, seed, pos, top_p=1.0, min_p=0.0, R=1.0, window=(), what=""):
        r = rule(logits, T, k, top_p, min_p, R, window)
        self.n += 1
        self.undetermined += not r.determined
        dev = r.kept
        if record is not None:
            n_kept, low_bits, n_pen = int(record[0]), int(record[1]), int(record[2])
            low = np.array([low_bits], dtype=np.int32).view(np.float32)[0]
            dev = r.z >= low
            assert n_kept == int(dev.sum()), f"{what}: {n_kept} kept, but {int(dev.sum())} tokens have z >= {low!r}"
            assert n_pen == r.n_pen and int(record[3]) == 0, f"{what}: penalised {n_pen}, reference {r.n_pen}"
            missing, extra = r.kept & ~r.near & ~dev, dev & ~(r.kept | r.near)
            assert not missing.any() and not extra.any(), \
                f"{what}: kept set differs from the reference's ({int(r.kept.sum())} kept, determined " \
                f"{r.determined}): missing {np.nonzero(missing)[0][:8]}, extra {np.nonzero(extra)[0][:8]}"
        ref, acc = draw_check(r.z, dev, seed, pos)
        self.ambiguous += len(acc) > 1
        assert int(token) in acc, f"{what}: token {int(token)} not acceptable (reference {ref}, set {acc[:8]})"
        if len(acc) == 1:
            assert int(token) == ref, what

    def assert_caps(self, cap, what=""):
        share = self.undetermined / max(self.n, 1)
        print(f"{what}: {self.undetermined} / {self.n} rows with an undetermined nucleus ({share:.3%}, "
              f"cap {UNDETERMINED_CAP:.0%})")
        assert share <= UNDETERMINED_CAP, (what, self.undetermined, self.n)
        self.assert_cap(cap, what)

"""CPU reference of the sampled select (include/llmvox.h, lvx_stream_sampling; numpy only).

``check`` says which tokens a device may return for (logits, T, k, seed, pos): the kept set from fp32
z = logits / T, the CDF of the kept weights in float64, and the draw u from Philox4x32-10. The
reference token is the first i with cdf[i] > u; the acceptable set is every kept token whose interval
[cdf[i-1], cdf[i]], widened by EPS on both sides, contains u. A device token must be in the acceptable
set, and equal the reference token where that set has one element.

EPS = 2^-16: the device forms its running sums as a 16-term sum per thread plus a tree over the 256
thread sums, at most ~24 fp32 roundings (1.5e-6 relative), and exp and u * S add a few ulp; 2^-16 is
about 10 x that, and 16 x below what a 4,096-term serial fp32 sum could reach. The share of draws with
more than one acceptable token is capped per case (AMBIGUOUS_CAP_*), so the tolerance cannot hide a
wrong kernel: the reference alone gives 3.7-4.5 % on full-vocabulary N(0, 3^2) rows and at most 0.4 %
with top_k <= 40.
"""
import numpy as np

VOCAB = 4096
EPS = 2.0 ** -16
AMBIGUOUS_CAP_FULL = 0.08   # full-vocabulary cases
AMBIGUOUS_CAP_TOPK = 0.02   # cases with top_k <= 40
_M32 = 0xFFFFFFFF


def philox4x32_10(counter, key):
    c0, c1, c2, c3 = (int(x) & _M32 for x in counter)
    k0, k1 = (int(x) & _M32 for x in key)
    for _ in range(10):
        p0, p1 = 0xD2511F53 * c0, 0xCD9E8D57 * c2
        c0, c1, c2, c3 = (p1 >> 32) ^ c1 ^ k0, p1 & _M32, (p0 >> 32) ^ c3 ^ k1, p0 & _M32
        k0, k1 = (k0 + 0x9E3779B9) & _M32, (k1 + 0xBB67AE85) & _M32
    return c0, c1, c2, c3


def draw(seed, pos):
    """u of the step at position ``pos`` of a slot seeded ``seed`` (24 bits)."""
    x0 = philox4x32_10((pos, 0, 0, 0), (seed & _M32, (seed >> 32) & _M32))[0]
    return (x0 >> 8) * 2.0 ** -24


def scaled(logits, T):
    return (np.asarray(logits, dtype=np.float32) / np.float32(T)).astype(np.float32)


def kept_set(logits, T, k):
    """Boolean mask of the indices kept by the top-k crop of z = logits / T (ties at the k-th value kept)."""
    z = scaled(logits, T)
    if k <= 0 or k >= z.size:
        return np.ones(z.size, dtype=bool)
    thr = np.partition(z, z.size - k)[z.size - k]  # the k-th largest
    return z >= thr


def check(logits, T, k, seed, pos):
    """-> (reference token, sorted acceptable tokens)."""
    z = scaled(logits, T).astype(np.float64)
    kept = kept_set(logits, T, k)
    w = np.where(kept, np.exp(z - z[kept].max()), 0.0)
    cdf = np.cumsum(w) / w.sum()
    u = draw(seed, pos)
    lo = np.concatenate(([0.0], cdf[:-1]))
    over = np.nonzero(cdf > u)[0]
    ref = int(over[0]) if len(over) else int(np.nonzero(kept)[0][-1])
    ok = kept & (lo - EPS <= u) & (u <= cdf + EPS)
    acc = sorted(set(np.nonzero(ok)[0].tolist()) | {ref})
    return ref, acc


class Tally:
    """Checks device tokens against the reference and counts the ambiguous draws of a case."""

    def __init__(self):
        self.n = 0
        self.ambiguous = 0

    def add(self, token, logits, T, k, seed, pos, what=""):
        ref, acc = check(logits, T, k, seed, pos)
        self.n += 1
        self.ambiguous += len(acc) > 1
        assert int(token) in acc, f"{what}: token {int(token)} not acceptable (reference {ref}, set {acc[:8]}) " \
                                  f"T={T} k={k} seed={seed:#x} pos={pos}"
        if len(acc) == 1:
            assert int(token) == ref, what

    def assert_cap(self, cap, what=""):
        share = self.ambiguous / max(self.n, 1)
        print(f"{what}: {self.ambiguous} / {self.n} draws with more than one acceptable token ({share:.3%}, cap {cap:.0%})")
        assert share <= cap, (what, self.ambiguous, self.n)

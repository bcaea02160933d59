"""The CPU side of the sampled select: the Philox known answers (the tests' helper, the package's
``philox4x32_10`` and, where a compiler is at hand, the library's own host form), the helper's kept
set against torch's crop as the reference writes it (src/model.py:398-401), and the segment seeds."""
import numpy as np
import pytest
import torch

from llmvox_amd.sampling import Sampling, philox4x32_10, segment_seed
from tests import sampling_ref as SR

KAT = [((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
       ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
       ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0),
        (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1))]


@pytest.mark.parametrize("fn", [SR.philox4x32_10, philox4x32_10], ids=["helper", "package"])
def test_philox_known_answers(fn):
    for counter, key, want in KAT:
        assert tuple(fn(counter, key)) == want


def test_draw_is_24_bits_of_the_first_word():
    x0 = SR.philox4x32_10((7, 0, 0, 0), (0x89abcdef, 0x01234567))[0]
    u = SR.draw(0x0123456789abcdef, 7)
    assert u == (x0 >> 8) / 2 ** 24 and 0.0 <= u < 1.0


@pytest.mark.parametrize("k", [1, 5, 40, 4095, 4096])
@pytest.mark.parametrize("T", [1.0, 0.7])
def test_kept_set_is_the_reference_crop(k, T):
    """Tie-heavy rows (values on a 0.25 grid): logits / T, then logits < topk(logits, k).values[-1] dropped."""
    rng = np.random.default_rng(100 * k + int(10 * T))
    for _ in range(4):
        row = (np.round(rng.normal(0, 3, SR.VOCAB) * 4) / 4).astype(np.float32)
        lg = torch.from_numpy(row).view(1, -1) / T
        v, _ = torch.topk(lg, min(k, lg.size(-1)))
        want = ~(lg < v[:, [-1]])[0].numpy()
        got = SR.kept_set(row, T, k)
        np.testing.assert_array_equal(got, want)
        assert got.sum() >= min(k, SR.VOCAB)
    assert SR.kept_set(row, T, 0).all()


def test_reference_token_and_acceptable_set():
    row = np.full(SR.VOCAB, -30.0, dtype=np.float32)
    row[[10, 20]] = 0.0  # two tokens of probability ~1/2
    seen = set()
    for pos in range(64):
        u = SR.draw(5, pos)
        ref, acc = SR.check(row, 1.0, 0, 5, pos)
        assert 0.0 < u < 1.0 and ref == (10 if u < 0.5 else 20)  # (u is a multiple of 2^-24, cdf[10] = 0.5 - 2e-10)
        assert acc == [ref] or abs(u - 0.5) <= 2 * SR.EPS
        seen.add(ref)
    assert seen == {10, 20}
    # k = 1 keeps the tie set of the maximum, k = 2 here too
    for k in (1, 2):
        assert SR.kept_set(row, 1.0, k).nonzero()[0].tolist() == [10, 20]
        assert SR.check(row, 1.0, k, 5, 0)[0] == (10 if SR.draw(5, 0) < 0.5 else 20)


def test_segment_seed():
    s = segment_seed(1234, 0, 0)
    assert s == segment_seed(1234, 0, 0) and 0 <= s < 2 ** 64
    x = philox4x32_10((3, 1, 0, 0), (1234, 0))
    assert segment_seed(1234, 1, 3) == x[0] | (x[1] << 32)
    seeds = {segment_seed(1234, i, g) for i in range(2) for g in range(8)}
    assert len(seeds) == 16
    assert segment_seed(1234, 0, 0) != segment_seed(1235, 0, 0)
    assert segment_seed(1 << 40, 0, 0) != segment_seed(0, 0, 0)  # the high word is part of the key


def test_sampling_validation():
    assert Sampling(0.8, 50, 7) == Sampling(0.8, 50, 7)
    assert Sampling(0).top_k == 0
    for bad in [dict(temperature=-1.0), dict(temperature=float("nan")), dict(temperature=float("inf")),
                dict(temperature=1.0, top_k=-1), dict(temperature=1.0, seed=-1), dict(temperature=1.0, seed=1 << 64),
                dict(temperature=1.0, top_k=1.5)]:
        with pytest.raises(ValueError):
            Sampling(**bad)

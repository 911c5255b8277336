"""gsss_target_moments on the device against an independent reference: seeded random unit vectors from numpy (not from the
sampler), summed in numpy longdouble.

Tolerance, derived: a sum of N = m R terms in ANY order obeys |err| <= N u sum|term| with u = 2^-53, and forming a product adds
at most one rounding per term, so every entry must satisfy |got - ref| <= 2 N u sum|term| (sum|term| from the reference; at the
largest case, N = 39 000, 8.7e-12 relative to sum|term|).  A dropped or doubled chain misses that by orders of magnitude.  The
count row is exact.  Inputs lie inside NaN-filled allocations: a read outside the block shows as NaN."""
import numpy as np
import pytest
import torch

from geosss_amd import diagnostics

pytestmark = pytest.mark.gpu
U = 2.0 ** -53

# (d, full triangle, m, M, R, chain-major): every d, m, R of the two forms and both layouts at least once; n = M m is never a
# multiple of 256
CASES = [
    (2, True, 1, 7, 1, False),
    (3, True, 1, 130, 3, True),
    (3, True, 8, 7, 130, False),
    (5, True, 24, 7, 3, False),
    (5, True, 24, 7, 130, True),
    (5, True, 256, 7, 130, False),
    (10, True, 64, 7, 3, False),
    (10, True, 100, 7, 130, True),
    (16, True, 256, 7, 3, False),
    (16, True, 300, 7, 130, False),
    (16, True, 8, 7, 1, True),
    (2, True, 300, 7, 130, True),
    (16, False, 300, 7, 3, True),
    (16, False, 64, 7, 130, False),
    (17, False, 24, 7, 130, False),
    (17, False, 8, 7, 3, True),
    (50, False, 100, 7, 3, False),
    (50, False, 1, 130, 1, True),
]


def _draws(d, m, M, R, seed):
    g = np.random.default_rng(seed)
    x = g.standard_normal((R, d, M * m))
    return x / np.linalg.norm(x, axis=1, keepdims=True)


def _reference(x, m, full):
    """(sums (M, rows - 1), sums of |term| likewise, chain sums (d, n), their |term| sums) in longdouble."""
    R, d, n = x.shape
    M = n // m
    xl = x.astype(np.longdouble)

    def per_target(v):                                   # (R, n) -> (M,)
        return v.reshape(R, M, m).sum((0, 2))

    pairs = [(i, j) for i in range(d) for j in range(i, d)] if full else [(i, i) for i in range(d)]
    cols = [xl[:, j] for j in range(d)] + [xl[:, i] * xl[:, j] for i, j in pairs]
    ref = np.stack([per_target(c) for c in cols], 1)
    mag = np.stack([per_target(np.abs(c)) for c in cols], 1)
    return ref, mag, xl.sum(0), np.abs(xl).sum(0)


def _embed(x, chain_major):
    """The block as a device tensor view inside a larger NaN-filled allocation."""
    R, d, n = x.shape
    xt = torch.from_numpy(x).cuda()
    if chain_major:                                       # rows 2 .. 2 + R - 1 of an (n, R + 5, d) buffer
        big = torch.full((n, R + 5, d), float("nan"), dtype=torch.float64, device="cuda")
        big[:, 2:2 + R] = xt.permute(2, 0, 1)
        return big[:, 2:2 + R]
    big = torch.full((R + 4, d, n), float("nan"), dtype=torch.float64, device="cuda")
    big[2:2 + R] = xt
    return big[2:2 + R]


def _rows(view, chain_major, lo, hi):
    return view[:, lo:hi] if chain_major else view[lo:hi]


def _check(acc, cs, ref, mag, cref, cmag, m, R, what):
    acc, cs = acc.cpu().numpy(), cs.cpu().numpy()
    assert np.all(acc[:, 0] == m * R), what                               # the count is exact
    err = np.abs(acc[:, 1:].astype(np.longdouble) - ref)
    bound = 2 * m * R * U * mag
    print(f"{what}: max |err| / bound = {float(np.max(err / bound)):.3g}")
    assert np.all(np.isfinite(acc)) and np.all(err <= bound), (what, float(np.max(err / bound)))
    cerr = np.abs(cs.astype(np.longdouble) - cref)
    assert np.all(np.isfinite(cs)) and np.all(cerr <= 2 * R * U * cmag), (what, "chain_sum")


@pytest.mark.parametrize("d, full, m, M, R, chain_major", CASES)
def test_moments_against_longdouble(d, full, m, M, R, chain_major):
    x = _draws(d, m, M, R, seed=1000 * d + m + R)
    ref, mag, cref, cmag = _reference(x, m, full)
    view = _embed(x, chain_major)
    n = M * m

    def run(lo, hi, acc=None, cs=None):
        cs = torch.zeros((d, n), dtype=torch.float64, device="cuda") if cs is None else cs
        acc = diagnostics.target_moments(_rows(view, chain_major, lo, hi), m, chain_major=chain_major, second_moment=full,
                                         acc=acc, chain_sum=cs)
        return acc, cs

    acc, cs = run(0, R)
    assert tuple(acc.shape) == (M, ref.shape[1] + 1)
    _check(acc, cs, ref, mag, cref, cmag, m, R, "one call")
    # the same call again: the same bits (no atomics, a fixed summation order)
    acc2, cs2 = run(0, R)
    assert torch.equal(acc, acc2) and torch.equal(cs, cs2)
    # two calls over the halves of the block add up to the whole
    h = R // 2
    acc3, cs3 = run(0, h)
    acc3, cs3 = run(h, R, acc3, cs3)
    _check(acc3, cs3, ref, mag, cref, cmag, m, R, "two halves")


def test_without_chain_sum_and_default_form():
    """chain_sum is optional, and second_moment=None keeps the triangle up to d = 16 and the diagonal beyond."""
    for d, rows in ((5, 1 + 5 + 15), (17, 1 + 34)):
        x = _draws(d, 24, 7, 3, seed=d)
        ref, mag, _, _ = _reference(x, 24, d <= 16)
        acc = diagnostics.target_moments(torch.from_numpy(x).cuda(), 24)
        assert tuple(acc.shape) == (7, rows)
        assert np.all(np.abs(acc.cpu().numpy()[:, 1:].astype(np.longdouble) - ref) <= 2 * 24 * 3 * U * mag)
    with pytest.raises(ValueError):
        diagnostics.target_moments(torch.zeros((3, 17, 8), dtype=torch.float64, device="cuda"), 8, second_moment=True)
    with pytest.raises(ValueError):
        diagnostics.target_moments(torch.zeros((3, 5, 8), dtype=torch.float64, device="cuda"), 3)

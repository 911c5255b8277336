"""The documented summation order of the per-target statistics, held bit for bit.

gsss_target_fold.h states how a batch's chains are cut at target boundaries, when the rows are split over workgroups as well, and
the four steps in which a target's sum is formed.  The other GPU tests hold the kernels to a longdouble reference within a
rounding bound and check that two calls agree; this one carries a float64 numpy model of the cut and of steps 1 - 4, written from
that comment, and asserts np.array_equal -- no tolerance -- for the sums that are plain additions:
    moments: the d rows sum x_j of acc, and chain_sum (one case through diagnostics.scalar_moments);
    autocov: P_0 = sum x_r, and Q_l = sum x_{r-l} for every lag (a row before the history reads as 0; adding 0.0 is exact).
Products (fma) and mixing's acos are not modelled: numpy has neither the fused multiply-add nor the device's acos.
The inputs are seeded standard_normal values, so that every addition rounds and another order shows in the last bits."""
import numpy as np
import pytest
import torch

from geosss_amd import diagnostics

pytestmark = pytest.mark.gpu

WANT_GRID = 1024                     # workgroups below which the rows are split as well
WAVE = 64


def _ceil_div(a, b):
    return -(-a // b)


class Cut:
    """How n = M m chains, R rows and `series` series are cut into workgroups of cw lanes."""

    def __init__(self, n, m, cw, R, min_split_rows, series=1):
        self.m, self.M, self.cw, self.R = m, n // m, cw, R
        if m <= cw:                  # a workgroup takes floor(cw / m) whole targets
            self.tpw, self.cpt = cw // m, 0
            self.n_chunks = _ceil_div(self.M, self.tpw)
        else:                        # a target takes ceil(m / cw) workgroups
            self.tpw, self.cpt = 0, _ceil_div(m, cw)
            self.n_chunks = self.M * self.cpt
        self.rsplit = 1
        if self.n_chunks * series < WANT_GRID:
            most, want = R // min_split_rows, _ceil_div(WANT_GRID, self.n_chunks * series)
            self.rsplit = 1 if most < 1 else min(want, most)

    def rows(self, sp):
        return self.R * sp // self.rsplit, self.R * (sp + 1) // self.rsplit

    def chunk(self, b):
        """(first target, targets, first chain, chains, chains per target within the chunk)"""
        if self.tpw:
            t0 = b * self.tpw
            nt = min(self.tpw, self.M - t0)
            return t0, nt, t0 * self.m, nt * self.m, self.m
        t0, first = b // self.cpt, (b % self.cpt) * self.cw
        nc = min(self.cw, self.m - first)
        return t0, 1, t0 * self.m + first, nc, nc

    def chunks_of(self, t):
        return [t // self.tpw] if self.tpw else list(range(t * self.cpt, (t + 1) * self.cpt))

    @property
    def single_partial(self):
        return self.tpw > 0 and self.rsplit == 1


def _wave_sum(v, lt):
    """Step 2: offsets 1, 2, .. 32; a lane adds the lane `off` further on only if that lane belongs to the same target."""
    v = v.copy()
    for s in range(6):
        off = 1 << s
        other = np.concatenate([v[off:], v[:off]])
        same = np.zeros(WAVE, dtype=bool)
        same[:WAVE - off] = lt[off:] == lt[:WAVE - off]
        v = np.where(same, v + other, v)
    return v


def _chunk_sums(cut, b, lane_sum):
    """Steps 2 and 3 for chunk b: lane_sum (n,), one sum per chain -> (first target, [a sum per target of the chunk])."""
    t0, nt, c0, nc, m_loc = cut.chunk(b)
    v = np.zeros(cut.cw)
    v[:nc] = lane_sum[c0:c0 + nc]
    lane = np.arange(cut.cw)
    lt = np.where(lane < nc, lane // m_loc, -1 - lane)       # lanes without a chain: a segment each
    lds = {}
    for w in range(cut.cw // WAVE):
        sl = slice(w * WAVE, (w + 1) * WAVE)
        red = _wave_sum(v[sl], lt[sl])
        for i in range(WAVE):                                # the first lane of each target in the wavefront
            if lt[sl][i] >= 0 and (i == 0 or lt[sl][i - 1] != lt[sl][i]):
                lds[w, lt[sl][i]] = red[i]
    out = []
    for t in range(nt):                                      # the wavefronts a target spans, in wavefront order
        lo, hi = (t * m_loc) // WAVE, ((t + 1) * m_loc - 1) // WAVE
        s = lds[lo, t]
        for w in range(lo + 1, hi + 1):
            s = s + lds[w, t]
        out.append(s)
    return t0, out


def _target_sums(cut, lane_sum_of):
    """Steps 2 - 4.  lane_sum_of(r0, r1) -> (n,): step 1 for the rows r0 .. r1 - 1.  Returns what is added to a zero acc, (M,)."""
    part = {}                                                # (row split, chunk, target) -> partial
    for sp in range(cut.rsplit):
        lane_sum = lane_sum_of(*cut.rows(sp))
        for b in range(cut.n_chunks):
            t0, sums = _chunk_sums(cut, b, lane_sum)
            for i, s in enumerate(sums):
                part[sp, b, t0 + i] = s
    out = np.zeros(cut.M)
    for t in range(cut.M):
        if cut.single_partial:
            out[t] = 0.0 + part[0, cut.chunks_of(t)[0], t]
        else:                                                # the workspace, in (row split, chunk) order
            s = 0.0
            for sp in range(cut.rsplit):
                for b in cut.chunks_of(t):
                    s = s + part[sp, b, t]
            out[t] = 0.0 + s
    return out


def _in_row_order(x, r0, r1, n):
    """Step 1: x (rows, n); a lane adds its chain's rows r0 .. r1 - 1 in row order."""
    s = np.zeros(n)
    for r in range(r0, r1):
        s = s + x[r]
    return s


def _chain_sums(cut, x):
    """chain_sum of one component, x (R, n): a chain's partials of the row splits, added in split order."""
    n = x.shape[1]
    if cut.rsplit == 1:
        return 0.0 + _in_row_order(x, 0, cut.R, n)
    s = np.zeros(n)
    for sp in range(cut.rsplit):
        s = s + _in_row_order(x, *cut.rows(sp), n)
    return 0.0 + s


# (d, full triangle, m, M, R): the cut's branches at the smallest shapes -- M m is far below 1024 chunks, R alone decides the split
MOMENTS = [
    (3, True, 24, 7, 3),      # tpw = 10, targets straddle wavefronts, a single partial goes straight into acc
    (3, True, 24, 7, 40),     # rsplit = 5, workspace with tpw > 0
    (10, True, 100, 7, 3),    # CW = 128, a target over two wavefronts
    (16, True, 300, 3, 17),   # CW = 64, cpt = 5, rsplit = 2
    (17, False, 300, 3, 3),   # the any-d diagonal kernel, cpt = 2
    (5, True, 1, 130, 1),     # m = 1
]


def _moments_cw(d, full):
    return 256 if (not full or d <= 8 or d > 16) else (128 if d <= 12 else 64)


def _assert_same_bits(got, want, what):
    diff = int(np.count_nonzero(got != want))
    print(f"{what}: {diff} of {got.size} entries differ")
    assert got.shape == want.shape and np.array_equal(got, want), (what, diff)


@pytest.mark.parametrize("d, full, m, M, R", MOMENTS)
def test_moments_sums_in_the_documented_order(d, full, m, M, R):
    n = M * m
    x = np.random.default_rng(31 * d + m + R).standard_normal((R, d, n))
    cs = torch.zeros((d, n), dtype=torch.float64, device="cuda")
    acc = diagnostics.target_moments(torch.from_numpy(x).cuda(), m, second_moment=full, chain_sum=cs)
    acc, cs = acc.cpu().numpy(), cs.cpu().numpy()
    cut = Cut(n, m, _moments_cw(d, full), R, 8)
    want = np.stack([_target_sums(cut, lambda r0, r1, j=j: _in_row_order(x[:, j], r0, r1, n)) for j in range(d)], 1)
    _assert_same_bits(acc[:, 1:1 + d], want, "sum x_j")
    _assert_same_bits(cs, np.stack([_chain_sums(cut, x[:, j]) for j in range(d)]), "chain_sum")
    assert np.all(acc[:, 0] == m * R)


def test_scalar_moments_sums_in_the_documented_order():
    m, M, R = 24, 7, 40                                      # rsplit = 5 through the any-d diagonal kernel
    n = M * m
    v = np.random.default_rng(5).standard_normal((R, n))
    cs = torch.zeros((n,), dtype=torch.float64, device="cuda")
    acc = diagnostics.scalar_moments(torch.from_numpy(v).cuda(), m, chain_sum=cs).cpu().numpy()
    cut = Cut(n, m, 256, R, 8)
    assert cut.rsplit == 5
    _assert_same_bits(acc[:, 1], _target_sums(cut, lambda r0, r1: _in_row_order(v, r0, r1, n)), "sum v")
    _assert_same_bits(cs.cpu().numpy(), _chain_sums(cut, v), "chain_sum")


# (d, L, m, M, R, n_hist)
AUTOCOV = [
    (2, 8, 24, 7, 70, 0),     # CW = 256, rsplit = 2
    (2, 20, 100, 3, 70, 5),   # CW = 128, with history
    (1, 40, 70, 3, 33, 0),    # CW = 64, cpt = 2
]


@pytest.mark.parametrize("d, L, m, M, R, n_hist", AUTOCOV)
def test_autocov_plain_sums_in_the_documented_order(d, L, m, M, R, n_hist):
    n = M * m
    g = np.random.default_rng(1000 * L + m + R)
    x, hist = g.standard_normal((R, d, n)), g.standard_normal((n_hist, d, n))
    acc = diagnostics.target_autocov(torch.from_numpy(x).cuda(), m, L,
                                     hist=torch.from_numpy(hist).cuda() if n_hist else None).cpu().numpy()
    assert acc.shape == (M, d, L + 1, 3)
    cut = Cut(n, m, 256 if L <= 16 else (128 if L <= 32 else 64), R, 32, series=d)
    # row q of the block is row L + q of `ext`: L rows of zeros (before the history), the history, the block
    ext = np.concatenate([np.zeros((L - n_hist, d, n)), hist, x])
    for j in range(d):
        for lag in range(L + 1):
            delayed = ext[L - lag:L - lag + R, j]            # x_{r - lag} for r = 0 .. R - 1
            want = _target_sums(cut, lambda r0, r1: _in_row_order(delayed, r0, r1, n))
            _assert_same_bits(acc[:, j, lag, 2], want, f"Q_{lag} of series {j}")
            if lag == 0:
                _assert_same_bits(acc[:, j, 0, 1], want, f"P_0 of series {j}")

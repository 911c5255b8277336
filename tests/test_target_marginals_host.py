"""Per-target marginal histograms without a GPU: the row counts and refusals of gsss_target_marginals (no device is touched),
the register budget of its kernels, the conditions on the shared cases of marginal_cases.py, from_target_marginals and
marginal_quantile on hand-made counts against the quantile rule restated in numpy, and what TargetMoments and summarize check
before any launch."""
import numpy as np
import pytest
import torch

import marginal_cases as mc
from geosss_amd import _lib, diagnostics

E_INVALID, E_UNSUPPORTED = -1, -2
STEP = 1


def test_marginal_rows():
    lib = _lib.load()
    for P, B in ((1, 2), (5, 64), (32, 256), (8, 1024)):
        assert lib.gsss_marginal_rows(P, B, 0) == P * B
    for P, B in ((0, 64), (5, 64), (7, 1024), (31, 256)):
        assert lib.gsss_marginal_rows(P, B, STEP) == (P + 1) * B
    for P, B, flags in ((-1, 64, 0), (0, 64, 0), (3, 1, 0), (3, 0, STEP), (3, 64, 2), (3, 64, 3)):
        assert lib.gsss_marginal_rows(P, B, flags) == E_INVALID, (P, B, flags)
    for P, B, flags in ((33, 64, 0), (3, 1025, 0), (9, 1024, 0), (8, 1024, STEP), (32, 256, STEP)):
        assert lib.gsss_marginal_rows(P, B, flags) == E_UNSUPPORTED, (P, B, flags)
    assert _lib.MARGINALS_STEP == STEP


def test_abi_version_is_unchanged():
    assert _lib.load().gsss_abi_version() == 10 == _lib.ABI_VERSION


# (ring, ring_rows, first_row, n_rows, n_hist, n_chains, d, m, dirs, n_dirs, n_bins, flags, count) -> code; pointers: 1 = some
# non-NULL address that is never read
@pytest.mark.parametrize("args, code", [
    ((1, 12, 0, 4, 0, 8, 1, 4, 1, 3, 64, 0, 1), E_INVALID),          # d < 2
    ((1, 12, 0, 4, 0, 8, 3, 0, 1, 3, 64, 0, 1), E_INVALID),          # m < 1
    ((1, 12, 0, 4, 0, 8, 3, 3, 1, 3, 64, 0, 1), E_INVALID),          # n_chains % m
    ((1, 12, 0, -1, 0, 8, 3, 4, 1, 3, 64, 0, 1), E_INVALID),         # negative row count
    ((1, 12, -1, 4, 0, 8, 3, 4, 1, 3, 64, 0, 1), E_INVALID),         # negative first row
    ((1, 12, 0, 4, -1, 8, 3, 4, 1, 3, 64, STEP, 1), E_INVALID),      # negative history
    ((1, 12, 0, 4, 0, -8, 3, 4, 1, 3, 64, 0, 1), E_INVALID),         # negative chain count
    ((1, -12, 0, 4, 0, 8, 3, 4, 1, 3, 64, 0, 1), E_INVALID),         # negative ring
    ((1, 12, 9, 4, 0, 8, 3, 4, 1, 3, 64, 0, 1), E_INVALID),          # first_row + n_rows > ring_rows
    ((1, 12, 0, 4, 2, 8, 3, 4, 1, 3, 64, STEP, 1), E_INVALID),       # n_hist > 1
    ((1, 12, 0, 4, 2, 8, 3, 4, 1, 3, 64, 0, 1), E_INVALID),          # ... without the steps too
    ((1, 12, 0, 12, 1, 8, 3, 4, 1, 3, 64, STEP, 1), E_INVALID),      # n_hist > ring_rows - n_rows
    ((1, 12, 0, 4, 0, 8, 3, 4, 1, -1, 64, STEP, 1), E_INVALID),      # n_dirs < 0
    ((1, 12, 0, 4, 0, 8, 3, 4, 1, 0, 64, 0, 1), E_INVALID),          # no directions and no steps
    ((1, 12, 0, 4, 0, 8, 3, 4, 1, 3, 1, 0, 1), E_INVALID),           # n_bins < 2
    ((1, 12, 0, 4, 0, 8, 3, 4, 1, 3, 64, 2, 1), E_INVALID),          # unknown flags
    ((0, 12, 0, 4, 0, 8, 3, 4, 1, 3, 64, 0, 1), E_INVALID),          # NULL ring
    ((1, 12, 0, 4, 0, 8, 3, 4, 0, 3, 64, 0, 1), E_INVALID),          # NULL dirs with n_dirs > 0
    ((1, 12, 0, 4, 0, 8, 3, 4, 1, 3, 64, 0, 0), E_INVALID),          # NULL count
    ((1, 12, 0, 4, 0, 8, 3, 4, 1, 33, 64, 0, 1), E_UNSUPPORTED),     # more than 32 directions
    ((1, 12, 0, 4, 0, 8, 3, 4, 1, 3, 1025, 0, 1), E_UNSUPPORTED),    # more than 1024 bins
    ((1, 12, 0, 4, 0, 8, 3, 4, 1, 9, 1024, 0, 1), E_UNSUPPORTED),    # S B > 8192
    ((1, 12, 0, 4, 0, 8, 3, 4, 1, 8, 1024, STEP, 1), E_UNSUPPORTED),
    ((1, 2 ** 23 + 1, 0, 2 ** 23 + 1, 0, 8, 3, 4, 1, 3, 64, 0, 1), E_UNSUPPORTED),   # a 32-bit LDS counter could overflow
])
def test_refusals_need_no_device(args, code):
    lib = _lib.load()
    r, ring_rows, first_row, n_rows, n_hist, n, d, m, dr, P, B, flags, c = args
    bogus = 4096
    assert lib.gsss_target_marginals(bogus if r else None, ring_rows, first_row, n_rows, n_hist, n, d, m, bogus if dr else None, P, B,
                                     flags, bogus if c else None, 0, None) == code
    assert lib.gsss_last_error()


def test_no_rows_is_a_no_op():
    lib = _lib.load()
    assert lib.gsss_target_marginals(4096, 12, 3, 0, 1, 8, 3, 4, 4096, 3, 64, STEP, 4096, 0, None) == 0
    assert lib.gsss_target_marginals(None, 0, 0, 0, 0, 8, 2, 4, None, 2, 64, 0, None, 0, None) == 0
    # a history row without the steps is accepted (and not read): an empty block shows that it passes the checks
    assert lib.gsss_target_marginals(4096, 12, 3, 0, 1, 8, 3, 4, 4096, 3, 64, 0, 4096, 0, None) == 0


def test_marginals_kernels_do_not_spill():
    """The fifteen builds with a compile-time d = 2 .. 16 and the one with a run-time d keep a lane's draws and products in
    registers: no scratch.  There is no second kernel."""
    from geosss_amd import build
    ru = build.resource_usage("gsss_marginals.hip")
    assert sum("marginals_kernel" in k for k in ru) == 16 and len(ru) == 16, sorted(ru)
    for name, r in ru.items():
        assert r["scratch"] == 0, (name, r)


@pytest.mark.parametrize("name", sorted(mc.CASES))
def test_case_conditions(name):
    """What the exact comparison on the device rests on: no value of the case within 1e-9 of a bin edge (the cap on excluded
    values is zero), the derived bound on the device's error in t below that margin, and the reference's own totals."""
    M, m, rows, d, kind, P, bins, steps, n_hist, specials = mc.CASES[name]
    x, hist, dirs, ref = mc.case(name)
    assert x.shape == (rows, d, M * m) and hist.shape == (n_hist, d, M * m)
    assert ref.on_edge == 0
    assert ref.t_error < mc.EDGE, ref.t_error
    assert ref.counts.shape == (M, P + steps, bins) and ref.counts.dtype == np.int64
    assert np.all(ref.counts[:, :P].sum(-1) == m * rows)
    if steps:
        assert np.all(ref.counts[:, P].sum(-1) == m * (rows - 1 + n_hist)) and ref.pairs == M * m * (rows - 1 + n_hist)
    if specials:       # the placed draws: x_0 = -1 in the first bin, +1 in the last, 0 at the middle edge's upper side
        assert (x[:, 0] == 1.0).any() and (x[:, 0] == -1.0).any() and (x[:, 0] == 0.0).any()
        b = mc.axis_bins(np.array([-1.0, 0.0, 1.0]), bins)
        assert list(b) == [0, bins // 2, bins - 1]


def test_cases_cover_what_they_name():
    c = mc.CASES.values()
    assert {v[3] for v in c} >= {2, 3, 16, 17, 600} and {v[1] for v in c} >= {1, 7, 64, 256, 259, 600}
    assert {v[2] for v in c} == {1, 5, 70} and {v[6] for v in c} >= {2, 64, 1024} and {v[8] for v in c} == {0, 1}
    assert sum((v[5] + v[7]) * v[6] == 8192 for v in c) == 1 and all((v[5] + v[7]) * v[6] <= 8192 for v in c)
    dirs = mc.own_directions(3, 4, 5, seed=1)
    norms = np.linalg.norm(dirs, axis=-1)
    assert np.array_equal(dirs[0, 0], -np.eye(5)[0]) and abs(norms[1, 3] - 0.5) < 1e-15 and abs(norms[2, 2] - 2.0) < 1e-15
    assert not np.array_equal(dirs[0, 1], dirs[1, 1])


def test_axis_reference_is_exact_and_matches_longdouble_off_the_edges():
    """The two references agree where both apply: axis directions given as an explicit identity go through the longdouble path."""
    x = mc.walk(6, 4, 30, seed=3)
    none = mc.Reference(x, x[:0], 5, None, 64, False)
    eye = mc.Reference(x, x[:0], 5, np.eye(4), 64, False)
    assert eye.on_edge == 0 and np.array_equal(none.counts, eye.counts)
    y = x.copy()
    y[2] = np.nan
    nan = mc.Reference(y, y[:0], 5, None, 64, True)
    assert nan.counts[:, :4].sum() == 30 * 4 * 5 and nan.counts[:, 4].sum() == 30 * 3     # a NaN row: its draws and both its pairs


# ---------------------------------------------------------------------------------------------------------------------------
# from_target_marginals and marginal_quantile

HAND = {
    "one full bin": [0, 0, 9, 0],
    "two bins 1 : 3": [0, 5, 15, 0],
    "empty": [0, 0, 0, 0],
    "flat": [4, 4, 4, 4],
    "ends": [7, 0, 0, 1],
}


@pytest.mark.parametrize("what", sorted(HAND))
def test_quantiles_against_the_rule(what):
    counts = np.array(HAND[what], dtype=np.int64)
    edges = np.linspace(-1.0, 1.0, 5)
    for q in (0.0, 0.025, 0.25, 0.5, 0.75, 0.975, 1.0, 1 / 3):
        got = float(diagnostics.marginal_quantile(torch.from_numpy(counts), edges, q))
        want = mc.quantile_rule(counts, edges, q)
        if what == "empty":
            assert np.isnan(got) and np.isnan(want)
        else:
            assert abs(got - want) <= 1e-12 * abs(want), (what, q, got, want)
    many = diagnostics.marginal_quantile(torch.from_numpy(counts), edges, [0.25, 0.5])
    assert tuple(many.shape) == (2,)
    with pytest.raises(ValueError):
        diagnostics.marginal_quantile(counts, edges, 1.5)
    with pytest.raises(ValueError):
        diagnostics.marginal_quantile(counts, edges[:-1], 0.5)


def test_quantile_values_by_hand():
    edges = np.linspace(-1.0, 1.0, 5)
    q = lambda c, level: float(diagnostics.marginal_quantile(np.array(c), edges, level))
    assert q([0, 0, 9, 0], 0.5) == 0.25 and q([0, 0, 9, 0], 0.0) == 0.0 and q([0, 0, 9, 0], 1.0) == 0.5   # spread over its bin
    assert q([0, 5, 15, 0], 0.25) == 0.0           # q N = cum of bin 1 exactly: the boundary, taken from the bin below
    assert q([0, 5, 15, 0], 0.625) == 0.25         # half of the upper bin's draws
    assert q([4, 4, 4, 4], 0.5) == 0.0 and q([4, 4, 4, 4], 0.75) == 0.5
    assert q([7, 0, 0, 1], 0.875) == -0.5 and q([7, 0, 0, 1], 1.0) == 1.0      # the empty bins between are skipped


def test_from_target_marginals():
    g = np.random.default_rng(5)
    M, P, B = 3, 2, 8
    counts = g.integers(0, 50, (M, P + 1, B))
    counts[1, 0] = 0                                     # an empty row
    counts[2, 1] = 0
    counts[2, 1, 3] = 11                                 # a single full bin
    out = diagnostics.from_target_marginals(torch.from_numpy(counts), P, steps=True)
    edges, step_edges = np.linspace(-1, 1, B + 1), np.linspace(0, np.pi, B + 1)
    assert np.array_equal(out["marginal_edges"].numpy(), edges) and np.array_equal(out["step_edges"].numpy(), step_edges)
    for key, shape in (("marginal_density", (M, P, B)), ("marginal_cdf", (M, P, B)), ("marginal_quantiles", (M, P, 5)),
                       ("marginal_median", (M, P)), ("step_density", (M, B)), ("step_quantiles", (M, 5))):
        assert tuple(out[key].shape) == shape and out[key].dtype == torch.float64, key
    dens, cdf = out["marginal_density"].numpy(), out["marginal_cdf"].numpy()
    assert np.isnan(dens[1, 0]).all() and np.isnan(cdf[1, 0]).all() and np.isnan(out["marginal_quantiles"].numpy()[1, 0]).all()
    full = np.ones((M, P), dtype=bool)
    full[1, 0] = False
    assert np.allclose((dens * (2 / B)).sum(-1)[full], 1.0, rtol=1e-14) and np.allclose(cdf[..., -1][full], 1.0, rtol=0, atol=0)
    assert np.allclose((out["step_density"].numpy() * (np.pi / B)).sum(-1), 1.0, rtol=1e-14)
    for t in range(M):
        for p in range(P):
            for i, level in enumerate(diagnostics.MARGINAL_QUANTILES):
                want = mc.quantile_rule(counts[t, p], edges, level)
                got = float(out["marginal_quantiles"][t, p, i])
                assert (np.isnan(want) and np.isnan(got)) or abs(got - want) <= 1e-12 * abs(want)
        for i, level in enumerate(diagnostics.MARGINAL_QUANTILES):
            want = mc.quantile_rule(counts[t, P], step_edges, level)
            assert abs(float(out["step_quantiles"][t, i]) - want) <= 1e-12 * abs(want)
    assert np.array_equal(out["marginal_median"].numpy(), out["marginal_quantiles"][..., 2].numpy(), equal_nan=True)
    assert float(out["marginal_median"][2, 1]) == edges[3] + 0.5 * (2 / B)
    plain = diagnostics.from_target_marginals(counts[:, :P], P)
    assert "step_density" not in plain and "step_quantiles" not in plain
    assert np.array_equal(plain["marginal_quantiles"].numpy(), out["marginal_quantiles"].numpy(), equal_nan=True)
    with pytest.raises(ValueError):
        diagnostics.from_target_marginals(counts, P)                       # three series, two directions, no steps
    with pytest.raises(ValueError):
        diagnostics.from_target_marginals(counts[0], P, steps=True)


# ---------------------------------------------------------------------------------------------------------------------------
# TargetMoments and the argument checks of summarize, on the CPU

def test_target_moments_with_marginals():
    n, d, m = 12, 3, 4
    cpu = torch.device("cpu")
    tm = diagnostics.TargetMoments.begin(n, d, m, cpu, marginals=dict(bins=16, directions=None, steps=False))
    assert tuple(tm.marg_counts.shape) == (3, 3, 16) and tm.marg_counts.dtype == torch.int64 and not tm.marg_counts.any()
    assert tuple(tm.marg_dirs.shape) == (3, 3, 3) and torch.equal(tm.marg_dirs[1], torch.eye(3, dtype=torch.float64))
    assert tm.marg_bins == 16 and tm.marg_steps is False and tm.hist_rows == 0
    v = np.random.default_rng(1).standard_normal((2, d))
    steps = diagnostics.TargetMoments.begin(n, d, m, cpu, marginals=dict(bins=16, directions=v, steps=True))
    assert tuple(steps.marg_counts.shape) == (3, 3, 16) and tuple(steps.marg_dirs.shape) == (3, 2, 3) and steps.marg_steps is True
    assert torch.equal(steps.marg_dirs[2], torch.from_numpy(v)) and steps.marg_dirs.is_contiguous()
    assert steps.hist_rows == 1
    own = np.random.default_rng(2).standard_normal((3, 5, d))
    lagged = diagnostics.TargetMoments.begin(n, d, m, cpu, lags=4, marginals=dict(bins=2, directions=own, steps=True))
    assert lagged.hist_rows == 4 and tuple(lagged.marg_counts.shape) == (3, 6, 2) and torch.equal(lagged.marg_dirs, torch.from_numpy(own))
    plain = diagnostics.TargetMoments.begin(n, d, m, cpu)
    assert plain.marg_counts is None and plain.marg_dirs is None and plain.marg_bins is None and plain.marg_steps is False
    assert plain.hist_rows == 0 and not {"marginal_edges", "marginal_density", "step_edges"} & set(plain.stats())
    with pytest.raises(ValueError, match="begun without marginals"):
        plain.quantile(0.5)

    ask = dict(bins=16, directions=None, steps=False)
    tm.check_continues(n, d, m, marginals=ask)
    tm.check_continues(n, d, m)                                         # a summary that carries them goes on carrying them
    tm.check_continues(n, d, m, marginals=dict(ask, directions=np.ones((3, d))))     # the same number of directions
    for other in (dict(ask, bins=32), dict(ask, steps=True), dict(ask, directions=v), dict(ask, directions=own)):
        with pytest.raises(ValueError, match="begun without these marginals"):
            tm.check_continues(n, d, m, marginals=other)
    with pytest.raises(ValueError, match="begun without these marginals"):
        plain.check_continues(n, d, m, marginals=ask)

    # stats() and quantile() from counts put in by hand
    tm.marg_counts[0, 1, 3] = 5
    tm.marg_counts[0, 1, 4] = 15
    st = tm.stats()
    edges = np.linspace(-1, 1, 17)
    assert tuple(st["marginal_quantiles"].shape) == (3, 3, 5) and "step_density" not in st
    assert abs(float(st["marginal_median"][0, 1]) - mc.quantile_rule(tm.marg_counts[0, 1].numpy(), edges, 0.5)) <= 1e-12
    assert abs(float(tm.quantile(0.9)[0, 1]) - mc.quantile_rule(tm.marg_counts[0, 1].numpy(), edges, 0.9)) <= 1e-12
    assert tuple(tm.quantile([0.1, 0.9]).shape) == (3, 3, 2) and np.isnan(float(tm.quantile(0.5)[1, 0]))

    for bad, exc in ((dict(bins=1, directions=None, steps=False), "bins"), (dict(bins=1025, directions=None, steps=False), "bins"),
                     (dict(bins=64, directions=np.ones((33, d)), steps=False), "32 directions"),
                     (dict(bins=1024, directions=np.ones((8, d)), steps=True), "8192"),
                     (dict(bins=64, directions=np.ones((0, d)), steps=False), "nothing to count"),
                     (dict(bins=64, directions=np.ones((2, d + 1)), steps=False), "directions must be"),
                     (dict(bins=64, directions=np.ones((2, 2, d)), steps=False), "directions must be")):
        with pytest.raises(ValueError, match=exc):
            diagnostics.TargetMoments.begin(n, d, m, cpu, marginals=bad)


def test_argument_checks_need_no_device():
    plan = diagnostics._marginals_plan
    assert plan(True) == dict(bins=64, directions=None, steps=False)
    assert plan(dict(bins=100)) == dict(bins=100, directions=None, steps=False)
    u = np.ones((1, 5))
    got = plan(dict(directions=u, steps=1))
    assert got["directions"] is u and got["steps"] is True and got["bins"] == 64
    for bad in ("yes", 64, dict(bin=64), dict(bins=64, direction=u), dict(bins=1), dict(bins=2.5), dict(bins=True), dict(bins=4096)):
        with pytest.raises(ValueError):
            plan(bad)
    x = torch.zeros((5, 3, 12), dtype=torch.float64)
    with pytest.raises(ValueError, match="CUDA"):
        diagnostics.target_marginals(x, 4)                                       # not a device tensor
    with pytest.raises(ValueError):
        diagnostics.target_marginals(x, 5)                                       # n_chains % m
    with pytest.raises(ValueError, match="bins"):
        diagnostics.target_marginals(x, 4, bins=1)
    with pytest.raises(ValueError, match="directions must be"):
        diagnostics.target_marginals(x, 4, directions=np.ones((2, 4)))
    with pytest.raises(ValueError, match="directions must be"):
        diagnostics.target_marginals(x, 4, directions=np.ones((2, 2, 3)))        # three targets
    with pytest.raises(ValueError, match="8192"):
        diagnostics.target_marginals(x, 4, bins=1024, directions=np.ones((8, 3)), steps=True)
    with pytest.raises(ValueError):
        diagnostics.target_marginals(x.to(torch.float32), 4)
    with pytest.raises(ValueError, match="two coordinates"):
        diagnostics.target_marginals(torch.zeros((5, 1, 12), dtype=torch.float64), 4)

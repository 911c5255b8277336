"""gsss_target_marginals and summarize(marginals=) on the device.

The counts are held to the host reference of marginal_cases.py and must be EQUAL: the cases are conditioned (asserted on the
CPU, tests/test_target_marginals_host.py) so that no value lies within 1e-9 of a bin edge while the device's t provably lies
within 1e-9 of the exact one; for coordinate axes the host bins by the device's own double arithmetic and no margin is needed.
Blocks are also laid into NaN-filled rings: a read outside the block and its history row shows as a missing count.
summarize(marginals=) is held to target_marginals on the stored draws of an identically seeded twin, exactly."""
import warnings

import numpy as np
import pytest
import torch

import geosss_amd as gs
import marginal_cases as mc
from geosss_amd import diagnostics

pytestmark = pytest.mark.gpu
SEED = 977


def _cuda(a):
    return torch.tensor(a, dtype=torch.float64, device="cuda")


def _own(dirs):
    return None if dirs is None else dirs.copy()


def _run(name, x=None, hist=None, **kw):
    """diagnostics.target_marginals on the case's inputs (or on x / hist in their place)."""
    M, m, rows, d, kind, P, bins, steps, n_hist, specials = mc.CASES[name]
    cx, chist, dirs, _ = mc.case(name)
    x = cx if x is None else x
    hist = chist if hist is None else hist
    return diagnostics.target_marginals(_cuda(x), m, bins=bins, directions=_own(dirs), steps=steps,
                                        hist=_cuda(hist) if len(hist) else None, **kw)


@pytest.mark.parametrize("name", sorted(mc.CASES))
def test_counts_against_the_host_reference(name):
    M, m, rows, d, kind, P, bins, steps, n_hist, specials = mc.CASES[name]
    x, hist, dirs, ref = mc.case(name)
    counts = _run(name)
    assert tuple(counts.shape) == (M, P + steps, bins) and counts.dtype == torch.int64
    got = counts.cpu().numpy()
    print(f"{name}: {int(np.abs(got - ref.counts).sum())} of {int(ref.counts.sum())} counts differ")
    assert np.array_equal(got, ref.counts)
    # the same call again: the same counts; `counts=` is added to, from a start that is not zero
    start = torch.arange(counts.numel(), dtype=torch.int64, device="cuda").reshape(counts.shape) % 7
    again = _run(name, counts=start.clone())
    assert torch.equal(again, start + counts)
    # the block inside NaN-filled rings larger than itself: at row 2 behind its history row, and at row 0 with the history row
    # round the ring's end
    dirs_t, _ = diagnostics._marginal_dirs(_own(dirs), M, d, torch.device("cuda"))
    for first in (2, 0):
        ring = torch.full((rows + 3, d, M * m), float("nan"), dtype=torch.float64, device="cuda")
        ring[first:first + rows] = _cuda(x)
        if n_hist:
            ring[(first - 1) % (rows + 3)] = _cuda(hist[0])
        c = torch.zeros_like(counts)
        diagnostics._marginals_fold(ring, first, rows, n_hist, m, dirs_t, bins, steps, c)
        assert torch.equal(c, counts), first


@pytest.mark.parametrize("name", ["d2_m1_axes", "d3_m7_own", "d16_m259_split", "d17_m600_own", "d600_m7_global", "d3_m256_split"])
def test_two_calls_equal_one(name):
    """Rows 0 .. k - 1, then k .. behind one row of history: the pair at the seam is counted once."""
    M, m, rows, d, kind, P, bins, steps, n_hist, specials = mc.CASES[name]
    x, hist, dirs, ref = mc.case(name)
    assert steps
    for k in sorted({1, rows // 2, rows - 1}):
        c = _run(name, x=x[:k])
        c = _run(name, x=x[k:], hist=x[k - 1:k], counts=c)
        assert np.array_equal(c.cpu().numpy(), ref.counts), k
    # without the history row the seam's pairs are missing, and nothing else
    c = _run(name, x=x[:1])
    c = _run(name, x=x[1:], hist=x[:0], counts=c)
    missing = ref.counts - c.cpu().numpy()
    assert np.all(missing[:, :P] == 0) and np.all(missing[:, P].sum(-1) == m)


@pytest.mark.parametrize("name", ["d3_m256_split", "d17_m7_axes_b2", "d2_m1_axes", "d17_m600_own"])
def test_a_nan_row_is_counted_nowhere(name):
    M, m, rows, d, kind, P, bins, steps, n_hist, specials = mc.CASES[name]
    x, hist, dirs, ref = mc.case(name)
    r = rows // 2                                     # (70 rows: the first row of the second run of the row split)
    y = x.copy()
    y[r] = np.nan
    got = _run(name, x=y).cpu().numpy()
    assert np.array_equal(got, mc.Reference(y, hist, m, dirs, bins, steps).counts)
    # what is gone: the row's own draws and the two pairs it belongs to -- every other count is unchanged
    gone = ref.counts - got
    assert np.array_equal(gone[:, :P], mc.Reference(x[r:r + 1], x[:0], m, dirs, bins, False).counts)
    if steps:
        assert np.array_equal(gone[:, P], mc.Reference(x[r - 1:r + 2], x[:0], m, dirs, bins, True).counts[:, P])


@pytest.mark.parametrize("name", ["d3_m7_own", "d16_m259_split"])
def test_chain_major_input(name):
    M, m, rows, d, kind, P, bins, steps, n_hist, specials = mc.CASES[name]
    x, hist, dirs, ref = mc.case(name)
    xc, hc = _cuda(x).permute(2, 0, 1).contiguous(), _cuda(hist).permute(2, 0, 1).contiguous()        # (n, R, d)
    counts = diagnostics.target_marginals(xc, m, bins=bins, directions=_own(dirs), steps=steps, chain_major=True,
                                          hist=hc if n_hist else None)
    assert np.array_equal(counts.cpu().numpy(), ref.counts)
    view = torch.empty((M * m, rows + 2, d), dtype=torch.float64, device="cuda")[:, 1:1 + rows]       # a strided slice of rows
    view.copy_(xc)
    assert torch.equal(diagnostics.target_marginals(view, m, bins=bins, directions=_own(dirs), steps=steps, chain_major=True,
                                                    hist=hc if n_hist else None), counts)


# ---------------------------------------------------------------------------------------------------------------------------
# summarize(marginals=) against the stored run of an identically seeded twin

N_SAMPLES, BURNIN, THIN = 24, 6, 2


def _x0(d, n, seed=5):
    x = np.random.default_rng(seed).standard_normal((n, d))
    return x / np.linalg.norm(x, axis=1, keepdims=True)


def _vmf_mixtures(M, d=3, K=3, seed=11):
    g = np.random.default_rng(seed)
    out = []
    for _ in range(M):
        mu = g.standard_normal((K, d))
        mu *= (10.0 + 30.0 * g.random((K, 1))) / np.linalg.norm(mu, axis=1, keepdims=True)
        out.append(gs.MixtureModel([gs.VonMisesFisher(v) for v in mu], g.random(K) + 0.5))
    return out


def _binghams(M, d=5, seed=12):
    g = np.random.default_rng(seed)
    return [gs.random_bingham(d, vmax=20.0, vmin=0.0, seed=int(g.integers(1 << 30))) for _ in range(M)]


def _make(which):
    """-> (a function that builds the identically seeded sampler, M, m, d, per-target directions (M, P, d))"""
    def batch(pdfs, m, mode, tempered=None):
        d = pdfs[0].d
        target = gs.TargetBatch.tempered(list(pdfs), tempered) if tempered else gs.TargetBatch(pdfs)
        M = len(target)
        x0 = _x0(d, M * m)

        def build():
            with warnings.catch_warnings(record=True):
                warnings.simplefilter("always")
                return gs.ShrinkageSphericalSliceSampler(target, x0, SEED, mode=mode, chains_per_target=m)
        return build, M, m, d
    if which in ("bingham_fast", "bingham_exact"):
        pdfs = _binghams(6)
        build, M, m, d = batch(pdfs, 40, which.split("_")[1])
        own = np.stack([np.stack([p.mode, -p.mode, 0.5 * np.roll(p.mode, 1)]) for p in pdfs])          # u_d^T x, as the paper plots it
    elif which == "vmfmix_m300":
        build, M, m, d = batch(_vmf_mixtures(3), 300, "fast")
        own = np.random.default_rng(3).standard_normal((M, 2, d))
    elif which == "tempered":
        build, M, m, d = batch(_vmf_mixtures(2, seed=21), 40, "fast", tempered=[1.0, 0.5, 0.2])
        own = np.random.default_rng(4).standard_normal((M, 2, d))
    elif which == "single_target":
        pdf, n, d = gs.VonMisesFisher(20.0 * np.eye(3)[2]), 64, 3
        x0 = _x0(d, n, seed=8)
        build, M, m = (lambda: gs.ShrinkageSphericalSliceSampler(pdf, x0, SEED)), 1, n
        own = np.random.default_rng(5).standard_normal((1, 4, d))
    else:
        raise KeyError(which)
    return build, M, m, d, own


def _same_chains(a, b):
    assert torch.equal(a.state_rows(), b.state_rows()) and a._step == b._step
    assert np.array_equal(a.n_tries_per_chain, b.n_tries_per_chain)


@pytest.mark.parametrize("which", ["bingham_fast", "bingham_exact", "vmfmix_m300", "single_target", "tempered"])
def test_summarize_marginals_is_the_stored_run(which):
    build, M, m, d, own = _make(which)
    ex = dict(exchange=dict(ladder=3, every=2)) if which == "tempered" else {}
    twin = build()
    draws = twin.sample(N_SAMPLES, burnin=BURNIN, thin=THIN, as_tensor=True, **ex)                      # (n, R, d)
    x = draws.permute(1, 2, 0).cpu().numpy()
    marg = dict(bins=100, directions=own, steps=True)
    want = diagnostics.target_marginals(draws, m, chain_major=True, **marg)
    P = own.shape[1]
    assert int(want[:, :P].sum()) == M * P * m * N_SAMPLES and int(want[:, P].sum()) == M * m * (N_SAMPLES - 1)

    s = build()
    tm = s.summarize(N_SAMPLES, burnin=BURNIN, thin=THIN, marginals=marg, **ex)
    assert tm.marg_bins == 100 and tm.marg_steps is True and tuple(tm.marg_dirs.shape) == (M, P, d)
    assert tm.marg_counts.dtype == torch.int64 and torch.equal(tm.marg_counts, want)
    assert tm.lags is None and tm.mix_step is None and tuple(tm.hist.shape) == (1, d, M * m)
    _same_chains(s, twin)
    # the ring of lags=4 and small windows that wrap it: the same counts
    s = build()
    assert torch.equal(s.summarize(N_SAMPLES, burnin=BURNIN, thin=THIN, lags=4, marginals=marg, **ex).marg_counts, want)
    s = build()
    assert torch.equal(s.summarize(N_SAMPLES, burnin=BURNIN, thin=THIN, window=3, marginals=marg, **ex).marg_counts, want)
    # into= over two calls: the pair at the seam counted once.  (Not under exchange=: a call's draw 0 is the state AFTER the sweep
    # that ends its burn-in, a later row the state before its sweep, so two calls retain another row at the seam than one.)
    s = build()
    half = s.summarize(N_SAMPLES // 2, burnin=BURNIN, thin=THIN, window=5, marginals=marg, **ex)
    both = s.summarize(N_SAMPLES // 2, burnin=THIN, thin=THIN, window=5, into=half, **ex)
    assert both is half and int(both.marg_counts[:, P].sum()) == M * m * (N_SAMPLES - 1)
    if not ex:
        assert torch.equal(both.marg_counts, want)
        _same_chains(s, twin)
    with pytest.raises(ValueError, match="begun without these marginals"):
        build().summarize(N_SAMPLES, marginals=dict(marg, bins=64), into=both)
    with pytest.raises(ValueError, match="begun without these marginals"):
        build().summarize(N_SAMPLES, marginals=True, into=build().summarize(3))
    with pytest.raises(ValueError):
        build().summarize(N_SAMPLES, marginals="yes")

    # coordinate axes, no steps: np.histogram-style host binning of the stored draws by the exact rule, the plain buffer
    s = build()
    axes = s.summarize(N_SAMPLES, burnin=BURNIN, thin=THIN, marginals=True, **ex)
    assert axes.hist is None and axes.marg_bins == 64 and axes.marg_steps is False
    assert torch.equal(axes.marg_counts, diagnostics.target_marginals(draws, m, chain_major=True))
    host = mc.Reference(x, x[:0], m, None, 64, False).counts
    assert np.array_equal(axes.marg_counts.cpu().numpy(), host)
    for t in range(M):                                         # ... which is np.histogram off the edges
        for j in range(d):
            v = x[:, j, t * m:(t + 1) * m].ravel()
            assert np.array_equal(host[t, j], np.histogram(v, bins=64, range=(-1.0, 1.0))[0])
    # stats() against the rule restated in numpy, on the counts kept
    st, counts = axes.stats(), axes.marg_counts.cpu().numpy()
    edges = np.linspace(-1.0, 1.0, 65)
    assert np.array_equal(st["marginal_edges"].cpu().numpy(), edges) and "step_density" not in st
    got = st["marginal_quantiles"].cpu().numpy()
    for t in range(M):
        for j in range(d):
            ref = [mc.quantile_rule(counts[t, j], edges, q) for q in diagnostics.MARGINAL_QUANTILES]
            assert np.all(np.abs(got[t, j] - ref) <= 1e-12 * np.abs(ref))
    q90 = axes.quantile(0.9).cpu().numpy()
    assert abs(q90[0, 0] - mc.quantile_rule(counts[0, 0], edges, 0.9)) <= 1e-12
    dens = st["marginal_density"].cpu().numpy()
    assert np.allclose((dens * (2 / 64)).sum(-1), 1.0, rtol=1e-14)
    # what marginals must not change: every accumulator of the plain summary, bit for bit
    plain = build()
    base = plain.summarize(N_SAMPLES, burnin=BURNIN, thin=THIN, **ex)
    assert base.marg_counts is None and not {"marginal_edges", "marginal_quantiles"} & set(base.stats())
    assert torch.equal(axes.acc, base.acc) and torch.equal(axes.chain_sum, base.chain_sum)
    _same_chains(plain, twin)


@pytest.mark.parametrize("which", ["bingham_fast", "tempered"])
def test_every_other_accumulator_is_untouched(which):
    """lags, log_prob, mixing (and log_z along the ladder) with and without marginals=: the same ring, the same bits."""
    build, M, m, d, own = _make(which)
    kw = dict(lags=4, log_prob=True, mixing=True, window=7)
    if which == "tempered":
        kw.update(exchange=dict(ladder=3, every=2), log_z=True)
    a, b = build(), build()
    with_m = a.summarize(N_SAMPLES, burnin=BURNIN, thin=THIN, marginals=dict(bins=64, directions=own, steps=True), **kw)
    without = b.summarize(N_SAMPLES, burnin=BURNIN, thin=THIN, **kw)
    for key in ("acc", "chain_sum", "lp_acc", "lp_chain_sum", "lp_best", "x_best", "acov", "lp_acov", "hist", "lp_hist", "mix_step",
                "mix_counts", "ladder_acc"):
        u, v = getattr(with_m, key), getattr(without, key)
        assert (u is None and v is None) or torch.equal(u, v), key
    _same_chains(a, b)
    assert with_m.marg_counts is not None and without.marg_counts is None
    st = with_m.stats()
    assert {"acf", "lp_mean", "geodesic_step", "marginal_quantiles", "step_quantiles"} <= set(st)
    # the step series agrees with the mixing fold's count of pairs
    assert torch.equal(with_m.marg_counts[:, own.shape[1]].sum(-1), with_m.mix_counts[:, 1])

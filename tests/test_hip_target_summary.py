"""Sampler.summarize on the device: the per-target accumulators of a run against the stored draws of an identically seeded twin
(the chains are the same bit for bit, so only the summation differs: |got - ref| <= 2 N u sum|term|, N = m R draws per target,
u = 2^-53, the reference a numpy longdouble sum -- the bound of tests/test_hip_target_moments.py), the sampler's state and
accounting against the twin's, and one physical check on a single von Mises-Fisher target."""
import warnings

import numpy as np
import pytest
import torch

import geosss_amd as gs
from geosss_amd import diagnostics

pytestmark = pytest.mark.gpu
U = 2.0 ** -53
SEED = 977
N_SAMPLES, BURNIN, THIN = 40, 10, 2


def _x0(d, n, seed=5):
    x = np.random.default_rng(seed).standard_normal((n, d))
    return x / np.linalg.norm(x, axis=1, keepdims=True)


def _batch(which):
    """(members, m, mode)"""
    g = np.random.default_rng(11)
    if which == "bingham_d5_m24":         # the shared-workgroup layout of the fast kernels
        return [gs.random_bingham(5, vmax=20.0, vmin=0.0, seed=int(g.integers(1 << 30))) for _ in range(6)], 24, "fast"
    if which == "vmfmix_d3_m256":         # one target per workgroup
        out = []
        for _ in range(3):
            mu = g.standard_normal((2, 3))
            mu *= (10.0 + 30.0 * g.random((2, 1))) / np.linalg.norm(mu, axis=1, keepdims=True)
            out.append(gs.MixtureModel([gs.VonMisesFisher(v) for v in mu], g.random(2) + 0.5))
        return out, 256, "fast"
    if which == "binghamfisher_d17_m8":   # no batch fast kernel at d = 17: mode "auto" runs the exact kernels and says so
        return [gs.BinghamFisher(gs.random_bingham(17, vmax=20.0, vmin=0.0, seed=int(g.integers(1 << 30))).A,
                                 3.0 * g.standard_normal(17)) for _ in range(4)], 8, "auto"
    if which == "vmfmix_d130_m7":         # exact mode in a sixty-four-lane layout (coop64x4), a ragged workgroup per target
        out = []
        for _ in range(4):
            mu = g.standard_normal((2, 130))
            mu *= (10.0 + 30.0 * g.random((2, 1))) / np.linalg.norm(mu, axis=1, keepdims=True)
            out.append(gs.MixtureModel([gs.VonMisesFisher(v) for v in mu], g.random(2) + 0.5))
        return out, 7, "auto"
    raise KeyError(which)


def _sampler(pdfs, m, mode, x0, t0=0, t1=None):
    t1 = len(pdfs) if t1 is None else t1
    with warnings.catch_warnings(record=True):
        warnings.simplefilter("always")
        return gs.ShrinkageSphericalSliceSampler(gs.TargetBatch(pdfs), x0[t0 * m:t1 * m], SEED, mode=mode, chain_offset=t0 * m,
                                                 chains_per_target=m)


def _reference(x, m, full):
    """x (R, d, n) -> per target: sums (M, d + T), sums of |term|; per chain: sums (d, n), sums of |term|; in longdouble."""
    R, d, n = x.shape
    xl = x.astype(np.longdouble)
    pairs = [(i, j) for i in range(d) for j in range(i, d)] if full else [(i, i) for i in range(d)]
    cols = [xl[:, j] for j in range(d)] + [xl[:, i] * xl[:, j] for i, j in pairs]
    ref = np.stack([c.reshape(R, n // m, m).sum((0, 2)) for c in cols], 1)
    mag = np.stack([np.abs(c).reshape(R, n // m, m).sum((0, 2)) for c in cols], 1)
    return ref, mag, xl.sum(0), np.abs(xl).sum(0)


def _within(tm, ref, mag, cref, cmag, m, R, what, targets=slice(None)):
    acc, cs = tm.acc.cpu().numpy(), tm.chain_sum.cpu().numpy()
    assert np.all(acc[:, 0] == m * R), what
    err = np.abs(acc[:, 1:].astype(np.longdouble) - ref[targets])
    bound = 2 * m * R * U * mag[targets]
    print(f"{what}: max |err| / bound = {float(np.max(err / bound)):.3g}")
    assert np.all(err <= bound), (what, float(np.max(err / bound)))
    chains = slice(None) if targets == slice(None) else slice(targets.start * m, targets.stop * m)
    assert np.all(np.abs(cs.astype(np.longdouble) - cref[:, chains]) <= 2 * R * U * cmag[:, chains]), (what, "chain_sum")


@pytest.mark.parametrize("which", ["bingham_d5_m24", "vmfmix_d3_m256", "binghamfisher_d17_m8", "vmfmix_d130_m7"])
def test_summarize_is_the_stored_run_summed(which):
    pdfs, m, mode = _batch(which)
    M, d = len(pdfs), pdfs[0].d
    full = d <= 16
    x0 = _x0(d, M * m)
    twin = _sampler(pdfs, m, mode, x0)
    assert twin.mode == ("exact" if which in ("binghamfisher_d17_m8", "vmfmix_d130_m7") else "fast")
    draws = twin.sample(N_SAMPLES, burnin=BURNIN, thin=THIN, as_tensor=True)          # (n, R, d)
    ref, mag, cref, cmag = _reference(draws.permute(1, 2, 0).cpu().numpy(), m, full)

    s = _sampler(pdfs, m, mode, x0)
    tm = s.summarize(N_SAMPLES, burnin=BURNIN, thin=THIN, window=7)
    assert tm.n_targets == M and tm.d == d and tm.chains_per_target == m and tm.second_moment == full
    _within(tm, ref, mag, cref, cmag, m, N_SAMPLES, "window 7")
    # the sampler is where the equivalent advance calls leave it
    assert torch.equal(s.state_rows(), twin.state_rows())
    assert s._step == twin._step == BURNIN + (N_SAMPLES - 1) * THIN
    assert s._tries_reported == twin._tries_reported
    assert np.array_equal(s.n_tries_per_chain, twin.n_tries_per_chain)
    assert np.array_equal(s.n_reject_per_chain, twin.n_reject_per_chain)
    # one window for all rows
    _within(_sampler(pdfs, m, mode, x0).summarize(N_SAMPLES, burnin=BURNIN, thin=THIN, window=N_SAMPLES), ref, mag, cref, cmag, m,
            N_SAMPLES, "window 40")
    # a sampler on the targets from the third on (two of them where the batch has four) summarises them as its rows 0 ..
    t1 = min(M, 4)
    part = _sampler(pdfs, m, mode, x0, 2, t1).summarize(N_SAMPLES, burnin=BURNIN, thin=THIN, window=7, chains_per_target=m)
    assert part.n_targets == t1 - 2
    _within(part, ref, mag, cref, cmag, m, N_SAMPLES, "targets 2 ..", targets=slice(2, t1))
    # two half-length calls, the second continuing the first
    s2 = _sampler(pdfs, m, mode, x0)
    half = s2.summarize(N_SAMPLES // 2, burnin=BURNIN, thin=THIN, window=7)
    both = s2.summarize(N_SAMPLES // 2, burnin=THIN, thin=THIN, window=7, into=half)
    assert both is half
    _within(both, ref, mag, cref, cmag, m, N_SAMPLES, "into=")
    assert torch.equal(s2.state_rows(), twin.state_rows()) and s2._step == twin._step
    # the summaries themselves
    st = tm.stats()
    assert tuple(st["mean"].shape) == (M, d) and tuple(st["rhat"].shape) == (M, d) and tuple(st["ess_between"].shape) == (M, d)
    assert ("second_moment" in st) == full and bool(torch.isfinite(st["rhat"]).all())
    # (the sum's bound over N, and one rounding of the quotient)
    N = m * N_SAMPLES
    assert np.all(np.abs(st["mean"].cpu().numpy().astype(np.longdouble) - ref[:, :d] / N) <= 2 * U * mag[:, :d] + U)
    # running statistics still refuse a batch
    with pytest.raises(ValueError):
        s.enable_stats()


def test_summarize_is_the_public_functions_along_the_ring_plan():
    """Every feature at once, 23 draws in three calls chained with into= (windows cut by the ring's end, seams that carry
    history): the accumulators are, bit for bit, what target_moments, target_log_prob + scalar_moments + best_draw,
    target_autocov, target_mixing and target_ladder give on the stored draws of a twin, applied window by window as
    diagnostics.ring_plan cuts them, behind the same rows of history."""
    d, m, R, L, window = 3, 8, 2, 4, 5
    g = np.random.default_rng(23)
    base = []
    for _ in range(2):
        mu = g.standard_normal((2, d))
        mu *= (10.0 + 30.0 * g.random((2, 1))) / np.linalg.norm(mu, axis=1, keepdims=True)
        base.append(gs.MixtureModel([gs.VonMisesFisher(v) for v in mu], g.random(2) + 0.5))
    batch = gs.TargetBatch.tempered(base, [1.0, 0.5])
    M, n = len(batch), len(batch) * m
    assert M == 4 and batch.ladder == R
    hop, modes, weights = batch.mixing_directions()
    mix = dict(hop=hop, modes=modes, weights=weights, transitions=True)
    K = modes.shape[1]
    x0, ex, calls = _x0(d, n, seed=9), dict(ladder=R, every=2), (8, 8, 7)

    def make():
        return gs.ShrinkageSphericalSliceSampler(batch, x0, SEED, chains_per_target=m)
    twin = make()
    x = twin.sample(sum(calls), burnin=3, thin=2, as_tensor=True, exchange=ex).permute(1, 2, 0).contiguous()      # (23, d, n)

    s, tm = make(), None
    for i, n_samples in enumerate(calls):
        tm = s.summarize(n_samples, burnin=2 if i else 3, thin=2, window=window, lags=L, log_prob=True, mixing=mix, log_z=True,
                         exchange=ex, into=tm)

    def zeros(*shape, dtype=torch.float64):
        return torch.zeros(shape, dtype=dtype, device="cuda")
    acc, chain_sum, lp_acc, lp_chain_sum = zeros(M, 1 + d + d * (d + 1) // 2), zeros(d, n), zeros(M, 3), zeros(n)
    lp_best, x_best = torch.full((M,), float("-inf"), dtype=torch.float64, device="cuda"), zeros(M, d)
    acov, lp_acov, step = zeros(M, d, L + 1, 3), zeros(M, 1, L + 1, 3), zeros(M, 2)
    counts, ladder_acc = zeros(M, 3 + K + K * K, dtype=torch.int64), zeros(M // R, R - 1, m, diagnostics.LADDER_SLOTS)
    lp_all = zeros(sum(calls), n)
    at, cut_by_the_end = 0, 0
    for n_samples in calls:
        rows, draw0, windows, keep = diagnostics.ring_plan(n_samples - 1, window, L, min(L, at))
        assert rows == L + window and draw0 == (min(L, at), 1, min(L, at))
        for first, w, h in [draw0] + windows:
            cut_by_the_end += first + w == rows and w < window
            xw = x[at:at + w]
            diagnostics.target_moments(xw, m, acc=acc, chain_sum=chain_sum)
            lp = lp_all[at:at + w] = diagnostics.target_log_prob(batch, xw)
            diagnostics.scalar_moments(lp, m, acc=lp_acc, chain_sum=lp_chain_sum)
            best, row, chain = diagnostics.best_draw(lp, m)
            better = best > lp_best                                   # (strictly: the earliest of equal draws stays)
            lp_best, x_best = torch.where(better, best, lp_best), torch.where(better[:, None], xw[row, :, chain], x_best)
            diagnostics.target_autocov(xw, m, L, acc=acov, hist=x[at - h:at])
            diagnostics.target_autocov(lp, m, L, acc=lp_acov, hist=lp_all[at - h:at])
            diagnostics.target_mixing(xw, m, hop=hop, modes=modes, transitions=True, step=step, counts=counts,
                                      hist=x[at - min(1, h):at])
            diagnostics.target_ladder(batch, xw, R, acc=ladder_acc)
            at += w
    assert at == sum(calls) and cut_by_the_end >= 2
    for name, want in (("acc", acc), ("chain_sum", chain_sum), ("lp_acc", lp_acc), ("lp_chain_sum", lp_chain_sum),
                       ("lp_best", lp_best), ("x_best", x_best), ("mix_counts", counts), ("ladder_acc", ladder_acc),
                       ("hist", x[-L:]), ("lp_hist", lp_all[-L:, None, :]), ("acov", acov), ("lp_acov", lp_acov),
                       ("mix_step", step)):
        got = getattr(tm, name)
        differ = int((got != want).sum())
        print(f"{name}: {differ} of {want.numel()} entries differ")
        assert got.shape == want.shape and got.dtype == want.dtype and torch.equal(got, want), name
    assert float(acc[:, 0].min()) == m * sum(calls) and int(counts[:, 1].min()) == m * (sum(calls) - 1)
    assert torch.equal(s.state_rows(), twin.state_rows()) and s._step == twin._step == 3 + 2 * (sum(calls) - 1)


def test_pooled_vmf_mean_and_rhat():
    """One von Mises-Fisher target, kappa = 20 on S^2, 4096 chains pooled: E[x . mu / kappa] = coth kappa - 1 / kappa.  The
    standard error is the summary's own: sqrt(between / chains), the variance of the chain means over the number of chains."""
    kappa, n = 20.0, 4096
    pdf = gs.VonMisesFisher(kappa * np.eye(3)[2])
    s = gs.ShrinkageSphericalSliceSampler(pdf, _x0(3, n, seed=8), SEED)
    tm = s.summarize(50, burnin=200, thin=5)
    assert tm.n_targets == 1 and tm.chains_per_target == n
    st = tm.stats()
    assert float(st["n"][0]) == 50 * n
    want = 1.0 / np.tanh(kappa) - 1.0 / kappa
    se = float(torch.sqrt(st["between"][0, 2] / n))
    got = float(st["mean"][0, 2])
    print(f"mean . mu / kappa = {got:.6f}, coth k - 1/k = {want:.6f}, se = {se:.2e}")
    assert se > 0 and abs(got - want) <= 5 * se
    rhat = st["rhat"][0]
    assert bool(torch.isfinite(rhat).all()) and float(rhat.max()) < 1.1

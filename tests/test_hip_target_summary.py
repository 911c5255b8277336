"""Sampler.summarize on the device: the per-target accumulators of a run against the stored draws of an identically seeded twin
(the chains are the same bit for bit, so only the summation differs: |got - ref| <= 2 N u sum|term|, N = m R draws per target,
u = 2^-53, the reference a numpy longdouble sum -- the bound of tests/test_hip_target_moments.py), the sampler's state and
accounting against the twin's, and one physical check on a single von Mises-Fisher target."""
import warnings

import numpy as np
import pytest
import torch

import geosss_amd as gs

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

"""gsss_target_autocov and summarize(lags=) on the device.

The accumulators are held to an independent reference: seeded series from numpy (not from the sampler), the sums
C_l = sum x_r x_{r-l}, P_l = sum x_r, Q_l = sum x_{r-l} over a target's chains and the rows r >= l in numpy longdouble.

Tolerance, derived: a sum of k terms in ANY order obeys |err| <= (k - 1) u sum|term| (1 + O(k u)), u = 2^-53, and a product
formed by a fused multiply-add adds no rounding of its own, so every entry must satisfy |got - ref| <= k 2^-52 sum|term| with
k = m max(R - l, 0) the number of its terms (sum|term| from the reference); an entry without terms is exactly 0.  A pair dropped
or counted twice at a window's edge misses that by orders of magnitude: the series are centred near 3, every term is of size 9.
Inputs lie inside NaN-filled allocations: a read outside the block and its history shows as NaN."""
import warnings

import numpy as np
import pytest
import torch

import geosss_amd as gs
from geosss_amd import diagnostics

pytestmark = pytest.mark.gpu
EPS = 2.0 ** -52
SEED = 977

# (M, m, d, L, R): every m with two d and two L at least; every L >= 2 with R < L; the lag counts on both sides of a change of
# kernel (8 | 9, 16 | 17, 32 | 33); R = 130 where the few chains make the launcher split the rows over workgroups as well
CASES = [
    (1, 1, 1, 1, 1), (1, 1, 3, 7, 50), (1, 1, 5, 33, 130),
    (5, 1, 5, 2, 1), (5, 1, 16, 32, 33), (5, 1, 1, 64, 50), (5, 1, 3, 8, 50), (5, 1, 1, 7, 130),
    (7, 3, 3, 7, 7), (7, 3, 40, 64, 1), (7, 3, 5, 1, 2), (7, 3, 5, 9, 50),
    (3, 16, 5, 32, 50), (3, 16, 1, 2, 3), (3, 16, 16, 7, 1), (3, 16, 3, 16, 50), (3, 16, 5, 32, 130),
    (4, 64, 3, 64, 65), (4, 64, 5, 7, 8), (4, 64, 1, 32, 1), (4, 64, 3, 17, 50),
    (3, 100, 16, 2, 2), (3, 100, 3, 32, 32), (3, 100, 5, 64, 50), (3, 100, 1, 33, 50),
    (2, 300, 1, 7, 50), (2, 300, 5, 64, 64), (2, 300, 40, 1, 1), (2, 300, 3, 64, 130),
    (1, 1000, 3, 2, 50), (1, 1000, 5, 32, 1), (1, 1000, 1, 64, 1),
]


def _series(R, d, n, seed):
    g = np.random.default_rng(seed)
    return 3.0 + g.standard_normal((R, d, n))


def _reference(x, m, L):
    """x (R, d, n) -> (sums (M, d, L + 1, 3), sums of |term| likewise, terms per lag (L + 1,)) in longdouble."""
    R, d, n = x.shape
    M = n // m
    xl = x.astype(np.longdouble).reshape(R, d, M, m)
    ref = np.zeros((M, d, L + 1, 3), dtype=np.longdouble)
    mag = np.zeros_like(ref)
    for lag in range(min(L, R - 1) + 1):
        for c, v in enumerate((xl[lag:] * xl[:R - lag], xl[lag:], xl[:R - lag])):
            ref[:, :, lag, c] = v.sum((0, 3)).T
            mag[:, :, lag, c] = np.abs(v).sum((0, 3)).T
    return ref, mag, m * np.maximum(R - np.arange(L + 1), 0)


def _check(acc, ref, mag, k, what):
    acc = acc.cpu().numpy()
    assert acc.shape == ref.shape, what
    err = np.abs(acc.astype(np.longdouble) - ref)
    bound = k[None, None, :, None] * EPS * mag
    worst = float(np.max(np.where(bound > 0, err / np.where(bound > 0, bound, 1), 0)))
    print(f"{what}: max |err| / bound = {worst:.3g}")
    assert np.all(np.isfinite(acc)) and np.all(err <= bound), (what, worst)


def _embed(x):
    """The block as a view of rows inside a larger NaN-filled allocation."""
    R = x.shape[0]
    big = torch.full((R + 4,) + tuple(x.shape[1:]), float("nan"), dtype=torch.float64, device="cuda")
    big[2:2 + R] = torch.from_numpy(x).cuda()
    return big[2:2 + R]


@pytest.mark.parametrize("M, m, d, L, R", CASES)
def test_accumulators_against_longdouble(M, m, d, L, R):
    x = _series(R, d, M * m, seed=100000 * d + 1000 * L + m + R)
    ref, mag, k = _reference(x, m, L)
    view = _embed(x)
    acc = diagnostics.target_autocov(view, m, L)
    assert tuple(acc.shape) == (M, d, L + 1, 3)
    _check(acc, ref, mag, k, "one call")
    # the same call again: the same bits (no atomics, a fixed summation order)
    assert torch.equal(acc, diagnostics.target_autocov(view, m, L))
    # a scalar series is the case d = 1
    if d == 1:
        assert torch.equal(acc, diagnostics.target_autocov(view[:, 0], m, L))
    # two calls, the second with the first's last rows as its history
    if R >= 2:
        h = R // 2
        acc2 = diagnostics.target_autocov(view[:h], m, L)
        acc2 = diagnostics.target_autocov(view[h:], m, L, acc=acc2, hist=view[max(0, h - L):h])
        _check(acc2, ref, mag, k, "two halves")


def _stream(x, m, L, window):
    """The series fed in windows through a NaN-filled ring of L + window rows the way summarize lays them: one behind the other,
    cut where the ring ends, the history never copied."""
    n_draws, d, n = x.shape
    rows = L + window
    ring = torch.full((rows, d, n), float("nan"), dtype=torch.float64, device="cuda")
    xt = torch.from_numpy(x).cuda()
    acc = torch.zeros((n // m, d, L + 1, 3), dtype=torch.float64, device="cuda")
    pos = done = wraps = 0
    while done < n_draws:
        pos %= rows
        w = min(window, n_draws - done, rows - pos)
        wraps += pos == 0 and done > 0
        ring[pos:pos + w] = xt[done:done + w]
        diagnostics._autocov_fold(ring, pos, w, min(L, done), m, L, acc)
        pos, done = pos + w, done + w
    assert wraps >= 1
    return acc


@pytest.mark.parametrize("M, m, d, L", [(7, 3, 5, 2), (3, 16, 5, 7), (2, 300, 3, 32), (5, 1, 1, 64), (4, 64, 3, 17)])
def test_streaming_through_a_ring(M, m, d, L):
    n_draws = 2 * L + 23
    x = _series(n_draws, d, M * m, seed=7 * L + m)
    ref, mag, k = _reference(x, m, L)
    _check(diagnostics.target_autocov(_embed(x), m, L), ref, mag, k, "one piece")
    for window in sorted({1, 3, max(1, L - 1), L + 5}):
        _check(_stream(x, m, L, window), ref, mag, k, f"windows of {window}")


# ---------------------------------------------------------------------------------------------------------------------------
# summarize(lags=L) against the stored run of an identically seeded twin

N_SAMPLES, BURNIN, THIN, LAGS = 40, 10, 2, 7


def _x0(d, n, seed=5):
    x = np.random.default_rng(seed).standard_normal((n, d))
    return x / np.linalg.norm(x, axis=1, keepdims=True)


def _targets(which):
    """(members, m, mode)"""
    g = np.random.default_rng(11)
    if which == "bingham_d5_m16":          # the packed layout of the fast kernels
        return [gs.random_bingham(5, vmax=20.0, vmin=0.0, seed=int(g.integers(1 << 30))) for _ in range(6)], 16, "fast"
    if which in ("vmfmix_d3_m8", "vmfmix_d3_m1"):
        out = []
        for _ in range(3 if which == "vmfmix_d3_m8" else 5):
            mu = g.standard_normal((2, 3))
            mu *= (10.0 + 30.0 * g.random((2, 1))) / np.linalg.norm(mu, axis=1, keepdims=True)
            out.append(gs.MixtureModel([gs.VonMisesFisher(v) for v in mu], g.random(2) + 0.5))
        return out, (8 if which == "vmfmix_d3_m8" else 1), "exact"
    if which == "vmfmix_d130_m7":          # tests/test_hip_target_summary.py's: a sixty-four-lane layout, a ragged workgroup per target
        out = []
        for _ in range(4):
            mu = g.standard_normal((2, 130))
            mu *= (10.0 + 30.0 * g.random((2, 1))) / np.linalg.norm(mu, axis=1, keepdims=True)
            out.append(gs.MixtureModel([gs.VonMisesFisher(v) for v in mu], g.random(2) + 0.5))
        return out, 7, "exact"
    raise KeyError(which)


LAGS_OF = {"vmfmix_d130_m7": 4}   # every other case runs LAGS


def _sampler(pdfs, m, mode, x0):
    with warnings.catch_warnings(record=True):
        warnings.simplefilter("always")
        return gs.ShrinkageSphericalSliceSampler(gs.TargetBatch(pdfs), x0, SEED, mode=mode, chains_per_target=m)


def _acf_reference(x, m, L):
    """x (R, d, n) -> (acf (M, d, L + 1) by the estimator of from_target_autocov in longdouble, its tolerance (M, d, 1))."""
    R = x.shape[0]
    ref, _, k = _reference(x, m, L)
    c, p, q = ref[..., 0], ref[..., 1], ref[..., 2]
    mu = p[..., :1] / (m * R)
    cov = (c - mu * (p + q)) / k + mu * mu
    assert np.all(cov[..., 0] >= 1e-3)
    # every covariance is a difference of terms of the size of E[x^2], each summed over k <= m R terms
    tol = 8 * m * R * EPS * (c[..., :1] / (m * R)) / cov[..., :1]
    return cov / cov[..., :1], tol


def _acf_within(got, x, m, L, what):
    want, tol = _acf_reference(x, m, L)
    err = np.abs(got.cpu().numpy().astype(np.longdouble) - want)
    print(f"{what}: max |err| / tol = {float(np.max(err / tol)):.3g}")
    assert np.all(err <= tol), (what, float(np.max(err / tol)))


@pytest.mark.parametrize("which", ["bingham_d5_m16", "vmfmix_d3_m8", "vmfmix_d3_m1", "vmfmix_d130_m7"])
def test_summarize_lags_is_the_stored_run(which):
    _summarize_lags_is_the_stored_run(which, LAGS_OF.get(which, LAGS))


def _summarize_lags_is_the_stored_run(which, LAGS):
    pdfs, m, mode = _targets(which)
    M, d = len(pdfs), pdfs[0].d
    x0 = _x0(d, M * m)
    twin = _sampler(pdfs, m, mode, x0)
    assert twin.mode == mode
    draws = twin.sample(N_SAMPLES, burnin=BURNIN, thin=THIN, as_tensor=True)            # (n, R, d)
    x = draws.permute(1, 2, 0).cpu().numpy()
    ref, mag, k = _reference(x, m, LAGS)
    lp = diagnostics.target_log_prob(gs.TargetBatch(pdfs), draws, chain_major=True).t().cpu().numpy()[:, None, :]   # (R, 1, n)
    lp_ref, lp_mag, _ = _reference(lp, m, LAGS)

    s = _sampler(pdfs, m, mode, x0)
    tm = s.summarize(N_SAMPLES, burnin=BURNIN, thin=THIN, window=7, lags=LAGS, log_prob=True)
    assert tm.lags == LAGS and tuple(tm.hist.shape) == (LAGS, d, M * m) and tuple(tm.lp_hist.shape) == (LAGS, 1, M * m)
    _check(tm.acov, ref, mag, k, "acov, window 7")
    _check(tm.lp_acov, lp_ref, lp_mag, k, "lp_acov, window 7")
    assert np.array_equal(tm.hist.cpu().numpy(), x[-LAGS:])
    st = tm.stats()
    assert tuple(st["acf"].shape) == (M, d, LAGS + 1) and tuple(st["lp_acf"].shape) == (M, LAGS + 1)
    for key in ("iat", "ess_within", "iat_truncated"):
        assert tuple(st[key].shape) == (M, d) and tuple(st["lp_" + key].shape) == (M,)
    _acf_within(st["acf"], x, m, LAGS, "acf")
    _acf_within(st["lp_acf"][:, None, :], lp, m, LAGS, "lp_acf")
    assert torch.allclose(st["ess_within"], m * N_SAMPLES / st["iat"], rtol=4 * EPS, atol=0)
    if m == 1:      # the chains' own diagnostics.acf
        own = diagnostics.acf(draws.permute(0, 2, 1).contiguous(), n_max=LAGS + 1)           # (n, d, L + 1)
        _, tol = _acf_reference(x, m, LAGS)
        assert np.all(np.abs((st["acf"] - own).cpu().numpy()) <= tol)
        assert torch.allclose(st["iat"], diagnostics.iat_from_acf(own), rtol=1e-9, atol=0)

    # What lags must not change: the moments, R-hat, the chains and their accounting.  (The default window: the ring of
    # L + window rows cuts a window of 7 where the plain buffer does not, and per-window partial sums are added.)
    plain, s1 = _sampler(pdfs, m, mode, x0), _sampler(pdfs, m, mode, x0)
    base = plain.summarize(N_SAMPLES, burnin=BURNIN, thin=THIN, log_prob=True)
    tm1 = s1.summarize(N_SAMPLES, burnin=BURNIN, thin=THIN, log_prob=True, lags=LAGS)
    _check(tm1.acov, ref, mag, k, "default window")
    assert base.lags is None and base.acov is None and "acf" not in base.stats()
    assert torch.equal(tm1.acc, base.acc) and torch.equal(tm1.chain_sum, base.chain_sum) and torch.equal(tm1.lp_acc, base.lp_acc)
    assert torch.equal(tm1.stats()["rhat"], base.stats()["rhat"]) or m == 1             # (one chain: NaN on both sides)
    for other in (s1, s):
        assert torch.equal(other.state_rows(), plain.state_rows()) and torch.equal(other.state_rows(), twin.state_rows())
        assert other._step == plain._step == twin._step
        assert np.array_equal(other.n_reject_per_chain, plain.n_reject_per_chain)
        assert np.array_equal(other.n_tries_per_chain, plain.n_tries_per_chain)

    # two half-length calls of which the second continues the first
    s2 = _sampler(pdfs, m, mode, x0)
    half = s2.summarize(N_SAMPLES // 2, burnin=BURNIN, thin=THIN, window=5, lags=LAGS, log_prob=True)
    both = s2.summarize(N_SAMPLES // 2, burnin=THIN, thin=THIN, window=5, into=half)
    assert both is half and both.lags == LAGS
    _check(both.acov, ref, mag, k, "into=")
    _check(both.lp_acov, lp_ref, lp_mag, k, "into=, lp")
    assert torch.equal(s2.state_rows(), twin.state_rows())

    # refusals
    with pytest.raises(ValueError):
        _sampler(pdfs, m, mode, x0).summarize(N_SAMPLES, lags=LAGS, into=base)          # begun without lags
    with pytest.raises(ValueError):
        _sampler(pdfs, m, mode, x0).summarize(LAGS, lags=LAGS)                          # n_samples <= lags
    with pytest.raises(ValueError):
        _sampler(pdfs, m, mode, x0).summarize(N_SAMPLES, lags=65)


def test_single_target_with_chains_per_target():
    n, m, d = 64, 16, 3
    pdf = gs.VonMisesFisher(20.0 * np.eye(3)[2])
    x0 = _x0(d, n, seed=8)
    draws = gs.ShrinkageSphericalSliceSampler(pdf, x0, SEED).sample(N_SAMPLES, burnin=BURNIN, as_tensor=True)
    x = draws.permute(1, 2, 0).cpu().numpy()
    ref, mag, k = _reference(x, m, LAGS)
    s = gs.ShrinkageSphericalSliceSampler(pdf, x0, SEED)
    tm = s.summarize(N_SAMPLES, burnin=BURNIN, chains_per_target=m, lags=LAGS)
    assert tm.n_targets == n // m and tm.lp_acov is None
    _check(tm.acov, ref, mag, k, "single target")
    st = tm.stats()
    _acf_within(st["acf"], x, m, LAGS, "acf, single target")
    assert "lp_acf" not in st and bool(torch.isfinite(st["ess_within"]).all())
    # the MH baseline keeps refusing summarize
    with pytest.raises(ValueError):
        gs.MetropolisHastings(pdf, x0, SEED).summarize(N_SAMPLES, lags=LAGS)

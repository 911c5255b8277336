"""gsss_target_mixing and summarize(mixing=) on the device.

The accumulators are held to an independent reference: seeded random walks on the sphere from numpy (not from the sampler),
every target with its own seeded directions, the sums and counts in numpy longdouble from the stored series.

Counters must be EQUAL.  The case builder asserts, on the CPU, that every |x . h| and every gap between the largest and the
second-largest x . mode_k is at least 2^-40 -- far above the d 2^-52 by which a double-precision product of unit vectors can
move -- so the sign and the argmax are the same in double and in longdouble.

Tolerance of step = (sum theta, sum theta^2), derived.  The device's product x_r . x_{r-1} is a chain of d fused multiply-adds:
it lies within delta = (d + 1) 2^-52 of the exact one.  acos has the slope 1 / sin(theta), so theta moves by
b_r = delta / sin(theta_r) where sin(theta_r) >= 2 sqrt(delta), and by at most 3 sqrt(delta) otherwise (acos is Hoelder-1/2 at
+-1); the device's acos is allowed 4 ulp of pi on top (an assumption).  A sum of k terms in ANY order errs by at most
k 2^-52 sum|term|.  So |got - ref| <= sum_r b_r + k 2^-52 sum theta_r, and for theta^2 the same with (2 theta_r + b_r) b_r.
The series carry exact repeats (theta = 0, a product that may round above 1) and antipodal rows (theta = pi).
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
LD = np.longdouble

# (M, m, rows): many targets per workgroup with a per-lane LDS base and the LDS budget | 64 does not divide m, the segmented
# reduction | a wavefront is a target | a target spans two workgroups, ragged | rows split over workgroups, workspace and fold
SHAPES = [(300, 1, 9), (7, 5, 40), (3, 64, 40), (3, 259, 40), (1, 4096, 70)]
DIMS = [2, 3, 16, 17, 40]          # 17 and 40: the build with a run-time d
MODES = [0, 1, 3, 16]


def _cases():
    """Every shape with every d; K and the transitions thinned so that every pair of values of any two axes still meets."""
    out = []
    for i, shape in enumerate(SHAPES):
        for j, d in enumerate(DIMS):
            out.append(shape + (d, MODES[(i + j) % 4], bool((i + 2 * j + (i + j) // 4) % 2)))
    out += [(300, 1, 9, 16, 16, False), (1, 4096, 70, 3, 0, True), (7, 5, 40, 2, 16, True), (3, 64, 40, 17, 3, False),
            (3, 259, 40, 40, 3, False)]
    out.append((7, 5, 40, 400, 16, True))     # one target's directions exceed the LDS budget: read from global memory
    axes = [[c[:3] for c in out], [c[3] for c in out], [c[4] for c in out], [c[5] for c in out]]
    for a in range(4):
        for b in range(a + 1, 4):
            have = set(zip(axes[a], axes[b]))
            assert all((u, v) in have for u in set(axes[a]) for v in set(axes[b]) if 400 not in (u, v)), (a, b)   # (400: extra)
    return out


def _walk(rows, d, n, seed):
    """(rows, d, n): random walks with steps log-uniform in 1e-4 .. pi; two rows repeat the row before exactly, two are its
    antipode."""
    g = np.random.default_rng(seed)
    special = g.permutation(np.arange(1, rows))[:4] if rows >= 5 else []
    repeat, anti = set(special[:2]), set(special[2:])
    x = np.empty((rows, n, d))
    x[0] = g.standard_normal((n, d))
    x[0] /= np.linalg.norm(x[0], axis=1, keepdims=True)
    for r in range(1, rows):
        t = g.standard_normal((n, d))
        t -= (t * x[r - 1]).sum(1, keepdims=True) * x[r - 1]
        t /= np.linalg.norm(t, axis=1, keepdims=True)
        th = np.exp(g.uniform(np.log(1e-4), np.log(np.pi), (n, 1)))
        step = np.cos(th) * x[r - 1] + np.sin(th) * t
        step /= np.linalg.norm(step, axis=1, keepdims=True)
        x[r] = x[r - 1] if r in repeat else (-x[r - 1] if r in anti else step)
    return np.ascontiguousarray(x.transpose(0, 2, 1))


def _directions(M, K, d, seed):
    g = np.random.default_rng(seed)
    v = g.standard_normal((M, 1 + K, d))
    v /= np.linalg.norm(v, axis=-1, keepdims=True)
    return v[:, 0].copy(), v[:, 1:].copy()


class Reference:
    """Of a stored series x (R, d, n), target t owning the chains [t m, (t + 1) m), against hop (M, d) and modes (M, K, d), in
    longdouble: step (M, 2), counts (M, 3 + K [+ K K]), bound (M, 2) (the module's docstring) and sum_bound (M, 2), its
    summation part alone -- what two device results over the same pairs may differ by."""

    def __init__(self, x, m, hop, modes, transitions):
        R, d, n = x.shape
        M, K = n // m, modes.shape[1]
        xl = x.astype(LD)
        hl = np.repeat(hop.astype(LD), m, axis=0)                                  # (n, d)
        ml = np.repeat(modes.astype(LD), m, axis=0)                                # (n, K, d)
        xh = np.einsum("rdn,nd->rn", xl, hl)
        self.margin = float(np.abs(xh).min()) if hop.any() else np.inf
        dot = (xl[1:] * xl[:-1]).sum(1)                                            # (R - 1, n)
        theta = np.arccos(np.clip(dot, LD(-1), LD(1)))
        sin = np.sqrt(np.maximum(1 - dot * dot, 0))
        delta = LD((d + 1) * EPS)
        b = np.where(sin >= 2 * np.sqrt(delta), delta / np.maximum(sin, 2 * np.sqrt(delta)), 3 * np.sqrt(delta)) + 4 * EPS * np.pi
        k = m * (R - 1)

        def per_target(v):
            return v.reshape(R - 1, M, m).sum((0, 2))
        self.step = np.stack([per_target(theta), per_target(theta * theta)], 1)
        self.sum_bound = k * EPS * self.step
        self.bound = np.stack([per_target(b), per_target((2 * theta + b) * b)], 1) + self.sum_bound
        self.pairs = k
        side = np.sign(xh)
        self.counts = np.zeros((M, 3 + K + (K * K if transitions else 0)), dtype=np.int64)
        self.counts[:, 0], self.counts[:, 1] = m * R, k
        self.counts[:, 2] = (side[1:] != side[:-1]).reshape(R - 1, M, m).sum((0, 2))
        if K:
            v = np.einsum("rdn,nkd->rnk", xl, ml)
            if K > 1:
                top = np.sort(v, -1)
                self.margin = min(self.margin, float((top[..., -1] - top[..., -2]).min()))
            mode = np.argmax(v, -1).reshape(R, M, m)
            for t in range(M):
                self.counts[t, 3:3 + K] = np.bincount(mode[:, t].ravel(), minlength=K)
                if transitions:
                    self.counts[t, 3 + K:] = np.bincount((mode[:-1, t] * K + mode[1:, t]).ravel(), minlength=K * K)
        # the condition on the inputs: signs and argmax are the same in double and in longdouble
        assert self.margin >= 2.0 ** -40, self.margin


def _check(step, counts, ref, what, bound=None):
    assert np.array_equal(counts.cpu().numpy(), ref.counts), what
    got = step.cpu().numpy()
    bound = ref.bound if bound is None else bound
    err = np.abs(got.astype(LD) - ref.step)
    worst = float(np.max(np.where(bound > 0, err / np.where(bound > 0, bound, 1), 0)))
    print(f"{what}: max |err| / bound = {worst:.3g}")
    assert np.all(np.isfinite(got)) and np.all(err <= bound), (what, worst)


def _embed(x):
    """The block as a view of rows inside a larger NaN-filled allocation."""
    R = x.shape[0]
    big = torch.full((R + 4,) + tuple(x.shape[1:]), float("nan"), dtype=torch.float64, device="cuda")
    big[2:2 + R] = torch.from_numpy(x).cuda()
    return big[2:2 + R]


@pytest.mark.parametrize("M, m, rows, d, K, transitions", _cases())
def test_accumulators_against_longdouble(M, m, rows, d, K, transitions):
    x = _walk(rows, d, M * m, seed=100000 * d + 1000 * K + m + rows)
    hop, modes = _directions(M, K, d, seed=31 * d + K + M)
    ref = Reference(x, m, hop, modes, transitions)
    view = _embed(x)
    step, counts = diagnostics.target_mixing(view, m, hop=hop, modes=modes, transitions=transitions)
    assert tuple(step.shape) == (M, 2) and tuple(counts.shape) == (M, 3 + K + (K * K if transitions else 0))
    assert counts.dtype == torch.int64
    _check(step, counts, ref, "one call")
    # the same call again: the same bits in step (a fixed summation order), the same counts
    again, counts2 = diagnostics.target_mixing(view, m, hop=hop, modes=modes, transitions=transitions)
    assert torch.equal(step, again) and torch.equal(counts, counts2)
    # accumulators are added to
    diagnostics.target_mixing(view, m, hop=hop, modes=modes, transitions=transitions, step=again, counts=counts2)
    assert torch.equal(counts2, 2 * counts) and torch.allclose(again, 2 * step, rtol=4 * EPS, atol=0)


def _stream(x, m, dirs, K, transitions, window):
    """The series fed in windows through a NaN-filled ring of 1 + window rows the way summarize lays them: one behind the other,
    cut where the ring ends, the history never copied."""
    n_draws, d, n = x.shape
    rows = 1 + window
    ring = torch.full((rows, d, n), float("nan"), dtype=torch.float64, device="cuda")
    xt = torch.from_numpy(x).cuda()
    step = torch.zeros((n // m, 2), dtype=torch.float64, device="cuda")
    counts = torch.zeros((n // m, 3 + K + (K * K if transitions else 0)), dtype=torch.int64, device="cuda")
    pos = done = wraps = 0
    while done < n_draws:
        pos %= rows
        w = min(window, n_draws - done, rows - pos)
        wraps += pos == 0 and done > 0
        ring[pos:pos + w] = xt[done:done + w]
        diagnostics._mixing_fold(ring, pos, w, min(1, done), m, dirs, K, transitions, step, counts)
        pos, done = pos + w, done + w
    assert wraps >= 1 or n_draws <= rows      # (the ring of 1 + (n - 1) rows holds the whole series)
    return step, counts


@pytest.mark.parametrize("M, m, rows, d, K", [(300, 1, 9, 3, 3), (7, 5, 40, 16, 16), (3, 259, 40, 17, 3), (1, 4096, 70, 5, 1)])
def test_blocks_and_streaming_through_a_ring(M, m, rows, d, K):
    x = _walk(rows, d, M * m, seed=7 * rows + m)
    hop, modes = _directions(M, K, d, seed=m + K)
    ref = Reference(x, m, hop, modes, True)
    view = _embed(x)
    one, counts = diagnostics.target_mixing(view, m, hop=hop, modes=modes, transitions=True)
    _check(one, counts, ref, "one call")

    def same_pairs(step, what):    # the same pairs in another order of summation
        assert np.all(np.abs((step - one).cpu().numpy()) <= ref.sum_bound.astype(np.float64)), what
    for j in sorted({1, rows // 2, rows - 1}):
        s, c = diagnostics.target_mixing(view[:j], m, hop=hop, modes=modes, transitions=True)
        s, c = diagnostics.target_mixing(view[j:], m, hop=hop, modes=modes, transitions=True, step=s, counts=c, hist=view[j - 1:j])
        _check(s, c, ref, f"two calls, cut at {j}")
        same_pairs(s, f"two calls, cut at {j}")
    dirs, _ = diagnostics._mixing_dirs(hop, modes, M, d, torch.device("cuda"))
    for window in (1, 3, rows - 1):
        s, c = _stream(x, m, dirs, K, True, window)
        _check(s, c, ref, f"windows of {window}")
        same_pairs(s, f"windows of {window}")


# ---------------------------------------------------------------------------------------------------------------------------
# summarize(mixing=) against the stored run of an identically seeded twin

N_SAMPLES, BURNIN, THIN = 40, 10, 2


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


def _targets(which):
    """(members, m, mode)"""
    if which == "vmfmix_d3_k3_m8":       # the packed layout of the fast kernels
        return _vmf_mixtures(6), 8, "fast"
    if which == "bingham_d5_m100":
        g = np.random.default_rng(12)
        return [gs.random_bingham(5, vmax=20.0, vmin=0.0, seed=int(g.integers(1 << 30))) for _ in range(4)], 100, "exact"
    raise KeyError(which)


def _sampler(pdfs, m, mode, x0, t0=0, t1=None):
    t1 = len(pdfs) if t1 is None else t1
    with warnings.catch_warnings(record=True):
        warnings.simplefilter("always")
        return gs.ShrinkageSphericalSliceSampler(gs.TargetBatch(pdfs), x0[t0 * m:t1 * m], SEED, mode=mode, chain_offset=t0 * m,
                                                 chains_per_target=m)


def _stored(sampler, n_samples=N_SAMPLES, burnin=BURNIN, thin=THIN):
    """-> (draws (n, R, d) on the device, x (R, d, n) numpy)"""
    draws = sampler.sample(n_samples, burnin=burnin, thin=thin, as_tensor=True)
    return draws, draws.permute(1, 2, 0).cpu().numpy()


@pytest.mark.parametrize("which", ["vmfmix_d3_k3_m8", "bingham_d5_m100"])
def test_summarize_mixing_is_the_stored_run(which):
    pdfs, m, mode = _targets(which)
    M, d = len(pdfs), pdfs[0].d
    batch = gs.TargetBatch(pdfs)
    hop, modes, weights = batch.mixing_directions()
    K = modes.shape[1]
    x0 = _x0(d, M * m)
    twin = _sampler(pdfs, m, mode, x0)
    assert twin.mode == mode
    draws, x = _stored(twin)
    ref = Reference(x, m, hop, modes, False)

    s = _sampler(pdfs, m, mode, x0)
    tm = s.summarize(N_SAMPLES, burnin=BURNIN, thin=THIN, mixing=True)
    assert tm.mix_modes == K and tm.lags is None and tm.acov is None and tuple(tm.hist.shape) == (1, d, M * m)
    assert (tm.mix_weights is None) == (weights is None)
    _check(tm.mix_step, tm.mix_counts, ref, "summarize")
    assert np.array_equal(tm.hist.cpu().numpy(), x[-1:])
    st = tm.stats()
    for key in ("geodesic_step", "geodesic_step_sd", "hop_frequency"):
        assert tuple(st[key].shape) == (M,)
    assert tuple(st["mode_occupancy"].shape) == (M, K) and ("mode_kl" in st) == (weights is not None)
    assert "acf" not in st and "mode_transitions" not in st
    # diagnostics.distance on the stored draws
    per = diagnostics.distance(draws[:, 1:], draws[:, :-1]).reshape(M, -1).mean(1)
    assert np.all(np.abs((st["geodesic_step"] - per).cpu().numpy()) <= 2 * ref.bound[:, 0].astype(np.float64) / ref.pairs + 8 * EPS * np.pi)
    hops = torch.stack([diagnostics.hopping_frequency(draws[t * m:(t + 1) * m], torch.from_numpy(hop[t]).cuda()).mean()
                        for t in range(M)])
    assert torch.allclose(st["hop_frequency"], hops, rtol=8 * EPS, atol=0)
    if K:
        occ = torch.stack([diagnostics.mode_occupancy(draws[t * m:(t + 1) * m], torch.from_numpy(modes[t]).cuda()) for t in range(M)])
        assert torch.allclose(st["mode_occupancy"], occ, rtol=4 * EPS, atol=0)      # (the counts are held to be equal above)
        for t in range(M):
            assert abs(float(st["mode_kl"][t]) - float(diagnostics.mode_kl(occ[t], torch.from_numpy(weights[t]).cuda()))) <= 1e-14

    # What mixing must not change: the chains, the final state, acc and chain_sum are those of the ring of lags=1.
    plain = _sampler(pdfs, m, mode, x0)
    base = plain.summarize(N_SAMPLES, burnin=BURNIN, thin=THIN, lags=1)
    assert base.mix_step is None and base.mix_counts is None
    assert torch.equal(tm.acc, base.acc) and torch.equal(tm.chain_sum, base.chain_sum)
    for other in (s, plain):
        assert torch.equal(other.state_rows(), twin.state_rows()) and other._step == twin._step
        assert np.array_equal(other.n_reject_per_chain, twin.n_reject_per_chain)
        assert np.array_equal(other.n_tries_per_chain, twin.n_tries_per_chain)

    # with lags and log_prob, in one call and in two of which the second continues the first
    mix = dict(hop=hop, modes=modes, weights=weights, transitions=True)
    reft = Reference(x, m, hop, modes, True)
    s1 = _sampler(pdfs, m, mode, x0)
    one = s1.summarize(N_SAMPLES, burnin=BURNIN, thin=THIN, window=7, lags=4, log_prob=True, mixing=mix)
    _check(one.mix_step, one.mix_counts, reft, "with lags and log_prob")
    assert ("mode_transitions" in one.stats()) == (K > 0) and "acf" in one.stats() and "lp_mean" in one.stats()
    s2 = _sampler(pdfs, m, mode, x0)
    half = s2.summarize(N_SAMPLES // 2, burnin=BURNIN, thin=THIN, window=5, lags=4, log_prob=True, mixing=mix)
    both = s2.summarize(N_SAMPLES // 2, burnin=THIN, thin=THIN, window=5, into=half)
    assert both is half and tuple(both.hist.shape) == (4, d, M * m)
    _check(both.mix_step, both.mix_counts, reft, "into=")
    assert torch.equal(both.mix_counts, one.mix_counts)
    assert np.all(np.abs((both.mix_step - one.mix_step).cpu().numpy()) <= reft.sum_bound.astype(np.float64))
    assert torch.equal(s2.state_rows(), twin.state_rows())
    # ... and without lags: the one history row carries the pair at the seam
    s3 = _sampler(pdfs, m, mode, x0)
    half = s3.summarize(N_SAMPLES // 2, burnin=BURNIN, thin=THIN, mixing=True)
    both = s3.summarize(N_SAMPLES // 2, burnin=THIN, thin=THIN, into=half)
    assert tuple(both.hist.shape) == (1, d, M * m)
    _check(both.mix_step, both.mix_counts, ref, "into=, no lags")

    # refusals
    with pytest.raises(ValueError, match="begun without mixing"):
        _sampler(pdfs, m, mode, x0).summarize(N_SAMPLES, mixing=True, into=base)
    with pytest.raises(ValueError):
        _sampler(pdfs, m, mode, x0).summarize(N_SAMPLES, mixing="yes")
    with pytest.raises(ValueError):
        _sampler(pdfs, m, mode, x0).summarize(N_SAMPLES, mixing=dict(hops=hop))


def test_a_sampler_on_a_run_of_targets_uses_their_directions():
    pdfs, m, mode = _vmf_mixtures(4, seed=21), 8, "exact"
    hop, modes, _ = gs.TargetBatch(pdfs).mixing_directions()
    x0 = _x0(3, 4 * m, seed=6)
    _, x = _stored(_sampler(pdfs, m, mode, x0, 1, 4))
    ref = Reference(x, m, hop[1:], modes[1:], False)
    tm = _sampler(pdfs, m, mode, x0, 1, 4).summarize(N_SAMPLES, burnin=BURNIN, thin=THIN, mixing=True)
    assert tm.n_targets == 3
    _check(tm.mix_step, tm.mix_counts, ref, "targets 1 .. 3")
    assert not np.array_equal(Reference(x, m, hop[:3], modes[:3], False).counts, ref.counts)
    whole = _sampler(pdfs, m, mode, x0).summarize(N_SAMPLES, burnin=BURNIN, thin=THIN, mixing=True)
    assert torch.equal(whole.mix_counts[1:], tm.mix_counts) and torch.equal(whole.mix_step[1:], tm.mix_step)


def test_against_the_running_statistics_of_a_single_target():
    n, d, n_keep, thin = 64, 3, 30, 3
    pdf = _vmf_mixtures(1, seed=33)[0]
    modes = np.array(pdf._modes())
    hop = modes[0]
    x0 = _x0(d, n, seed=8)
    plain = gs.ShrinkageSphericalSliceSampler(pdf, x0, SEED, mode="exact").enable_stats(lags=0, hop=hop, modes=modes)
    plain.advance(n_keep * thin, thin=thin, keep=False)
    acc = plain._stats["acc"].cpu().numpy()                     # rows x chains
    r_dist = 1 + 2 * d + d * (d + 1) // 2
    assert np.all(acc[0] == n_keep)
    with warnings.catch_warnings(record=True):
        warnings.simplefilter("always")
        s = gs.ShrinkageSphericalSliceSampler(gs.TargetBatch([pdf]), x0, SEED, mode="exact", chains_per_target=n)
    tm = s.summarize(n_keep, burnin=thin, thin=thin, mixing=dict(hop=hop, modes=modes))
    assert torch.equal(s.state_rows(), plain.state_rows())
    counts = tm.mix_counts.cpu().numpy()[0]
    assert counts[0] == n * n_keep and counts[1] == n * (n_keep - 1)
    assert counts[2] == acc[r_dist + 1].sum()
    assert np.array_equal(counts[3:], acc[r_dist + 2:r_dist + 2 + len(modes)].sum(1))
    total = float(acc[r_dist].sum())
    assert abs(float(tm.mix_step[0, 0]) - total) <= 1e-12 * total


def test_single_target_with_chains_per_target_and_the_default():
    n, m, d = 64, 16, 3
    pdf = gs.VonMisesFisher(20.0 * np.eye(3)[2])
    x0 = _x0(d, n, seed=8)
    hop, modes = _directions(1, 3, d, seed=3)
    _, x = _stored(gs.ShrinkageSphericalSliceSampler(pdf, x0, SEED), burnin=BURNIN, thin=1)
    ref = Reference(x, m, np.repeat(hop, n // m, 0), np.repeat(modes, n // m, 0), True)
    s = gs.ShrinkageSphericalSliceSampler(pdf, x0, SEED)
    tm = s.summarize(N_SAMPLES, burnin=BURNIN, chains_per_target=m, mixing=dict(hop=hop[0], modes=modes[0], transitions=True))
    assert tm.n_targets == n // m and tm.mix_weights is None
    _check(tm.mix_step, tm.mix_counts, ref, "single target")
    assert "mode_kl" not in tm.stats() and "mode_switch_frequency" in tm.stats()
    with pytest.raises(ValueError, match="TargetBatch"):
        gs.ShrinkageSphericalSliceSampler(pdf, x0, SEED).summarize(N_SAMPLES, mixing=True)
    # without the argument: the plain buffer, no ring, no new key
    plain = gs.ShrinkageSphericalSliceSampler(pdf, x0, SEED).summarize(5)
    assert plain.hist is None and plain.mix_step is None and plain.mix_counts is None and plain.mix_dirs is None
    assert not {"geodesic_step", "geodesic_step_sd", "hop_frequency", "mode_occupancy", "mode_kl", "mode_transitions",
                "mode_switch_frequency"} & set(plain.stats())

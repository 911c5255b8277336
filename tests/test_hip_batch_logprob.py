"""log_prob / gradient of a whole TargetBatch in one launch, and the log-density summaries of Sampler.summarize.

(a) TargetBatch.log_prob / .gradient ARE the members' own, bit for bit (np.array_equal), and upload no member.
(b) They hold the bound tests/test_hip_logprob_layouts.py holds gsss_logprob to in the same layouts, against the same independent
    reference (tests/reference_math.py): layout_cases.rel / gradient_error < 1e-10 of the value's scale.
The component-major entry (diagnostics.target_log_prob) gives the same bits as log_prob of the gathered points; the scalar
moments hold the summation bound of tests/test_hip_target_moments.py, |got - ref| <= 2 N u sum|term| (N = m R terms, u = 2^-53,
ref a numpy longdouble sum of the values the device wrote); summarize(log_prob=True) is held against an identically seeded twin
that stores its draws."""
import warnings

import numpy as np
import pytest
import torch
from scipy.special import i0

import batch_layout_cases as bc

pytestmark = pytest.mark.gpu
assert bc.TOL == 1e-10  # the bound of (b)
U = 2.0 ** -53
LD = np.longdouble
README_MUS = 80.0 * np.array([[0.87, -0.37, 0.33], [-0.20, -0.89, -0.40], [0.19, 0.22, -0.96]])
SIZES = (1, 37, 300)     # 300 crosses a workgroup of 256 points at L = 1, 37 every cooperative group count


@pytest.fixture(scope="module")
def gs():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    import geosss_amd
    geosss_amd._lib.require_device()
    return geosss_amd


def _rotation(g, d):
    q, r = np.linalg.qr(g.standard_normal((d, d)))
    return q * np.sign(np.diag(r))


def _unit(v):
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


def members(gs, case, M):
    """M members that really differ: one case per row of the matrix (family x d)."""
    g = np.random.default_rng(sum(case.encode()) + 7)
    seed = lambda: int(g.integers(1 << 30))  # noqa: E731
    if case == "vmfmix_d3_k3":        # lane3
        out = [gs.MixtureModel([gs.VonMisesFisher(m) for m in README_MUS])]
        for _ in range(M - 1):
            mus = (0.25 + 1.5 * g.random()) * README_MUS @ _rotation(g, 3).T
            out.append(gs.MixtureModel([gs.VonMisesFisher(m) for m in mus], g.random(3) + 0.5))
        return out
    if case == "vmf_d4":
        return [gs.VonMisesFisher(k * v) for k, v in zip(np.geomspace(0.5, 500.0, M), _unit(g.standard_normal((M, 4))))]
    if case in ("bingham_d5_dense", "bingham_d12_dense", "bingham_d24_dense"):   # d = 12: coop4x4
        d = int(case.split("_")[1][1:])
        return [gs.random_bingham(d, vmax=10.0 + 40.0 * g.random(), vmin=0.0, seed=seed()) for _ in range(M)]
    if case == "bingham_d10_mixed":   # diagonal and dense A in one batch
        return [gs.random_bingham(10, vmax=10.0 + 40.0 * g.random(), vmin=0.0, eigensystem=(t % 2 == 0), seed=seed()) for t in range(M)]
    if case in ("binghamfisher_d6", "binghamfisher_d17"):
        d = int(case.split("_d")[1])
        return [gs.BinghamFisher(gs.random_bingham(d, vmax=20.0, vmin=0.0, seed=seed()).A, (1.0 + 9.0 * g.random()) * g.standard_normal(d))
                for _ in range(M)]
    if case == "vmfmix_d130_k2":      # a wide cooperative layout
        out = []
        for _ in range(M):
            mus = _unit(g.standard_normal((2, 130))) * (20.0 + 80.0 * g.random((2, 1)))
            out.append(gs.MixtureModel([gs.VonMisesFisher(m) for m in mus], g.random(2) + 0.2))
        return out
    if case == "vmf_k7000_d3":        # the shape of layout_cases' global case: the means stay in global memory
        out = []
        for _ in range(M):
            dirs = _unit(g.standard_normal((7000, 3)))
            out.append(gs.MixtureModel([gs.VonMisesFisher(k * m) for k, m in zip(g.uniform(10.0, 100.0, 7000), dirs)],
                                       g.uniform(0.5, 2.0, 7000)))
        return out
    raise KeyError(case)


CASES = ["vmfmix_d3_k3", "vmf_d4", "bingham_d5_dense", "binghamfisher_d6", "bingham_d10_mixed", "bingham_d12_dense",
         "binghamfisher_d17", "bingham_d24_dense", "vmfmix_d130_k2"]


def _points(case, M, n, d):
    return _unit(np.random.default_rng(sum(case.encode()) + 1000 * M + n).standard_normal((M, n, d)))


def _check(gs, case, M, sizes=SIZES, device_tensors=True):
    pdfs = members(gs, case, M)
    d = pdfs[0].d
    if case == "bingham_d10_mixed" and M > 1:
        diag = [bool(np.array_equal(p.A, np.diag(np.diag(p.A)))) for p in pdfs]
        assert any(diag) and not all(diag)
    # (a) and (b) of the module's docstring: the check the layout sweep shares (tests/batch_layout_cases.py)
    bc.check_logprob(gs, pdfs, case, sizes, device_tensors=device_tensors, xs=[_points(case, M, n, d) for n in sizes])


@pytest.mark.parametrize("M", [1, 3, 6])
@pytest.mark.parametrize("case", CASES)
def test_batch_is_the_members_and_the_reference(gs, case, M):
    _check(gs, case, M)


def test_rows_in_global_memory(gs):
    """K = 7000 means at d = 3 do not fit the LDS (VmfMixture::in_lds is false): the second member's rows are read from global
    memory at blob + stride."""
    batch = gs.TargetBatch(members(gs, "vmf_k7000_d3", 2))
    name = batch._device_target().lib.gsss_kernel_name(batch._device_target().handle, 0, 0, 0).decode()
    assert "<coop64x4," in name and "batch" in name, name
    _check(gs, "vmf_k7000_d3", 2, device_tensors=False)


def test_refusals_and_shapes(gs):
    pdfs = members(gs, "bingham_d5_dense", 3)
    batch = gs.TargetBatch(pdfs)
    x = _points("r", 3, 4, 5)
    with pytest.raises(ValueError, match=r"\(M, n, d\)"):
        batch.log_prob(x[0])
    with pytest.raises(ValueError, match=r"\(M, n, d\)"):
        batch.gradient(x[:2])
    with pytest.raises(ValueError, match="GPU"):
        batch.log_prob(torch.from_numpy(x))
    assert batch.log_prob(x[:, :0]).shape == (3, 0) and batch.gradient(x[:, :0]).shape == (3, 0, 5)
    before = gs.TargetBatch.log_prob.num_calls
    batch.log_prob(x)
    assert gs.TargetBatch.log_prob.num_calls == before + 1
    # the C ABI: a single target's handle is no batch; the single-target entries keep refusing a batch
    lib = gs._lib.load()
    xt = torch.from_numpy(x).cuda()
    out = torch.empty((3, 4), dtype=torch.float64, device="cuda")
    single, h = pdfs[0]._device_target().handle, batch._device_target(chains_per_target=4).handle
    assert lib.gsss_batch_logprob(single, xt.data_ptr(), 4, out.data_ptr(), None) == -2 and b"batch" in lib.gsss_last_error()
    assert lib.gsss_batch_logprob_draws(single, xt.data_ptr(), 1, 4, 0, out.data_ptr(), None) == -2
    assert lib.gsss_logprob(h, xt.data_ptr(), 4, out.data_ptr(), None) == -2 and b"members' own handles" in lib.gsss_last_error()
    assert lib.gsss_batch_logprob(h, None, 4, out.data_ptr(), None) == -1
    assert lib.gsss_batch_logprob(h, xt.data_ptr(), -1, out.data_ptr(), None) == -1
    assert lib.gsss_batch_logprob(h, None, 0, None, None) == 0
    for n_rows, n_chains, t0, code in ((1, 6, 0, -1), (1, 8, 2, -1), (1, 4, 3, -1), (-1, 4, 0, -1), (1, 4, -1, -1), (0, 4, 0, 0),
                                       (1, 0, 3, 0)):
        assert lib.gsss_batch_logprob_draws(h, xt.data_ptr(), n_rows, n_chains, t0, out.data_ptr(), None) == code, (n_rows, n_chains, t0)
    assert lib.gsss_batch_logprob_draws(h, None, 1, 4, 0, out.data_ptr(), None) == -1
    from geosss_amd import diagnostics
    with pytest.raises(ValueError):
        diagnostics.target_log_prob(batch, torch.zeros((2, 5, 7), dtype=torch.float64, device="cuda"))       # 7 chains, 3 targets
    with pytest.raises(ValueError):
        diagnostics.target_log_prob(batch, torch.zeros((2, 5, 6), dtype=torch.float64, device="cuda"), target0=3)
    with pytest.raises(ValueError):
        diagnostics.target_log_prob(batch, torch.zeros((2, 4, 6), dtype=torch.float64, device="cuda"))       # another d


@pytest.mark.parametrize("m,R", [(1, 1), (7, 5), (24, 3), (256, 2), (300, 2)])
@pytest.mark.parametrize("case", ["vmfmix_d3_k3", "bingham_d12_dense"])
def test_component_major_draws(gs, case, m, R):
    """target_log_prob on (R, d, N) blocks == log_prob of the same points gathered into (M, R m, d), bit for bit; target0 > 0
    serves the later targets; the chain-major form gives the same values."""
    from geosss_amd import diagnostics
    M = 4
    pdfs = members(gs, case, M)
    d = pdfs[0].d
    batch = gs.TargetBatch(pdfs)
    for t0 in (0, 2):
        Mc = M - t0
        N = Mc * m
        x = torch.from_numpy(np.ascontiguousarray(_points(case, R, N, d).transpose(0, 2, 1))).cuda()        # (R, d, N)
        got = diagnostics.target_log_prob(batch, x, target0=t0)
        assert tuple(got.shape) == (R, N)
        gathered = x.reshape(R, d, Mc, m).permute(2, 0, 3, 1).reshape(Mc, R * m, d).contiguous()
        want = gs.TargetBatch(pdfs[t0:]).log_prob(gathered)                                               # (Mc, R m)
        assert torch.equal(got.reshape(R, Mc, m).permute(1, 0, 2).reshape(Mc, R * m), want), (case, m, R, t0)
        cm = diagnostics.target_log_prob(batch, x.permute(2, 0, 1).contiguous(), chain_major=True, target0=t0)
        assert tuple(cm.shape) == (N, R) and torch.equal(cm, got.t())
    assert not any("_targets" in p.__dict__ for p in pdfs)


@pytest.mark.parametrize("R", [1, 5])
@pytest.mark.parametrize("m", [1, 7, 64, 100, 300])
def test_scalar_moments(gs, m, R):
    from geosss_amd import diagnostics
    M = 5
    N = M * m
    v = torch.from_numpy(-40.0 + 25.0 * np.random.default_rng(m + R).standard_normal((R, N))).cuda()
    cs = torch.zeros(N, dtype=torch.float64, device="cuda")
    acc = diagnostics.scalar_moments(v, m, chain_sum=cs)
    vl = v.cpu().numpy().astype(LD)
    a, c = acc.cpu().numpy(), cs.cpu().numpy()
    assert a.shape == (M, 3) and np.all(a[:, 0] == m * R)
    per_target = lambda w: w.reshape(R, M, m).sum((0, 2))  # noqa: E731
    for col, term in ((1, vl), (2, vl * vl)):
        err = np.abs(a[:, col].astype(LD) - per_target(term))
        bound = 2 * m * R * U * per_target(np.abs(term))
        print(f"m={m} R={R} column {col}: max |err| / bound = {float(np.max(err / bound)):.3g}")
        assert np.all(err <= bound), (m, R, col, float(np.max(err / bound)))
    assert np.all(np.abs(c.astype(LD) - vl.sum(0)) <= 2 * R * U * np.abs(vl).sum(0))
    # the same bits every time, and added to
    cs2 = torch.zeros_like(cs)
    acc2 = diagnostics.scalar_moments(v, m, chain_sum=cs2)
    assert torch.equal(acc2, acc) and torch.equal(cs2, cs)
    diagnostics.scalar_moments(v, m, acc=acc2, chain_sum=cs2)
    assert torch.equal(acc2[:, 0], 2 * acc[:, 0]) and torch.equal(cs2, 2 * cs)


# ------------------------------------------------------------------------------------------ summarize(log_prob=True)
SEED = 977
N_SAMPLES, BURNIN, THIN = 40, 10, 2


def _x0(d, n, seed=5):
    x = np.random.default_rng(seed).standard_normal((n, d))
    return x / np.linalg.norm(x, axis=1, keepdims=True)


def _batch(gs, which):
    """(members, m, mode): the batches of tests/test_hip_target_summary.py"""
    g = np.random.default_rng(11)
    if which == "bingham_d5_m24":
        return [gs.random_bingham(5, vmax=20.0, vmin=0.0, seed=int(g.integers(1 << 30))) for _ in range(6)], 24, "fast"
    if which == "vmfmix_d3_m256":
        out = []
        for _ in range(3):
            mu = g.standard_normal((2, 3))
            mu *= (10.0 + 30.0 * g.random((2, 1))) / np.linalg.norm(mu, axis=1, keepdims=True)
            out.append(gs.MixtureModel([gs.VonMisesFisher(v) for v in mu], g.random(2) + 0.5))
        return out, 256, "fast"
    if which == "binghamfisher_d17_m8":
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


def _sampler(gs, pdfs, m, mode, x0, t0=0, t1=None):
    t1 = len(pdfs) if t1 is None else t1
    with warnings.catch_warnings(record=True):
        warnings.simplefilter("always")
        return gs.ShrinkageSphericalSliceSampler(gs.TargetBatch(pdfs), x0[t0 * m:t1 * m], SEED, mode=mode, chain_offset=t0 * m,
                                                 chains_per_target=m)


def _twin(gs, pdfs, m, mode, x0):
    """The stored run: draws (n, R, d) and their log_prob (n, R), by batch.log_prob on the stored draws."""
    M, d = len(pdfs), pdfs[0].d
    twin = _sampler(gs, pdfs, m, mode, x0)
    draws = twin.sample(N_SAMPLES, burnin=BURNIN, thin=THIN, as_tensor=True)
    lp = gs.TargetBatch(pdfs).log_prob(draws.reshape(M, m * N_SAMPLES, d)).reshape(M * m, N_SAMPLES)
    return twin, draws.cpu().numpy(), lp.cpu().numpy()


def _lp_within(tm, lp, m, R, what, targets=slice(None)):
    """lp (n, R): the twin's values of ALL chains; the summary covers `targets`."""
    M = lp.shape[0] // m
    vl = lp.astype(LD).reshape(M, m, R)[targets]
    acc, cs = tm.lp_acc.cpu().numpy(), tm.lp_chain_sum.cpu().numpy()
    assert np.all(acc[:, 0] == m * R), what
    for col, term in ((1, vl), (2, vl * vl)):
        err = np.abs(acc[:, col].astype(LD) - term.sum((1, 2)))
        bound = 2 * m * R * U * np.abs(term).sum((1, 2))
        print(f"{what}: lp_acc column {col}: max |err| / bound = {float(np.max(err / bound)):.3g}")
        assert np.all(err <= bound), (what, col, float(np.max(err / bound)))
    assert np.all(np.abs(cs.astype(LD) - vl.sum(2).reshape(-1)) <= 2 * R * U * np.abs(vl).sum(2).reshape(-1)), (what, "lp_chain_sum")


def _best_is_the_twins(tm, draws, lp, m, what, targets=slice(None)):
    """Exactly the twin's argmax in (draw, chain) order -- np.argmax takes the first occurrence -- and its row."""
    n, R = lp.shape
    M = n // m
    ts = range(M)[targets]
    got_lp, got_x = tm.lp_best.cpu().numpy(), tm.x_best.cpu().numpy()
    assert got_lp.shape == (len(ts),) and got_x.shape == (len(ts), draws.shape[2])
    for i, t in enumerate(ts):
        flat = lp[t * m:(t + 1) * m].T.reshape(-1)                      # index: draw m + chain
        k = int(np.argmax(flat))
        assert got_lp[i] == flat[k], (what, t)
        assert np.array_equal(got_x[i], draws[t * m + k % m, k // m]), (what, t)


@pytest.mark.parametrize("which", ["bingham_d5_m24", "vmfmix_d3_m256", "binghamfisher_d17_m8", "vmfmix_d130_m7"])
def test_summarize_with_log_prob(gs, which):
    pdfs, m, mode = _batch(gs, which)
    M, d = len(pdfs), pdfs[0].d
    x0 = _x0(d, M * m)
    twin, draws, lp = _twin(gs, pdfs, m, mode, x0)

    s = _sampler(gs, pdfs, m, mode, x0)
    tm = s.summarize(N_SAMPLES, burnin=BURNIN, thin=THIN, window=7, log_prob=True)          # draw 0, then windows 7 .. 7, 4
    assert tuple(tm.lp_acc.shape) == (M, 3) and tuple(tm.lp_chain_sum.shape) == (M * m,)
    _lp_within(tm, lp, m, N_SAMPLES, "window 7")
    _best_is_the_twins(tm, draws, lp, m, "window 7")
    # the coordinates' moments, the chains and the accounting are those of summarize() without the flag
    plain_s = _sampler(gs, pdfs, m, mode, x0)
    plain = plain_s.summarize(N_SAMPLES, burnin=BURNIN, thin=THIN, window=7)
    assert plain.lp_acc is None and plain.lp_best is None and "lp_mean" not in plain.stats()
    assert torch.equal(tm.acc, plain.acc) and torch.equal(tm.chain_sum, plain.chain_sum)
    assert torch.equal(s.state_rows(), plain_s.state_rows()) and torch.equal(s.state_rows(), twin.state_rows())
    assert s._step == plain_s._step == twin._step and s._tries_reported == plain_s._tries_reported
    assert np.array_equal(s.n_tries_per_chain, plain_s.n_tries_per_chain)
    # a sampler on the targets 2 .. (2 .. 4 of the six) summarises them as its rows 0 ..
    t1 = min(M, 5)
    part = _sampler(gs, pdfs, m, mode, x0, 2, t1).summarize(N_SAMPLES, burnin=BURNIN, thin=THIN, window=7, log_prob=True)
    assert part.n_targets == t1 - 2
    _lp_within(part, lp, m, N_SAMPLES, "targets 2 ..", targets=slice(2, t1))
    _best_is_the_twins(part, draws, lp, m, "targets 2 ..", targets=slice(2, t1))
    # two half-length calls, the second continuing the first
    s2 = _sampler(gs, pdfs, m, mode, x0)
    half = s2.summarize(N_SAMPLES // 2, burnin=BURNIN, thin=THIN, window=7, log_prob=True)
    both = s2.summarize(N_SAMPLES // 2, burnin=THIN, thin=THIN, window=7, into=half, log_prob=True)
    assert both is half and torch.equal(s2.state_rows(), twin.state_rows())
    _lp_within(both, lp, m, N_SAMPLES, "into=")
    _best_is_the_twins(both, draws, lp, m, "into=")
    assert torch.equal(both.lp_best, tm.lp_best) and torch.equal(both.x_best, tm.x_best)
    # the summaries
    st = tm.stats()
    for k in ("lp_mean", "lp_var", "lp_rhat", "lp_ess_between", "lp_best"):
        assert tuple(st[k].shape) == (M,) and bool(torch.isfinite(st[k]).all()), k
    assert tuple(st["x_best"].shape) == (M, d)
    N = m * N_SAMPLES
    vl = lp.astype(LD).reshape(M, N)
    assert np.all(np.abs(st["lp_mean"].cpu().numpy().astype(LD) - vl.sum(1) / N) <= 2 * U * np.abs(vl).sum(1) + U * np.abs(vl.sum(1) / N))
    assert bool((st["lp_best"] >= st["lp_mean"]).all())
    # a summary begun without log_prob cannot take it up
    with pytest.raises(ValueError, match="log_prob"):
        plain_s.summarize(5, burnin=THIN, thin=THIN, into=plain, log_prob=True)


def test_log_prob_summary_needs_a_batch(gs):
    s = gs.ShrinkageSphericalSliceSampler(gs.VonMisesFisher(20.0 * np.eye(3)[2]), _x0(3, 64), SEED)
    with pytest.raises(ValueError, match="TargetBatch of one"):
        s.summarize(5, log_prob=True)
    # ... which works
    one = gs.ShrinkageSphericalSliceSampler(gs.TargetBatch([gs.VonMisesFisher(20.0 * np.eye(3)[2])]), _x0(3, 64), SEED)
    tm = one.summarize(5, log_prob=True)
    assert tm.n_targets == 1 and float(tm.lp_acc[0, 0]) == 5 * 64


def test_best_draw_of_vmf_members(gs):
    """Single von Mises-Fisher members: no draw is more probable than the mode, log p(mode) = kappa - log 2 pi - log i0(kappa),
    and the best draw's cosine to the mode lies in the range the stored twin's draws attain."""
    M, m = 4, 64
    g = np.random.default_rng(21)
    kappas = np.geomspace(0.5, 100.0, M)
    dirs = _unit(g.standard_normal((M, 3)))
    pdfs = [gs.VonMisesFisher(k * v) for k, v in zip(kappas, dirs)]
    x0 = _x0(3, M * m)
    twin, draws, lp = _twin(gs, pdfs, m, "auto", x0)
    tm = _sampler(gs, pdfs, m, "auto", x0).summarize(N_SAMPLES, burnin=BURNIN, thin=THIN, window=16, log_prob=True)
    _best_is_the_twins(tm, draws, lp, m, "vmf")
    lp_best, x_best = tm.lp_best.cpu().numpy(), tm.x_best.cpu().numpy()
    at_mode = kappas - np.log(2 * np.pi) - np.log(i0(kappas))
    print("lp_best - log p(mode):", lp_best - at_mode)
    assert np.all(lp_best <= at_mode + 1e-12)
    for t in range(M):
        cos = draws[t * m:(t + 1) * m] @ dirs[t]
        assert cos.min() <= x_best[t] @ dirs[t] <= cos.max()

"""GPU tests of the angular central Gaussian target (gs.AngularCentralGaussian, GSSS_ACG): log_prob and gradient in every
exact layout against the longdouble values of tests/acg_cases.py; the longdouble reference chains of the two slice samplers
replayed through the exact kernels and, at d <= 10, the fast ones; fast against exact on the library stream; the native target
against the same density written as a user target (slice samplers, RWMH, HMC); the sampled law against exact draws; edges.

The bar throughout is the project's TOL = 1e-10 on |got - want| / max(1, |want|) (test_hip_parity.py, test_hip_logprob_layouts.py);
tries, rejections, accept counts and error bits are compared exactly."""
import numpy as np
import pytest

import acg_cases as ac
import layout_cases as lc
from layout_cases import rel
from user_sources import ACG as ACG_SOURCE

pytestmark = pytest.mark.gpu

TOL = 1e-10
LAYOUTS = ["lane2", "lane3", "lane4", "lane5", "lane6", "lane8", "lane10", "coop4x4", "coop4x8", "coop16x4", "coop16x8", "coop64x4",
           "coop64x8", "coop64x16", "coop64x32"]  # GSSS_VEC_LIST ids 1 .. 15


@pytest.fixture(scope="module")
def gs():
    import torch
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    import geosss_amd
    geosss_amd._lib.require_device()
    yield geosss_amd
    ac.release()  # the cached targets' device copies go with the module
    torch.cuda.synchronize()


@pytest.fixture(scope="module")
def cache(tmp_path_factory):
    return str(tmp_path_factory.mktemp("gsss_user_modules"))  # one compile per user module for the whole file


def sampler_cls(gs, sampler):
    return gs.ShrinkageSphericalSliceSampler if sampler == "shrink" else gs.RejectionSphericalSliceSampler


def kernel_name(s, mode, placement=0):
    return s._lib.gsss_kernel_name(s._target_dev.handle, 1 if mode == "fast" else 0, 0, placement).decode()


# ------------------------------------------------------------------------------------------ 1. layouts
def gradient_error(got, want):
    """max over rows of |got - want| / max(1, the row's |want|_inf), as layout_cases.gradient_error."""
    got, want = np.asarray(got, dtype=ac.LD), np.asarray(want, dtype=ac.LD)
    return float(np.max(np.abs(got - want) / np.maximum(1, np.max(np.abs(want), axis=-1, keepdims=True))))


def test_sweep_reaches_every_layout(gs):
    lib = gs._lib.load()
    assert {lib.gsss_exact_layout(d) for d in lc.DIMS} == set(range(1, len(LAYOUTS) + 1))


@pytest.mark.parametrize("d", lc.DIMS)
def test_logprob_and_gradient(gs, d):
    pdf, X, ref = ac.target(d), ac.points(d), ac.reference(d)
    layout = LAYOUTS[gs._lib.load().gsss_exact_layout(d) - 1]
    name = pdf._device_target().lib.gsss_kernel_name(pdf._device_target().handle, 0, 0, 0).decode()
    assert f"<{layout}," in name and name.endswith("Acg>"), name
    worst = {}
    for tag, P in (("unit", X), ("off", lc.OFF_SPHERE * X)):
        want_lp, want_gr = ref[tag]
        e = [rel(pdf.log_prob(P), want_lp), gradient_error(pdf.gradient(P), want_gr)]
        e[0] = max(e[0], rel(pdf.log_prob(P[1]), want_lp[1]))  # a single point (d,)
        e[1] = max(e[1], gradient_error(pdf.gradient(P[1])[None], want_gr[1:2]))
        worst[tag] = e
    print(f"acg d={d} {layout}: log_prob {worst['unit'][0]:.1e} / {worst['off'][0]:.1e}, gradient {worst['unit'][1]:.1e} / "
          f"{worst['off'][1]:.1e} (unit rows / norm 0.998)")
    assert max(worst["unit"][0], worst["off"][0]) < TOL, ("log_prob", worst)
    assert max(worst["unit"][1], worst["off"][1]) < TOL, ("gradient", worst)


# ------------------------------------------------------------------------------------------ 2. replayed chains
def _replay_params():
    out = []
    for d in sorted(set(ac.CHAIN_DIMS + ac.FAST_DIMS)):
        for sampler in ac.SAMPLERS:
            if d in ac.CHAIN_DIMS:
                out += [(d, sampler, "exact", "auto"), (d, sampler, "exact", "packed")]
            if d in ac.FAST_DIMS:
                out += [(d, sampler, "fast", "auto"), (d, sampler, "fast", "packed")]
    return out


@pytest.mark.parametrize("d,sampler,mode,placement", _replay_params())
def test_replay_reproduces_reference_chain(gs, d, sampler, mode, placement):
    pdf, ref = ac.target(d), ac.reference_chain(d, sampler)
    assert ref["margin"] > ac.MIN_MARGIN
    s = sampler_cls(gs, sampler)(pdf, ref["x0"], seed=1, mode=mode, placement=placement)
    assert s.mode == mode
    name = kernel_name(s, mode, 2 if placement == "auto" else 1)
    assert (f"FastAcg<{d}>" in name) if mode == "fast" else name.endswith("Acg>"), name
    got = s.advance(ac.N_STEPS, thin=1, replay=ref["replay"]).cpu().numpy().transpose(0, 2, 1)
    assert np.all(s.errors == 0)
    print(f"acg d={d} {sampler} {mode} {placement} ({name}): max |dx| {np.max(np.abs(got - ref['states'])):.1e}, margin {ref['margin']:.1e}")
    assert np.array_equal(np.asarray(s.n_tries_per_chain), ref["tries"])
    assert np.array_equal(np.asarray(s.n_reject_per_chain), ref["rejections"])
    assert np.max(np.abs(got - ref["states"])) < TOL


def test_fast_mode_is_refused_beyond_the_lane_kernels(gs):
    """d > 10 (and d = 2): mode='auto' runs the exact kernels with the usual warning, mode='fast' is refused."""
    from geosss_amd import mcmc
    lib = gs._lib.load()
    for d in (2, 12):
        pdf = ac.target(d)
        x0 = gs.sample_sphere(d - 1, 32, seed=1)
        assert lib.gsss_mode_supported(pdf._device_target().handle, gs._lib.MODE_FAST) == 0
        mcmc._warned_shapes.discard(("AngularCentralGaussian", d))  # (the warning is given once per shape and process)
        with pytest.warns(RuntimeWarning, match="no fast-mode kernel covers this AngularCentralGaussian"):
            s = gs.ShrinkageSphericalSliceSampler(pdf, x0, seed=1, mode="auto")
        assert s.mode == "exact"
        s.advance(3)
        assert np.all(s.errors == 0)
        f = gs.ShrinkageSphericalSliceSampler(pdf, x0, seed=1, mode="fast")
        with pytest.raises(ValueError, match="fast mode is not built for an angular central Gaussian"):
            f.advance(1)
    pdf = ac.target(5)
    assert lib.gsss_mode_supported(pdf._device_target().handle, gs._lib.MODE_FAST) == 1
    assert lib.gsss_variant_name(pdf._device_target().handle, gs._lib.MODE_FAST, 0) == b"fast-lane"


# ------------------------------------------------------------------------------------------ 3. fast against exact, library stream
@pytest.mark.parametrize("sampler", ac.SAMPLERS)
@pytest.mark.parametrize("d", [3, 5, 8, 10])
def test_fast_equals_exact_on_the_library_stream(gs, d, sampler):
    pdf = ac.target(d)
    x0 = gs.sample_sphere_device(d - 1, 4096, seed=3).T
    a = sampler_cls(gs, sampler)(pdf, x0, seed=17, mode="fast")
    assert kernel_name(a, "fast", 1) == f"fast_kernel<{d}, FastAcg<{d}>>"
    b = sampler_cls(gs, sampler)(pdf, x0, seed=17, mode="exact")
    a.advance(20, keep=False)
    b.advance(20, keep=False)
    assert np.all(a.errors == 0) and np.all(b.errors == 0)
    print(f"acg d={d} {sampler}: fast against exact, max |dx| {np.max(np.abs(a.state - b.state)):.1e}, "
          f"{a.n_reject / (4096 * 20):.2f} rejections per step")
    assert np.max(np.abs(a.state - b.state)) < TOL
    assert np.array_equal(a.n_reject_per_chain, b.n_reject_per_chain)


@pytest.mark.parametrize("sampler", ac.SAMPLERS)
@pytest.mark.parametrize("d", [3, 4, 7, 10])
def test_one_wavefront_kernel_equals_exact(gs, d, sampler):
    """A small ensemble spread one chain per wavefront: wave_kernel<D, FastAcg<D>> (the third site that forms the threshold,
    eight speculative tries per batch) against the exact kernel on the Philox stream; 96 chains fill 24 workgroups."""
    pdf = ac.target(d)
    x0 = gs.sample_sphere(d - 1, 96, seed=12)
    a = sampler_cls(gs, sampler)(pdf, x0, seed=19, mode="fast", placement="spread")
    assert kernel_name(a, "fast", 2) == f"wave_kernel<{d}, FastAcg<{d}>>"
    b = sampler_cls(gs, sampler)(pdf, x0, seed=19, mode="exact", placement="spread")
    got = a.advance(40, thin=1).cpu().numpy()
    want = b.advance(40, thin=1).cpu().numpy()
    assert np.all(a.errors == 0) and np.all(b.errors == 0)
    print(f"acg d={d} {sampler}: one-wavefront kernel against exact, max |dx| {np.max(np.abs(got - want)):.1e}")
    assert np.max(np.abs(got - want)) < TOL
    assert np.array_equal(a.n_reject_per_chain, b.n_reject_per_chain)
    assert np.array_equal(a.n_tries_per_chain, b.n_tries_per_chain)
    # the default placement of a small ensemble is this kernel too, with the same chains
    c = sampler_cls(gs, sampler)(pdf, x0, seed=19, mode="auto")
    assert c.mode == "fast"
    c.advance(40)
    assert np.array_equal(np.asarray(c.state), np.asarray(a.state))


# ------------------------------------------------------------------------------------------ 4. native against the user target
@pytest.mark.parametrize("d", [5, 17])
def test_native_equals_user_target(gs, cache, d):
    """The same density as a DeviceDistribution (tests/user_sources.py::ACG): 1024 chains x 20 steps from the same seed.  Slice
    samplers: states < TOL, rejections equal.  RWMH and HMC: states within layout_cases.MH_CAPS, accept counts equal."""
    native = ac.target(d)
    user = gs.DeviceDistribution(d, ACG_SOURCE, native.precision, cache_dir=cache)
    x0 = gs.sample_sphere(d - 1, 1024, seed=4)
    for sampler in ac.SAMPLERS:
        a = sampler_cls(gs, sampler)(native, x0, seed=23, mode="exact")
        b = sampler_cls(gs, sampler)(user, x0, seed=23, mode="exact")
        a.advance(20, keep=False)
        b.advance(20, keep=False)
        assert np.all(a.errors == 0) and np.all(b.errors == 0)
        print(f"acg d={d} {sampler}: native against user target, max |dx| {np.max(np.abs(a.state - b.state)):.1e}")
        assert np.max(np.abs(a.state - b.state)) < TOL
        assert np.array_equal(a.n_reject_per_chain, b.n_reject_per_chain)
    for kind, cap in (("rw", lc.MH_CAPS["rw"][0]), ("hmc", lc.MH_CAPS["hmc"][0])):
        def make(pdf):
            if kind == "rw":
                return gs.MetropolisHastings(pdf, x0, 29, stepsize=0.5)
            return gs.SphericalHMC(pdf, x0, 29, stepsize=0.1, n_steps=3)
        a, b = make(native), make(user)
        for s in (a, b):
            s.reset(10)
            s.advance(20, keep=False)
        assert np.all(a.errors == 0) and np.all(b.errors == 0)
        share = a.n_accept / (1024 * 20)
        print(f"acg d={d} {kind}: native against user target, max |dx| {np.max(np.abs(a.state - b.state)):.1e}, accepted {share:.2f}")
        assert 0.05 < share < 0.999  # both branches of the accept test are taken
        assert np.max(np.abs(a.state - b.state)) < cap
        assert np.array_equal(a.n_accept_per_chain, b.n_accept_per_chain)
        assert np.max(np.abs(a.stepsize / b.stepsize - 1.0)) < lc.MH_STEPSIZE_TOL


def test_independence_and_mixture_samplers_run(gs):
    """The two further Metropolis-Hastings classes on the native target: finite unit states, proposals of both kinds accepted."""
    pdf = ac.target(6)
    x0 = gs.sample_sphere(5, 512, seed=6)
    for s in (gs.IndependenceSampler(pdf, x0, 31), gs.MixtureRWMHIndependenceSampler(pdf, x0, 31, stepsize=0.5, mixing_probability=0.5)):
        s.advance(30, keep=False)
        assert np.all(s.errors == 0) and 0 < s.n_accept < 512 * 30
        assert np.max(np.abs(np.linalg.norm(s.state, axis=1) - 1.0)) < 1e-12


# ------------------------------------------------------------------------------------------ 5. the law
def test_second_moment_matches_exact_draws(gs):
    """d = 5, fast mode: 20 000 independent chains, 100 burn-in steps, one kept draw each, so the standard error of E[x_i x_j] is
    exact.  Against 10^6 exact draws of rand.sample_acg: max |z| over the 15 entries < 5."""
    d, n = 5, 20_000
    pdf = ac.target(d)
    s = gs.ShrinkageSphericalSliceSampler(pdf, gs.sample_sphere(d - 1, n, seed=0), seed=1, mode="fast")
    assert "FastAcg<5>" in kernel_name(s, "fast", 1)
    s.advance(100, keep=False)
    assert int(np.count_nonzero(s.errors)) == 0
    x = np.asarray(s.state)
    iu = np.triu_indices(d)
    xx = (x[:, :, None] * x[:, None, :])[:, iu[0], iu[1]]
    u = gs.sample_acg(pdf, 1_000_000, seed=2024)
    uu = (u[:, :, None] * u[:, None, :])[:, iu[0], iu[1]]
    z = (xx.mean(0) - uu.mean(0)) / np.sqrt(xx.var(0, ddof=1) / n + uu.var(0, ddof=1) / len(u))
    print(f"acg d=5: max |E_chain - E_exact| = {np.max(np.abs(xx.mean(0) - uu.mean(0))):.2e}, max |z| {np.max(np.abs(z)):.2f}")
    assert z.shape == (15,) and np.max(np.abs(z)) < 5.0, z


# ------------------------------------------------------------------------------------------ 6. edges
@pytest.mark.parametrize("mode", ["exact", "fast"])
def test_nan_start_row_sets_nonfinite(gs, mode):
    d = 5
    pdf = ac.target(d)
    x0 = gs.sample_sphere(d - 1, 300, seed=8)
    bad = x0.copy()
    bad[7] = np.nan
    for placement in ("packed", "spread"):
        a = gs.ShrinkageSphericalSliceSampler(pdf, bad, seed=3, mode=mode, placement=placement)
        b = gs.ShrinkageSphericalSliceSampler(pdf, x0, seed=3, mode=mode, placement=placement)
        a.advance(10, keep=False)
        b.advance(10, keep=False)
        err = np.asarray(a.errors)
        assert err[7] == gs._lib.CHAIN_NONFINITE and np.count_nonzero(err) == 1, err[:10]
        others = np.arange(300) != 7
        assert np.array_equal(np.asarray(a.state)[others], np.asarray(b.state)[others])
        assert np.array_equal(np.asarray(a.n_reject_per_chain)[others], np.asarray(b.n_reject_per_chain)[others])


@pytest.mark.parametrize("mode", ["exact", "fast"])
@pytest.mark.parametrize("n_chains", [1, 257])
def test_ragged_ensembles(gs, mode, n_chains):
    """One chain, and 257: a ragged last workgroup in the packed placement.  Chain c is the same chain whatever the ensemble."""
    d = 6
    pdf = ac.target(d)
    x0 = gs.sample_sphere(d - 1, 257, seed=9)
    full = gs.ShrinkageSphericalSliceSampler(pdf, x0, seed=5, mode=mode, placement="packed")
    full.advance(15, keep=False)
    part = gs.ShrinkageSphericalSliceSampler(pdf, x0[:n_chains], seed=5, mode=mode, placement="packed")
    part.advance(15, keep=False)
    assert np.all(full.errors == 0) and np.all(part.errors == 0)
    assert np.array_equal(np.asarray(part.state).reshape(n_chains, d), np.asarray(full.state)[:n_chains])
    assert np.max(np.abs(np.linalg.norm(np.asarray(full.state), axis=1) - 1.0)) < 1e-12


def test_sample_returns_unit_rows(gs):
    pdf = ac.target(4)
    for cls in (gs.ShrinkageSphericalSliceSampler, gs.RejectionSphericalSliceSampler):
        x = cls(pdf, np.array([1.0, 0.0, 0.0, 0.0]), seed=2).sample(5, burnin=5)
        assert x.shape == (5, 4) and np.max(np.abs(np.linalg.norm(x, axis=1) - 1.0)) < 1e-12
    many = gs.ShrinkageSphericalSliceSampler(pdf, gs.sample_sphere(3, 64, seed=1), seed=2)
    x = many.sample(5, burnin=5)
    assert x.shape[-1] == 4 and x.size == 64 * 5 * 4 and np.max(np.abs(np.linalg.norm(x, axis=-1) - 1.0)) < 1e-12
    # running statistics, checkpoint and summary against the stored draws of the same run
    x0 = gs.sample_sphere(3, 64, seed=1)
    s = gs.ShrinkageSphericalSliceSampler(pdf, x0, seed=2)
    s.enable_stats(lags=4)
    kept = s.advance(10, thin=1).cpu().numpy()                       # (10, d, chains)
    st, sd = s.stats(), s.state_dict()
    assert int(st["n"].min()) == 10 and int(st["n"].max()) == 10
    assert np.max(np.abs(st["mean"].cpu().numpy() - kept.mean(0).T)) < 1e-13
    sm = np.einsum("sic,sjc->cij", kept, kept) / 10
    assert np.max(np.abs(st["second_moment"].cpu().numpy() - sm)) < 1e-13
    assert np.array_equal(sd["state"], kept[-1].T) and sd["step"] == 10 and sd["mode"] == s.mode
    resumed = gs.ShrinkageSphericalSliceSampler(pdf, x0, seed=2)
    resumed.load_state_dict(sd)
    s.advance(5)
    resumed.advance(5)
    assert np.array_equal(np.asarray(resumed.state), np.asarray(s.state))
    draws = gs.ShrinkageSphericalSliceSampler(pdf, x0, seed=2).sample(20, burnin=5)            # (chains, 20, d)
    tm = gs.ShrinkageSphericalSliceSampler(pdf, x0, seed=2).summarize(20, burnin=5).stats()
    pooled = draws.reshape(-1, 4)
    import torch
    host = {k: torch.as_tensor(tm[k]).cpu().numpy() for k in ("n", "mean", "second_moment")}
    assert int(host["n"].ravel()[0]) == 64 * 20
    assert np.max(np.abs(host["mean"].ravel() - pooled.mean(0))) < 1e-13
    assert np.max(np.abs(host["second_moment"].reshape(4, 4) - pooled.T @ pooled / len(pooled))) < 1e-13

"""GPU tests of user-defined targets (DeviceDistribution): restatements of built-in targets in user C++ reproduce the reference's
recorded chains through the exact kernels (slice samplers, RWMH, HMC) in lane and cooperative layouts; their log_prob / gradient
equal the built-in ones; the angular central Gaussian, which the library lacks, samples its known second moment; the refusals."""
import warnings

import numpy as np
import pytest

from conftest import golden
from user_sources import ACG, ACG_NO_GRADIENT, BINGHAM, user_target

pytestmark = pytest.mark.gpu

TOL = 1e-10


@pytest.fixture(scope="module")
def gs():
    import torch
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    import geosss_amd
    geosss_amd._lib.require_device()
    return geosss_amd


@pytest.fixture(scope="module")
def cache(tmp_path_factory):
    return str(tmp_path_factory.mktemp("gsss_user_modules"))  # one compile per module for the whole file


REPLAY = [("traj_vmfmix_readme", "auto"), ("traj_vmfmix_readme", "packed"), ("traj_bingham_d10_vmax30", "auto"),
          ("traj_bingham_d10_vmax30", "packed"), ("traj_curve_d10_kappa800", "auto"), ("traj_curve_d10_kappa800", "packed"),
          ("traj_bingham_d50_vmax300", "auto"), ("traj_reject_vmfmix_readme", "auto"), ("traj_reject_bingham_d10_vmax30", "packed")]


@pytest.mark.parametrize("name,placement", REPLAY)
def test_golden_replay(gs, cache, name, placement):
    """The reference's recorded draws through the user target's exact kernels: every state (1e-10), tries and rejections exactly.
    d = 3 and 10 run in lane layouts (placement 'auto' spreads the one chain over a wavefront), d = 50 in a cooperative one."""
    z = golden(name + ".npz")
    pdf = user_target(gs, z, cache)
    cls = gs.RejectionSphericalSliceSampler if str(z["sampler"]) == "reject" else gs.ShrinkageSphericalSliceSampler
    s = cls(pdf, z["x0"], seed=1, mode="exact", placement=placement)
    assert s._lib.gsss_kernel_name(s._target_dev.handle, 0, 0, 1).decode().endswith("UserTarget>")
    n = len(z["states"]) - 1
    got = s.advance(n, thin=1, replay=z["draws"][None])[:, :, 0].cpu().numpy()
    assert s.errors[0] == 0
    assert np.max(np.abs(got - z["states"][1:])) < TOL
    assert s.n_reject == int(z["n_reject"])
    assert int(s.n_tries_per_chain[0]) == int(z["tries"].sum())


@pytest.mark.parametrize("d", [10, 50])
def test_bingham_known_answers(gs, cache, d):
    """log_prob and gradient of the user Bingham equal the built-in gs.Bingham on 10^4 random points (lane and cooperative layout)."""
    z = golden("traj_bingham_d10_vmax30.npz" if d == 10 else "traj_bingham_d50_vmax300.npz")
    A = z["target_A"]
    user, ref = gs.DeviceDistribution(d, BINGHAM, A, cache_dir=cache), gs.Bingham(A)
    X = gs.sample_sphere(d - 1, 10_000, seed=3)
    lp, want = user.log_prob(X), ref.log_prob(X)
    assert np.max(np.abs(lp - want) / np.maximum(1.0, np.abs(want))) < 1e-12
    g, gwant = user.gradient(X), ref.gradient(X)
    assert g.shape == (10_000, d)
    assert np.max(np.abs(g - gwant) / np.maximum(1.0, np.abs(gwant))) < 1e-12
    assert abs(user.log_prob(X[7]) - want[7]) < 1e-12 * max(1.0, abs(want[7]))


def _acg_cov(d=5, seed=11):
    rng = np.random.default_rng(seed)
    Q, _ = np.linalg.qr(rng.standard_normal((d, d)))
    return (Q * np.array([4.0, 2.0, 1.0, 0.5, 0.25])[:d]) @ Q.T


def test_acg_known_answers(gs, cache):
    C = _acg_cov()
    pdf = gs.DeviceDistribution(5, ACG, np.linalg.inv(C), cache_dir=cache)
    X = gs.sample_sphere(4, 10_000, seed=5)
    want = gs.ACG(C).log_prob(X)
    assert np.max(np.abs(pdf.log_prob(X) - want) / np.maximum(1.0, np.abs(want))) < 1e-12
    # gradient: -d C^-1 x / (x^T C^-1 x), the ambient derivative of -(d / 2) log(x^T C^-1 x)
    P = np.linalg.inv(C)
    r = X @ P
    gwant = -5 * r / np.sum(X * r, axis=1)[:, None]
    assert np.max(np.abs(pdf.gradient(X) - gwant) / np.maximum(1.0, np.abs(gwant))) < 1e-12


@pytest.mark.parametrize("name", ["mh_rwmh_bingham_d10_vmax30", "mh_hmc_bingham_d10_vmax30"])
def test_mh_family_replays_reference_chain(gs, cache, name):
    """RWMH and HMC on the user Bingham reproduce the reference's recorded chains (tolerances of test_hip_mh.py)."""
    z = golden(name + ".npz")
    pdf = gs.DeviceDistribution(10, BINGHAM, z["target_A"], cache_dir=cache)
    if str(z["sampler"]) == "rwmh":
        s, tol = gs.MetropolisHastings(pdf, z["x0"], 1, stepsize=float(z["stepsize0"])), 1e-10
    else:
        s, tol = gs.SphericalHMC(pdf, z["x0"], 1, stepsize=float(z["stepsize0"]), n_steps=int(z["n_leapfrog"])), 1e-9
    n = len(z["states"]) - 1
    s.reset(int(z["burnin"]))
    got = s.advance(n, thin=1, replay=z["draws"][None])[:, :, 0].cpu().numpy()
    assert s.errors[0] == 0
    acc = np.any(got != np.vstack([z["x0"][None], got[:-1]]), axis=1)
    assert np.array_equal(acc, z["accept"].astype(bool))
    assert np.max(np.abs(got - z["states"][1:])) < tol
    assert s.n_accept == int(z["n_accept"])
    assert abs(s.stepsize / z["stepsize_trace"][-1] - 1) < 1e-12


def test_acg_second_moment_matches_exact_draws(gs, cache):
    """A target the library lacks: ACG(C) at d = 5, 10^5 chains x 200 steps (100 kept).  E[x x^T] of the chains against 10^6
    exact draws z / |z|, z ~ N(0, C), within 5 Monte-Carlo standard errors; the running statistics give the stored draws' moments."""
    import torch
    d, n_chains = 5, 100_000
    C = _acg_cov()
    pdf = gs.DeviceDistribution(d, ACG, np.linalg.inv(C), cache_dir=cache)
    s = gs.ShrinkageSphericalSliceSampler(pdf, gs.sample_sphere(d - 1, n_chains, seed=0), seed=1, mode="exact")
    s.advance(100)                                                      # burn-in
    s.enable_stats(lags=0, second_moment=True)
    kept = s.advance(100, thin=1)                                       # [100][d][n_chains] on the device
    assert int(np.count_nonzero(s.errors)) == 0
    per_chain = torch.einsum("sic,sjc->cij", kept, kept) / kept.shape[0]  # (n_chains, d, d)
    st = s.stats()
    assert torch.max(torch.abs(st["second_moment"] - per_chain)).item() < 1e-12
    assert torch.all(st["n"] == 100)
    pc = per_chain.cpu().numpy()
    m_chain, se_chain = pc.mean(0), pc.std(0, ddof=1) / np.sqrt(n_chains)
    rng = np.random.default_rng(2024)
    z = rng.standard_normal((1_000_000, d)) @ np.linalg.cholesky(C).T
    u = z / np.linalg.norm(z, axis=1, keepdims=True)
    uu = u[:, :, None] * u[:, None, :]
    m_exact, se_exact = uu.mean(0), uu.std(0, ddof=1) / np.sqrt(len(u))
    zscore = np.abs(m_chain - m_exact) / np.sqrt(se_chain ** 2 + se_exact ** 2)
    print(f"ACG d=5: max |E_chain - E_exact| = {np.max(np.abs(m_chain - m_exact)):.2e}, max z-score {zscore.max():.2f}")
    assert zscore.max() < 5.0, zscore


def test_refusals(gs, cache):
    from geosss_amd import mcmc
    C = _acg_cov()
    pdf = gs.DeviceDistribution(5, ACG, np.linalg.inv(C), cache_dir=cache)
    x0 = gs.sample_sphere(4, 64, seed=1)
    assert pdf._device_target(0) and pdf.module.vec_id == 4
    assert gs._lib.load().gsss_mode_supported(pdf._device_target(0).handle, gs._lib.MODE_FAST) == 0
    with pytest.raises(ValueError, match="fast mode is not built for user targets"):
        gs.ShrinkageSphericalSliceSampler(pdf, x0, 1, mode="fast").advance(1)
    mcmc._warned_shapes.clear()
    with pytest.warns(RuntimeWarning, match="no fast-mode kernel"):
        s = gs.ShrinkageSphericalSliceSampler(pdf, x0, 1)
    assert s.mode == "exact"
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        s.advance(3)
    assert np.all(s.errors == 0)
    with pytest.raises(ValueError, match="layout"):                     # a forced variant other than the module's layout
        gs.ShrinkageSphericalSliceSampler(pdf, x0, 1, mode="exact", variant=8).advance(1)
    bare = gs.DeviceDistribution(5, ACG_NO_GRADIENT, np.linalg.inv(C), cache_dir=cache)
    with pytest.raises(ValueError, match="no gsss_user_gradient"):
        gs.SphericalHMC(bare, x0, 1)
    with pytest.raises(ValueError, match="no gsss_user_gradient"):
        bare.gradient(x0)
    assert np.all(np.isfinite(bare.log_prob(x0)))
    m = gs.MetropolisHastings(bare, x0, 1, stepsize=0.3)                # RWMH needs no gradient
    m.advance(5)
    assert np.all(m.errors == 0)


def test_edited_params_are_uploaded_again(gs, cache):
    z = golden("traj_bingham_d10_vmax30.npz")
    pdf = gs.DeviceDistribution(10, BINGHAM, z["target_A"], cache_dir=cache)
    X = gs.sample_sphere(9, 100, seed=4)
    a = pdf.log_prob(X)
    pdf.params *= 2.0
    assert np.max(np.abs(pdf.log_prob(X) - 2.0 * a)) < 1e-12 * np.max(np.abs(a))

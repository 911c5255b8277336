"""GPU parity of MixtureModel targets whose components are not all von Mises-Fisher (GSSS_MIXTURE: Bingham,
Fisher-Bingham, Uniform, curve-vMF and nested mixtures) against the reference's recorded chains (gmix_*.npz,
tests/golden/make_golden_mixtures.py), between the exact and the fast kernels, and of the C ABI's refusals.

Tolerance as in test_hip_parity.py: 1e-10 on states and log-densities; tries, rejections and error bits exact."""
import ctypes as C
import os

import numpy as np
import pytest

from conftest import GOLDEN, golden

pytestmark = pytest.mark.gpu

TOL = 1e-10
TRAJ = sorted(f[:-4] for f in os.listdir(GOLDEN) if f.startswith("gmix_traj_") and f.endswith(".npz"))
MH = sorted(f[:-4] for f in os.listdir(GOLDEN) if f.startswith("gmix_mh_") and f.endswith(".npz"))


@pytest.fixture(scope="module")
def gs():
    import torch
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    import geosss_amd
    geosss_amd._lib.require_device()
    return geosss_amd


def target(gs, z, prefix=""):
    """The fixture's MixtureModel, rebuilt from its flat component list."""
    comps = []
    for i, kind in enumerate(z[prefix + "spec_kinds"]):
        a = lambda name: z[f"{prefix}spec_{i}_{name}"]  # noqa: E731
        kind = str(kind)
        if kind == "vmf":
            comps.append(gs.VonMisesFisher(a("mu")))
        elif kind == "bingham":
            comps.append(gs.Bingham(a("A")))
        elif kind == "binghamfisher":
            comps.append(gs.BinghamFisher(a("A"), a("b")))
        elif kind == "uniform":
            comps.append(gs.Uniform())
        elif kind == "curve":
            comps.append(gs.CurvedVonMisesFisher(gs.SlerpCurve(a("knots")), float(a("kappa"))))
        else:
            comps.append(gs.MixtureModel([gs.VonMisesFisher(m) for m in a("mus")], a("w")))
    return gs.MixtureModel(comps, z[prefix + "spec_weights"])


def sampler_cls(gs, z):
    return gs.RejectionSphericalSliceSampler if str(z["sampler"]) == "reject" else gs.ShrinkageSphericalSliceSampler


def kernel_name(s, mode, placement=0):
    return s._lib.gsss_kernel_name(s._target_dev.handle, 1 if mode == "fast" else 0, 0, placement).decode()



def _traj_params():
    out = []
    for name in TRAJ:
        out += [(name, "exact", "auto"), (name, "exact", "packed")]
        if "curve" not in name:
            out += [(name, "fast", "auto"), (name, "fast", "packed")]
    return out


@pytest.mark.parametrize("name,mode,placement", _traj_params())
def test_replay_reproduces_reference_chain(gs, name, mode, placement):
    """The reference's recorded draws through the kernels: every state, the tries and the rejections."""
    z = golden(name + ".npz")
    assert float(z["min_margin"]) > 1e-8  # no proposal of the chain sits within rounding of its threshold
    pdf = target(gs, z)
    s = sampler_cls(gs, z)(pdf, z["x0"], seed=1, mode=mode, placement=placement)
    assert s.mode == mode
    if mode == "fast":
        assert "FastMixture<" in kernel_name(s, mode, 2 if placement == "auto" else 1)
    else:
        assert kernel_name(s, mode).endswith("Mixture>")
    n = len(z["states"]) - 1
    got = s.advance(n, thin=1, replay=z["draws"][None])[:, :, 0].cpu().numpy()
    assert s.errors[0] == 0
    assert np.max(np.abs(got - z["states"][1:])) < TOL
    assert s.n_reject == int(z["n_reject"])
    assert int(s.n_tries_per_chain[0]) == int(z["tries"].sum())


@pytest.mark.parametrize("name", TRAJ)
@pytest.mark.parametrize("mode", ["exact", "auto"])
def test_reference_chain_from_seed(gs, name, mode):
    """The reference chain from (pdf, x0, seed) alone on numpy's stream; 'auto' runs the fast kernels where built."""
    z = golden(name + ".npz")
    pdf = target(gs, z)
    s = sampler_cls(gs, z)(pdf, z["x0"], int(z["seed"]), rng="numpy", mode=mode)
    assert s.mode == ("exact" if mode == "exact" or "curve" in name else "fast")
    out = s.sample(len(z["states"]))
    assert np.max(np.abs(out - z["states"])) < TOL
    assert s.n_reject == int(z["n_reject"])


def _composites(gs):
    rng = np.random.default_rng(5)
    A = rng.standard_normal((4, 4))
    return {
        "d3": gs.MixtureModel([gs.VonMisesFisher([0.0, 30.0, 0.0]), gs.Bingham(np.diag([5.0, 0.0, -5.0])), gs.Uniform()],
                              [0.5, 0.3, 0.2]),
        "d4": gs.MixtureModel([gs.Bingham(A + A.T), gs.BinghamFisher(np.diag([2.0, 1.0, 0.0, 0.0]), [3.0, 0.0, 0.0, 1.0]),
                               gs.MixtureModel([gs.VonMisesFisher([10.0, 0, 0, 0]), gs.VonMisesFisher([0, 0, 0, -20.0])])]),
        "d5": gs.MixtureModel([gs.random_bingham(d=5, vmax=20.0, vmin=0.0, seed=11),
                               gs.random_bingham(d=5, vmax=15.0, vmin=0.0, seed=12)]),
    }


@pytest.mark.parametrize("key", ["d3", "d4", "d5"])
@pytest.mark.parametrize("sampler", ["shrink", "reject"])
def test_fast_equals_exact_on_the_philox_stream(gs, key, sampler):
    """10^5 chains on the library's stream: the restricted-circle kernel and the exact one give the same chains."""
    pdf = _composites(gs)[key]
    cls = gs.ShrinkageSphericalSliceSampler if sampler == "shrink" else gs.RejectionSphericalSliceSampler
    n, d = 100_000, pdf.d
    x0 = gs.sample_sphere_device(d - 1, n, seed=3).T
    a = cls(pdf, x0, seed=17, mode="fast")
    assert "FastMixture<" in kernel_name(a, "fast", 1)
    b = cls(pdf, x0, seed=17, mode="exact")
    a.advance(20, keep=False)
    b.advance(20, keep=False)
    assert np.all(a.errors == 0) and np.all(b.errors == 0)
    assert np.max(np.abs(a.state - b.state)) < TOL
    assert np.array_equal(a.n_reject_per_chain, b.n_reject_per_chain)


@pytest.mark.parametrize("mode", ["fast", "exact"])
def test_split_launches_give_the_same_bits(gs, mode):
    pdf = _composites(gs)["d4"]
    x0 = gs.sample_sphere_device(3, 50_000, seed=8).T
    a = gs.ShrinkageSphericalSliceSampler(pdf, x0, seed=23, mode=mode)
    a.advance(30, keep=False)
    b = gs.ShrinkageSphericalSliceSampler(pdf, x0, seed=23, mode=mode)
    for _ in range(3):
        b.advance(10, keep=False)
    assert np.array_equal(a.state, b.state)
    assert np.array_equal(a.n_reject_per_chain, b.n_reject_per_chain)


def _kat_cases():
    z = golden("gmix_kat.npz")
    return sorted({k.split("__")[0] for k in z.files})


@pytest.mark.parametrize("name", _kat_cases())
def test_logprob_and_gradient_kat(gs, name):
    """log_prob and gradient against the reference, on numpy rows, one point, and CUDA tensors."""
    import torch
    z = golden("gmix_kat.npz")
    pdf = target(gs, z, prefix=f"{name}__")
    X, lp, gr = z[f"{name}__X"], z[f"{name}__logp"], z[f"{name}__grad"]
    rel = lambda a, b: np.max(np.abs(a - b) / np.maximum(1.0, np.abs(b)))  # noqa: E731
    assert rel(pdf.log_prob(X), lp) < TOL
    assert rel(pdf.gradient(X), gr) < TOL
    assert abs(pdf.log_prob(X[5]) - lp[5]) / max(1.0, abs(lp[5])) < TOL
    assert rel(pdf.gradient(X[5]), gr[5]) < TOL
    Xt = torch.from_numpy(X).cuda()
    assert rel(pdf.log_prob(Xt).cpu().numpy(), lp) < TOL
    assert rel(pdf.gradient(Xt).cpu().numpy(), gr) < TOL


@pytest.mark.parametrize("mode", ["fast", "exact"])
def test_running_statistics_equal_stored_draw_estimators(gs, mode):
    import torch
    dg = gs.diagnostics
    pdf = _composites(gs)["d3"]
    n_chains, d, L, thin, n_keep = 2000, 3, 16, 2, 200
    x0 = gs.sample_sphere_device(d - 1, n_chains, seed=5).T
    w = np.linspace(1.0, 2.0, d)
    s = gs.ShrinkageSphericalSliceSampler(pdf, x0, seed=11, mode=mode).enable_stats(lags=L, projection=w)
    assert s._stats["modes"] == 2  # the vMF mean and the Bingham mode; Uniform has none
    X = s.advance(n_keep * thin, thin=thin).permute(2, 0, 1).contiguous()
    r = s.stats()
    assert torch.allclose(r["mean"], X.mean(1), rtol=0, atol=1e-13)
    assert torch.allclose(r["second_moment"], torch.einsum("cti,ctj->cij", X, X) / n_keep, rtol=0, atol=1e-13)
    assert torch.allclose(r["geodesic_step"], dg.distance(X[:, 1:], X[:, :-1]).mean(1), rtol=1e-12, atol=1e-14)
    modes = torch.as_tensor(np.array(pdf._modes()), device=X.device)
    for c in (0, n_chains - 1):
        assert torch.allclose(r["mode_occupancy"][c], dg.mode_occupancy(X[c], modes), rtol=0, atol=1e-15)
    P = X @ torch.as_tensor(w, device=X.device)
    assert torch.allclose(r["acf"], dg.acf(P, L + 1), rtol=0, atol=1e-11)


@pytest.mark.parametrize("name", MH)
def test_baselines_reproduce_reference_chain(gs, name):
    """RWMH and spherical HMC (the latter through the mixture's gradient) replaying the reference's draws."""
    z = golden(name + ".npz")
    pdf = target(gs, z)
    if str(z["sampler"]) == "rwmh":
        s = gs.MetropolisHastings(pdf, z["x0"], 1, stepsize=float(z["stepsize0"]))
    else:
        s = gs.SphericalHMC(pdf, z["x0"], 1, stepsize=float(z["stepsize0"]), n_steps=int(z["n_leapfrog"]))
    n = len(z["states"]) - 1
    s.reset(int(z["burnin"]))
    got = s.advance(n, thin=1, replay=z["draws"][None])[:, :, 0].cpu().numpy()
    assert s.errors[0] == 0
    if str(z["sampler"]) == "hmc":
        # the reference's own HMC chain is chaotic here: a relative change of 1e-14 in its gradient moves the d = 3 chain by
        # 1e-11 at step 50 and by O(1) after step 83 (d = 5: 7e-7 by step 300), so the comparison stops at step 40
        h = 40
        assert np.max(np.abs(got[:h] - z["states"][1:h + 1])) < 1e-9
        acc = np.any(got != np.vstack([z["x0"][None], got[:-1]]), axis=1)
        assert np.array_equal(acc[:h], z["accept"].astype(bool)[:h])
    else:
        assert np.max(np.abs(got - z["states"][1:])) < TOL
        assert s.n_accept == int(z["n_accept"])


def test_c_abi_refusals(gs):
    lib = gs._lib.load()
    A3 = np.ascontiguousarray(np.eye(3))
    A4 = np.ascontiguousarray(np.eye(4))

    def create(descs, logw):
        arr = (gs._lib.TargetDesc * len(descs))(*descs)
        lw = np.ascontiguousarray(logw, dtype=np.float64)
        h = C.c_void_p()
        rc = lib.gsss_target_create_mixture(arr, len(descs), lw.ctypes.data_as(C.c_void_p), 0, C.byref(h))
        if rc == 0:
            lib.gsss_target_destroy(h)
        return rc, lib.gsss_last_error().decode()

    def bingham(A):
        return gs._lib.TargetDesc(gs._lib.BINGHAM, len(A), 0, 0, None, None, A.ctypes.data_as(C.c_void_p), None, 0.0)

    assert create([bingham(A3), bingham(A3)], [0.0, -np.inf])[0] == 0
    rc, msg = create([bingham(A3), bingham(A4)], [0.0, 0.0])
    assert rc == -1 and "share d" in msg
    cpd = gs._lib.TargetDesc(gs._lib.CPD, 4, 8, 0, None, None, None, None, 0.0)
    rc, msg = create([bingham(A4), cpd], [0.0, 0.0])
    assert rc == -2 and "registration" in msg
    rc, msg = create([bingham(A3)] * 17, [0.0] * 17)
    assert rc == -2 and "at most 16" in msg


def test_readme_bingham_mixture_runs_in_fast_mode(gs):
    A1 = gs.random_bingham(d=5, vmax=20.0, vmin=0.0, seed=11).A
    A2 = gs.random_bingham(d=5, vmax=15.0, vmin=0.0, seed=12).A
    pdf = gs.MixtureModel([gs.Bingham(A1), gs.Bingham(A2)])
    s = gs.ShrinkageSphericalSliceSampler(pdf, gs.sample_sphere_device(4, 4096, seed=1).T, seed=3)
    assert s.mode == "fast"
    out = s.sample(50, burnin=10)
    assert out.shape[-1] == 5 and np.all(s.errors == 0)

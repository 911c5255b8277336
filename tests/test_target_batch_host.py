"""TargetBatch without a GPU: what it packs, when its device copy is renewed, every refusal that needs no device, the
rules that tie chains to targets, and the register / occupancy budget of the batch builds of d = 11 .. 16."""
import ctypes as C

import numpy as np
import pytest

import geosss_amd as gs
from geosss_amd import _lib, ensemble
from geosss_amd.mcmc import _MODES  # noqa: F401  (the module imports without a device)

README_MUS = 80.0 * np.array([[0.87, -0.37, 0.33], [-0.20, -0.89, -0.40], [0.19, 0.22, -0.96]])


def _mixtures(M, d=3, K=3, seed=0):
    g = np.random.default_rng(seed)
    out = []
    for _ in range(M):
        mu = g.standard_normal((K, d))
        mu *= (20.0 + 60.0 * g.random((K, 1))) / np.linalg.norm(mu, axis=1, keepdims=True)
        out.append(gs.MixtureModel([gs.VonMisesFisher(m) for m in mu], g.random(K) + 0.5))
    return out


def _binghams(M, d=5, seed=1, diagonal=False):
    return [gs.random_bingham(d, vmax=30.0, vmin=0.0, eigensystem=diagonal, seed=seed + t) for t in range(M)]


def test_len_d_pdfs():
    pdfs = _binghams(4)
    b = gs.TargetBatch(pdfs)
    assert len(b) == 4 and b.d == 5 and b.pdfs == pdfs and b.pdfs is not pdfs
    assert isinstance(b, gs.Distribution)
    assert gs.TargetBatch(iter(pdfs)).pdfs == pdfs


def test_pack_order_stride_and_flags():
    pdfs = _mixtures(5, d=4, K=3)
    kind, d, k, kappa, arrays, extra = gs.TargetBatch(pdfs)._pack(chains_per_target=64)
    assert (kind, d, k, kappa, arrays) == (_lib.VMF_MIXTURE, 4, 3, 0.0, ())
    assert extra["chains_per_target"] == 64 and len(extra["batch"]) == 5
    for member, p in zip(extra["batch"], pdfs):  # in order, each as the member packs itself: K d + K doubles, an equal stride
        mk, md, mkk, _, (mu, logc, A, knots) = member
        want = p._pack()
        assert (mk, md, mkk) == (_lib.VMF_MIXTURE, 4, 3) and A is None and knots is None
        assert np.array_equal(mu, want[4][0]) and np.array_equal(logc, want[4][1])
        assert mu.size + logc.size == 3 * 4 + 3
    # a single VonMisesFisher is a mixture of one term
    assert gs.TargetBatch([gs.VonMisesFisher(k * np.eye(3)[0]) for k in (1.0, 10.0)])._pack()[:3] == (_lib.VMF_MIXTURE, 3, 1)
    # Bingham: A, and b for Fisher-Bingham (its presence is the flag the library reads)
    bf = gs.TargetBatch([gs.BinghamFisher(p.A, np.arange(5.0)) for p in _binghams(3)])._pack()
    assert bf[0] == _lib.BINGHAM and all(m[4][0] is not None and m[4][2].shape == (5, 5) for m in bf[5]["batch"])
    bp = gs.TargetBatch(_binghams(3))._pack()
    assert all(m[4][0] is None for m in bp[5]["batch"])


def test_device_key_follows_member_edits_and_m():
    pdfs = _binghams(3)
    b = gs.TargetBatch(pdfs)
    k0 = b._device_key(b._pack(8))
    assert k0 == b._device_key(b._pack(8))
    assert k0 != b._device_key(b._pack(16))          # the handle carries m
    pdfs[1].A[0, 0] += 1.0                           # b.pdfs holds the same objects
    k1 = b._device_key(b._pack(8))
    assert k1 != k0
    b.pdfs[2] = gs.random_bingham(5, vmax=3.0, seed=99)
    assert b._device_key(b._pack(8)) != k1
    mix = gs.TargetBatch(_mixtures(2))
    k2 = mix._device_key(mix._pack(4))
    mix.pdfs[0].pdfs[1].mu[0] += 0.5
    assert mix._device_key(mix._pack(4)) != k2


def test_refused_members():
    curve = gs.CurvedVonMisesFisher(gs.SlerpCurve(gs.brownian_curve(5, 3)), 100.0)
    general = gs.MixtureModel([gs.VonMisesFisher(README_MUS[0]), gs.Bingham(np.diag([1.0, 2.0, 3.0]))])
    with pytest.raises(TypeError, match="at least one"):
        gs.TargetBatch([])
    with pytest.raises(TypeError, match="CurvedVonMisesFisher"):
        gs.TargetBatch([curve, curve])
    with pytest.raises(TypeError, match="GSSS_MIXTURE"):
        gs.TargetBatch([general, general])
    with pytest.raises(TypeError, match="TargetBatch is not a member"):
        gs.TargetBatch([gs.TargetBatch(_binghams(2)), gs.TargetBatch(_binghams(2))])
    with pytest.raises(TypeError, match="host-side"):
        gs.TargetBatch([gs.ACG(np.eye(3))])
    with pytest.raises(TypeError, match="not a device target"):
        gs.TargetBatch([object()])
    with pytest.raises(TypeError, match="one family"):
        gs.TargetBatch([gs.VonMisesFisher(README_MUS[0]), gs.Bingham(np.eye(3))])

    class UserLike(gs.Distribution):   # what DeviceDistribution sets (compiling one needs no GPU but minutes)
        _device_source = True
        d = 3
    with pytest.raises(TypeError, match="user target"):
        gs.TargetBatch([UserLike()])
    g = np.random.default_rng(3)
    cpd = gs.CoherentPointDrift(gs.PointCloud(g.standard_normal((12, 3))), gs.PointCloud(g.standard_normal((10, 3))), sigma=0.5, k=4)
    with pytest.raises(TypeError, match="CoherentPointDrift is not built as a batch member"):
        gs.TargetBatch([cpd, cpd])


def test_refused_shapes():
    with pytest.raises(ValueError, match="share the dimension"):
        gs.TargetBatch(_binghams(2, d=5) + _binghams(1, d=6))
    with pytest.raises(ValueError, match="number of terms"):
        gs.TargetBatch(_mixtures(2, K=3) + _mixtures(1, K=4))
    with pytest.raises(ValueError, match="linear term"):
        gs.TargetBatch([_binghams(1)[0], gs.BinghamFisher(np.eye(5), np.ones(5))])


def _x0(n, d):
    x = np.random.default_rng(5).standard_normal((n, d))
    return x / np.linalg.norm(x, axis=1, keepdims=True)


@pytest.mark.parametrize("cls", [gs.ShrinkageSphericalSliceSampler, gs.RejectionSphericalSliceSampler])
def test_sampler_refusals_need_no_device(cls):
    b = gs.TargetBatch(_binghams(4))
    with pytest.raises(ValueError, match="multiple of 4 chains"):
        cls(b, _x0(10, 5), seed=1)
    with pytest.raises(ValueError, match="multiple of chains_per_target"):
        cls(b, _x0(10, 5), seed=1, chains_per_target=4)
    with pytest.raises(ValueError, match="chain_offset .* multiple of the chains per target"):
        cls(b, _x0(8, 5), seed=1, chain_offset=3, chains_per_target=4)
    with pytest.raises(ValueError, match="reach past the last"):
        cls(b, _x0(8, 5), seed=1, chain_offset=12, chains_per_target=4)
    with pytest.raises(ValueError, match="rng='philox'"):
        cls(b, _x0(8, 5), seed=1, rng="numpy")
    with pytest.raises(ValueError, match="belongs to a TargetBatch"):
        cls(b.pdfs[0], _x0(8, 5), seed=1, chains_per_target=4)


@pytest.mark.parametrize("cls", [gs.MetropolisHastings, gs.SphericalHMC, gs.IndependenceSampler, gs.MixtureRWMHIndependenceSampler])
def test_mh_and_hmc_refuse_a_batch(cls):
    with pytest.raises(TypeError, match="does not sample a TargetBatch"):
        cls(gs.TargetBatch(_binghams(2)), _x0(8, 5), seed=1)


def test_shards_may_not_cut_a_target():
    b = gs.TargetBatch(_binghams(6))
    assert ensemble.batch_chains_per_target(b.pdfs[0], 600, 0, 300) is None
    assert ensemble.batch_chains_per_target(b, 600, 0, 600) == 100
    assert ensemble.batch_chains_per_target(b, 600, 200, 400) == 100
    with pytest.raises(ValueError, match="cuts a target's block"):
        ensemble.batch_chains_per_target(b, 600, 0, 150)       # four ranks: 150 chains each, 100 per target
    with pytest.raises(ValueError, match="multiple of 6 chains"):
        ensemble.batch_chains_per_target(b, 601, 0, 601)


def test_library_exports_the_batch_entry_point():
    lib = _lib.load()
    assert lib.gsss_abi_version() == 10                        # a further entry point, the same ABI
    assert "gsss_target_create_batch" in _lib.SIGNATURES
    h = C.c_void_p()
    assert lib.gsss_target_create_batch(None, 1, 1, 0, C.byref(h)) == -1   # GSSS_E_INVALID, before any device is looked for
    assert b"null" in lib.gsss_last_error()


WIDE_UNITS = {"gsss_batch_vmf_wide_a.hip": (11, 12, 13), "gsss_batch_vmf_wide_b.hip": (14, 15, 16),
              "gsss_batch_bingham_wide_a.hip": (11, 12, 13), "gsss_batch_bingham_wide_b.hip": (14, 15, 16)}


def test_wide_batch_kernels_do_not_spill():
    """The batch builds of the one-chain-per-lane kernels at d = 11 .. 16 are held to the budget of the screened kernels they
    stand beside (tests/test_abi.py::test_wide_lane_kernels_do_not_spill): no scratch, at least two wavefronts per SIMD.
    Screened -- vMF: three component buckets per dimension; Bingham: the diagonal and the general target.  All-double
    (fast_kernel) -- vMF: the buckets 4 and 10; Bingham: one."""
    from geosss_amd import build
    screened = double = 0
    for src, dims in WIDE_UNITS.items():
        for name, r in build.resource_usage(src).items():
            if "screened_kernel" in name or "fast_kernel" in name:
                assert "BatchBlock" in name, name        # batch builds only in these units
                screened += "screened_kernel" in name
                double += "fast_kernel" in name
                assert r["scratch"] == 0 and r["occupancy"] >= 2, (name, r)
    assert screened == 6 * 3 + 6 * 2 and double == 6 * 2 + 6


def test_no_batch_build_in_the_counted_units():
    """tests/test_abi.py counts the screened_kernel instantiations of four units by name: the batch builds live elsewhere."""
    import os
    csrc = os.path.join(os.path.dirname(gs.__file__), "csrc")
    for src in ("gsss_fast_vmf_d12.hip", "gsss_fast_vmf_d16.hip", "gsss_fast_bingham_wide_a.hip", "gsss_fast_bingham_wide_b.hip"):
        assert "batch" not in open(os.path.join(csrc, src)).read()
    assert all(os.path.exists(os.path.join(csrc, u)) for u in WIDE_UNITS)

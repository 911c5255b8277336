"""The fast-mode launch plan of a TargetBatch (gsss_batch_plan, TargetBatch.launch_plan) without a GPU: the arithmetic of the
plan, the LDS budget behind it, and the register budget of the shared batch builds of d = 11 .. 16.

The rule restated here, independently of the library: m a multiple of 256 -- one target per workgroup,
256 chains; otherwise a workgroup takes the largest run of consecutive chains (<= 256) that touches no more targets than its LDS
share holds.  The share: the CU's 128 LDS granules of 1280 B divided among the workgroups the batch builds of the shape keep
resident (five on S^2, three for mixtures of K >= 5, else four), less the 130 doubles of draw tables.  A target is budgeted the
widest rows any batch kernel of the shape stages -- K_C (d + 1) doubles in the larger of the screened and the all-double
bucket, d d + d for Bingham -- padded to an odd count."""
import ctypes as C
import re

import numpy as np
import pytest

import geosss_amd as gs
from geosss_amd import _lib

DIMS = (3, 5, 10, 11, 16)
MS = (1, 3, 16, 64, 100, 256, 300, 1024)
M = 4096


def shapes():
    for d in DIMS:
        for fam in ("bingham_diag", "bingham_dense", "bingham_b"):
            yield fam, d, 0
        for K in (1, 3, 10, 16):
            if d <= 10 or K <= 10:      # d = 11 .. 16: lane kernels for K <= 10
                yield "vmf", d, K


def bucket(k, bs):
    return next((b for b in bs if k <= b), bs[-1])


def padded_blob_doubles(fam, d, K):
    if fam != "vmf":
        return (d * d + d) | 1
    kc = max(bucket(K, (3, 6, 10)), bucket(K, (4, 10))) if d >= 11 else max(bucket(K, (3, 4, 6, 10, 16)), bucket(K, (4, 16)))
    return (kc * (d + 1)) | 1


def resident(fam, d, K):
    if fam == "vmf" and K >= 5:
        return 3
    return 5 if d == 3 else 4


def lds_share_doubles(fam, d, K):
    return (128 // resident(fam, d, K)) * 1280 // 8 - 130


def plan(fam, d, K, n_targets, m):
    out = C.c_int32(), C.c_int32(), C.c_int64(), C.c_double()
    kind = _lib.VMF_MIXTURE if fam == "vmf" else _lib.BINGHAM
    k = K if fam == "vmf" else int(fam == "bingham_diag")
    rc = _lib.load().gsss_batch_plan(kind, d, k, int(fam == "bingham_b"), n_targets, m, *(C.byref(o) for o in out))
    assert rc == 0, _lib.load().gsss_last_error()
    return tuple(o.value for o in out)


def touched(c, m, n):
    """the most targets a workgroup's run touches: runs [w c, (w + 1) c) of n chains, targets of m chains"""
    starts = np.arange(0, n, c)
    ends = np.minimum(starts + c, n) - 1
    return int(np.max(ends // m - starts // m + 1))


def test_exported_and_bound():
    lib = _lib.load()
    assert "gsss_batch_plan" in _lib.SIGNATURES and hasattr(lib, "gsss_batch_plan")
    assert lib.gsss_abi_version() == 10
    assert lib.gsss_batch_plan(_lib.BINGHAM, 5, 0, 0, 8, 64, None, None, None, None) == 0        # any pointer may be NULL
    assert lib.gsss_batch_plan(_lib.BINGHAM, 24, 0, 0, 8, 64, None, None, None, None) == -2      # GSSS_E_UNSUPPORTED, no device needed
    assert b"no fast-mode batch kernel" in lib.gsss_last_error()
    assert lib.gsss_batch_plan(_lib.VMF_MIXTURE, 12, 16, 0, 8, 64, None, None, None, None) == -2
    assert lib.gsss_batch_plan(_lib.CURVE_VMF, 10, 5, 0, 8, 64, None, None, None, None) == -2


@pytest.mark.parametrize("fam,d,K", list(shapes()))
def test_plan_arithmetic_and_lds_budget(fam, d, K):
    for m in MS:
        cpw, tpw, grid, use = plan(fam, d, K, M, m)
        assert 1 <= cpw <= 256 and grid == -(-M * m // cpw), (m, cpw, grid)
        assert use == M * m / (grid * cpw), (m, use)
        assert tpw * padded_blob_doubles(fam, d, K) <= lds_share_doubles(fam, d, K), (m, tpw)
        assert tpw == touched(cpw, m, M * m), (m, cpw, tpw)      # the LDS a launch takes covers every workgroup's run, and no more
        if m % 256 == 0:
            assert (cpw, tpw, grid, use) == (256, 1, M * m // 256, 1.0), m      # today's launch
        else:
            fit = lds_share_doubles(fam, d, K) // padded_blob_doubles(fam, d, K)
            assert cpw == max(c for c in range(1, 257) if touched(c, m, M * m) <= fit), (m, cpw, fit)
        if m >= 16:
            assert use >= 0.9, (m, use)       # (no shape of the list misses it)


def test_small_batches_and_one_target():
    for n_targets in (1, 2, 5):
        for m in (1, 3, 16, 100, 300):
            cpw, tpw, grid, use = plan("bingham_dense", 5, 0, n_targets, m)
            assert grid == -(-n_targets * m // cpw) and touched(cpw, m, n_targets * m) <= tpw <= n_targets


def test_launch_plan_is_the_c_function():
    b = gs.TargetBatch([gs.random_bingham(5, vmax=30.0, vmin=0.0, seed=t) for t in range(12)])
    for m in (16, 100, 256):
        cpw, tpw, grid, use = plan("bingham_dense", 5, 0, 12, m)
        assert b.launch_plan(m) == {"chains_per_workgroup": cpw, "targets_per_workgroup": tpw, "grid": grid, "lane_use": use}
    mix = gs.TargetBatch([gs.MixtureModel([gs.VonMisesFisher(mu) for mu in 50.0 * np.eye(3)]) for _ in range(7)])
    assert mix.launch_plan(64) == dict(zip(("chains_per_workgroup", "targets_per_workgroup", "grid", "lane_use"), plan("vmf", 3, 3, 7, 64)))
    with pytest.raises(ValueError, match="no fast-mode batch kernel"):
        gs.TargetBatch([gs.random_bingham(24, vmax=30.0, vmin=0.0, seed=t) for t in range(2)]).launch_plan(8)


SHARED_WIDE_UNITS = ("gsss_batch_shared_vmf_wide_a.hip", "gsss_batch_shared_vmf_wide_b.hip",
                     "gsss_batch_shared_bingham_wide_a.hip", "gsss_batch_shared_bingham_wide_b.hip")


def test_shared_wide_kernels_do_not_spill():
    """The shared batch builds of d = 11 .. 16 keep the budget of the batch builds beside them
    (tests/test_target_batch_host.py::test_wide_batch_kernels_do_not_spill): no scratch, at least two wavefronts per SIMD -- and no
    code object is resident more often than the plan's LDS share assumes."""
    from geosss_amd import build
    screened = double = 0
    for src in SHARED_WIDE_UNITS:
        for name, r in build.resource_usage(src).items():
            if "screened_kernel" in name or "fast_kernel" in name:
                assert "BatchShared" in name, name        # shared builds only in these units
                screened += "screened_kernel" in name
                double += "fast_kernel" in name
                assert r["scratch"] == 0 and r["occupancy"] >= 2, (name, r)
                d = int(re.search(r"_kernelILi(\d+)E", name).group(1))
                kc = re.search(r"VmfILi\d+ELi(\d+)E", name)     # (the bucket stands for its largest K)
                assert 11 <= d <= 16 and r["occupancy"] <= resident("vmf" if kc else "bingham", d, int(kc.group(1)) if kc else 0), (name, r)
    assert screened == 6 * 3 + 6 * 2 and double == 6 * 2 + 6

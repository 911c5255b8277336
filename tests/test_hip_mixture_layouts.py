"""Chains of the generic mixture (GSSS_MIXTURE) beyond the lane layouts: the exact kernels in the cooperative layouts, with the
components' rows in LDS and in global memory, and FastMixture at d = 6 .. 16, against a restatement of the two slice-sampler
transitions on the extended-precision log_prob (layout_cases.slice_chain).  The device replays the reference chain's draws.

States at 1e-10; tries, rejections and error bits exact.  Every case's reference chain keeps its proposals further than 1e-8
from their thresholds (asserted here, evaluated on the CPU by test_reference_math.py::test_chain_margins), so no accept / reject
decision hangs on rounding."""
import numpy as np
import pytest

import layout_cases as lc

pytestmark = pytest.mark.gpu

TOL = 1e-10


@pytest.fixture(scope="module")
def gs():
    import torch
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    import geosss_amd
    geosss_amd._lib.require_device()
    yield geosss_amd
    lc.release()  # the cached targets' device copies go with the module
    torch.cuda.synchronize()


def sampler_cls(gs, sampler):
    return gs.ShrinkageSphericalSliceSampler if sampler == "shrink" else gs.RejectionSphericalSliceSampler


def kernel_name(s, mode, placement=0):
    return s._lib.gsss_kernel_name(s._target_dev.handle, 1 if mode == "fast" else 0, 0, placement).decode()


def _params():
    out = []
    for case in lc.CHAIN_CASES:
        for sampler in ("shrink", "reject"):
            out += [(case, sampler, "exact", "auto"), (case, sampler, "exact", "packed")]
            if case[0] == "d" and "curve" not in case and 3 <= int(case[1:]) <= 16:
                out += [(case, sampler, "fast", "auto"), (case, sampler, "fast", "packed")]
    return out


@pytest.mark.parametrize("case,sampler,mode,placement", _params())
def test_replay_reproduces_reference_chain(gs, case, sampler, mode, placement):
    pdf, fast_built = lc.chain_target(case)
    assert fast_built or mode == "exact"
    ref = lc.reference_chain(case, sampler)
    assert ref["margin"] > lc.MIN_MARGIN
    s = sampler_cls(gs, sampler)(pdf, ref["x0"], seed=1, mode=mode, placement=placement)
    assert s.mode == mode
    if mode == "fast":
        assert "FastMixture<" in kernel_name(s, mode, 2 if placement == "auto" else 1)
    else:
        name = kernel_name(s, mode)
        assert name.endswith("Mixture>")
        if case.startswith("gmix_"):
            assert f"<{lc.global_case(case)[2]}," in name
    got = s.advance(lc.N_STEPS, thin=1, replay=ref["replay"]).cpu().numpy().transpose(0, 2, 1)
    assert np.all(s.errors == 0)
    print(f"{case} {sampler} {mode} {placement}: max |dx| {np.max(np.abs(got - ref['states'])):.1e}, margin {ref['margin']:.1e}")
    assert np.array_equal(np.asarray(s.n_tries_per_chain), ref["tries"])
    assert np.array_equal(np.asarray(s.n_reject_per_chain), ref["rejections"])
    assert np.max(np.abs(got - ref["states"])) < TOL


@pytest.mark.parametrize("sampler", ["shrink", "reject"])
@pytest.mark.parametrize("d", [6, 8, 11, 13, 16])
def test_fast_equals_exact_on_the_library_stream(gs, d, sampler):
    """FastMixture against the exact kernel of the dimension's own layout (lane6, lane8, coop4x4) on the Philox stream."""
    pdf, fast_built = lc.chain_target(f"d{d}")
    assert fast_built
    x0 = gs.sample_sphere_device(d - 1, 4096, seed=3).T
    a = sampler_cls(gs, sampler)(pdf, x0, seed=17, mode="fast")
    assert "FastMixture<" in kernel_name(a, "fast", 1)
    b = sampler_cls(gs, sampler)(pdf, x0, seed=17, mode="exact")
    a.advance(20, keep=False)
    b.advance(20, keep=False)
    assert np.all(a.errors == 0) and np.all(b.errors == 0)
    assert np.max(np.abs(a.state - b.state)) < TOL
    assert np.array_equal(a.n_reject_per_chain, b.n_reject_per_chain)

"""Where the lane kernels put a kept row (kept_row, gsss_device.h: the row's first component by one 32 x 32 -> 64 bit
multiply-add, the further components a wave-uniform stride apart -- in the keep path of screened_kernel and fast_kernel, the
rows held back in LDS included).  Both layouts (component-major [row][d][chain], chain-major [chain][row][d] appended at
row0 > 0), both packings of the lanes, d = 3 and d = 5, a ragged 300 chains, thin = 3, two launches of 10 steps: every kept row
is the state a twin sampler holds after that step when it is advanced one step a launch (chains are keyed by (chain, step)),
and nothing else of the buffer is touched: a guard of NaN around it, and the chain-major rows no launch writes, stay NaN."""
import pytest

from conftest import golden
from helpers import product_target

pytestmark = pytest.mark.gpu

N, THIN, LAUNCH = 300, 3, 10
KEPT_STEPS = (3, 6, 9, 13, 16, 19)  # a launch keeps every third of ITS steps
GUARD = 1024
TARGETS = {"readme_d3": ("traj_vmfmix_readme", "ScreenVmf<3"), "bingham_d5": ("traj_bingham_d5_dense", "ScreenBingham<5")}


@pytest.fixture(scope="module")
def gs():
    import torch
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    import geosss_amd
    geosss_amd._lib.require_device()
    return geosss_amd


_twins = {}


def _twin(gs, name):
    """(x0, the states [6][d][chain] after the kept steps, the last state) of a sampler advanced one step a launch"""
    import torch
    if name not in _twins:
        pdf = product_target(golden(TARGETS[name][0] + ".npz"))
        x0 = gs.sample_sphere_device(pdf.d - 1, N, seed=43).T
        s = gs.ShrinkageSphericalSliceSampler(pdf, x0, seed=17, mode="fast", placement="packed", chain_offset=9, step_offset=4)
        kept = []
        for step in range(1, 2 * LAUNCH + 1):
            s.advance(1)
            if step in KEPT_STEPS:
                kept.append(s.state_device.clone())
        assert int((s._err != 0).sum()) == 0
        _twins[name] = (pdf, x0, torch.stack(kept), s.state_device.clone())
    return _twins[name]


@pytest.mark.parametrize("packing", ["two_per_lane", "one_per_lane"])
@pytest.mark.parametrize("layout", ["component_major", "chain_major"])
@pytest.mark.parametrize("name", list(TARGETS))
def test_kept_rows_are_the_twin_states(gs, name, layout, packing, monkeypatch):
    """(bingham_d5, chain_major, one_per_lane: the build that holds rows of 40 bytes back in LDS until a run of them ends on a
    32-byte sector, and stores what is left when the launch ends)"""
    import torch
    monkeypatch.delenv("GSSS_ONE_PER_LANE", raising=False)  # the twin: the library's own choice
    pdf, x0, want, last = _twin(gs, name)
    d = pdf.d
    monkeypatch.setenv("GSSS_ONE_PER_LANE", "0" if packing == "two_per_lane" else "2")
    s = gs.ShrinkageSphericalSliceSampler(pdf, x0, seed=17, mode="fast", placement="packed", chain_offset=9, step_offset=4)
    kernel = s._lib.gsss_kernel_name(s._target_dev.handle, 1, 0, 1).decode()
    assert kernel.startswith("screened_kernel") and TARGETS[name][1] in kernel, kernel
    per = LAUNCH // THIN
    nan = float("nan")
    if layout == "component_major":
        flats = [torch.full((2 * GUARD + per * d * N,), nan, dtype=torch.float64, device="cuda") for _ in range(2)]
        for flat in flats:
            s.advance(LAUNCH, thin=THIN, out=flat[GUARD:GUARD + per * d * N].view(per, d, N))
        got = torch.cat([flat[GUARD:GUARD + per * d * N].view(per, d, N) for flat in flats], dim=0)
        assert torch.equal(got, want)
        for flat in flats:
            assert bool(torch.isnan(flat[:GUARD]).all()) and bool(torch.isnan(flat[-GUARD:]).all())
    else:
        R = 8                                     # rows 1 .. 3 by the first launch, 4 .. 6 by the second; 0 and 7 by none
        flat = torch.full((2 * GUARD + N * R * d,), nan, dtype=torch.float64, device="cuda")
        buf = flat[GUARD:GUARD + N * R * d].view(N, R, d)
        s.advance(LAUNCH, thin=THIN, out=buf, chain_major=True, row0=1)
        s.advance(LAUNCH, thin=THIN, out=buf, chain_major=True, row0=1 + per)
        assert torch.equal(buf[:, 1:1 + 2 * per].permute(1, 2, 0), want)
        assert bool(torch.isnan(buf[:, 0]).all()) and bool(torch.isnan(buf[:, 7]).all())
        assert bool(torch.isnan(flat[:GUARD]).all()) and bool(torch.isnan(flat[-GUARD:]).all())
    assert torch.equal(s.state_device, last) and int((s._err != 0).sum()) == 0

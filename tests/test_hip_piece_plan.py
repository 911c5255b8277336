"""The piece plan of the lane kernels on the GPU (piece_plan, SliceSched::take_piece in gsss_device.h; tests/test_piece_plan.py
checks the plan itself without one): a launch whose chunks of chains are no whole number of rounds of resident workgroups runs
every chunk whole or as a head and a tail on two workgroups, the chunk's state, counters, flags and statistics handed over once
through HBM.  Chains are keyed by (chain, step), so every bit is the one the unsplit launch (GSSS_SLICE_STEPS=0) leaves.

Small plans: GSSS_RESIDENT_PER_CU=1 plans for 256 resident workgroups on every box."""
import ctypes as C

import pytest

from conftest import golden
from helpers import product_target

pytestmark = pytest.mark.gpu

RESIDENT = 256
ROUNDS = {"1.02": 262, "1.53": 392, "2.3": 589}        # chunks of chains on 256 slots
LAUNCHES = (1000, 300)                                 # two launches in a row
# name of the golden target, environment, chains per chunk, what is kept
KERNELS = {
    "readme_two_per_lane": ("vmfmix_readme", {"GSSS_ONE_PER_LANE": "0"}, 512, "rows"),
    "k10_kappa500_one_per_lane": ("vmfmix_k10_kappa500", {"GSSS_ONE_PER_LANE": "2"}, 256, "rows"),
    "bingham_d10_rows_held_in_lds": ("bingham_d10_vmax30", {"GSSS_ONE_PER_LANE": "2"}, 256, "chain_major"),
    "readme_statistics": ("vmfmix_readme", {}, 256, "stats"),
}


@pytest.fixture(scope="module")
def gs():
    import torch
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    import geosss_amd
    geosss_amd._lib.require_device()
    return geosss_amd


def _last_launch(s):
    grid, steps, frac = C.c_int64(0), C.c_int32(0), C.c_double(-1.0)
    s._lib.gsss_last_launch(C.byref(grid), C.byref(steps), C.byref(frac))
    return int(grid.value), int(steps.value), float(frac.value)


def _run(gs, pdf, x0, sampler, keep, planned, n_chunks):
    """two launches; the tensors to compare, the rows of every launch, and what the launches reported"""
    import torch
    cls = gs.RejectionSphericalSliceSampler if sampler == "reject" else gs.ShrinkageSphericalSliceSampler
    s = cls(pdf, x0, seed=6, mode="fast", placement="packed", step_offset=91, max_tries=24 if sampler == "shrink" else 1 << 20)
    assert s._lib.gsss_kernel_name(s._target_dev.handle, 1, 0, 1).decode().startswith("screened_kernel")
    if keep == "stats":
        s.enable_stats(lags=8)
    n, d = x0.shape
    rows, reports = [], []
    for n_steps in LAUNCHES:
        if keep == "stats":
            s.advance(n_steps, thin=13, keep=False)
        elif keep == "chain_major":            # (chains, draws, dims): rows of 80 bytes, held back in LDS until a run ends on a sector
            buf = torch.zeros((n, n_steps // 13, d), dtype=torch.float64, device="cuda")
            s.advance(n_steps, thin=13, out=buf, chain_major=True)
            rows.append(buf)
        else:
            rows.append(s.advance(n_steps, thin=13).clone())
        grid, steps, frac = _last_launch(s)
        reports.append((steps, frac))
        if planned:
            assert steps == (n_steps + 1) // 2 and 0.0 < frac < 1.0, (n_steps, steps, frac)
            assert n_chunks < grid < n_chunks + RESIDENT and grid - n_chunks == round(frac * n_chunks), (grid, n_chunks, frac)
        else:
            assert (grid, steps, frac) == (n_chunks, 0, 0.0)
    out = [s.state_device.clone(), s._n_tries.clone(), s._n_reject.clone(), s._err.clone()]
    if keep == "stats":
        out.append(s._stats["acc"].clone())
    return out, rows


def _compare(whole, planned, keep, sampler, n_chains):
    import torch
    (w, w_rows), (p, p_rows) = whole, planned
    for i, (a, b) in enumerate(zip(w, p)):
        assert torch.equal(a, b), i
    ok = w[3] == 0                              # (a stopped chain writes no further rows: those slots of the buffer are unspecified)
    for a, b in zip(w_rows, p_rows):
        if keep == "chain_major":
            assert torch.equal(a[ok], b[ok])
        else:
            assert torch.equal(a[:, :, ok], b[:, :, ok])
    if sampler == "shrink":
        assert 0 < int((~ok).sum()) < n_chains   # chains stop inside a head and stay stopped in the tail; healthy ones beside them
    else:
        assert int((~ok).sum()) == 0


def _cases():
    for kernel in KERNELS:
        for rounds in ROUNDS:
            yield kernel, rounds, "shrink"
    yield "readme_two_per_lane", "1.53", "reject"
    yield "k10_kappa500_one_per_lane", "2.3", "reject"
    yield "bingham_d10_rows_held_in_lds", "1.02", "reject"


@pytest.mark.parametrize("kernel,rounds,sampler", list(_cases()))
def test_planned_launch_equals_the_unsplit_one(gs, kernel, rounds, sampler, monkeypatch):
    """States, kept rows of chains without error (thin = 13: rows straddle piece boundaries), tries, rejections, error flags and
    statistics rows of two planned launches in a row (1000 and 300 steps from step_offset 91, a ragged last chunk) equal those of
    the launches run one workgroup per chunk, and each planned launch reports its plan."""
    name, env, per_chunk, keep = KERNELS[kernel]
    z = golden(f"traj_{name}.npz")
    pdf = product_target(z)
    d = len(z["x0"])
    n_chunks = ROUNDS[rounds]
    n_chains = n_chunks * per_chunk - 77
    monkeypatch.setenv("GSSS_RESIDENT_PER_CU", str(RESIDENT // 256))
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    x0 = gs.sample_sphere_device(d - 1, n_chains, seed=43).T
    monkeypatch.setenv("GSSS_SLICE_STEPS", "0")
    whole = _run(gs, pdf, x0, sampler, keep, False, n_chunks)
    monkeypatch.delenv("GSSS_SLICE_STEPS")
    monkeypatch.setenv("GSSS_PIECE_PLAN", "1")
    planned = _run(gs, pdf, x0, sampler, keep, True, n_chunks)
    _compare(whole, planned, keep, sampler, n_chains)


def test_planned_headline_launch_equals_uniform_slices(gs, monkeypatch):
    """The bench's headline launch -- 10^6 README chains x 1000 steps, 1954 chunks on 1280 slots -- planned (about 1240 chunks
    split once, each head's state written through from XCD to XCD) against the uniform 128-step slices of the last round
    (GSSS_PIECE_PLAN=0): every state bit, every retained row, every counter."""
    import torch
    z = golden("traj_vmfmix_readme.npz")
    pdf = product_target(z)
    n = 1_000_000
    x0 = gs.sample_sphere_device(2, n, seed=49).T
    monkeypatch.setenv("GSSS_RESIDENT_PER_CU", "5")          # five workgroups per CU: the headline's plan
    monkeypatch.delenv("GSSS_SLICE_STEPS", raising=False)
    out, report = {}, {}
    for label in ("0", "1"):
        monkeypatch.setenv("GSSS_PIECE_PLAN", label)
        s = gs.ShrinkageSphericalSliceSampler(pdf, x0, seed=9, mode="fast", placement="packed")
        kept = s.advance(1000, thin=100)
        s.advance(1000)
        report[label] = _last_launch(s)
        out[label] = (s.state_device.clone(), kept.clone(), s._n_tries.clone(), s._n_reject.clone(), s._err.clone())
    assert report["0"] == (1280 + 674 * 9, 128, 674 / 1954)    # the second launch starts at step 1000: a first slice of 24 steps, then 8
    grid, steps, frac = report["1"]
    assert steps == 500 and 1954 < grid < 1954 + 1280 and grid - 1954 == round(frac * 1954)
    for i in range(5):
        assert torch.equal(out["0"][i], out["1"][i]), i
    assert int((out["0"][4] != 0).sum()) == 0

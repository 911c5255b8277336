"""The trade of a lane's two chains (trade() in screened_kernel and fast_kernel; lds_trade, gsss_fast.h / gsss_screen.h): the
parked words that hold two 32-bit fields -- q[i] q[i+1]; q[2] steps_done of the compact layout; steps_done row; n_try flags --
trade their halves one by one in the builds whose policy says so (lean_words, gsss_fast.h: the vMF mixtures on S^2 up to 10
terms) and as one 64-bit value in the others.  A chain is keyed by (chain id, step), so a launch that parks a second chain per lane
(GSSS_ONE_PER_LANE=0) must leave every bit that the launch with one chain per lane and nothing parked (GSSS_ONE_PER_LANE=2)
leaves: a field that came back from its slot in the wrong half, or from the wrong slot, changes the chain.

2 * 256 + 37 chains: a workgroup whose lanes all hold two chains, and one whose second slots are empty past lane 36."""
import numpy as np
import pytest

from conftest import golden
from helpers import product_target

pytestmark = pytest.mark.gpu

N_CHAINS, N_STEPS, THIN = 2 * 256 + 37, 64, 4


@pytest.fixture(scope="module")
def gs():
    import torch
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    import geosss_amd
    geosss_amd._lib.require_device()
    return geosss_amd


def _unit_rows(seed, k, d):
    m = np.random.default_rng(seed).standard_normal((k, d))
    return m / np.linalg.norm(m, axis=1, keepdims=True)


def _target(gs, name):
    """the target and the policy its screened kernel is built on"""
    if name == "readme":                       # plain layout: q0 q1 | q2 q3 | steps_done row | n_try flags
        return product_target(golden("traj_vmfmix_readme.npz")), "ScreenVmf<3"
    if name == "vmf_d4_k6":                    # kParkSkip > 0: the leading floats of q are formed again at take-up
        return gs.MixtureModel([gs.VonMisesFisher(m) for m in 40.0 * _unit_rows(46, 6, 4)], np.linspace(0.5, 2.0, 6)), "ScreenVmf<4"
    if name == "bingham_diag_d4":              # compact layout: q0 q1 | q2 steps_done (a float / int word) | n_try flags
        return gs.random_bingham(d=4, vmax=25.0, vmin=-2.0, eigensystem=True, seed=4), "ScreenBinghamDiag<4"
    if name == "curve_d3":
        return product_target(golden("traj_curve_d3_kappa300.npz")), "ScreenCurve"
    raise ValueError(name)


def _run(gs, pdf, x0, packing, monkeypatch, policy=None, **kw):
    monkeypatch.setenv("GSSS_ONE_PER_LANE", packing)
    s = gs.ShrinkageSphericalSliceSampler(pdf, x0, seed=31, mode="fast", placement="packed", chain_offset=12, step_offset=5, **kw)
    variant = 0 if kw.get("screen", True) else 100
    name = s._lib.gsss_kernel_name(s._target_dev.handle, 1, variant, 1).decode()
    print(f"GSSS_ONE_PER_LANE={packing} {kw}: {name}")
    if policy is not None:
        assert name.startswith("screened_kernel") and policy in name, name
    else:
        assert name.startswith("fast_kernel"), name
    rows = s.advance(N_STEPS, thin=THIN).clone()
    return s.state_device.clone(), s._n_tries.clone(), s._n_reject.clone(), s._err.clone(), rows


def _equal(two, one):
    import torch
    for i, (a, b) in enumerate(zip(two[:4], one[:4])):
        assert torch.equal(a, b), ("state", "n_tries", "n_reject", "err")[i]
    ok = one[3] == 0  # (a stopped chain writes no further rows: those slots of the buffer are unspecified)
    assert two[4].shape == (N_STEPS // THIN, two[0].shape[0], N_CHAINS)
    assert torch.equal(two[4][:, :, ok], one[4][:, :, ok])
    return int((~ok).sum())


@pytest.mark.parametrize("name", ["readme", "vmf_d4_k6", "bingham_diag_d4", "curve_d3"])
def test_two_chains_per_lane_equal_one(gs, name, monkeypatch):
    """State, n_tries, n_reject, err and the kept rows of the launch that trades, bit for bit those of the launch that does not."""
    pdf, policy = _target(gs, name)
    x0 = gs.sample_sphere_device(pdf.d - 1, N_CHAINS, seed=43).T
    two = _run(gs, pdf, x0, "0", monkeypatch, policy)
    one = _run(gs, pdf, x0, "2", monkeypatch, policy)
    assert _equal(two, one) == 0
    assert int(two[1].min()) >= N_STEPS  # every chain made its steps


def test_all_double_kernel_trades_the_same_chains(gs, monkeypatch):
    """fast_kernel (screen=False) always parks a second chain, and the screened kernel is held to it bit for bit: its launch
    against the screened one with one chain per lane."""
    pdf, policy = _target(gs, "readme")
    x0 = gs.sample_sphere_device(2, N_CHAINS, seed=43).T
    two = _run(gs, pdf, x0, "0", monkeypatch, screen=False)
    one = _run(gs, pdf, x0, "2", monkeypatch, policy)
    assert _equal(two, one) == 0


def test_chains_that_stop_while_parked(gs, monkeypatch):
    """max_tries = 3: chains stop with GSSS_CHAIN_MAX_TRIES, many of them while the lane's other chain runs -- the flags
    travel in the packed word's high bits.  err and the frozen states are those of the launch with nothing parked."""
    pdf, policy = _target(gs, "readme")
    x0 = gs.sample_sphere_device(2, N_CHAINS, seed=43).T
    two = _run(gs, pdf, x0, "0", monkeypatch, policy, max_tries=3)
    one = _run(gs, pdf, x0, "2", monkeypatch, policy, max_tries=3)
    stopped = _equal(two, one)
    # (five tries a step on average: within 64 steps nearly every chain has met a step that needs more than three)
    assert stopped > N_CHAINS // 2 and int((one[3][one[3] != 0] & 1).min()) == 1
    assert int(one[1].min()) < int(one[1].max())  # ... at different steps: chains stop beside chains that run on

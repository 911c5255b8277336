"""The Philox counter words of the lane kernels (PhiloxDraws::init_step, gsss_device.h; counter_words, gsss_counter_words.h):
a launch that stays inside one block of 2^32 chain ids and one of 2^32 step ids forms words 1 and 2 as 32-bit sums and takes
word 3 from the launch (RunBlock::ctr32); any other launch adds in 64 bits as before.  Both give the counter of
(chain id, step id): a launch across a boundary (64-bit path) equals the launches on either side of it (32-bit path), and the
32-bit path with non-zero high words equals the CPU oracle.  README mixture, 512 chains, both packings of the lanes."""
import numpy as np
import pytest

from conftest import golden
from helpers import product_target

pytestmark = pytest.mark.gpu

N = 512
TOL = 1e-10
PACKINGS = {"two_per_lane": "0", "one_per_lane": "2"}


@pytest.fixture(scope="module")
def gs():
    import torch
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    import geosss_amd
    geosss_amd._lib.require_device()
    return geosss_amd


@pytest.fixture(scope="module")
def pdf(gs):
    return product_target(golden("traj_vmfmix_readme.npz"))


def _sampler(gs, pdf, x0, **kw):
    s = gs.ShrinkageSphericalSliceSampler(pdf, x0, seed=2024, mode="fast", placement="packed", **kw)
    assert s._lib.gsss_kernel_name(s._target_dev.handle, 1, 0, 1).decode().startswith("screened_kernel")
    return s


def _out(s, rows):
    return s.state_device.clone(), s._n_tries.clone(), s._n_reject.clone(), s._err.clone(), rows.clone()


@pytest.mark.parametrize("packing", list(PACKINGS))
def test_launch_across_a_chain_block_equals_the_launches_beside_it(gs, pdf, packing, monkeypatch):
    """chain_offset = 2^32 - 200: one sampler of 512 chains (ids on both sides of 2^32: the 64-bit path) against a sampler of
    the 200 chains below the boundary and one of the 312 from it on (the 32-bit path, the second with word 3 = 1)."""
    import torch
    monkeypatch.setenv("GSSS_ONE_PER_LANE", PACKINGS[packing])
    x0 = gs.sample_sphere_device(2, N, seed=43).T
    off = 2**32 - 200
    whole = _sampler(gs, pdf, x0, chain_offset=off, step_offset=3)
    whole = _out(whole, whole.advance(24, thin=2))
    parts = []
    for lo, hi in ((0, 200), (200, N)):
        s = _sampler(gs, pdf, x0[lo:hi], chain_offset=off + lo, step_offset=3)
        parts.append(_out(s, s.advance(24, thin=2)))
    for i in range(5):
        assert torch.equal(whole[i], torch.cat([parts[0][i], parts[1][i]], dim=-1)), i
    assert int((whole[3] != 0).sum()) == 0


@pytest.mark.parametrize("packing", list(PACKINGS))
def test_launch_across_a_step_block_equals_two_launches(gs, pdf, packing, monkeypatch):
    """step_offset = 2^32 - 8: one launch of 16 steps (step ids on both sides of 2^32) against two launches of 8 (the second
    starts at 2^32: the 32-bit path with word 3 = 1 << 16)."""
    import torch
    monkeypatch.setenv("GSSS_ONE_PER_LANE", PACKINGS[packing])
    x0 = gs.sample_sphere_device(2, N, seed=43).T
    one = _sampler(gs, pdf, x0, chain_offset=77, step_offset=2**32 - 8)
    one = _out(one, one.advance(16, thin=1))
    two = _sampler(gs, pdf, x0, chain_offset=77, step_offset=2**32 - 8)
    rows = torch.cat([two.advance(8, thin=1).clone(), two.advance(8, thin=1).clone()], dim=0)
    two = _out(two, rows)
    for i in range(5):
        assert torch.equal(one[i], two[i]), i
    assert int((one[3] != 0).sum()) == 0


@pytest.fixture(scope="module")
def oracle_chains(oracle):
    """the oracle's chains far from the first block of either kind, computed once for both packings"""
    z = golden("traj_vmfmix_readme.npz")
    chain_offset, step_offset, n_steps = 5 * 2**32 + 7, 3 * 2**32, 12
    x0 = oracle.sample_sphere(11, N, len(z["x0"]), chain_offset=chain_offset)
    want = oracle.run(oracle.Target.from_fixture(z), x0, n_steps, seed=2024, chain_offset=chain_offset, step_offset=step_offset,
                      sampler=oracle.SHRINK, n_threads=8)
    return x0, chain_offset, step_offset, n_steps, want


@pytest.mark.parametrize("packing", list(PACKINGS))
def test_high_words_equal_the_oracle(gs, pdf, oracle_chains, packing, monkeypatch):
    """chain_offset = 5 * 2^32 + 7 and step_offset = 3 * 2^32: the 32-bit path with word 3 = 5 | 3 << 16, held to the CPU oracle
    as tests/test_hip_parity.py::test_philox_stream_matches_oracle holds the first block: states within 1e-10 after every step,
    tries and rejections exactly."""
    monkeypatch.setenv("GSSS_ONE_PER_LANE", PACKINGS[packing])
    x0, chain_offset, step_offset, n_steps, want = oracle_chains
    s = _sampler(gs, pdf, x0, chain_offset=chain_offset, step_offset=step_offset)
    kept = s.advance(n_steps, thin=1).permute(2, 0, 1).cpu().numpy()  # (chains, steps, d)
    assert np.all(s.errors == 0) and np.all(want["err"] == 0)
    assert np.array_equal(s.n_tries_per_chain, want["n_tries"])
    assert np.array_equal(s.n_reject_per_chain, want["n_reject"])
    assert np.max(np.abs(kept - want["samples"])) < TOL

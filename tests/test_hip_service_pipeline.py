"""The headline lane kernel (screened_kernel<3, ScreenVmf<3, 3>>) computes the same chains however its work is scheduled: one
launch or launches split at odd step counts, one or two chains per lane, sliced or not, with running statistics on -- and they
are the chains of the all-double kernel (fast_kernel).  States bit for bit, tries and rejections exactly."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

README_MUS = 80.0 * np.array([[0.87, -0.37, 0.33], [-0.20, -0.89, -0.40], [0.19, 0.22, -0.96]])
N_CHAINS, N_STEPS, SEED = 100_000, 300, 2024


@pytest.fixture(scope="module")
def gs():
    import torch
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    import geosss_amd
    geosss_amd._lib.require_device()
    return geosss_amd


def _run(gs, splits=(), screen=True, stats=False):
    pdf = gs.MixtureModel([gs.VonMisesFisher(m) for m in README_MUS])
    x0 = gs.sample_sphere_device(2, N_CHAINS, seed=11).T
    s = gs.ShrinkageSphericalSliceSampler(pdf, x0, seed=SEED, mode="fast", placement="packed", screen=screen)
    name = s._lib.gsss_kernel_name(s._target_dev.handle, 1, 0 if screen else 100, 1).decode()
    assert name.startswith("screened_kernel" if screen else "fast_kernel"), name
    if stats:
        s.enable_stats(lags=8)
    done = 0
    for n in list(splits) + [N_STEPS - sum(splits)]:
        if stats:
            s.advance(n, thin=1, keep=False)
        else:
            s.advance(n)
        done += n
    assert done == N_STEPS
    assert int((s._err != 0).sum().item()) == 0
    return s.state_device.clone(), s._n_tries.clone(), s._n_reject.clone()


@pytest.fixture(scope="module")
def reference(gs):
    return _run(gs, screen=False)


def _same(a, b):
    import torch
    return all(torch.equal(x, y) for x, y in zip(a, b))


@pytest.fixture
def clean_env(monkeypatch):
    for var in ("GSSS_ONE_PER_LANE", "GSSS_SLICE_STEPS", "GSSS_STATS_ONCHIP"):
        monkeypatch.delenv(var, raising=False)
    return monkeypatch


@pytest.mark.parametrize("one_per_lane", [None, "0", "2"])
@pytest.mark.parametrize("slice_steps", [None, "0", "128"])
def test_schedules_give_the_all_double_chains(gs, reference, clean_env, one_per_lane, slice_steps):
    for var, val in (("GSSS_ONE_PER_LANE", one_per_lane), ("GSSS_SLICE_STEPS", slice_steps)):
        if val is not None:
            clean_env.setenv(var, val)
    assert _same(_run(gs), reference)


@pytest.mark.parametrize("splits", [(1,), (7, 131), (1, 7, 131, 1)])
def test_split_launches_give_the_all_double_chains(gs, reference, clean_env, splits):
    assert _same(_run(gs, splits), reference)


@pytest.mark.parametrize("splits", [(), (7, 131)])
def test_statistics_launches_give_the_all_double_chains(gs, reference, clean_env, splits):
    assert _same(_run(gs, splits, stats=True), reference)

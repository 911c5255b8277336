"""The screen's set-up of the lane kernels (gsss_screen.h; S^2, K <= 3: from rows staged in log2 units) changes no chain: the
screened kernels give the chains of the all-double ones -- states bit for bit, tries and rejections exactly -- for both samplers,
one and two chains per lane, padded and zero-weight components, the wider buckets and dimensions, and a chain that starts at a
NaN.  The Philox counter words (chain and step ids as 64-bit sums, their hi16 fields in word 3) are held to themselves across a
multiple of 2^32 in the chain ids and in the step ids: a launch that straddles one gives the chains of launches that do not."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

README_MUS = 80.0 * np.array([[0.87, -0.37, 0.33], [-0.20, -0.89, -0.40], [0.19, 0.22, -0.96]])
N_CHAINS, N_STEPS, SEED = 2048, 200, 2025
CHAIN_OFFSET, STEP_OFFSET = 123_456, 7_000


@pytest.fixture(scope="module")
def gs():
    import torch
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    import geosss_amd
    geosss_amd._lib.require_device()
    return geosss_amd


def _mixture(gs, d, k, kappa, zero_weight=False):
    mus = kappa * gs.sample_sphere(d - 1, k, seed=100 * d + k)
    w = np.ones(k)
    if zero_weight:
        w[1] = 0.0
    return gs.MixtureModel([gs.VonMisesFisher(m) for m in mus], w)


TARGETS = {
    "k1": lambda gs: _mixture(gs, 3, 1, 80.0),
    "k2": lambda gs: _mixture(gs, 3, 2, 80.0),
    "k3_readme": lambda gs: gs.MixtureModel([gs.VonMisesFisher(m) for m in README_MUS]),
    "k5": lambda gs: _mixture(gs, 3, 5, 60.0),
    "k10_kappa500": lambda gs: _mixture(gs, 3, 10, 500.0),
    "d4_k3": lambda gs: _mixture(gs, 4, 3, 80.0),
    "d10_k3": lambda gs: _mixture(gs, 10, 3, 80.0),
    "k3_zero_weight": lambda gs: _mixture(gs, 3, 3, 80.0, zero_weight=True),
}


def _x0(gs, d, n=N_CHAINS):
    return gs.sample_sphere_device(d - 1, n, seed=11).T.contiguous()


def _run(gs, pdf, x0, *, shrink=True, screen=True, chain_offset=CHAIN_OFFSET, step_offset=STEP_OFFSET, splits=(), steps=N_STEPS,
         expect_kernel=None, errors_ok=False):
    cls = gs.ShrinkageSphericalSliceSampler if shrink else gs.RejectionSphericalSliceSampler
    s = cls(pdf, x0, seed=SEED, mode="fast", placement="packed", screen=screen, chain_offset=chain_offset, step_offset=step_offset)
    if expect_kernel is not None:
        name = s._lib.gsss_kernel_name(s._target_dev.handle, 1, 0 if screen is True else 100, 1).decode()
        assert name.startswith(expect_kernel), name
    for n in list(splits) + [steps - sum(splits)]:
        s.advance(n)
    if not errors_ok:
        assert int((s._err != 0).sum().item()) == 0
    return s.state_device.clone(), s._n_tries.clone(), s._n_reject.clone(), s._err.clone()


def _same(a, b):
    import torch
    return all(torch.equal(x, y) for x, y in zip(a, b))


def _cat(a, b):
    import torch
    return tuple(torch.cat([x, y], dim=-1) for x, y in zip(a, b))


_references = {}


def _reference(gs, name, shrink):
    """the all-double chains of a target and sampler, computed once"""
    key = (name, shrink)
    if key not in _references:
        pdf = TARGETS[name](gs)
        _references[key] = _run(gs, pdf, _x0(gs, pdf.d), shrink=shrink, screen=False, expect_kernel="fast_kernel")
    return _references[key]


@pytest.mark.parametrize("one_per_lane", ["0", "2"])
@pytest.mark.parametrize("shrink", [True, False], ids=["shrinkage", "rejection"])
@pytest.mark.parametrize("name", sorted(TARGETS))
def test_screened_equals_all_double(gs, monkeypatch, name, shrink, one_per_lane):
    monkeypatch.setenv("GSSS_ONE_PER_LANE", one_per_lane)
    pdf = TARGETS[name](gs)
    got = _run(gs, pdf, _x0(gs, pdf.d), shrink=shrink, expect_kernel="screened_kernel")
    assert _same(got, _reference(gs, name, shrink))


@pytest.mark.parametrize("shrink", [True, False], ids=["shrinkage", "rejection"])
def test_d12_screened_equals_its_verification_run(gs, monkeypatch, shrink):
    """d = 12 has no all-double lane sibling: every try of the GSSS_VARIANT_FAST_VERIFY run is decided in double precision"""
    monkeypatch.delenv("GSSS_ONE_PER_LANE", raising=False)
    pdf = _mixture(gs, 12, 3, 80.0)
    x0 = _x0(gs, 12)
    assert _same(_run(gs, pdf, x0, shrink=shrink), _run(gs, pdf, x0, shrink=shrink, screen="verify"))


@pytest.mark.parametrize("screen", [True, False], ids=["screened", "all_double"])
def test_chains_that_straddle_a_block_of_chain_ids(gs, monkeypatch, screen):
    """2048 chains from 2^32 - 1000 on in one sampler against the same chains as two samplers of 1000 and 1048, each inside one
    block of 2^32 chain ids: the counter's chain words carry over the boundary"""
    monkeypatch.delenv("GSSS_ONE_PER_LANE", raising=False)
    pdf = TARGETS["k3_readme"](gs)
    x0 = _x0(gs, 3)
    first = 2 ** 32 - 1000
    whole = _run(gs, pdf, x0, screen=screen, chain_offset=first)
    head = _run(gs, pdf, x0[:1000], screen=screen, chain_offset=first)
    tail = _run(gs, pdf, x0[1000:], screen=screen, chain_offset=2 ** 32)
    assert _same(whole, _cat(head, tail))


@pytest.mark.parametrize("screen", [True, False], ids=["screened", "all_double"])
def test_steps_that_straddle_a_block_of_step_ids(gs, monkeypatch, screen):
    """one launch of 200 steps from step 2^32 - 100 on against launches of 100 + 100, each inside one block of 2^32 step ids:
    the counter's step words carry over the boundary"""
    monkeypatch.delenv("GSSS_ONE_PER_LANE", raising=False)
    pdf = TARGETS["k3_readme"](gs)
    x0 = _x0(gs, 3)
    first = 2 ** 32 - 100
    whole = _run(gs, pdf, x0, screen=screen, step_offset=first)
    split = _run(gs, pdf, x0, screen=screen, step_offset=first, splits=(100,))
    assert _same(whole, split)


def test_straddling_launches_screened_equal_all_double(gs, monkeypatch):
    monkeypatch.delenv("GSSS_ONE_PER_LANE", raising=False)
    pdf = TARGETS["k3_readme"](gs)
    x0 = _x0(gs, 3)
    for kw in ({"chain_offset": 2 ** 32 - 1000}, {"step_offset": 2 ** 32 - 100}):
        assert _same(_run(gs, pdf, x0, **kw), _run(gs, pdf, x0, screen=False, **kw))


@pytest.mark.parametrize("one_per_lane", ["0", "2"])
def test_nan_chain_ends_nonfinite_like_the_all_double_kernel(gs, monkeypatch, one_per_lane):
    """a chain whose x0 holds a NaN stops with GSSS_CHAIN_NONFINITE and its state as stored; the all-double kernel says what that is"""
    import torch
    from geosss_amd import _lib
    monkeypatch.setenv("GSSS_ONE_PER_LANE", one_per_lane)
    pdf = TARGETS["k3_readme"](gs)
    x0 = _x0(gs, 3).clone()
    bad = 777
    x0[bad, 1] = float("nan")
    want = _run(gs, pdf, x0, screen=False, errors_ok=True)
    got = _run(gs, pdf, x0, errors_ok=True)
    assert int(want[3][bad].item()) == _lib.CHAIN_NONFINITE
    assert int((want[3] != 0).sum().item()) == 1
    assert torch.equal(got[3], want[3])
    assert torch.equal(got[0].view(torch.int64), want[0].view(torch.int64))  # bit patterns: the NaN too
    assert torch.equal(got[1], want[1]) and torch.equal(got[2], want[2])

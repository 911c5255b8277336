"""The registration kernels (gsss_target_cpd.hip: GaussianMixtureModel / CoherentPointDrift on unit quaternions) against the
extended-precision restatement of tests/reference_math.py, in all four builds -- 8 or 24 list slots, uniform source weights or
weights carried through the insertion network -- with weighted source and target clouds, both target dimensions, both models,
k = 1 .. 24, single points, clouds that fill two thirds of the LDS budget, on and off the sphere (tests/registration_cases.py).

log_prob and gradient at 1e-10 of the value's scale (the gradient near a good pose is a cancelling sum: its scale is the sum of
the absolute values of what is accumulated).  The two slice samplers replay the draws of a reference chain run on the longdouble
log_prob; RWMH and SphericalHMC on the weighted builds are held to the CPU oracle, which test_reference_math.py holds to the same
restatement on every case."""
import time

import numpy as np
import pytest

import layout_cases as lc
import registration_cases as rc

pytestmark = pytest.mark.gpu

TOL = 1e-10          # of the value's scale
CHAIN_TOL = 2e-14    # states of a replayed chain, as test_hip_mixture_layouts.py measures its own
WORST = {}           # (variant, target dimension) -> [log_prob, gradient]: the largest share of the scale met


@pytest.fixture(scope="module")
def gs():
    import torch
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    import geosss_amd
    geosss_amd._lib.require_device()
    yield geosss_amd
    if WORST:
        print("\nbuild, target dimension: largest error of log_prob / gradient as a share of the scale")
        for (v, dt), (a, b) in sorted(WORST.items()):
            print(f"  {['Cpd8U', 'Cpd8W', 'Cpd24U', 'Cpd24W'][v]} {dt}-D  {a:.1e}  {b:.1e}")
    rc.release()  # the cached targets' device copies go with the module
    lc.release()
    torch.cuda.synchronize()


@pytest.mark.parametrize("name", rc.CASES)
def test_log_prob_and_gradient_against_reference(gs, name):
    pdf, X, n_unit = rc.case(name)
    ref = rc.reference(name)
    pdf.log_prob(X[:1])                                  # (the target's upload stays out of the time printed below)
    t0 = time.perf_counter()
    lp, gr = pdf.log_prob(X), pdf.gradient(X)
    seconds = time.perf_counter() - t0
    assert lp.shape == (len(X),) and gr.shape == (len(X), 4)
    e_lp, e_gr = rc.errors(lp, gr, ref)
    e_unit, e_off = rc.errors(lp[:n_unit], gr[:n_unit], ref, slice(0, n_unit)), rc.errors(lp[n_unit:], gr[n_unit:], ref, slice(n_unit, None))
    s = rc.spec(name)
    key = (rc.variant(s), s["dt"])
    WORST[key] = np.maximum(WORST.get(key, (0.0, 0.0)), (e_lp, e_gr))
    print(f"{name} (variant {key[0]}): log_prob {e_unit[0]:.1e} / {e_off[0]:.1e}, gradient {e_unit[1]:.1e} / {e_off[1]:.1e} of the "
          f"scale (on / off the sphere); both calls {seconds:.3f} s")
    assert e_lp < TOL and e_gr < TOL
    # a row and its negative are the same rotation: the same score, the opposite gradient (the Jacobian is odd in q)
    assert lp[2] == lp[3] and np.array_equal(gr[2], -gr[3])
    if name == "sweep_2d_k9_wboth_cpd":    # the one single-row call
        one, g1 = pdf.log_prob(X[5]), pdf.gradient(X[5])
        assert isinstance(one, float) and one == lp[5] and g1.shape == (4,) and np.array_equal(g1, gr[5])


def test_every_build_runs_in_both_dimensions():
    """The library does not report which build it picked, so the choice is restated (registration_cases.variant, from k and the
    source weights as gsss_capi.hip makes it): by construction the cases above fill every cell of (8 / 24 slots) x (uniform /
    weighted) x (3-D / projected)."""
    cells = {(rc.variant(s), s["dt"]) for s in map(rc.spec, rc.CASES)}
    assert cells == {(v, dt) for v in range(4) for dt in (2, 3)}


def sampler_cls(gs, sampler):
    return gs.ShrinkageSphericalSliceSampler if sampler == "shrink" else gs.RejectionSphericalSliceSampler


@pytest.mark.parametrize("sampler", ["shrink", "reject"])
@pytest.mark.parametrize("name", rc.CHAIN_CASES)
def test_replay_reproduces_reference_chain(gs, name, sampler):
    """32 chains x 20 steps of either slice sampler on the draws of the longdouble chain: every try on the same side of its
    threshold (none within 1e-8 of it), so tries and rejections are equal and the states differ by rounding alone."""
    pdf = rc.chain_target(name)
    ref = rc.reference_chain(name, sampler)
    assert ref["margin"] > lc.MIN_MARGIN
    s = sampler_cls(gs, sampler)(pdf, ref["x0"], seed=1)
    assert s.mode == "exact"
    got = s.advance(lc.N_STEPS, thin=1, replay=ref["replay"]).cpu().numpy().transpose(0, 2, 1)
    assert np.all(s.errors == 0)
    print(f"{name} {sampler}: max |dx| {np.max(np.abs(got - ref['states'])):.1e}, margin {ref['margin']:.1e}")
    assert np.array_equal(np.asarray(s.n_tries_per_chain), ref["tries"])
    assert np.array_equal(np.asarray(s.n_reject_per_chain), ref["rejections"])
    assert np.max(np.abs(got - ref["states"])) < CHAIN_TOL


WEIGHTED = ["chain_2d_k8_wboth_cpd", "chain_3d_k24_wboth_cpd"]   # Cpd8W projected, Cpd24W 3-D


@pytest.mark.parametrize("name", WEIGHTED)
def test_rwmh_on_a_weighted_build_matches_oracle(gs, oracle, name):
    """Free-running random-walk Metropolis on the Philox stream, as test_hip_registration.py runs it on uniform weights."""
    pdf = rc.chain_target(name)
    tgt = rc.oracle_target(oracle, pdf)
    n, steps = 300, 25
    x0 = oracle.sample_sphere(9, n, 4)
    want = oracle.mh_run(tgt, x0, steps, sampler=oracle.RWMH, stepsize=0.1, adapt_steps=steps // 2, seed=4, n_threads=8)

    def run(x, cuts=(steps,), **kw):
        s = gs.MetropolisHastings(pdf, x, 4, stepsize=0.1, **kw)
        s.reset(steps // 2)
        done = 0
        for c in cuts:
            s.advance(c - done)
            done = c
        return s

    whole = run(x0)
    assert np.array_equal(whole.n_accept_per_chain, want["n_accept"])
    assert 0 < want["n_accept"].sum() < n * steps
    assert np.max(np.abs(whole.state - want["state"])) < 1e-10
    split, shard = run(x0, cuts=(11, steps)), run(x0[137:], chain_offset=137)
    assert np.array_equal(split.state, whole.state) and np.array_equal(split.n_accept_per_chain, whole.n_accept_per_chain)
    assert np.array_equal(shard.state, whole.state[137:]) and np.array_equal(shard.n_accept_per_chain, whole.n_accept_per_chain[137:])


@pytest.mark.parametrize("name", WEIGHTED)
def test_hmc_on_a_weighted_build_matches_oracle(gs, oracle, name):
    """SphericalHMC as single transitions from 200 poses (free chains part once rounding flips a nearest neighbour:
    tests/test_oracle_mh.py::horizon): the leapfrog evaluates the weighted gradient off the sphere."""
    pdf = rc.chain_target(name)
    tgt = rc.oracle_target(oracle, pdf)
    x0 = oracle.sample_sphere(2, 200, 4)
    want = oracle.mh_run(tgt, x0, 1, sampler=oracle.HMC, stepsize=0.05, n_leapfrog=10, seed=8, n_threads=8)
    h = gs.SphericalHMC(pdf, x0, 8, stepsize=0.05, n_steps=10)
    h.advance(1)
    assert np.array_equal(h.n_accept_per_chain, want["n_accept"])
    assert 0 < want["n_accept"].sum()
    assert np.max(np.abs(h.state[:, :4] - want["state"])) < 1e-10
    assert np.max(np.abs(h.momenta - want["momenta"])) < 1e-9
    # three transitions in one launch, as two launches, and the upper chains as a shard of their own: the same bits
    whole, split, shard = (gs.SphericalHMC(pdf, x, 8, stepsize=0.05, n_steps=10, **kw) for x, kw in
                           ((x0, {}), (x0, {}), (x0[71:], dict(chain_offset=71))))
    whole.advance(3)
    split.advance(1)
    split.advance(2)
    shard.advance(3)
    assert np.array_equal(split.state, whole.state) and np.array_equal(split.n_accept_per_chain, whole.n_accept_per_chain)
    assert np.array_equal(shard.state, whole.state[71:]) and np.array_equal(shard.n_accept_per_chain, whole.n_accept_per_chain[71:])

"""The baselines -- MetropolisHastings, IndependenceSampler, MixtureRWMHIndependenceSampler and SphericalHMC, all through
mh_kernel<V, TT, DR, SAMPLER> (geosss_amd/csrc/gsss_mh.h) -- in every exact layout:

(a) replaying the draws of a restatement of the four transitions in longdouble (layout_cases.mh_chain) at every d of
    layout_cases.DIMS for a vMF mixture, a Fisher-Bingham (the diagonal Bingham above d = 512), a ten-knot curve and the generic
    mixture, and on the targets whose rows are read from global memory; at d = 5, 12 and 40 also in every further cooperative
    layout that covers d, most of its slots empty;
(b) on the library's Philox stream against the CPU oracle, where the radius of the random-walk proposal is the norm of a second
    set of d normals taken at block offset (d + 3) >> 2 and reduced over the lane group;
(c) on numpy's own stream against the oracle's restatement of it, gamma shapes 1.5 .. 8.5.

Accept flags, counters and the NaN pattern of the stepsize trace are exact, stepsizes agree to 1e-12; states and momenta are held
to layout_cases.mh_bars: 16 times what the CPU oracle differs from the longdouble chain by (measured on the CPU by
test_reference_math.py::test_oracle_mh_against_reference_chain), rounded up to a power of ten, never above the suite's 1e-10 /
1e-9 / 1e-7.  Every case keeps its proposals further than 1e-8 from their thresholds and every chain both accepts and rejects
(test_reference_math.py::test_mh_chain_margins), so no decision hangs on rounding; no chain and no step is left out."""
import re

import numpy as np
import pytest

import layout_cases as lc
from helpers import variants_for

pytestmark = pytest.mark.gpu

LAYOUTS = ["lane2", "lane3", "lane4", "lane5", "lane6", "lane8", "lane10", "coop4x4", "coop4x8", "coop16x4", "coop16x8", "coop64x4",
           "coop64x8", "coop64x16", "coop64x32"]  # GSSS_VEC_LIST ids 1 .. 15
# the sweep's generic mixture holds more rows than coop16x8 has LDS for and runs d = 65 .. 128 in coop64x4 (layout_cases.LAYOUT_CASES)
GMIX_MOVED = {65: "coop64x4", 128: "coop64x4"}
ORACLE_CASES = [(f, d) for f, d in lc.MH_CASES if not f.startswith("gmix")]
CHI_DIMS = [2, 7, 9, 11, 17, 33, 65, 129, 257, 513, 1025]  # (d + 3) >> 2 blocks of normals and the layout's component map do not line up
NUMPY_DIMS = [3, 4, 6, 7, 8, 9, 11, 16, 17]


@pytest.fixture(scope="module")
def gs():
    import torch
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    import geosss_amd
    geosss_amd._lib.require_device()
    yield geosss_amd
    lc.release()  # the cached targets' device copies go with the module
    torch.cuda.synchronize()


def build(gs, kind, pdf, x0, seed, stepsize, **kw):
    if kind == "rwmh":
        return gs.MetropolisHastings(pdf, x0, seed, stepsize=stepsize, record_stepsize=True, **kw)
    if kind == "indep":
        return gs.IndependenceSampler(pdf, x0, seed, stepsize=stepsize, record_stepsize=True, **kw)
    if kind == "mix":
        return gs.MixtureRWMHIndependenceSampler(pdf, x0, seed, stepsize=stepsize, mixing_probability=lc.MH_ALPHA,
                                                 record_stepsize=True, **kw)
    return gs.SphericalHMC(pdf, x0, seed, stepsize=stepsize, n_steps=lc.MH_LEAPFROG, **kw)


def layout_of(s, variant=0):
    return re.match(r"run_kernel<(\w+), ", s._lib.gsss_kernel_name(s._target_dev.handle, 0, variant, 0).decode()).group(1)


def default_layout(gs, family, d, pdf):
    if d == 0:
        return lc.global_case(family)[2]
    if family == "gmix" and d in GMIX_MOVED:
        return GMIX_MOVED[d]
    return LAYOUTS[gs._lib.load().gsss_exact_layout(pdf.d) - 1]


def test_sweep_reaches_every_layout(gs):
    """Every layout the library selects for some d is reached by the cases below, at its first and its last dimension: a layout
    added to GSSS_VEC_LIST fails here until the sweep covers it."""
    lib = gs._lib.load()
    by_layout = {}
    d = 2
    while lib.gsss_exact_layout(d) > 0:
        by_layout.setdefault(lib.gsss_exact_layout(d), []).append(d)
        d += 1
    assert d - 1 == 2048 and sorted(by_layout) == list(range(1, len(LAYOUTS) + 1))
    swept = {d for _, d in lc.MH_CASES if d}
    for vec, dims in by_layout.items():
        assert dims[0] in swept and dims[-1] in swept, (LAYOUTS[vec - 1], dims[0], dims[-1])
    assert set(CHI_DIMS) <= swept and {lc.layout_family(d) for d in swept} == {"lane", "coop4", "coop16", "coop64"}


def check_replay(gs, family, d, kind, variant=0, layout=None):
    pdf, x0, _ = lc.mh_case(family, d)
    ref = lc.mh_reference(family, d, kind)
    assert ref["margin"] > lc.MIN_MARGIN and ref["ties"] == 0
    n, dd = x0.shape
    steps = ref["steps"]
    s = build(gs, kind, pdf, x0, 1, ref["stepsize0"], variant=variant)
    got_layout = layout_of(s, variant)
    assert got_layout == (layout or default_layout(gs, family, d, pdf)), got_layout
    s.reset(ref["adapt"])
    got = s.advance(steps, thin=1, replay=ref["replay"]).cpu().numpy().transpose(0, 2, 1)   # (steps, chains, d)
    assert np.all(s.errors == 0)
    bar_x, bar_v = lc.mh_bars(kind, dd)
    e_x = float(np.max(np.abs(got - ref["states"])))
    e_eps = float(np.max(np.abs(s.stepsize / ref["stepsize"] - 1)))
    label = f"{family} d={dd} {kind} {got_layout}"
    print(f"{label}: states {e_x:.1e} of {bar_x:.0e}, stepsizes {e_eps:.1e}, margin {ref['margin']:.1e}, accepted {ref['share']:.2f}")
    moved = np.any(got != np.concatenate([x0[None], got[:-1]]), axis=2)           # the state moved = the proposal was accepted
    assert np.array_equal(moved, ref["accept"])
    assert np.array_equal(s.n_accept_per_chain, ref["n_accept"])
    assert e_eps < lc.MH_STEPSIZE_TOL
    if kind == "hmc":
        e_v = lc.rel(s.momenta, ref["momenta"])
        print(f"{label}: momenta {e_v:.1e} of {bar_v:.0e}")
        assert e_v < bar_v
    else:
        trace = s.stepsize_trace().cpu().numpy()
        assert trace.shape == ref["trace"].shape and np.array_equal(np.isnan(trace), np.isnan(ref["trace"]))
        used = ~np.isnan(trace)
        assert used.sum() == 0 or np.max(np.abs(trace[used] / ref["trace"][used] - 1)) < lc.MH_STEPSIZE_TOL
    if kind == "mix":
        assert np.array_equal(s.rwmh_counter_per_chain, ref["n_rwmh"])
        assert s.indep_counter == steps * n - int(ref["n_rwmh"].sum())
        assert np.array_equal(s._adapt_left.cpu().numpy(), ref["adapt_left"])
        vals = s.rwmh_stepsize_vals
        assert [len(v) for v in vals] == list(ref["n_rwmh"])
    assert e_x < bar_x


@pytest.mark.parametrize("kind", lc.MH_KINDS)
@pytest.mark.parametrize("family,d", lc.MH_CASES)
def test_replay_reproduces_reference_chain(gs, family, d, kind):
    check_replay(gs, family, d, kind)


def _forced():
    return [(f, d, v) for f, d in lc.MH_FORCED for v in variants_for(d, max_coop=6)[1:]]


@pytest.mark.parametrize("kind", lc.MH_KINDS)
@pytest.mark.parametrize("family,d,variant", _forced())
def test_replay_in_forced_cooperative_layouts(gs, family, d, variant, kind):
    """The same chains in every further cooperative layout that covers d: a layout with most of its slots empty."""
    from helpers import COOP_VARIANTS
    layout = {8: "coop4x4", 9: "coop4x8", 10: "coop16x4", 11: "coop16x8", 12: "coop64x4", 13: "coop64x8"}[variant]
    assert d <= COOP_VARIANTS[variant]
    check_replay(gs, family, d, kind, variant=variant, layout=layout)


def momenta_case(d):
    """vMF mixture at d, one numpy generator per chain: (pdf, x0, seeds, the draws each chain's generator yields for HMC -- d
    normals, then the accept uniform, per step)."""
    pdf, x0, _ = lc.mh_case("vmf3", d)
    x0 = x0[:67]                      # two workgroups and a ragged third where a chain takes four lanes or more
    seeds = [1000 + c for c in range(len(x0))]
    steps, burn = 6, 3
    draws = np.empty((len(x0), steps * (d + 1)))
    for c, seed in enumerate(seeds):
        rng = np.random.default_rng(seed)
        for s in range(steps):
            draws[c, s * (d + 1): s * (d + 1) + d] = rng.standard_normal(d)
            draws[c, s * (d + 1) + d] = rng.random()
    return pdf, x0, seeds, steps, burn, draws


@pytest.mark.parametrize("d", [7, 17, 65, 257])
def test_hmc_sample_returns_momenta_of_every_row(gs, d):
    """SphericalHMC.sample(..., return_momenta=True) in one layout of each family, a numpy generator per chain: the positions and
    the momenta of every retained row against the longdouble chain fed the same generators' draws."""
    pdf, x0, seeds, steps, burn, draws = momenta_case(d)
    eps = lc.mh_stepsize("vmf3", d, "hmc")
    ref = lc.mh_chain(pdf, x0, "hmc", 0, steps, burn, eps, n_leapfrog=lc.MH_LEAPFROG, draws=draws)
    assert ref["margin"] > lc.MIN_MARGIN and 0.1 <= ref["share"] <= 0.9
    s = build(gs, "hmc", pdf, x0, seeds, eps, rng="numpy")
    pos, mom = s.sample(steps + 1 - burn, burn, return_momenta=True, return_all_samples=True)
    assert pos.shape == mom.shape == (len(x0), steps + 1, d)
    assert np.array_equal(pos[:, 0], x0) and np.all(mom[:, 0] == 0.0)
    bar_x, bar_v = lc.mh_bars("hmc", d)
    e_x = float(np.max(np.abs(pos[:, 1:].transpose(1, 0, 2) - ref["states"])))
    e_v = lc.rel(mom[:, 1:].transpose(1, 0, 2), ref["momenta_steps"])
    print(f"d={d} {layout_of(s)}: states {e_x:.1e} of {bar_x:.0e}, momenta of every row {e_v:.1e} of {bar_v:.0e}, accepted {ref['share']:.2f}")
    assert np.array_equal(s.n_accept_per_chain, ref["n_accept"])
    assert np.max(np.abs(s.stepsize / ref["stepsize"] - 1)) < lc.MH_STEPSIZE_TOL
    assert e_x < bar_x and e_v < bar_v and lc.rel(s.momenta, ref["momenta"]) < bar_v


@pytest.mark.parametrize("kind", lc.MH_KINDS)
@pytest.mark.parametrize("family,d", ORACLE_CASES)
def test_philox_stream_matches_oracle(gs, oracle, family, d, kind):
    """The library stream at chain offset 50 and step offset 3, the steps split over two launches inside the adaptation window:
    device = oracle (counts exactly, stepsizes to 1e-12, states at the suite's 1e-10 / 1e-8)."""
    pdf, x0, _ = lc.mh_case(family, d)
    steps, adapt = lc.mh_steps(family, d)
    eps = lc.mh_stepsize(family, pdf.d, kind)
    sampler = {"rwmh": oracle.RWMH, "hmc": oracle.HMC, "indep": oracle.INDEP, "mix": oracle.MIX}[kind]
    want = oracle.mh_run(lc.oracle_target(oracle, pdf), x0, steps, sampler=sampler, stepsize=eps, adapt_steps=adapt,
                         n_leapfrog=lc.MH_LEAPFROG, seed=31, chain_offset=50, step_offset=3, mixing_probability=lc.MH_ALPHA,
                         n_threads=8)
    s = build(gs, kind, pdf, x0, 31, eps, chain_offset=50, step_offset=3)
    s.reset(adapt)
    s.advance(3)
    s.advance(steps - 3)
    e_x = float(np.max(np.abs(s.state[:, :pdf.d] - want["state"])))
    print(f"{family} d={pdf.d} {kind} {layout_of(s)}: states {e_x:.1e}, accepted {want['n_accept'].sum() / (steps * len(x0)):.2f}")
    assert np.array_equal(s.n_accept_per_chain, want["n_accept"])
    if kind == "mix":
        assert np.array_equal(s.rwmh_counter_per_chain, want["n_rwmh"]) and 0 < s.rwmh_counter < len(x0) * steps
        assert np.array_equal(s._adapt_left.cpu().numpy(), want["adapt_left"])
    assert np.max(np.abs(s.stepsize / want["stepsize"] - 1)) < lc.MH_STEPSIZE_TOL
    assert e_x < (1e-8 if kind == "hmc" else 1e-10)
    if kind == "hmc":
        assert lc.rel(s.momenta, want["momenta"]) < 1e-7


@pytest.mark.parametrize("kind", ["rwmh", "mix"])
@pytest.mark.parametrize("d", NUMPY_DIMS)
def test_numpy_stream_matches_oracle(gs, oracle, d, kind):
    """rng='numpy', a generator per chain: Generator.standard_gamma(d / 2) at shapes 1.5 .. 8.5, integers and half-integers,
    then the normals and the uniforms, against the oracle's restatement of the stream."""
    pdf, x0, _ = lc.mh_case("vmf3", d)
    x0 = x0[:131]
    seeds = [7000 + c for c in range(len(x0))]
    eps = lc.mh_stepsize("vmf3", d, kind)
    sampler = oracle.RWMH if kind == "rwmh" else oracle.MIX
    want = oracle.mh_run(lc.oracle_target(oracle, pdf), x0, lc.MH_STEPS, sampler=sampler, stepsize=eps, adapt_steps=lc.MH_ADAPT,
                         numpy_seed=seeds, mixing_probability=lc.MH_ALPHA, n_threads=8)
    s = build(gs, kind, pdf, x0, seeds, eps, rng="numpy")
    s.reset(lc.MH_ADAPT)
    s.advance(3)
    s.advance(lc.MH_STEPS - 3)
    e_x = float(np.max(np.abs(s.state - want["state"])))
    print(f"vmf3 d={d} {kind} {layout_of(s)}: states {e_x:.1e}, accepted {want['n_accept'].sum() / (lc.MH_STEPS * len(x0)):.2f}")
    assert np.array_equal(s.n_accept_per_chain, want["n_accept"]) and 0 < want["n_accept"].sum() < lc.MH_STEPS * len(x0)
    if kind == "mix":
        assert np.array_equal(s.rwmh_counter_per_chain, want["n_rwmh"])
    assert np.max(np.abs(s.stepsize / want["stepsize"] - 1)) < lc.MH_STEPSIZE_TOL
    assert e_x < 1e-10


@pytest.mark.parametrize("kind", ["rwmh", "mix"])
def test_numpy_stream_refuses_d2(gs, kind):
    """gamma(1) is numpy's exponential ziggurat, which is not restated."""
    pdf, x0, _ = lc.mh_case("vmf3", 2)
    s = build(gs, kind, pdf, x0[:5], [1, 2, 3, 4, 5], 0.1, rng="numpy")
    with pytest.raises(Exception, match="needs d >= 3"):
        s.advance(1)

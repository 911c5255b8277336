"""Replica exchange without a GPU: TargetBatch.tempered, the refusals that need no device, the resource budget of the exchange
kernels against batch_logprob_kernel's, and the reference itself (exchange_cases.run_ladder: the CPU oracle's chains plus
reference_sweep) on the d = 10 ladder -- what the device tests are then held to.  Step counts and figures: exchange_cases."""
import re

import numpy as np
import pytest

import exchange_cases as ec
import geosss_amd as gs
from geosss_amd import _lib, mcmc

E_INVALID = -1
BOGUS = 4096  # some non-NULL address that is never read


# ------------------------------------------------------------------------------------------ tempered
def _sym(d, seed):
    a = np.random.default_rng(seed).standard_normal((d, d))
    return a + a.T


def test_tempered_members_of_all_four_classes():
    betas = [1.0, 0.5, 0.125]
    A, b = _sym(4, 1), np.array([1.0, -2.0, 0.5, 3.0])
    bing = gs.TargetBatch.tempered(gs.Bingham(A), betas)
    assert len(bing) == 3 and bing.ladder == 3 and np.array_equal(bing.betas, betas)
    assert all(type(p) is gs.Bingham and np.array_equal(p.A, beta * A) for p, beta in zip(bing.pdfs, betas))
    fb = gs.TargetBatch.tempered(gs.BinghamFisher(A, b), betas)
    assert all(type(p) is gs.BinghamFisher and np.array_equal(p.A, beta * A) and np.array_equal(p.b, beta * b)
               for p, beta in zip(fb.pdfs, betas))
    mu = np.array([3.0, 4.0, 12.0])
    vmf = gs.TargetBatch.tempered(gs.VonMisesFisher(mu), betas)
    assert all(type(p) is gs.VonMisesFisher and np.array_equal(p.mu, beta * mu) for p, beta in zip(vmf.pdfs, betas))
    assert [p.kappa for p in vmf.pdfs] == [13.0, 6.5, 1.625]
    mus = [np.array([10.0, 0.0, 0.0]), np.array([0.0, 20.0, 0.0]), np.array([0.0, 0.0, -5.0])]
    mix = gs.MixtureModel([gs.VonMisesFisher(v) for v in mus], [1.0, 2.0, 5.0])
    lad = gs.TargetBatch.tempered(mix, betas)
    for p, beta in zip(lad.pdfs, betas):
        assert type(p) is gs.MixtureModel and np.array_equal(p.weights, mix.weights)        # the weights stay
        assert all(np.array_equal(q.mu, beta * v) for q, v in zip(p.pdfs, mus))             # every term's kappa scales
    assert lad.pdfs[0] is not mix and "not a power" in gs.TargetBatch.tempered.__doc__.lower()


def test_tempered_is_ladder_major():
    betas = [1.0, 0.25]
    pdfs = [gs.VonMisesFisher(k * np.eye(3)[k - 1]) for k in (1, 2, 3)]
    batch = gs.TargetBatch.tempered(pdfs, betas)
    assert len(batch) == 6 and batch.ladder == 2
    want = [beta * p.mu for p in pdfs for beta in betas]
    assert all(np.array_equal(p.mu, w) for p, w in zip(batch.pdfs, want))


@pytest.mark.parametrize("pdf, name", [(gs.Uniform(3), "Uniform"), (gs.AngularCentralGaussian(np.eye(3)), "AngularCentralGaussian"),
                                       (gs.CurvedVonMisesFisher(gs.SlerpCurve(np.eye(3)), 10.0), "CurvedVonMisesFisher"),
                                       (object(), "object")])
def test_tempered_refuses_other_classes_by_name(pdf, name):
    with pytest.raises(TypeError, match=name):
        gs.TargetBatch.tempered(pdf, [1.0, 0.5])


def test_tempered_refuses_a_generic_mixture_and_bad_betas():
    mix = gs.MixtureModel([gs.VonMisesFisher(np.array([5.0, 0.0, 0.0])), gs.Bingham(np.diag([1.0, 2.0, 3.0]))])
    with pytest.raises(TypeError, match="MixtureModel"):
        gs.TargetBatch.tempered(mix, [1.0, 0.5])
    vmf = gs.VonMisesFisher(np.array([5.0, 0.0, 0.0]))
    for betas in ([1.0], [0.9, 0.5], [1.0, 1.0], [1.0, 0.5, 0.7], [1.0, -0.1], [[1.0, 0.5]]):
        with pytest.raises(ValueError, match="betas"):
            gs.TargetBatch.tempered(vmf, betas)
    with pytest.raises(TypeError):
        gs.TargetBatch.tempered([], [1.0, 0.5])


# ------------------------------------------------------------------------------------------ argument checks
class _NoDevice(mcmc.ShrinkageSphericalSliceSampler):
    """The sampler's argument checks, which come before anything touches a device, on an object that has none."""

    def __init__(self, batch_m, n_chains, chain_offset=0):
        self._batch_m, self.n_chains, self.chain_offset = batch_m, n_chains, chain_offset


def test_sampler_refusals():
    single = _NoDevice(None, 64)
    for call in (lambda: single.exchange(2), lambda: single.advance(4, exchange=dict(ladder=2, every=1)),
                 lambda: single.sample(4, exchange=dict(ladder=2, every=1)),
                 lambda: single.summarize(4, exchange=dict(ladder=2, every=1))):
        with pytest.raises(ValueError, match="holds no TargetBatch"):
            call()
    s = _NoDevice(8, 6 * 8)
    with pytest.raises(ValueError, match="whole ladders"):      # M = 6 is no multiple of 4
        s.advance(4, exchange=dict(ladder=4, every=1))
    with pytest.raises(ValueError, match="whole ladders"):
        s.exchange(1)
    with pytest.raises(ValueError, match="every"):
        s.advance(4, exchange=dict(ladder=3, every=0))
    with pytest.raises(ValueError, match="multiple of thin"):
        s.advance(12, thin=4, exchange=dict(ladder=3, every=6))
    with pytest.raises(ValueError, match="dict"):
        s.advance(4, exchange=dict(ladder=3, each=2))
    with pytest.raises(ValueError, match="whole ladders"):      # a shard that starts inside a ladder
        _NoDevice(8, 6 * 8, chain_offset=8).advance(4, exchange=dict(ladder=3, every=1))


def test_symbols_are_exported_and_bound():
    lib = _lib.load()
    for name in ("gsss_batch_exchange", "gsss_exchange_scratch_doubles"):
        assert name in _lib.SIGNATURES and getattr(lib, name).argtypes == _lib.SIGNATURES[name][1]
    assert lib.gsss_abi_version() == 10 == _lib.ABI_VERSION
    assert lib.gsss_exchange_scratch_doubles(0) == 0 and lib.gsss_exchange_scratch_doubles(1000) == 2000
    assert lib.gsss_exchange_scratch_doubles(-1) == E_INVALID


# (handle, n_chains, target0, ladder, parity) -> the word its message carries
@pytest.mark.parametrize("args, word", [
    ((1, 24, 0, 1, 0), "ladder"),           # ladder < 2
    ((1, 24, 0, 0, 0), "ladder"),
    ((1, 24, 0, 3, 2), "parity"),           # parity outside {0, 1}
    ((1, 24, 0, 3, -1), "parity"),
    ((1, 24, 4, 3, 0), "target0"),          # target0 no multiple of the ladder
    ((1, 24, -3, 3, 0), "target0"),
    ((1, -24, 0, 3, 0), "n_chains"),
    ((0, 24, 0, 3, 0), "null handle"),
])
def test_batch_exchange_refusals_need_no_device(args, word):
    lib = _lib.load()
    h, n, t0, ladder, parity = args
    rc = lib.gsss_batch_exchange(BOGUS if h else None, BOGUS, BOGUS, n, t0, ladder, parity, 1, 0, 0, BOGUS, None, None, None, None)
    assert rc == E_INVALID and word in lib.gsss_last_error().decode()


# ------------------------------------------------------------------------------------------ resource budget
def _layout_family(name, pattern):
    """The template arguments <V, TT> of a mangled kernel name."""
    m = re.search(pattern, name)
    return m.group(1) if m else None


# The three builds that miss batch_logprob_kernel's eight wavefronts per SIMD, held to their own figure: the vMF
# mixture at three, eight and ten components a lane comes out at 66 to 68 vector registers, two to four past the 64 that eight
# wavefronts allow, and seven wavefronts; asked for eight, the compiler spills 12 to 20 bytes a lane, which is worse.
OWN_WAVES = {"NS_7LaneVecILi3EEENS_10VmfMixtureE": 7, "NS_7LaneVecILi8EEENS_10VmfMixtureE": 7, "NS_7LaneVecILi10EEENS_10VmfMixtureE": 7}


def test_resource_budget():
    """The 30 builds of exchange_eval_kernel (15 layouts x {VmfMixture, Bingham}) against the value build of batch_logprob_kernel
    in the same layout and family: no more scratch, no fewer wavefronts per SIMD (OWN_WAVES: the three that are held to their
    own figure); the swap kernel spills nothing."""
    from geosss_amd import build
    ru = build.resource_usage("gsss_exchange.hip")
    evals = {_layout_family(k, r"20exchange_eval_kernelI(.+)EEvNS_11TargetBlockE"): r for k, r in ru.items() if "exchange_eval_kernel" in k}
    swaps = [r for k, r in ru.items() if "exchange_swap_kernel" in k]
    assert len(ru) == 31 and len(evals) == 30 and None not in evals and len(swaps) == 1, sorted(ru)
    parent = {}
    for name, r in build.resource_usage("gsss_batch_logprob.hip").items():
        key = _layout_family(name, r"20batch_logprob_kernelI(.+)Lb0EEEvNS_11TargetBlockE")   # (the value builds)
        if key is not None:
            parent[key] = r
    assert len(parent) == 30 and set(parent) == set(evals), (sorted(parent), sorted(evals))
    for key, r in sorted(evals.items()):
        p = parent[key]
        print(f"{key}: vgprs {r['vgprs']} ({p['vgprs']}), scratch {r['scratch']} ({p['scratch']}), waves {r['occupancy']} ({p['occupancy']})")
        waves = OWN_WAVES.get(key, p["occupancy"])
        assert r["scratch"] <= p["scratch"] and r["occupancy"] >= waves, (key, r, p)
    print("swap:", swaps[0])
    assert swaps[0]["scratch"] == 0 and swaps[0]["occupancy"] >= 8


# ------------------------------------------------------------------------------------------ the reference is right
def test_sweep_cases_keep_the_decision_margin():
    """No pair of any GPU case lies within MARGIN of its decision (the condition the seeds were chosen for), and every case has
    swaps, refusals by the draw, the error chain and the NaN column."""
    refused = 0
    for key in ec.SWEEP_CASES + ec.SWEEP_GLOBAL:
        pdfs, m, x, err, refs = ec.sweep_case(key)
        assert len(pdfs) == 6 and x.shape == (6 * m, pdfs[0].d)
        for parity, ref in enumerate(refs):
            may = np.isfinite(ref["margin"])
            assert ref["margin"].min() > ec.MARGIN, (key, parity, ref["margin"].min())
            assert ref["lower"].sum() == 2 * m and may.sum() == 2 * m - 2, (key, parity)        # one error pair, one NaN pair
            assert ref["swap"].sum() > 0, (key, parity)
            assert ref["attempts"].sum() == 2 * m and ref["accepts"].sum() == ref["swap"].sum()
            # members that sit out: untouched
            out = 2 if parity == 0 else 0
            for g in range(2):
                rows = slice((3 * g + out) * m, (3 * g + out + 1) * m)
                assert np.array_equal(ref["x"][rows], x[rows], equal_nan=True) and not ref["lower"][rows].any()
            assert np.array_equal(ref["x"], x[ref["replica"]], equal_nan=True)
            refused += int((np.isfinite(ref["margin"]) & ~ref["swap"]).sum())
    assert refused > 100        # (a case of m = 7 may swap all of its 12 pairs; the cases together have both decisions in number)


@pytest.fixture(scope="module")
def ladder_runs():
    pdf, batch, x0 = ec.ladder_case()
    m = ec.LADDER_M
    with_x = ec.run_ladder(batch.pdfs, x0, m, ec.LADDER_R, ec.LADDER_EVERY, ec.N_STEPS, ec.LADDER_SEED)
    # (without exchange the members do not meet: the coldest alone is the coldest of the batch)
    without = ec.run_ladder(batch.pdfs[:1], x0[:m], m, 1, ec.LADDER_EVERY, ec.N_STEPS, ec.LADDER_SEED, exchange=False)
    return with_x, without


def test_without_exchange_the_coldest_member_is_stuck(ladder_runs):
    _, without = ladder_runs
    modes = ec.ladder_modes()
    draws = without["draws"]
    assert draws.shape == (ec.N_STEPS, ec.LADDER_M, ec.LADDER_D)
    assert ec.occupancy(draws, modes)[1] == 0.0
    side = np.sign(draws @ (modes[0] - modes[1]))
    assert int((side[1:] != side[:-1]).sum()) == 0


def test_with_exchange_the_coldest_member_finds_both_modes(ladder_runs):
    with_x, _ = ladder_runs
    occ = ec.occupancy(with_x["draws"][ec.BURNIN:], ec.ladder_modes())[1]
    rate = with_x["accepts"][:-1] / with_x["attempts"][:-1]
    print(f"occupancy of mode 2: {occ:.4f} (tolerance {ec.OCC_TOL:.4f}); rates {np.round(rate, 3)}; margin {with_x['min_margin']:.2e}")
    assert with_x["min_margin"] > ec.MARGIN
    assert abs(occ - 0.5) <= ec.OCC_TOL
    assert np.all((rate > 0) & (rate < 1)) and with_x["attempts"][-1] == 0


def test_every_rung_keeps_its_own_law():
    """Every rung started from i.i.d. draws of its own member: the mean log-density of each rung over the run stays within 5
    standard errors of the i.i.d. mean -- the standard error from the i.i.d. variance and the integrated autocorrelation time of
    the run's series of rung means.  A sign error in alpha fills the cold rungs with the hot rungs' states and fails this by
    hundreds of standard errors; the occupancy test cannot see it."""
    import reference_math as rm
    _, batch, _ = ec.ladder_case()
    m, n_steps = ec.LADDER_M, 600
    rng = np.random.default_rng(5)
    x0 = np.concatenate([ec.sample_member(p, m, rng) for p in batch.pdfs])
    run = ec.run_ladder(batch.pdfs, x0, m, ec.LADDER_R, ec.LADDER_EVERY, n_steps, 301)
    assert run["min_margin"] > ec.MARGIN
    for t, p in enumerate(batch.pdfs):
        v = np.asarray(rm.log_prob(p, ec.sample_member(p, 100000, rng)), dtype=np.float64)
        s = run["lp"][:, t]
        c = s - s.mean()
        acf = np.array([np.mean(c[:len(c) - k] * c[k:]) for k in range(50)]) / np.mean(c * c)
        cut = int(np.argmax(acf < 0.05)) if (acf < 0.05).any() else len(acf)
        iat = max(1.0, 1.0 + 2.0 * float(acf[1:cut].sum()))
        se = np.sqrt(v.var() * iat / (m * len(s)) + v.var() / len(v))
        z = (s.mean() - v.mean()) / se
        print(f"rung {t}: i.i.d. mean {v.mean():.4f}, run mean {s.mean():.4f}, iat {iat:.2f}, z = {z:+.2f}")
        assert abs(z) < 5.0, (t, z)

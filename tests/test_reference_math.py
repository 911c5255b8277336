"""The extended-precision reference (tests/reference_math.py) against what is known independently of it -- every log_prob and
gradient the reference project recorded, the registration targets' included -- then the CPU oracle against it over the dimension
sweep of the layout tests and over the registration cases (tests/registration_cases.py), and its own longdouble arithmetic
against mpmath at 50 digits.  CPU only.  The last tests evaluate, with the reference alone, the conditions the GPU modules assert
of their cases: the try margins of the reference chains and the curve's near-ties."""
import math
import os

import mpmath
import numpy as np
import pytest

import layout_cases as lc
import reference_math as rm
import registration_cases as rc
from conftest import GOLDEN, golden
from helpers import mixture_target, product_target
from layout_cases import gradient_error, near_tie_rows, rel

KAT_TOL = 1e-12  # relative-or-absolute: the bar the oracle is held to on the same answers (test_oracle_golden.py, test_oracle_mh.py)
LOGPROB_KAT = sorted({k.split("__")[0] for k in golden("logprob_kat.npz").files})
GMIX_KAT = sorted({k.split("__")[0] for k in golden("gmix_kat.npz").files})
MH_GRAD = sorted(f[:-4] for f in os.listdir(GOLDEN) if f.startswith("mh_") and f.endswith(".npz") and "grad_X" in golden(f).files
                 and len(golden(f)["grad_X"]) > 0)
REGISTRATION_KAT = ["cpd_protein", "gmm_protein_k10", "cpd_cube_3d2d"]


def test_longdouble_is_extended():
    assert np.finfo(np.longdouble).nmant >= 63 and rm.HAVE_LONGDOUBLE


@pytest.mark.parametrize("name", LOGPROB_KAT)
def test_reproduces_recorded_logprob(name):
    z = golden("logprob_kat.npz")
    pdf = product_target(z, prefix=f"{name}__target_")
    X = z[f"{name}__X"]
    got = rm.log_prob(pdf, X)
    assert rel(got, z[f"{name}__logp"]) < KAT_TOL
    assert rel(got, z[f"{name}__logp_batched"]) < KAT_TOL
    assert rel(rm.log_prob(pdf, X[3]), z[f"{name}__logp"][3]) < KAT_TOL


@pytest.mark.parametrize("name", GMIX_KAT)
def test_reproduces_recorded_mixture_logprob_and_gradient(name):
    z = golden("gmix_kat.npz")
    pdf = mixture_target(z, prefix=f"{name}__")
    X = z[f"{name}__X"]
    assert rel(rm.log_prob(pdf, X), z[f"{name}__logp"]) < KAT_TOL
    assert rel(rm.gradient(pdf, X), z[f"{name}__grad"]) < KAT_TOL
    lp, gr = rm.log_prob_and_gradient(pdf, X[5])
    assert rel(lp, z[f"{name}__logp"][5]) < KAT_TOL and rel(gr, z[f"{name}__grad"][5]) < KAT_TOL


@pytest.mark.parametrize("name", MH_GRAD)
def test_reproduces_recorded_gradient(name):
    z = golden(name + ".npz")
    pdf = product_target(z)
    if str(z["target_kind"]) == "cpd":          # a cancelling sum: the error as a share of the sum's scale, not of max(1, |value|)
        ref = rm.registration(pdf, z["grad_X"])
        assert np.array_equal(ref["gr"], rm.gradient(pdf, z["grad_X"]))
        assert share(z["grad"], ref["gr"], ref["gr_scale"]) < KAT_TOL
        return
    assert rel(rm.gradient(pdf, z["grad_X"]), z["grad"]) < KAT_TOL


# ------------------------------------------------------------------------------------------ the registration targets
def share(got, want, scale):
    """max |got - want| / scale, elementwise: the error as a share of the value's scale."""
    return float(np.max(np.abs(np.asarray(got, dtype=rm.LD) - want) / scale))


@pytest.mark.parametrize("name", REGISTRATION_KAT)
def test_reproduces_recorded_registration_logprob(name):
    """kat_q holds unit quaternions and rows of norm 0.5 .. 1.5: log_prob normalises."""
    z = golden(f"traj_{name}.npz")
    pdf = product_target(z)
    ref = rm.registration(pdf, z["kat_q"], want_grad=False)
    print(f"{name}: {share(z['kat_logp'], ref['lp'], ref['lp_scale']):.1e} of the scale, smallest neighbour gap {ref['gap']:.1e}")
    assert share(z["kat_logp"], ref["lp"], ref["lp_scale"]) < KAT_TOL
    assert np.array_equal(rm.log_prob(pdf, z["kat_q"]), ref["lp"]) and rm.log_prob(pdf, z["kat_q"][3]) == ref["lp"][3]


@pytest.mark.parametrize("omega", [0.0, 0.2])
@pytest.mark.parametrize("tag", ["3d", "2d"])
def test_reproduces_recorded_cube_registration(tag, omega):
    """helpers_kat.npz: the cube of the reference's own test, log_prob with a translation (the score of the target moved the
    other way: it depends on the differences only, and the outlier box on the target's extent) and the gradient without."""
    import geosss_amd as gs
    z = golden("helpers_kat.npz")
    cube = np.array([[x, y, zz] for zz in (-1, 1) for y in (-1, 1) for x in (-1, 1)], dtype=float)
    src = gs.PointCloud(cube) if tag == "3d" else gs.RotationProjection(cube)
    key = f"cpdt_{tag}_w{int(10 * omega)}"
    qs = z["cpdt_qs"]
    moved = gs.CoherentPointDrift(gs.PointCloud(z[f"cpdt_{tag}_target"] - z[f"cpdt_{tag}_t"]), src, sigma=0.5, k=8, omega=omega)
    ref = rm.registration(moved, qs)
    assert share(z[key + "_logp_qs"], ref["lp"], ref["lp_scale"]) < KAT_TOL
    assert share(z[key + "_grad_qs"], ref["gr"], ref["gr_scale"]) < KAT_TOL
    ref = rm.registration(gs.CoherentPointDrift(gs.PointCloud(z[f"cpdt_{tag}_target"]), src, sigma=0.5, k=8, omega=omega), qs)
    assert share(z[key + "_grad_qs_not"], ref["gr"], ref["gr_scale"]) < KAT_TOL


@pytest.mark.parametrize("model", ["gmm", "cpd"])
@pytest.mark.parametrize("k", [1, 8, 9, 24])
@pytest.mark.parametrize("tag", ["3d", "2d"])
def test_reproduces_recorded_weighted_registration(tag, k, model):
    """cpd_weighted_kat.npz: the reference's log_prob and gradient with non-uniform weights on both clouds."""
    import geosss_amd as gs
    z = golden("cpd_weighted_kat.npz")
    assert k in z["ks"]
    source = (gs.PointCloud if tag == "3d" else gs.RotationProjection)(z[f"{tag}_source"], z[f"{tag}_source_w"])
    target = gs.PointCloud(z[f"{tag}_target"], z[f"{tag}_target_w"])
    if model == "gmm":
        pdf = gs.GaussianMixtureModel(target, source, float(z["sigma"]), k, beta=float(z["beta"]))
    else:
        pdf = gs.CoherentPointDrift(target, source, float(z["sigma"]), k, beta=float(z["beta"]), omega=float(z["omega"]))
    ref = rm.registration(pdf, z[f"{tag}_q"])
    e_lp = share(z[f"{tag}_k{k}_{model}_logp"], ref["lp"], ref["lp_scale"])
    e_gr = share(z[f"{tag}_k{k}_{model}_grad"], ref["gr"], ref["gr_scale"])
    print(f"{tag} k={k} {model}: {e_lp:.1e} (log_prob) {e_gr:.1e} (gradient) of the scale")
    assert e_lp < KAT_TOL and e_gr < KAT_TOL


@pytest.mark.parametrize("name", rc.CASES)
def test_oracle_against_registration_reference(oracle, name):
    """oracle.Target.cpd -- until now run on uniform weights only -- at every row of every case, on and off the sphere: 1e-12 of
    the value's scale.  What that leaves to rounding: the oracle's d^2 carries a few 2^-53 of itself, so a term carries a few
    2^-53 |term|, and gamma the same as a relative error."""
    pdf, X, n_unit = rc.case(name)
    ref = rc.reference(name)
    tgt = rc.oracle_target(oracle, pdf)
    e_lp, e_gr = rc.errors(tgt.log_prob(X), np.array([oracle.gradient(tgt, x) for x in X]), ref)
    print(f"{name}: oracle {e_lp:.1e} (log_prob) {e_gr:.1e} (gradient) of the scale; neighbour gap {ref['gap']:.1e}, "
          f"largest part of a term {ref['term']:.0f}")
    assert abs(tgt.log_prob(X[5]) - float(ref["lp"][5])) <= KAT_TOL * float(ref["lp_scale"][5])
    assert e_lp < KAT_TOL and e_gr < KAT_TOL
    # a row and its negative: the same rotation, the opposite Jacobian
    assert ref["lp"][2] == ref["lp"][3] and np.array_equal(ref["gr"][2], -ref["gr"][3])


def test_registration_sweep_reaches_every_kernel_build():
    """Each of the four builds (8 / 24 slots x uniform / weighted source) gets both target dimensions and both models."""
    seen = {(rc.variant(s), s["dt"], s["model"]) for s in map(rc.spec, rc.SWEEP + ["k20_weighted"])}
    assert seen >= {(v, dt, m) for v in range(4) for dt in (2, 3) for m in ("gmm", "cpd")}


MP_CASES = ["one_point", "one_target_point", "ns24_k24", "sweep_2d_k9_wboth_cpd", "sweep_3d_k8_wsrc_gmm", "sharp_sigma"]


@pytest.mark.parametrize("name", MP_CASES)
def test_registration_longdouble_against_mpmath(name):
    """The longdouble path against its mpmath twin, at 1e-17 of the largest term.  A term is log w - d^2 / (2 sigma^2) + const;
    with T the largest of the three parts, longdouble holds it to T 2^-64 and no better, whatever it cancels to.  That is the
    absolute error of a logsumexp, so log_prob is held to 1e-17 max(its scale, beta sum_l tw_l T); and it is the relative error of
    exp(term - lse), of every gamma, so the gradient is held to 1e-17 max(1, T) of its scale."""
    pdf, X, n_unit = rc.case(name)
    pick = np.r_[0:4, n_unit:n_unit + 3]
    ref = rm._registration_ld(pdf, X[pick], True)
    lp_mp, gr_mp, _, _ = rm._registration_mp(pdf, X[pick])
    T = max(1.0, ref["term"])
    floor = T * float(pdf.beta) * float(np.sum(pdf.target.weights))
    worst_lp = worst_gr = 0.0
    with mpmath.workdps(rm.MP_DIGITS):
        for i in range(len(pick)):
            worst_lp = max(worst_lp, float(abs(_mp(ref["lp"][i]) - lp_mp[i]) / max(_mp(ref["lp_scale"][i]), floor)))
            worst_gr = max(worst_gr, max(float(abs(_mp(a) - b) / _mp(s)) for a, b, s in zip(ref["gr"][i], gr_mp[i], ref["gr_scale"][i])) / T)
        assert rm.log_prob_mp(pdf, X[pick[1]]) == lp_mp[1] and list(rm.gradient_mp(pdf, X[pick[1]])) == list(gr_mp[1])
    print(f"{name}: longdouble against mpmath {worst_lp:.1e} (log_prob) {worst_gr:.1e} (gradient), largest part of a term {ref['term']:.0f}")
    assert worst_lp <= 1e-17 and worst_gr <= 1e-17


# ------------------------------------------------------------------------------------------ the oracle, at every d of the sweep
oracle_target = lc.oracle_target  # (shared with test_hip_mh_layouts.py)


# The bar is the oracle's own 1e-12, scaled by max(1, |value|): for log_prob the value itself, for a gradient the row's largest
# entry, as on the device (a softmax weight inherits kappa 2^-53 from its exponent, so every entry of a mixture's gradient errs
# in proportion to the largest |mu|, not to its own size).  It holds unchanged up to d = 2048: the reference's own error
# (test_longdouble_against_mpmath) is below 1e-17, and the oracle's double sums of d terms err by about sqrt(d) 2^-53 of the
# value's scale.  The one exception is a sum whose terms are far larger than the value they cancel to: at a mean direction of
# the sweep's kappa = 800 vMF terms the oracle's double dot x.mu of d terms carries about sqrt(d) 2^-53 kappa (a random walk of
# half-ulp roundings at partial sums up to kappa), 4e-12 at d = 2048, while log_prob = x.mu - log I0 is a few units.  So for
# d = 1025 .. 2048 the bar is max(1e-12, sqrt(d) 2^-53 magnitude(pdf)), from d, the number format and the parameters alone; the
# reference's own share of it (magnitude 2^-64, checked against mpmath below) is 4e-17.
@pytest.mark.parametrize("d", lc.DIMS)
def test_oracle_against_reference(oracle, d):
    worst = {}
    for family in lc.ORACLE_FAMILIES:
        pdf, X = lc.sweep_case(family, d)
        tgt = oracle_target(oracle, pdf)
        tol = KAT_TOL if d <= 1024 else max(KAT_TOL, np.sqrt(d) * 2.0 ** -53 * magnitude(pdf))
        for tag, P in (("unit", X), ("off", lc.OFF_SPHERE * X)):
            want_lp, want_gr = lc.reference("sweep", family, d)[tag]
            rows = range(len(P)) if family.startswith("curve") or d <= 128 else range(0, len(P), 2)  # (the dense d^2 gradients)
            e_lp = rel(tgt.log_prob(P), want_lp)
            got_gr = np.array([oracle.gradient(tgt, P[i]) for i in rows])
            e_gr = gradient_error(pdf, P[list(rows)], got_gr, want_gr[list(rows)], d)
            worst[family, tag] = (e_lp / tol, e_gr / tol)
        assert abs(tgt.log_prob(X[0]) - float(lc.reference("sweep", family, d)["unit"][0][0])) <= tol * max(1.0, abs(tgt.log_prob(X[0])))
    print(f"d={d}, errors as shares of the bar: " + ", ".join(f"{f}/{t} {a:.1e} {b:.1e}" for (f, t), (a, b) in worst.items()))
    bad = {k: v for k, v in worst.items() if not max(v) < 1.0}
    assert not bad, bad


# ------------------------------------------------------------------------------------------ the reference's own error
def _mp(v):
    hi = float(v)
    return mpmath.mpf(hi) + mpmath.mpf(float(v - rm.LD(hi)))


def magnitude(pdf):
    """The largest quantity the definition forms on the way to its value at a point of norm <= 1: |mu| of a vMF term (x.mu and
    log I0 cancel to a few units at kappa = 800), |A|_inf + |b| of a Bingham, kappa of a curve."""
    kind = rm._kind(pdf)
    if kind == "MixtureModel":
        return max(magnitude(p) for p in pdf.pdfs)
    if kind == "VonMisesFisher":
        return float(np.linalg.norm(pdf.mu))
    if kind == "Uniform":
        return 0.0
    if kind == "CurvedVonMisesFisher":
        return float(pdf.kappa)
    return float(np.abs(pdf.A).sum(axis=1).max() + np.abs(getattr(pdf, "b", 0.0)).sum())


@pytest.mark.parametrize("family", lc.FAMILIES)
@pytest.mark.parametrize("d", [2, 3, 5, 7, 10])
def test_longdouble_against_mpmath(family, d):
    """The longdouble path against the same definitions in mpmath at 50 digits: 1e-17 relative, the reference's own error
    budget.  Relative to max(1, |value|, magnitude(pdf)): a longdouble holds a term of size 800 to 800 * 2^-64 = 4e-17 and no
    better, whatever the size of the value the terms cancel to.  At the sweep's largest magnitude that is 8e-15 absolute, against
    the 1e-12 the oracle and the 1e-10 the device are held to."""
    pdf, X = lc.sweep_case(family, d)
    pick = np.r_[0:8, 8:len(X):37]
    P = np.concatenate([X[pick], lc.OFF_SPHERE * X[pick[:6]]])
    lp, gr = rm.log_prob_and_gradient(pdf, P)
    lp_mp, gr_mp = rm.log_prob_mp(pdf, P), rm.gradient_mp(pdf, P)
    mag = magnitude(pdf)
    worst_lp = worst_gr = 0.0
    with mpmath.workdps(rm.MP_DIGITS):
        for i in range(len(P)):
            worst_lp = max(worst_lp, float(abs(_mp(lp[i]) - lp_mp[i]) / max(1, abs(lp_mp[i]), mag)))
            scale = max(1, mag, max(abs(v) for v in gr_mp[i]))
            worst_gr = max(worst_gr, float(max(abs(_mp(a) - b) for a, b in zip(gr[i], gr_mp[i])) / scale))
    print(f"{family} d={d}: longdouble against mpmath {worst_lp:.1e} (log_prob) {worst_gr:.1e} (gradient)")
    assert worst_lp <= 1e-17 and worst_gr <= 1e-17


@pytest.mark.parametrize("family", ["vmf1", "vmf3", "bingham_dense", "binghamfisher"])
@pytest.mark.parametrize("d", [2, 5, 17, 130])
def test_flat_member_against_the_closed_form(family, d):
    """The member TargetBatch.tempered gives for beta = 0 (every mu = 0; A = 0 and b = 0), which the documented formulas cover
    as they stand: kappa -> 0 takes the vMF term's -log(2 pi) - log I0(kappa) to -log(2 pi), and x^T 0 x + 0^T x = 0.  The
    library's vMF constant is the reference's, the circle's in every dimension: the closed form of a flat mixture is
    -log(2 pi) + log(sum of the weights as MixtureModel._pack takes them), which is -log area(S^(d-1)) + log sum w at d = 2;
    a flat Bingham or Fisher-Bingham member is 0.  Both paths (longdouble, mpmath), points on and off the sphere."""
    import batch_layout_cases as bc
    import geosss_amd as gs
    flat = gs.TargetBatch.tempered(bc.members(family, d)[0], [1.0, 0.5, 0.0]).pdfs[2]
    X = bc.points("flat", 1, 9, d)[0]
    P = np.concatenate([X, lc.OFF_SPHERE * X[:3]])
    if family.startswith("vmf"):
        w = np.array([v for _, v in flat._terms()], dtype=np.float64) if family == "vmf3" else np.ones(1)
        assert not any(np.any(p.mu) for p in (flat.pdfs if family == "vmf3" else [flat]))
        with mpmath.workdps(rm.MP_DIGITS):
            log_2pi = rm._ld(mpmath.log(2 * mpmath.pi))
        want = -log_2pi + np.log(np.sum(w.astype(rm.LD)))
        # the reference normalises the weights once more, in longdouble: its sum is 1 where the doubles' is within K 2^-53 of 1
        bar = 0.0 if family == "vmf1" else 1e-15
        if d == 2:
            log_area = np.log(2.0) + 0.5 * d * np.log(np.pi) - math.lgamma(0.5 * d)
            assert abs(float(want) - np.log(float(np.sum(w))) + log_area) < 1e-15
    else:
        assert not np.any(flat.A) and not np.any(getattr(flat, "b", 0.0))
        want, bar = rm.LD(0), 0.0
    lp, gr = rm.log_prob_and_gradient(flat, P)
    assert lp.shape == (12,) and np.all(np.abs(lp - want) <= bar), (lp, want)
    assert np.all(lp == lp[0]) and not np.any(gr)           # one value at every point, and no slope
    with mpmath.workdps(rm.MP_DIGITS):
        for v in rm.log_prob_mp(flat, P[:4]):
            assert abs(v - _mp(want)) <= max(bar, 1e-17)
    assert float(rm.log_prob(flat, P[0])) == float(lp[0])


# ------------------------------------------------------------------------------------------ the GPU modules' case conditions
@pytest.mark.parametrize("sampler", ["shrink", "reject"])
@pytest.mark.parametrize("case", lc.CHAIN_CASES)
def test_chain_margins(case, sampler):
    """No proposal of a reference chain of test_hip_mixture_layouts.py sits within 1e-8 of its threshold."""
    ref = lc.reference_chain(case, sampler)
    print(f"{case} {sampler}: margin {ref['margin']:.2e}, tries {int(ref['tries'].sum())}, stride {ref['replay'].shape[1]}")
    assert ref["margin"] > lc.MIN_MARGIN


@pytest.mark.parametrize("sampler", ["shrink", "reject"])
@pytest.mark.parametrize("case", rc.CHAIN_CASES)
def test_registration_chain_margins(case, sampler):
    """No proposal of a reference chain of test_hip_registration_reference.py sits within 1e-8 of its threshold (and none of its
    evaluations met a near-tie of the k-th neighbour: reference_math asserts that of every one)."""
    ref = rc.reference_chain(case, sampler)
    print(f"{case} {sampler}: margin {ref['margin']:.2e}, tries {int(ref['tries'].sum())}, stride {ref['replay'].shape[1]}")
    assert ref["margin"] > lc.MIN_MARGIN


# ------------------------------------------------------------------------------------------ the baselines' reference chain
MH_FIXTURES = sorted(f[:-4] for f in os.listdir(GOLDEN) if f.startswith("mh_") and f.endswith(".npz")
                     and str(golden(f)["target_kind"]) != "cpd")
# HMC, longdouble against the reference's own double chain over the whole recorded horizon (the horizon test_oracle_mh.py uses
# for these targets): states differ by up to 1.1e-10 (the README mixture at stepsize 0.1, beyond the integrator's stability
# limit; 7.1e-11 on the dense Bingham, 2.3e-11 on the d = 10 curve, below 2e-11 elsewhere) and the momenta of every step by up
# to 3.9e-9 (README mixture; 1.1e-9 on the d = 10 curve) -- two correct implementations, rounding amplified along 300 .. 600
# transitions.  Sixteen times that, rounded up to a power of ten, is above what test_oracle_mh.py allows the oracle, so its bars
# stand: 1e-9 for states, 1e-7 for the momenta of every step.
HMC_FIXTURE_TOL, HMC_FIXTURE_MOMENTA_TOL = 1e-9, 1e-7


@pytest.mark.parametrize("name", MH_FIXTURES)
def test_mh_chain_reproduces_recorded_chain(name):
    """layout_cases.mh_chain on the reference project's own recorded draws: every state, every accept flag, the counters, every
    stepsize, HMC's momenta after every step."""
    z = golden(name + ".npz")
    kind, n = str(z["sampler"]), len(z["states"]) - 1
    out = lc.mh_chain(product_target(z), z["x0"][None], kind, 0, n, int(z["burnin"]), float(z["stepsize0"]),
                      n_leapfrog=int(z["n_leapfrog"]), mixing_probability=float(z["alpha"]) if kind == "mix" else 0.5,
                      draws=z["draws"][None])
    e_x = float(np.max(np.abs(out["states"][:, 0] - z["states"][1:])))
    print(f"{name}: states {e_x:.1e}, margin {out['margin']:.1e}, near-ties {out['ties']} + {out['same_knot']} at a shared knot")
    assert np.array_equal(out["accept"][:, 0], z["accept"].astype(bool))
    assert int(out["n_accept"][0]) == int(z["n_accept"])
    assert e_x < (HMC_FIXTURE_TOL if kind == "hmc" else KAT_TOL)
    assert np.max(np.abs(out["stepsizes"][:, 0] / z["stepsize_trace"] - 1)) < 1e-13 and out["stepsize"][0] == out["stepsizes"][-1, 0]
    assert out["ties"] == 0
    if kind == "hmc":
        e_v = float(np.max(np.abs(out["momenta_steps"][:, 0] - z["momenta_trace"][1:])))
        print(f"{name}: momenta {e_v:.1e}")
        assert e_v < HMC_FIXTURE_MOMENTA_TOL and np.max(np.abs(out["momenta"][0] - z["momenta"])) < HMC_FIXTURE_MOMENTA_TOL
        assert np.all(np.isnan(out["trace"]))
    else:
        used = ~np.isnan(out["trace"][:, 0])
        assert np.array_equal(used, z["use_rwmh"].astype(bool) if kind == "mix" else np.full(n, kind == "rwmh"))
        assert int(out["n_rwmh"][0]) == int(used.sum())
    if kind == "mix":
        assert int(out["n_rwmh"][0]) == int(z["rwmh_counter"]) and n - int(out["n_rwmh"][0]) == int(z["indep_counter"])
        assert np.max(np.abs(out["trace"][used, 0] / z["rwmh_stepsize_vals"] - 1)) < 1e-13
        assert int(out["adapt_left"][0]) == max(0, int(z["burnin"]) - int(z["rwmh_counter"]))
    # the recorded rows are the draws, in the order they were taken
    assert np.array_equal(out["replay"][0, :len(z["draws"])], z["draws"])


MH_ORACLE_CASES = [(f, d) for f, d in lc.MH_CASES if not f.startswith("gmix")]


@pytest.mark.parametrize("family,d", MH_ORACLE_CASES)
def test_oracle_mh_against_reference_chain(oracle, family, d):
    """oracle.mh_run replaying the longdouble chain's draws: flags and counters equal, the stepsizes to 1e-12, and states and
    momenta within the yardstick the device's bars are derived from (layout_cases.MH_YARDSTICK)."""
    pdf, x0, _ = lc.mh_case(family, d)
    tgt = lc.oracle_target(oracle, pdf)
    for kind in lc.MH_KINDS:
        ref = lc.mh_reference(family, d, kind)
        sampler = {"rwmh": oracle.RWMH, "hmc": oracle.HMC, "indep": oracle.INDEP, "mix": oracle.MIX}[kind]
        out = oracle.mh_run(tgt, x0, ref["steps"], sampler=sampler, stepsize=ref["stepsize0"], adapt_steps=ref["adapt"],
                            n_leapfrog=lc.MH_LEAPFROG, replay=ref["replay"], trace=True, mixing_probability=lc.MH_ALPHA, n_threads=8)
        assert np.all(out["err"] == 0)
        assert np.array_equal(out["accept"].T.astype(bool), ref["accept"]) and np.array_equal(out["n_accept"], ref["n_accept"])
        if kind == "mix":
            assert np.array_equal(out["n_rwmh"], ref["n_rwmh"]) and np.array_equal(out["adapt_left"], ref["adapt_left"])
            assert np.array_equal(out["use_rwmh"].T.astype(bool), ~np.isnan(ref["trace"]))
        e_x = float(np.max(np.abs(out["samples"].transpose(1, 0, 2) - ref["states"])))
        e_eps = float(np.max(np.abs(out["stepsize_trace"].T / ref["stepsizes"] - 1)))
        e_v = rel(out["momenta"], ref["momenta"]) if kind == "hmc" else 0.0
        y_x, y_v = lc.MH_YARDSTICK["hmc" if kind == "hmc" else "rw", lc.layout_family(pdf.d)]
        print(f"{family} d={pdf.d} {kind} ({lc.layout_family(pdf.d)}): states {e_x:.1e} of {y_x:.0e}, stepsizes {e_eps:.1e}, "
              f"momenta {e_v:.1e} of {y_v:.0e}")
        assert e_eps < lc.MH_STEPSIZE_TOL and np.max(np.abs(out["stepsize"] / ref["stepsize"] - 1)) < lc.MH_STEPSIZE_TOL
        assert e_x <= y_x and e_v <= y_v


# vmf_k7000_d3 is 7000 vMF terms of kappa 10 .. 100 scattered over S^2: the terms overlap, log p varies by less than a nat between
# the rows and their proposals, and no proposal kernel rejects a tenth of them at any stepsize (the independence sampler, whose
# proposal ignores the stepsize, accepts 94 in 100).  Its random-walk and mixture chains are held to accepting AND rejecting.
FLAT_CASES = {("vmf_k7000_d3", 0, "rwmh"), ("vmf_k7000_d3", 0, "mix")}


@pytest.mark.parametrize("family,d", lc.MH_CASES + [c for c in lc.MH_FORCED if c not in lc.MH_CASES])
def test_mh_chain_margins(family, d):
    """The conditions test_hip_mh_layouts.py asserts of its cases, with nothing excluded: no proposal within 1e-8 of its
    threshold, no gradient of HMC taken where a curve's candidates tie and differ, every chain set both accepting and
    rejecting (a share of 0.1 .. 0.9; the independence sampler: see test_independence_sampler_accepts)."""
    for kind in lc.MH_KINDS:
        ref = lc.mh_reference(family, d, kind)
        print(f"{family} d={d} {kind}: margin {ref['margin']:.1e}, accepted {ref['share']:.2f}, stepsize {ref['stepsize0']:.3g}, "
              f"near-ties {ref['ties']} + {ref['same_knot']} at a shared knot")
        assert ref["margin"] > lc.MIN_MARGIN
        assert ref["ties"] == 0
        assert len(ref["replay"]) == len(ref["x0"]) and (d == 0 or len(ref["x0"]) == lc.n_rows(d))
        if (family, d, kind) in FLAT_CASES:
            assert 0.0 < ref["share"] < 1.0
        elif kind != "indep":
            assert 0.1 <= ref["share"] <= 0.9
        if kind == "mix":
            assert 0 < ref["n_rwmh"].sum() < ref["accept"].size and np.any(ref["adapt_left"] == 0) and np.any(ref["adapt_left"] > 0)


@pytest.mark.parametrize("family", lc.MH_FAMILIES + lc.LAYOUT_CASES)
def test_independence_sampler_accepts(family):
    """A uniform proposal against a kappa = 800 target is nearly always rejected: every family accepts one somewhere."""
    cases = [(f, d) for f, d in lc.MH_CASES if f == family]
    assert sum(int(lc.mh_reference(f, d, "indep")["n_accept"].sum()) for f, d in cases) > 0


def test_curve_near_ties_are_rare():
    """The near-tie rule of test_hip_logprob_layouts.py leaves nothing out; this only records how often it applies."""
    n_tie = n_all = 0
    for d in lc.DIMS:
        for family in ("curve2", "curve10"):
            pdf, X = lc.sweep_case(family, d)
            for P in (X, lc.OFF_SPHERE * X):
                tie, _, _ = near_tie_rows(pdf, P, d)
                n_tie += int(tie.sum())
                n_all += len(P)
    print(f"near-tie rows of the curve sweep: {n_tie} of {n_all}")
    assert n_tie < 0.01 * n_all

"""The extended-precision reference (tests/reference_math.py) against what is known independently of it -- every log_prob and
gradient the reference project recorded -- then the CPU oracle against it over the dimension sweep of the layout tests, and
its own longdouble arithmetic against mpmath at 50 digits.  CPU only.  The last two tests evaluate, with the reference alone,
the conditions the GPU modules assert of their cases: the try margins of the reference chains and the curve's near-ties."""
import os

import mpmath
import numpy as np
import pytest

import layout_cases as lc
import reference_math as rm
from conftest import GOLDEN, golden
from helpers import mixture_target, product_target
from layout_cases import gradient_error, near_tie_rows, rel

KAT_TOL = 1e-12  # relative-or-absolute: the bar the oracle is held to on the same answers (test_oracle_golden.py, test_oracle_mh.py)
LOGPROB_KAT = sorted({k.split("__")[0] for k in golden("logprob_kat.npz").files})
GMIX_KAT = sorted({k.split("__")[0] for k in golden("gmix_kat.npz").files})
# the registration targets (CoherentPointDrift, GaussianMixtureModel) are not restated by the reference module
MH_GRAD = sorted(f[:-4] for f in os.listdir(GOLDEN) if f.startswith("mh_") and f.endswith(".npz") and "_cpd_" not in f
                 and "_gmm_protein" not in f and "grad_X" in golden(f).files and len(golden(f)["grad_X"]) > 0)


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
    assert rel(rm.gradient(pdf, z["grad_X"]), z["grad"]) < KAT_TOL


# ------------------------------------------------------------------------------------------ the oracle, at every d of the sweep
def oracle_target(orc, pdf):
    kind = rm._kind(pdf)
    if kind == "VonMisesFisher":
        return orc.Target.vmf_mixture(pdf.mu[None])
    if kind == "MixtureModel":
        # Target.vmf_mixture keeps the reference project's log(i0(kappa)), which overflows above kappa = 713; the sweep's
        # mixtures reach kappa = 800, so the normalisers are formed here from the exponentially scaled Bessel function
        from scipy.special import ive
        mu = np.array([p.mu for p in pdf.pdfs])
        kappa = np.linalg.norm(mu, axis=1)
        return orc.Target(orc.VMF_MIXTURE, mu.shape[1], len(mu), mu=mu, lognorm=np.log(2 * np.pi) + np.log(ive(0, kappa)) + kappa,
                          logw=np.log(pdf.weights))
    if kind == "CurvedVonMisesFisher":
        return orc.Target.curve_vmf(pdf.curve.knots, pdf.kappa)
    return orc.Target.bingham(pdf.A, getattr(pdf, "b", None))


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


# ------------------------------------------------------------------------------------------ the GPU modules' case conditions
@pytest.mark.parametrize("sampler", ["shrink", "reject"])
@pytest.mark.parametrize("case", lc.CHAIN_CASES)
def test_chain_margins(case, sampler):
    """No proposal of a reference chain of test_hip_mixture_layouts.py sits within 1e-8 of its threshold."""
    ref = lc.reference_chain(case, sampler)
    print(f"{case} {sampler}: margin {ref['margin']:.2e}, tries {int(ref['tries'].sum())}, stride {ref['replay'].shape[1]}")
    assert ref["margin"] > lc.MIN_MARGIN


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

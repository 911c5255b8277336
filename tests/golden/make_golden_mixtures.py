#!/usr/bin/env python3
"""Generate the gmix_*.npz fixtures of tests/test_hip_mixture.py by RUNNING the reference on MixtureModel targets whose
components are not all von Mises-Fisher (Bingham, Fisher-Bingham, Uniform, curve-vMF, nested mixtures).

    PYTHONDONTWRITEBYTECODE=1 python3 tests/golden/make_golden_mixtures.py

Uses the recorders of make_golden.py.  Every file is named gmix_*: the traj_* / mh_* prefixes are enumerated by the
existing parity and MH tests, which do not know this kind.  Each target is stored as a flat component list
(gmix_spec_* arrays) that tests/test_hip_mixture.py rebuilds with geosss_amd.
"""
import os
import sys

import numpy as np

sys.dont_write_bytecode = True
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from make_golden import record_mh, record_trajectory, save  # noqa: E402  (puts the reference on sys.path)

import geosss as gs  # noqa: E402
from geosss.distributions import Bingham, BinghamFisher, MixtureModel, Uniform, VonMisesFisher  # noqa: E402
from geosss.distributions import CurvedVonMisesFisher, random_bingham  # noqa: E402
from geosss.spherical_curve import SlerpCurve, brownian_curve  # noqa: E402


def unit(v):
    v = np.asarray(v, dtype=float)
    return v / np.linalg.norm(v)


def case_d3():
    """vMF(50 m) + Bingham(A) + Uniform, weights (.5, .3, .2)"""
    A = np.array([[4.0, 1.0, 0.0], [1.0, -2.0, 0.5], [0.0, 0.5, 3.0]])
    mu = 50.0 * unit([0.3, -0.5, 0.8])
    pdf = MixtureModel([VonMisesFisher(mu), Bingham(A), Uniform()], [0.5, 0.3, 0.2])
    spec = [("vmf", {"mu": mu}), ("bingham", {"A": A}), ("uniform", {})]
    return pdf, spec, [0.5, 0.3, 0.2]


def case_d5():
    """two dense Bingham from random_bingham (two seeds) + one Fisher-Bingham"""
    B1 = random_bingham(d=5, vmax=20.0, vmin=0.0, seed=11).A
    B2 = random_bingham(d=5, vmax=15.0, vmin=0.0, seed=12).A
    A3 = random_bingham(d=5, vmax=10.0, vmin=0.0, seed=13).A
    b3 = 4.0 * unit(np.arange(1.0, 6.0))
    pdf = MixtureModel([Bingham(B1), Bingham(B2), BinghamFisher(A3, b3)], [0.4, 0.4, 0.2])
    spec = [("bingham", {"A": B1}), ("bingham", {"A": B2}), ("binghamfisher", {"A": A3, "b": b3})]
    return pdf, spec, [0.4, 0.4, 0.2]


def case_d10_curve():
    """CurvedVonMisesFisher(brownian_curve, 300) + VonMisesFisher(100 m)"""
    knots = brownian_curve(n_points=10, dimension=10, step_size=0.5, seed=4321)
    mu = 100.0 * unit(np.linspace(-1.0, 1.0, 10))
    pdf = MixtureModel([CurvedVonMisesFisher(SlerpCurve(knots), 300.0), VonMisesFisher(mu)], [0.7, 0.3])
    spec = [("curve", {"knots": knots, "kappa": np.float64(300.0)}), ("vmf", {"mu": mu})]
    return pdf, spec, [0.7, 0.3]


def case_nested():
    """MixtureModel([MixtureModel(vMFs), Bingham]) at d = 4"""
    mus = 30.0 * np.array([unit([1, 0, 0, 1]), unit([0, 1, -1, 0]), unit([-1, -1, 0, 1])])
    A = np.diag([3.0, 1.0, 0.0, -2.0])
    inner = MixtureModel([VonMisesFisher(m) for m in mus], [0.2, 0.3, 0.5])
    pdf = MixtureModel([inner, Bingham(A)], [0.6, 0.4])
    spec = [("mixture_vmf", {"mus": mus, "w": np.array([0.2, 0.3, 0.5])}), ("bingham", {"A": A})]
    return pdf, spec, [0.6, 0.4]


CASES = {"d3_vmf_bingham_uniform": case_d3, "d5_bingham_fisher": case_d5, "d10_curve_vmf": case_d10_curve,
         "d4_nested": case_nested}
DIMS = {"d3_vmf_bingham_uniform": 3, "d5_bingham_fisher": 5, "d10_curve_vmf": 10, "d4_nested": 4}


def spec_arrays(spec, weights):
    out = {"spec_kinds": np.array([k for k, _ in spec]), "spec_weights": np.array(weights, dtype=float)}
    for i, (_, arrays) in enumerate(spec):
        for name, v in arrays.items():
            out[f"spec_{i}_{name}"] = np.asarray(v)
    return out


def x0_for(d, seed):
    return gs.sphere.sample_sphere(d - 1, seed=seed)


def main():
    for name, make in CASES.items():
        pdf, spec, w = make()
        d = spec_arrays(spec, w)
        dim = DIMS[name]
        x0 = x0_for(dim, 700 + dim)
        samplers = [("shrink", gs.ShrinkageSphericalSliceSampler)]
        if name.startswith("d3"):
            samplers.append(("reject", gs.RejectionSphericalSliceSampler))
        for sname, cls in samplers:
            for seed in range(31, 80):  # the first seed whose chain keeps a safe margin from every threshold
                rec = record_trajectory(cls, pdf, x0, seed, 300)
                if rec["min_margin"] > 1e-8:
                    break
            print(f"gmix_traj_{sname}_{name}: rej/step={rec['n_reject'] / 300:.3f}, min margin={rec['min_margin']:.2e}")
            save(f"gmix_traj_{sname}_{name}.npz", x0=np.array(x0), sampler=np.array(sname), **d, **rec)
        if name.startswith(("d3", "d5")):
            for kind in ("rwmh", "hmc"):
                rec = record_mh(kind, pdf, x0, 1500 + dim, 300, 100, 0.1)
                print(f"gmix_mh_{kind}_{name}: accept rate {rec['n_accept'] / 300:.3f}")
                save(f"gmix_mh_{kind}_{name}.npz", x0=np.array(x0), **d, **rec)
    # log_prob / gradient known answers: 64 points per case, among them points where one term dominates by > 700 nats
    kat = {}
    rng = np.random.default_rng(99)
    for name, make in CASES.items():
        pdf, spec, w = make()
        dim = DIMS[name]
        X = gs.sphere.radial_projection(rng.standard_normal((48, dim)))
        dom = []
        for kind, arrays in spec:  # the modes of the concentrated terms, where they dominate the others
            if kind == "vmf":
                dom.append(unit(arrays["mu"]))
            elif kind == "mixture_vmf":
                dom += [unit(m) for m in arrays["mus"]]
        while len(dom) < 16:
            dom.append(X[len(dom)])
        X = np.concatenate([X, np.array(dom[:16])])
        kat[f"{name}__X"] = X
        kat[f"{name}__logp"] = np.array([pdf.log_prob(x) for x in X])  # row by row: the batched call fails with Uniform
        kat[f"{name}__grad"] = np.array([pdf.gradient(x) for x in X])
        for k, v in spec_arrays(spec, w).items():
            kat[f"{name}__{k}"] = v
    # a dominance case: a vMF of kappa 700 beside a mild Bingham, the Bingham term ahead by > 1000 nats at the vMF's antipode
    # (kappa stays below the reference's overflow of np.log(i0(kappa)) at ~714)
    mu = 700.0 * unit([0.2, 0.9, -0.3])
    A = np.diag([1.0, 0.0, -1.0])
    pdf = MixtureModel([VonMisesFisher(mu), Bingham(A)], [0.5, 0.5])
    X = np.concatenate([gs.sphere.radial_projection(rng.standard_normal((56, 3))),
                        np.array([unit(mu)] * 4 + [unit(-mu)] * 4)])
    kat["d3_dominant__X"] = X
    kat["d3_dominant__logp"] = np.array([pdf.log_prob(x) for x in X])
    kat["d3_dominant__grad"] = np.array([pdf.gradient(x) for x in X])
    for k, v in spec_arrays([("vmf", {"mu": mu}), ("bingham", {"A": A})], [0.5, 0.5]).items():
        kat[f"d3_dominant__{k}"] = v
    save("gmix_kat.npz", **kat)


if __name__ == "__main__":
    main()

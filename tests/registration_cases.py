"""The registration targets (GaussianMixtureModel, CoherentPointDrift) and evaluation points shared by test_reference_math.py
and test_hip_registration_reference.py, with their extended-precision reference values (tests/reference_math.py) and the
reference chains of the two slice samplers.  A sibling of layout_cases.py: no device is touched here, everything is seeded and
cached, `release()` drops the cache.

Every cloud is a seeded standard-normal cloud.  The device picks its kernel from (k, weights): 8 or 24 list slots (k <= 8 or
not) times a build for uniform source weights and one that carries the weights through the list -- `variant()` below restates
that choice, and SWEEP with the k = 20 edge case puts both target dimensions and both models into each of the four."""
import functools
import itertools
import zlib

import numpy as np

import layout_cases as lc
import reference_math as rm

LD = np.longdouble
OFF_SPHERE = lc.OFF_SPHERE

KS = [1, 8, 9, 24]                # one neighbour; a full 8-slot list; the first k on the 24-slot list (15 dead slots); a full one
WEIGHTS = ["uniform", "wsrc", "wboth"]   # uniform / weighted source / weighted source and target
SWEEP = [f"sweep_{dt}d_k{k}_{w}_{model}" for dt, k, w, model in itertools.product((3, 2), KS, WEIGHTS, ("gmm", "cpd"))]
EDGE = ["ns24_k24", "one_point", "one_target_point", "omega0", "omega999", "sharp_sigma", "k20_weighted"]
LARGE = [f"large_{dt}d_k{k}" for dt in (3, 2) for k in (8, 24)]
CASES = SWEEP + EDGE + LARGE

# the cloud seed of a case: 0 unless the reference's near-tie assertion (reference_math.TIE_GAP) tripped on it.  None did: the
# smallest relative gap between a k-th and a (k+1)-th squared distance is 8.6e-8 on the small clouds and 6.2e-9 on the large
CLOUD_SEEDS = {}


def spec(name):
    """-> dict(ns, nt, dt, k, weights, model, omega, sigma, beta) of a case."""
    s = dict(ns=40, nt=30, dt=3, k=8, weights="wboth", model="cpd", omega=0.2, sigma=0.5, beta=1.0)
    if name.startswith("sweep_") or name.startswith("chain_"):
        _, dt, k, w, model = name.split("_")
        s.update(dt=int(dt[0]), k=int(k[1:]), weights=w, model=model)
        if name.startswith("chain_"):     # a dozen target points at sigma = 1: the rejection sampler accepts within tens of tries
            s.update(nt=12, sigma=1.0)
    elif name.startswith("large_"):
        # 4 * 3000 + 4 * 200 + 8 = 12 808 doubles of LDS, two thirds of the 150 KiB the library accepts
        _, dt, k = name.split("_")
        s.update(ns=3000, nt=200, dt=int(dt[0]), k=int(k[1:]))
    else:
        s.update({"ns24_k24": dict(ns=24, k=24),                       # every source point is a neighbour
                  "one_point": dict(ns=1, nt=1, k=1, model="gmm"),
                  # (no outlier column: the box of a single target point has no volume, and CoherentPointDrift's score is +inf)
                  "one_target_point": dict(nt=1, dt=2, model="gmm"),
                  "omega0": dict(omega=0.0, k=9),                      # the outlier column is log 1e-308
                  "omega999": dict(omega=0.999, dt=2, k=24),
                  # terms thousands of nats apart: most gamma sit on the e^-20 clip, the outlier term leads for many target points
                  "sharp_sigma": dict(sigma=0.02, beta=0.5),
                  "k20_weighted": dict(k=20, dt=2)}[name])             # the k of the reference's scripts
    if s["model"] == "gmm":
        s["omega"] = 0.0
    return s


def variant(s):
    """The kernel build the library picks (gsss_capi.hip: cpd_variant): 0 = 8 slots / uniform source weights, 1 = 8 / weighted,
    2 = 24 / uniform, 3 = 24 / weighted."""
    return (0 if s["k"] <= 8 else 2) + (0 if s["weights"] == "uniform" else 1)


def n_rows(name):
    """Two full workgroups of 256 chains and a ragged third on the small clouds; one lane scans ns * nt = 6 10^5 pairs per
    evaluation of a large one."""
    return 37 if name.startswith("large_") else 2 * 256 + 37


def _rng(*key):
    return np.random.default_rng(zlib.crc32(repr(key).encode()))


def build(s, rng):
    import geosss_amd as gs
    src = rng.standard_normal((s["ns"], 3))
    tgt = rng.standard_normal((s["nt"], s["dt"]))
    sw = np.exp(rng.uniform(-3.0, 3.0, s["ns"]))      # drawn in every case, so that a case's clouds do not depend on its weights
    tw = rng.uniform(0.5, 2.0, s["nt"])
    source = (gs.RotationProjection if s["dt"] == 2 else gs.PointCloud)(src, None if s["weights"] == "uniform" else sw)
    target = gs.PointCloud(tgt, tw if s["weights"] == "wboth" else None)
    if s["model"] == "gmm":
        return gs.GaussianMixtureModel(target, source, s["sigma"], s["k"], beta=s["beta"])
    return gs.CoherentPointDrift(target, source, s["sigma"], s["k"], beta=s["beta"], omega=s["omega"])


def points(rng, n):
    """n rows: unit quaternions -- (0,0,0,1), (1,0,0,0) and a row with its negative among them -- then the same rows (all but the
    last when n is odd) scaled to norm 0.998.  -> (X (n, 4), number of unit rows)"""
    n_unit = n - n // 2
    U = lc._unit(rng.standard_normal((n_unit, 4)))
    U[0], U[1] = (0.0, 0.0, 0.0, 1.0), (1.0, 0.0, 0.0, 0.0)
    U[3] = -U[2]
    return np.concatenate([U, OFF_SPHERE * U[: n // 2]]), n_unit


@functools.lru_cache(maxsize=None)
def case(name):
    """-> (pdf, X (n_rows, 4), number of leading unit rows).  The same object for every test of the case."""
    s = spec(name)
    rng = _rng("registration", name, CLOUD_SEEDS.get(name, 0))
    pdf = build(s, rng)
    X, n_unit = points(rng, n_rows(name))
    return pdf, X, n_unit


@functools.lru_cache(maxsize=None)
def reference(name):
    """reference_math.registration at the case's rows: dict(lp, lp_scale, gr, gr_scale, gap, term), computed once."""
    pdf, X, _ = case(name)
    return rm.registration(pdf, X)


def oracle_target(orc, pdf):
    return orc.Target.cpd(pdf.source.positions, pdf.source.weights, pdf.target.positions, pdf.target.weights, pdf.sigma, pdf.k,
                          pdf.beta, pdf.omega, rm._kind(pdf) == "CoherentPointDrift")


def errors(got_lp, got_gr, ref, rows=slice(None)):
    """(log_prob's, gradient's) largest error as a share of the value's scale."""
    e_lp = np.abs(np.asarray(got_lp, dtype=LD) - ref["lp"][rows]) / ref["lp_scale"][rows]
    e_gr = np.abs(np.asarray(got_gr, dtype=LD) - ref["gr"][rows]) / ref["gr_scale"][rows]
    return float(e_lp.max()), float(e_gr.max())


# ------------------------------------------------------------------------------------------ the slice samplers' reference chain
# the four weighted builds' own shapes (k = 8 and 24, 3-D and projected), a weighted mixture without the outlier column, and
# uniform weights at k = 9
CHAIN_CASES = ["chain_3d_k8_wboth_cpd", "chain_2d_k8_wboth_cpd", "chain_3d_k24_wboth_cpd", "chain_2d_k24_wboth_cpd",
               "chain_2d_k8_wboth_gmm", "chain_3d_k9_uniform_cpd"]
# the seed of each case's draws, chosen on the CPU (test_reference_math.py::test_registration_chain_margins) so that no proposal
# of the reference chain sits within layout_cases.MIN_MARGIN of its threshold.  Seed 0 serves every one of them: the smallest
# margin is 1.4e-5 (chain_2d_k8_wboth_gmm, rejection)
CHAIN_SEEDS = {(name, sampler): 0 for name in CHAIN_CASES for sampler in ("shrink", "reject")}


@functools.lru_cache(maxsize=None)
def chain_target(name):
    return build(spec(name), _rng("registration", name, CLOUD_SEEDS.get(name, 0)))


@functools.lru_cache(maxsize=None)
def reference_chain(name, sampler):
    """layout_cases.slice_chain on the longdouble log_prob: 32 chains x 20 steps from unit quaternions."""
    pdf = chain_target(name)
    x0 = lc._unit(_rng("x0", name).standard_normal((lc.N_CHAINS, 4)))
    out = lc.slice_chain(pdf, x0, sampler, CHAIN_SEEDS[name, sampler])
    out["x0"] = x0
    return out


def release():
    """Drop every cached case, and with it the device copies of the targets' parameters."""
    import gc
    for cache in (case, reference, chain_target, reference_chain):
        cache.cache_clear()
    gc.collect()

"""The targets and evaluation points of the layout sweeps (test_reference_math.py, test_hip_logprob_layouts.py,
test_hip_mixture_layouts.py), and the extended-precision reference chain of the two slice samplers.  No device is touched
here: the distribution objects are parameter carriers, the reference is tests/reference_math.py.  Everything is seeded and
cached, so the tests that share a case share its parameters and its reference values."""
import functools
import zlib

import numpy as np

import reference_math as rm

LD = np.longdouble

# every lane layout, and the first and last d of every cooperative one (GSSS_VEC_LIST, gsss_launch.h)
DIMS = [2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 16, 17, 32, 33, 64, 65, 128, 129, 256, 257, 512, 513, 1024, 1025, 2048]
FAMILIES = ["vmf1", "vmf3", "vmf17", "bingham_dense", "bingham_diag", "binghamfisher", "uniform", "curve2", "curve10", "gmix"]
ORACLE_FAMILIES = ["vmf1", "vmf3", "vmf17", "bingham_dense", "bingham_diag", "binghamfisher", "uniform", "curve2", "curve10"]
GLOBAL_CASES = ["vmf_k40_d600", "vmf_k7000_d3", "curve_k60_d300", "gmix_d100_moved", "gmix_d300_global"]
# the sweep's mixture holds three Bingham-type components of d + 1 rows each and leaves coop16x8 (d = 65 .. 128) for coop64x4:
# this mixture of one Fisher-Bingham, vMF terms and a curve stays there
LAYOUT_CASES = GLOBAL_CASES + ["gmix_d100_coop16x8"]
OFF_SPHERE = 0.998  # HMC's leapfrog evaluates log_prob and gradient slightly off the sphere


def n_rows(d):
    """Two full workgroups (256 lanes, 256 / L chains each) and a ragged third in every layout of the dimension."""
    return 517 if d <= 10 else 131 if d <= 128 else 11


def _rng(*key):
    return np.random.default_rng(zlib.crc32(repr(key).encode()))


def _unit(v):
    v = np.asarray(v, dtype=np.float64)
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


def _sym(rng, d, norm):
    """A dense symmetric matrix of spectral norm about `norm`: a scaled G + G^T (||G + G^T|| ~ 2 sqrt(2 d)), no
    eigendecomposition."""
    G = rng.standard_normal((d, d))
    return (G + G.T) * (norm / (2.0 * np.sqrt(2.0 * d)))


def _bingham(gs, A, b=None):
    """Bingham(A) / BinghamFisher(A, b).  The constructors take an eigendecomposition of A for `.mode` and `.max_log_prob`, which
    neither log_prob nor gradient reads: above d = 128 (seconds per matrix at d = 2048) the parameter carrier is made without
    it."""
    if len(A) <= 128:
        return gs.Bingham(A) if b is None else gs.BinghamFisher(A, b)
    assert np.array_equal(A, A.T)
    pdf = object.__new__(gs.Bingham if b is None else gs.BinghamFisher)
    pdf.A = np.array(A, dtype=np.float64)
    if b is not None:
        pdf.b = np.array(b, dtype=np.float64)
    return pdf


def _uniform(gs, d):
    if d <= 128:
        return gs.Uniform(d)
    pdf = object.__new__(gs.Uniform)
    pdf._d, pdf.A = d, np.zeros((d, d))
    return pdf


def _curve(gs, d, knots, seed):
    # arcs of about half a radian in every dimension (the walk's step has norm step_size * sqrt(d))
    return gs.SlerpCurve(gs.brownian_curve(knots, d, step_size=0.5 / np.sqrt(d), seed=seed))


def _vmf_mixture(gs, rng, d, K):
    """K weighted vMF terms; the first two are concentrated and nearly antipodal (kappa 800 and 400), so that at either mean
    direction one term leads every other by more than 700 nats."""
    dirs = _unit(rng.standard_normal((K, d)))
    dirs[1] = _unit(-dirs[0] + 0.05 * _unit(rng.standard_normal(d)))
    kappa = np.concatenate([[800.0, 400.0], rng.uniform(10.0, 100.0, K)])[:K]
    w = rng.uniform(0.5, 2.0, K)
    return gs.MixtureModel([gs.VonMisesFisher(k * m) for k, m in zip(kappa, dirs)], w), dirs


def _near(rng, anchors, n, spread):
    """n unit rows scattered about the anchor directions: normalise(anchor + spread * unit noise)."""
    a = np.asarray(anchors)[rng.integers(0, len(anchors), n)]
    return _unit(a + spread * _unit(rng.standard_normal(a.shape)))


def _curve_points(rng, curve, n):
    """normalise(curve(t) + 0.2 * noise), noise of unit norm: interior projections occur as well as clipped ones."""
    pts = curve(rng.uniform(0.0, 1.0, n))
    return _unit(pts + 0.2 * _unit(rng.standard_normal(pts.shape)))


def _generic_mixture(gs, rng, d, curve_knots=5, zero="vmf", binghams=1, kappa_pair=(800.0, 30.0), curve_kappa=25.0, conc=1.0):
    """{two vMF, Bingham(s), BinghamFisher, Uniform(), a curve, a nested vMF pair} with unequal weights, one exactly zero.
    -> (pdf, anchor directions)."""
    m = _unit(rng.standard_normal((4, d)))
    comps = [gs.VonMisesFisher(20.0 * conc * m[0]), gs.VonMisesFisher(35.0 * conc * m[1])]
    w = [0.2, 0.0 if zero == "vmf" else 0.1]
    for i in range(binghams):
        comps.append(_bingham(gs, _sym(rng, d, 15.0 * conc)))
        w.append(0.0 if (zero == "bingham" and i == 0) else 0.15)
    comps.append(_bingham(gs, _sym(rng, d, 10.0 * conc), 4.0 * conc * _unit(rng.standard_normal(d))))
    w.append(0.12)
    comps.append(gs.Uniform())
    w.append(0.08)
    anchors = list(m)
    if curve_knots:
        curve = _curve(gs, d, curve_knots, seed=int(rng.integers(1 << 30)))
        comps.append(gs.CurvedVonMisesFisher(curve, curve_kappa))
        w.append(0.25)
        anchors += list(curve.knots)
    comps.append(gs.MixtureModel([gs.VonMisesFisher(kappa_pair[0] * m[2]), gs.VonMisesFisher(kappa_pair[1] * m[3])], [0.3, 0.7]))
    w.append(0.17)
    return gs.MixtureModel(comps, w), np.array(anchors)


def _points(rng, d, n, anchors=None, exact=(), curve=None):
    """n unit rows: uniform ones, rows near the anchors, curve neighbours, and the adversarial rows `exact` as they are."""
    parts = [np.asarray(exact, dtype=np.float64).reshape(-1, d)]
    left = n - len(parts[0])
    if curve is not None:
        parts.append(_curve_points(rng, curve, left // 2))
        left -= left // 2
    if anchors is not None and len(anchors):
        parts.append(_near(rng, anchors, left // 2, 0.3))
        left -= left // 2
    parts.append(_unit(rng.standard_normal((left, d))))
    X = np.concatenate(parts)
    assert X.shape == (n, d)
    return X


@functools.lru_cache(maxsize=12)
def sweep_case(family, d):
    """-> (pdf, X (n_rows(d), d) unit rows).  The same object for every test of the case."""
    import geosss_amd as gs
    rng = _rng("sweep", family, d)
    n = n_rows(d)
    if family == "vmf1":
        m = _unit(rng.standard_normal(d))
        return gs.VonMisesFisher(40.0 * m), _points(rng, d, n, anchors=[m], exact=[m, -m])
    if family in ("vmf3", "vmf17"):
        pdf, dirs = _vmf_mixture(gs, rng, d, 3 if family == "vmf3" else 17)
        return pdf, _points(rng, d, n, anchors=dirs, exact=[dirs[0], -dirs[0], dirs[1], dirs[2], -dirs[2]])
    if family == "bingham_dense":
        return _bingham(gs, _sym(rng, d, 20.0)), _points(rng, d, n)
    if family == "bingham_diag":
        return _bingham(gs, np.diag(np.linspace(-10.0, 30.0, d))), _points(rng, d, n, anchors=np.eye(d)[-1:])
    if family == "binghamfisher":
        return _bingham(gs, _sym(rng, d, 20.0), 5.0 * _unit(rng.standard_normal(d))), _points(rng, d, n)
    if family == "uniform":
        return _uniform(gs, d), _points(rng, d, n)
    if family in ("curve2", "curve10"):
        curve = _curve(gs, d, 2 if family == "curve2" else 10, seed=d + 7)
        k = curve.knots
        n_ref = min(n, 7) if d >= 513 else n
        if len(k) == 2:
            # the antipode of an END knot lies on the branch cut of the segment's atan2 (numerator 0, denominator < 0), where the
            # definition itself jumps between the segment's two ends; with one segment nothing else wins there, so no reference
            # decides the row.  The two-knot curve takes the antipodes a thousandth of a radian off instead; the ten-knot curve
            # keeps the exact antipodes (of its first and its middle knot), where another segment is nearest.
            off = 1e-3 * _unit(rng.standard_normal((2, d)))
            exact = [k[0], k[1], _unit(-k[0] + off[0]), _unit(-k[1] + off[1])]
        else:
            exact = [k[0], -k[0], k[-1], k[len(k) // 2], -k[len(k) // 2]]
        return gs.CurvedVonMisesFisher(curve, 300.0), _points(rng, d, n_ref, exact=exact, curve=curve)
    if family == "gmix":
        pdf, anchors = _generic_mixture(gs, rng, d)
        nested = pdf.pdfs[-1].pdfs[0].mu
        n_ref = min(n, 7) if d >= 513 else n
        return pdf, _points(rng, d, n_ref, anchors=anchors, exact=[_unit(nested), -_unit(nested), _unit(pdf.pdfs[0].mu)],
                            curve=pdf.pdfs[-2].curve)
    raise ValueError(family)


@functools.lru_cache(maxsize=None)
def global_case(name):
    """Targets whose rows do not fit a workgroup's LDS and are read from global memory -> (pdf, X, layout name)."""
    import geosss_amd as gs
    rng = _rng("global", name)
    if name == "vmf_k40_d600":
        d, K = 600, 40
        dirs = _unit(rng.standard_normal((K, d)))
        pdf = gs.MixtureModel([gs.VonMisesFisher(k * m) for k, m in zip(rng.uniform(10.0, 100.0, K), dirs)], rng.uniform(0.5, 2.0, K))
        return pdf, _points(rng, d, 11, anchors=dirs, exact=[dirs[0], -dirs[0]]), "coop64x16"
    if name == "vmf_k7000_d3":
        d, K = 3, 7000
        dirs = _unit(rng.standard_normal((K, d)))
        pdf = gs.MixtureModel([gs.VonMisesFisher(k * m) for k, m in zip(rng.uniform(10.0, 100.0, K), dirs)], rng.uniform(0.5, 2.0, K))
        return pdf, _points(rng, d, 11, anchors=dirs, exact=[dirs[0], -dirs[0]]), "coop64x4"
    if name == "curve_k60_d300":
        curve = _curve(gs, 300, 60, seed=11)
        k = curve.knots
        return gs.CurvedVonMisesFisher(curve, 300.0), _points(rng, 300, 11, exact=[k[0], -k[0], k[30]], curve=curve), "coop64x8"
    if name == "gmix_d100_moved":   # 4 vMF rows + 2 (d + 1) Bingham rows + 40 knots > the ~137 rows of 128 doubles coop16x8 holds
        pdf, anchors = _generic_mixture(gs, rng, 100, curve_knots=40, zero="vmf")
        return pdf, _points(rng, 100, 131, anchors=anchors, curve=pdf.pdfs[-2].curve), "coop64x4"
    if name == "gmix_d300_global":  # two Bingham components and a BinghamFisher: their b rows stay in LDS, one of them unweighted
        pdf, anchors = _generic_mixture(gs, rng, 300, curve_knots=5, zero="bingham", binghams=2)
        return pdf, _points(rng, 300, 11, anchors=anchors, curve=pdf.pdfs[-2].curve), "coop64x8"
    if name == "gmix_d100_coop16x8":
        m = _unit(rng.standard_normal((3, 100)))
        curve = _curve(gs, 100, 5, seed=3)
        pdf = gs.MixtureModel([gs.VonMisesFisher(20.0 * m[0]), _bingham(gs, _sym(rng, 100, 12.0), 4.0 * m[1]),
                               gs.CurvedVonMisesFisher(curve, 25.0), gs.VonMisesFisher(30.0 * m[2])], [0.3, 0.3, 0.25, 0.15])
        return pdf, _points(rng, 100, 131, anchors=np.concatenate([m, curve.knots]), curve=curve), "coop16x8"
    raise ValueError(name)


@functools.lru_cache(maxsize=None)
def reference(kind, *key):
    """(log_prob, gradient) at the unit rows and at the rows scaled to norm 0.998, in longdouble: computed once per case."""
    pdf, X = (sweep_case(*key) if kind == "sweep" else global_case(*key)[:2])
    n = len(X)
    lp, gr = rm.log_prob_and_gradient(pdf, np.concatenate([X, OFF_SPHERE * X]))
    return {"unit": (lp[:n], gr[:n]), "off": (lp[n:], gr[n:])}


# ------------------------------------------------------------------------------------------ error measures
def rel(got, want):
    """max |got - want| / max(1, |want|), elementwise."""
    got, want = np.asarray(got, dtype=LD), np.asarray(want, dtype=LD)
    return float(np.max(np.abs(got - want) / np.maximum(1, np.abs(want)))) if want.size else 0.0


def near_tie_rows(pdf, P, d):
    """Rows of a curve target whose two best candidates differ in x.y by less than 64 d 2^-53: there the gradient may be
    that of either (the threshold comes from the reference and d alone).  -> (bool (n,), candidates' x.y, candidates' gradients)"""
    xy, gy = rm.curve_gradient_candidates(pdf, P)
    if xy.shape[1] == 1:
        return np.zeros(len(P), dtype=bool), xy, gy
    top = np.sort(xy, axis=1)
    return (top[:, -1] - top[:, -2]) < 64 * d * 2.0 ** -53, xy, gy


def gradient_error(pdf, P, got, want, d):
    """max over rows of |got - want| / max(1, the row's |want|_inf).  On a near-tie row of a curve target `want` is the tied
    candidate closest to `got`."""
    got, want = np.asarray(got, dtype=LD), np.array(want, dtype=LD)
    if rm._kind(pdf) == "CurvedVonMisesFisher":
        tie, xy, gy = near_tie_rows(pdf, P, d)
        for i in np.flatnonzero(tie):
            tied = np.flatnonzero(xy[i].max() - xy[i] < 64 * d * 2.0 ** -53)
            want[i] = gy[i, tied[np.argmin([np.max(np.abs(got[i] - gy[i, s])) for s in tied])]]
    if not want.size:
        return 0.0
    scale = np.maximum(1, np.max(np.abs(want), axis=-1, keepdims=True))
    return float(np.max(np.abs(got - want) / scale))


# ------------------------------------------------------------------------------------------ the slice samplers' reference chain
CHAIN_DIMS = [3, 6, 7, 9, 10, 12, 16, 17, 40, 130, 300]
CHAIN_CURVE_DIMS = [7, 12, 40]
CHAIN_CASES = [f"d{d}" for d in CHAIN_DIMS] + [f"d{d}_curve" for d in CHAIN_CURVE_DIMS] + ["gmix_d100_moved", "gmix_d300_global"]
N_CHAINS, N_STEPS = 32, 20
MIN_MARGIN = 1e-8  # what tests/test_hip_mixture.py asserts of its recorded chains
# the seed of each case's draws, chosen on the CPU (test_reference_math.py::test_chain_margins) so that no proposal of the
# reference chain sits within MIN_MARGIN of its threshold; a case that is not listed takes seed 0
CHAIN_SEEDS = {}


@functools.lru_cache(maxsize=None)
def chain_target(case):
    """-> (pdf, fast mode built?)  Moderately concentrated, so that the rejection sampler accepts within tens of tries."""
    import geosss_amd as gs
    if case.startswith("gmix_"):
        return global_case(case)[0], False
    d = int(case[1:].split("_")[0])
    curve = case.endswith("_curve")
    pdf, _ = _generic_mixture(gs, _rng("chain", case), d, curve_knots=4 if curve else 0, kappa_pair=(25.0, 10.0), curve_kappa=12.0,
                              conc=0.4)
    return pdf, (3 <= d <= 16 and not curve)


def slice_chain(pdf, x0, sampler, seed, n_steps=N_STEPS, max_tries=4000):
    """The two slice-sampler transitions restated on reference_math.log_prob in longdouble, for every row of x0 at once.
    Per step a chain consumes d normals, the threshold uniform, (shrinkage only) the uniform of the bracket's position, and
    one uniform per try mapped as lo + (hi - lo) u -- the order `replay=` expects; the draws come from a seeded numpy
    Generator and are recorded per chain.  -> dict(states (n_steps, n, d) float64, tries (n,), rejections (n,), replay
    (n, stride) padded with 0.5, margin: the smallest |p(y) - threshold| over all tries)."""
    rng = np.random.default_rng(seed)
    x = np.asarray(x0, dtype=np.float64).astype(LD)
    n, d = x.shape
    two_pi = 2 * LD(np.pi)  # the samplers' 2 pi is the double
    rows = np.full((n, n_steps * (d + 2 + 64)), 0.5)
    cur = np.zeros(n, dtype=np.int64)
    tries = np.zeros(n, dtype=np.int64)
    margin = np.inf
    states = np.empty((n_steps, n, d))
    idx = np.arange(n)

    def take(who, vals):
        nonlocal rows
        if cur[who].max() + 1 > rows.shape[1]:
            rows = np.concatenate([rows, np.full_like(rows, 0.5)], axis=1)
        rows[who, cur[who]] = vals
        cur[who] += 1
        return vals

    for s in range(n_steps):
        z = rng.standard_normal((n, d))
        for j in range(d):
            take(idx, z[:, j])
        nrm = x / (np.sqrt(np.sum(x * x, axis=1)) + LD(1e-100))[:, None]
        u = z.astype(LD) - np.sum(z * nrm, axis=1)[:, None] * nrm
        u = u / (np.sqrt(np.sum(u * u, axis=1)) + LD(1e-100))[:, None]
        thr = rm.log_prob(pdf, x.astype(np.float64)) + np.log(take(idx, rng.uniform(size=n)).astype(LD))
        if sampler == "shrink":
            hi = two_pi * take(idx, rng.uniform(size=n)).astype(LD)
            lo = hi - two_pi
        else:
            lo, hi = np.zeros(n, dtype=LD), np.full(n, two_pi, dtype=LD)
        active = np.ones(n, dtype=bool)
        for _ in range(max_tries):
            who = idx[active]
            theta = lo[who] + (hi[who] - lo[who]) * take(who, rng.uniform(size=len(who))).astype(LD)
            y = np.cos(theta)[:, None] * x[who] + np.sin(theta)[:, None] * u[who]
            # the device carries its states as doubles from try to try only through x; the proposal is formed from them
            py = rm.log_prob(pdf, y.astype(np.float64))
            tries[who] += 1
            margin = min(margin, float(np.min(np.abs(py - thr[who]))))
            ok = py > thr[who]
            x[who[ok]] = y[ok].astype(np.float64).astype(LD)
            rej = who[~ok]
            if sampler == "shrink":
                neg = theta[~ok] < 0
                lo[rej[neg]] = theta[~ok][neg]
                hi[rej[~neg]] = theta[~ok][~neg]
            active[who[ok]] = False
            if not active.any():
                break
        else:
            raise RuntimeError("the reference chain did not accept within max_tries")
        states[s] = x.astype(np.float64)
    stride = int(cur.max()) + 8
    return dict(states=states, tries=tries, rejections=tries - n_steps, replay=np.ascontiguousarray(rows[:, :stride]), margin=margin)


@functools.lru_cache(maxsize=None)
def reference_chain(case, sampler):
    pdf, _ = chain_target(case)
    seed = CHAIN_SEEDS.get((case, sampler), 0)
    rng = _rng("x0", case)
    x0 = _unit(rng.standard_normal((N_CHAINS, pdf.d)))
    out = slice_chain(pdf, x0, sampler, seed)
    out["x0"] = x0
    return out


def release():
    """Drop every cached case, and with it the device copies of the targets' parameters (gsss_target handles live on the
    distribution objects): a module that used the cases leaves the device as it found it."""
    import gc
    for cache in (sweep_case, global_case, reference, chain_target, reference_chain):
        cache.cache_clear()
    gc.collect()

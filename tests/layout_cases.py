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


# ------------------------------------------------------------------------------------------ the baselines' reference chain
MH_KINDS = ["rwmh", "indep", "mix", "hmc"]
MH_FAMILIES = ["vmf3", "binghamfisher", "curve10", "gmix"]
MH_CASES = [(f, d) for f in MH_FAMILIES for d in DIMS] + [(name, 0) for name in LAYOUT_CASES]
# d = 5, 12 and 40 also run in every further cooperative layout that covers them (test_hip_mh_layouts.py)
MH_FORCED = [(f, d) for d in (5, 12, 40) for f in ("vmf3", "binghamfisher")]
MH_STEPS, MH_ADAPT, MH_LEAPFROG, MH_ALPHA = 8, 4, 3, 0.5
# Two segments of a curve that both clip to the knot they share are a near-tie of near_tie_rows wherever the point lies in the
# knot's cone -- a region, not a coincidence, and the start rows at the knots are in it, so no seed avoids it.  Their candidates
# are the same knot up to the 1e-10 guard of the definition, y = sin(theta) b / (sin(theta) + 1e-10): the gradients differ by
# kappa 1e-10 |1 / sin(theta_a) - 1 / sin(theta_b)| < 1e-8 for kappa = 300 and arcs of 0.25 .. 1 radian, which moves a state by
# eps^2 1e-8 < 5e-11 per gradient.  mh_chain counts these apart (`same_knot`); a near-tie whose candidates' gradients differ by
# more than TIE_GRAD is one at which the chain depends on the choice (`ties`), and no case may meet one.
TIE_GRAD = 1e-8
# the seed of a (family or name, d, kind) whose seed-0 chain misses a condition of test_reference_math.py::test_mh_chain_margins
MH_SEEDS = {}


# What the CPU oracle -- double arithmetic in the kernels' order of operations -- differs from the longdouble chain by, replaying
# its draws: the largest (state, final momentum) deviation over every case of a (sampler class, layout family), rounded up to one
# digit (test_reference_math.py::test_oracle_mh_against_reference_chain holds the oracle to it).  The stepsizes agree exactly.
MH_YARDSTICK = {("rw", "lane"): (3e-15, 0.0), ("rw", "coop4"): (5e-16, 0.0), ("rw", "coop16"): (4e-16, 0.0), ("rw", "coop64"): (2e-16, 0.0),
                ("hmc", "lane"): (1e-11, 7e-12), ("hmc", "coop4"): (6e-14, 8e-14), ("hmc", "coop16"): (2e-14, 7e-14),
                ("hmc", "coop64"): (5e-15, 2e-13)}
MH_CAPS = {"rw": (1e-10, 0.0), "hmc": (1e-9, 1e-7)}  # what the suite already allows (tests/test_hip_mh.py)
MH_STEPSIZE_TOL = 1e-12


def mh_bars(kind, d):
    """-> (state bar, momentum bar) of the device against the longdouble chain: 16 times the yardstick -- a cooperative layout
    sums d terms as a tree over up to 64 lanes x 32 slots where the oracle sums in sequence, each within d 2^-53 of the exact
    value but not the same double -- rounded up to a power of ten, and never above what the suite already allows."""
    cls = "hmc" if kind == "hmc" else "rw"
    return tuple(min(cap, 10.0 ** np.ceil(np.log10(16.0 * y))) if y else 0.0
                 for y, cap in zip(MH_YARDSTICK[cls, layout_family(d)], MH_CAPS[cls]))


def layout_family(d):
    """The four kinds of layout (GSSS_VEC_LIST): a lane per chain, then 4, 16 and 64 lanes per chain."""
    return "lane" if d <= 10 else "coop4" if d <= 32 else "coop16" if d <= 128 else "coop64"


# family or global-row case -> (concentration kappa, the random walk's largest eps, HMC's eps sqrt(kappa) up to d = 16, the power
# of 16 / d it shrinks with above): what mh_stepsize starts from
MH_SCALES = {"vmf3": (800.0, 0.07, 1.9, 0.25), "binghamfisher": (40.0, 1.5, 0.3, 0.0), "curve10": (300.0, 0.12, 0.8, 0.25),
             "gmix": (50.0, 0.3, 1.6, 0.25), "vmf_k7000_d3": (10.0, 1.5, 1.0, 0.25), "vmf_k40_d600": (100.0, 0.2, 1.0, 0.25),
             "curve_k60_d300": (300.0, 0.12, 0.8, 0.25), "gmix_d100_moved": (50.0, 0.3, 1.6, 0.25),
             "gmix_d300_global": (50.0, 0.3, 1.6, 0.25), "gmix_d100_coop16x8": (30.0, 0.3, 1.6, 0.25)}
# the cases whose acceptance share the rule leaves outside [0.1, 0.9] (test_reference_math.py::test_mh_chain_margins)
MH_STEPSIZES = {("vmf3", 3, "rwmh"): 0.03, ("vmf3", 11, "rwmh"): 0.15, ("vmf3", 11, "hmc"): 0.15, ("curve10", 2, "hmc"): 0.08, ("gmix", 2, "hmc"): 0.3}


def mh_family(family, d):
    """The sweep family that stands for `family` at d: above d = 512 the dense Fisher-Bingham's place is taken by the diagonal
    Bingham, whose longdouble reference needs d products where the dense one needs d^2 per evaluation."""
    return "bingham_diag" if family == "binghamfisher" and d >= 513 else family


def mh_steps(family, d):
    """-> (steps, adapting steps): 8 and 4, so that the window ends inside the launch; the generic mixture above d = 1023 holds
    two dense matrices, a longdouble pass over which takes a third of a second, and runs 4 and 2."""
    return (4, 2) if family == "gmix" and d >= 1024 else (MH_STEPS, MH_ADAPT)


def mh_stepsize(family, d, kind):
    """The starting stepsize of a case, from the target's concentration kappa and d alone; test_mh_chain_margins holds every
    case's acceptance share to [0.1, 0.9] with it.  The random-walk proposal normalise(r x + eps z), r ~ sqrt(d), moves by
    eps z / sqrt(d): along the gradient log p changes by about kappa sin(angle to the mode) eps N(0, 1) / sqrt(d), several nats
    either way at eps = 8 sqrt(d) / kappa; the step's length eps costs kappa eps^2 / 2 at a mode, which caps eps for the
    concentrated families, while a Bingham of norm 20 is nearly flat in high dimension and takes steps of a radian.  HMC's
    leapfrog is stable for eps sqrt(kappa) below 2, and its energy error grows with d, which eps ~ d^(-1/4) offsets above
    d = 16."""
    if (family, d, kind) in MH_STEPSIZES:
        return MH_STEPSIZES[family, d, kind]
    conc, cap, hmc, power = MH_SCALES[family]
    if kind == "hmc":
        return hmc / np.sqrt(conc) * min(1.0, (16.0 / d) ** power)
    return min(8.0 * np.sqrt(d) / conc, cap)


def _normalised(a):
    return a / (np.sqrt(np.sum(a * a, axis=1)) + LD(1e-100))[:, None]


def _dot(a, b):
    return np.sum(a * b, axis=1)[:, None]


def mh_chain(pdf, x0, kind, seed, n_steps, adapt_steps, stepsize, n_leapfrog=3, mixing_probability=0.5, draws=None):
    """MetropolisHastings, IndependenceSampler, MixtureRWMHIndependenceSampler (`rwmh`, `indep`, `mix`) and SphericalHMC (`hmc`)
    restated on reference_math.log_prob / gradient in longdouble, for every row of x0 at once:

        rwmh    y = normalise(r x + eps z), r = sqrt(2 gamma(d / 2));  accept when log u < log p(y) - log p(x)
        indep   y = normalise(z)
        mix     a uniform below `mixing_probability` chooses rwmh, else indep; only rwmh proposals adapt eps, and only they count
                towards the adaptation window
        hmc     v = z - x (x.z);  H0 = v.v / 2 - log p(x);  w = v + eps / 2 P(x);  n_leapfrog times: with a = eps |w|,
                (x, w) <- (x cos a + w / |w| sin a, w cos a - x |w| sin a), then w += eps P(x), the last time eps / 2 P(x);
                x <- normalise(x);  H1 = w.w / 2 - log p(x);  accept when log u < H0 - H1 and then keep w as the momentum, else v.
                P(x) = g - x (x.g), g the target's gradient at x
        eps     x 1.02 after an accepted proposal, x 0.98 after a rejected one, for the first `adapt_steps` steps (mix: rwmh proposals)

    normalise(a) = a / (|a| + 1e-100).  A state is carried to the next step as the double a device carries (so is the point at
    which the target is evaluated: reference_math takes double rows), eps as a double product.  Per chain a step consumes -- the
    order the `replay=` argument of the samplers expects -- (mix) the choice uniform, (an rwmh proposal) the gamma variate, d
    normals, the accept uniform; they come from a seeded numpy Generator, or from `draws` (n, stride), and are recorded.

    -> dict(states (n_steps, n, d), accept (n_steps, n) bool, n_accept (n,), stepsize (n,) final, stepsizes (n_steps, n) after
    every step, trace: the same with NaN where the step made no rwmh proposal (every step of indep and hmc), n_rwmh, adapt_left
    (n,), momenta (n, d) and momenta_steps (n_steps, n, d) (hmc, else zeros), replay (n, stride) padded with 0.5, margin: the
    smallest |log u - log ratio|, share: accepted / proposed, ties / same_knot: gradients taken at a near-tie row of a curve target whose candidates differ / coincide, see TIE_GRAD)."""
    assert kind in MH_KINDS
    rng = np.random.default_rng(seed)
    x = np.array(x0, dtype=np.float64)
    n, d = x.shape
    rows = np.full((n, n_steps * (d + 3) + 8), 0.5) if draws is None else np.array(draws, dtype=np.float64)
    assert rows.shape[0] == n
    cur = np.zeros(n, dtype=np.int64)
    idx = np.arange(n)

    def take(who, make):
        if draws is None:
            rows[who, cur[who]] = make(len(who))
        vals = rows[who, cur[who]]
        cur[who] += 1
        return vals

    def normals():
        cols = cur[:, None] + np.arange(d)
        if draws is None:
            rows[idx[:, None], cols] = rng.standard_normal((n, d))
        cur[:] += d
        return rows[idx[:, None], cols].astype(LD)

    curve = rm._kind(pdf) == "CurvedVonMisesFisher"
    ties = same_knot = 0

    def projected_gradient(at):
        nonlocal ties, same_knot
        P = at.astype(np.float64)
        if curve:
            tie, xy, gy = near_tie_rows(pdf, P, d)
            for i in np.flatnonzero(tie):
                tied = gy[i, xy[i].max() - xy[i] < 64 * d * 2.0 ** -53]
                same_knot += 1
                if float(np.max(np.abs(tied - tied[0]))) > TIE_GRAD:
                    ties += 1
        g = rm.gradient(pdf, P)
        return g - at * _dot(at, g)

    eps = np.broadcast_to(np.asarray(stepsize, dtype=np.float64), (n,)).copy()
    left = np.full(n, int(adapt_steps), dtype=np.int64)
    n_rwmh = np.zeros(n, dtype=np.int64)
    n_accept = np.zeros(n, dtype=np.int64)
    v = np.zeros((n, d))
    states, momenta_steps = np.empty((n_steps, n, d)), np.zeros((n_steps, n, d))
    accept = np.zeros((n_steps, n), dtype=bool)
    stepsizes, trace = np.empty((n_steps, n)), np.full((n_steps, n), np.nan)
    margin = np.inf
    lp_x = rm.log_prob(pdf, x)
    for s in range(n_steps):
        xl = x.astype(LD)
        use = np.zeros(n, dtype=bool)
        if kind == "hmc":
            z = normals()
            p = z - xl * _dot(xl, z)
            h0 = np.sum(p * p, axis=1) / 2 - lp_x
            e = eps.astype(LD)[:, None]
            y = xl
            w = p + e / 2 * projected_gradient(y)
            for leap in range(n_leapfrog):
                nw = np.sqrt(_dot(w, w))
                c, sn = np.cos(e * nw), np.sin(e * nw)
                y, w = y * c + (w / nw) * sn, w * c - (y * nw) * sn
                w = w + (e if leap < n_leapfrog - 1 else e / 2) * projected_gradient(y)
            y = _normalised(y).astype(np.float64)
            lp_y = rm.log_prob(pdf, y)
            ratio = h0 - (np.sum(w * w, axis=1) / 2 - lp_y)
        else:
            if kind == "rwmh":
                use[:] = True
            elif kind == "mix":
                use = take(idx, rng.random) < mixing_probability
            r = np.zeros(n, dtype=LD)
            who = idx[use]
            if len(who):
                r[who] = np.sqrt(2 * take(who, lambda m: rng.standard_gamma(0.5 * d, m)).astype(LD))
            z = normals()
            y = np.where(use[:, None], r[:, None] * xl + eps.astype(LD)[:, None] * z, z)
            y = _normalised(y).astype(np.float64)
            lp_y = rm.log_prob(pdf, y)
            ratio = lp_y - lp_x
        log_u = np.log(take(idx, rng.random).astype(LD))
        ok = log_u < ratio
        margin = min(margin, float(np.min(np.abs(log_u - ratio))))
        x[ok] = y[ok]
        lp_x = np.where(ok, lp_y, lp_x)
        if kind == "hmc":
            v = np.where(ok[:, None], w, p).astype(np.float64)
            momenta_steps[s] = v
        n_accept += ok
        n_rwmh += use
        if kind == "mix":
            adapt = use & (left > 0)
            left[adapt] -= 1
        else:
            adapt = np.full(n, s < adapt_steps)
        eps[adapt] = eps[adapt] * np.where(ok[adapt], 1.02, 0.98)
        states[s], accept[s], stepsizes[s] = x, ok, eps
        trace[s, use] = eps[use]
    stride = int(cur.max()) + 8
    replay = np.full((n, stride), 0.5)
    replay[:, :min(stride, rows.shape[1])] = rows[:, :stride]
    return dict(states=states, accept=accept, n_accept=n_accept, stepsize=eps, stepsizes=stepsizes, trace=trace, n_rwmh=n_rwmh,
                adapt_left=left, momenta=v, momenta_steps=momenta_steps, replay=replay, margin=margin,
                share=float(accept.mean()), ties=ties, same_knot=same_knot)


@functools.lru_cache(maxsize=None)
def mh_case(family, d):
    """-> (pdf, x0 (n_rows(d), d), layout name or None): a sweep case (family, d) or a global-row target (name, 0) with the
    case's own rows as start points.  The curve and generic-mixture sweeps keep 7 rows above d = 512; seeded uniform rows bring
    those to the 11 that fill two workgroups and part of a third."""
    if d == 0:
        return global_case(family)
    pdf, X = sweep_case(mh_family(family, d), d)
    if len(X) < n_rows(d):
        X = np.concatenate([X, _unit(_rng("mh rows", family, d).standard_normal((n_rows(d) - len(X), d)))])
    return pdf, X, None


@functools.lru_cache(maxsize=None)
def mh_reference(family, d, kind):
    pdf, x0, _ = mh_case(family, d)
    steps, adapt = mh_steps(family, d)
    eps = mh_stepsize(family, pdf.d, kind)
    out = mh_chain(pdf, x0, kind, MH_SEEDS.get((family, d, kind), 0), steps, adapt, eps, n_leapfrog=MH_LEAPFROG,
                   mixing_probability=MH_ALPHA)
    out.update(x0=x0, stepsize0=eps, steps=steps, adapt=adapt)
    return out


def oracle_target(orc, pdf):
    """The CPU oracle's description of a target of ORACLE_FAMILIES (and of the vMF and curve targets of GLOBAL_CASES)."""
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


def release():
    """Drop every cached case, and with it the device copies of the targets' parameters (gsss_target handles live on the
    distribution objects): a module that used the cases leaves the device as it found it."""
    import gc
    for cache in (sweep_case, global_case, reference, chain_target, reference_chain, mh_case, mh_reference):
        cache.cache_clear()
    rm._MATRICES.clear()
    gc.collect()

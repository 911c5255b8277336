"""The angular central Gaussian cases shared by test_acg_host.py and test_hip_acg.py: the precision matrices, log_prob and
gradient restated in longdouble, and the longdouble reference chain of the two slice samplers.  No device is touched here: the
distribution objects are parameter carriers.  Everything is seeded and cached, so the tests that share a case share its
parameters and its reference values."""
import functools

import numpy as np

import layout_cases as lc

LD = np.longdouble

# the replayed chains: layout_cases.CHAIN_DIMS (every kind of exact layout, rows in LDS and in global memory) ...
CHAIN_DIMS = [3, 6, 7, 9, 10, 12, 16, 17, 40, 130, 300]
# ... and in fast mode every dimension the lane kernels are built for
FAST_DIMS = [3, 4, 5, 6, 7, 8, 9, 10]
SAMPLERS = ["shrink", "reject"]
N_CHAINS, N_STEPS = lc.N_CHAINS, lc.N_STEPS
MIN_MARGIN = lc.MIN_MARGIN
MAX_TRIES = 4000
# the seed of a (d, sampler) whose seed-0 chain misses a condition of test_acg_host.py::test_chain_margins; none does
CHAIN_SEEDS = {}


@functools.lru_cache(maxsize=None)
def precision(d):
    """Lambda(d) = Q diag(linspace(1, 1 + 40 / sqrt(d), d)) Q^T, Q from the QR of a seeded Gaussian matrix, symmetric to the last
    bit.  The spread of the spectrum shrinks with d so that the rejection sampler accepts within tens of tries everywhere."""
    rng = np.random.default_rng(1000 + d)
    Q, _ = np.linalg.qr(rng.standard_normal((d, d)))
    L = (Q * np.linspace(1.0, 1.0 + 40.0 / np.sqrt(d), d)) @ Q.T
    return 0.5 * (L + L.T)


@functools.lru_cache(maxsize=8)
def target(d):
    """gs.AngularCentralGaussian(precision(d)): the same object for every test of the dimension."""
    import geosss_amd as gs
    return gs.AngularCentralGaussian(precision(d))


@functools.lru_cache(maxsize=2)
def _precision_ld(d):
    return precision(d).astype(LD)


def log_prob_and_gradient(L, X):
    """-(d / 2) log(x^T L x) and -d L x / (x^T L x) at the double rows X, in longdouble.  L: a double or longdouble matrix."""
    L = np.asarray(L)
    if L.dtype != LD:
        L = L.astype(LD)
    X = np.atleast_2d(np.asarray(X, dtype=np.float64)).astype(LD)
    d = LD(X.shape[1])
    LX = X @ L  # (L symmetric)
    q = np.sum(LX * X, axis=1)
    return -(d / 2) * np.log(q), -d * LX / q[:, None]


def log_prob(L, X):
    return log_prob_and_gradient(L, X)[0]


@functools.lru_cache(maxsize=None)
def points(d):
    """lc.n_rows(d) unit rows: uniform ones, and rows near the two ends of the spectrum's axes."""
    rng = np.random.default_rng(2000 + d)
    n = lc.n_rows(d)
    X = rng.standard_normal((n, d))
    v = np.linalg.eigh(precision(d))[1] if d <= 512 else None
    if v is not None:  # near the mode axis and near the axis of least density
        X[:4] = v[:, 0] + 0.05 * X[:4]
        X[4:8] = v[:, -1] + 0.05 * X[4:8]
    return X / np.linalg.norm(X, axis=1, keepdims=True)


@functools.lru_cache(maxsize=None)
def reference(d):
    """(log_prob, gradient) at points(d) and at the rows scaled to norm 0.998, in longdouble: computed once per d."""
    X = points(d)
    n = len(X)
    lp, gr = log_prob_and_gradient(_precision_ld(d), np.concatenate([X, lc.OFF_SPHERE * X]))
    return {"unit": (lp[:n], gr[:n]), "off": (lp[n:], gr[n:])}


def slice_chain(log_prob_ld, x0, sampler, seed, n_steps=N_STEPS, max_tries=MAX_TRIES):
    """layout_cases.slice_chain on a log-density given as a function of double rows -> longdouble values: the two slice-sampler
    transitions in longdouble for every row of x0 at once, the same draw order (per step d normals, the threshold uniform,
    shrinkage's bracket uniform, one uniform per try), the same `replay` rows and the same `margin`."""
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
        thr = log_prob_ld(x.astype(np.float64)) + np.log(take(idx, rng.uniform(size=n)).astype(LD))
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
            py = log_prob_ld(y.astype(np.float64))
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
def reference_chain(d, sampler):
    """N_CHAINS x N_STEPS of the sampler on Lambda(d), from seeded uniform start rows."""
    L = _precision_ld(d)
    x0 = np.random.default_rng(3000 + d).standard_normal((N_CHAINS, d))
    x0 /= np.linalg.norm(x0, axis=1, keepdims=True)
    out = slice_chain(lambda X: log_prob(L, X), x0, sampler, CHAIN_SEEDS.get((d, sampler), 0))
    out["x0"] = x0
    return out


def release():
    """Drop every cached case, and with it the device copies of the targets' parameters."""
    import gc
    for cache in (precision, target, _precision_ld, points, reference, reference_chain):
        cache.cache_clear()
    gc.collect()

"""Extended-precision restatement of log_prob and gradient of the sampler targets, written from the formulas in the
docstrings of geosss_amd/distributions.py alone.  TEST INFRASTRUCTURE: a plain module, no pytest.

It reads the parameters of the distribution objects (`.mu`, `.A`, `.b`, `.curve.knots`, `.kappa`, `.weights`, `.pdfs`) and
calls none of the package's arithmetic, so it anchors both the CPU oracle and the device at any dimension:

    vMF term        x.mu - log(2 pi) - log I0(|mu|)                          (log I0 from mpmath)
    vMF mixture     logsumexp over the terms with normalised weights;  gradient: the softmax-weighted mean of the mu_k
                    (a single VonMisesFisher: mu)
    Bingham         x^T A x,          gradient 2 A x
    BinghamFisher   x^T A x + b.x,    gradient 2 A x  (without b: the class inherits Bingham's gradient)
    Uniform         0,                gradient 0
    curve           per segment a -> b of arc theta = acos(clip(a.b)):  t = clip(atan2(b.x - a.x cos theta, a.x sin theta), 0, theta),
                    y = (sin(theta - t) a + sin(t) b) / (sin(theta) + 1e-10),  distance acos(clip(x.y));  the first segment of
                    least distance wins;  log_prob = kappa x.y,  gradient kappa y
    MixtureModel    of anything, nested included: logsumexp over the flattened terms;  gradient: the softmax-weighted sum of the
                    components' own gradients

Vector work (dots, quadratic forms) and the scalar transcendentals run in np.longdouble where it carries a 64-bit significand
(x87 extended precision); `log_prob_mp` / `gradient_mp` evaluate the same definitions in mpmath at 50 digits -- the measure of
the longdouble path's own error (tests/test_reference_math.py), and the path taken where longdouble is only a double."""
import mpmath
import numpy as np

LD = np.longdouble
HAVE_LONGDOUBLE = np.finfo(LD).nmant >= 63
MP_DIGITS = 50


def _names(pdf):
    return [c.__name__ for c in type(pdf).__mro__]


def _kind(pdf):
    n = _names(pdf)
    for k in ("MixtureModel", "CurvedVonMisesFisher", "Uniform", "BinghamFisher", "Bingham", "VonMisesFisher"):
        if k in n:
            return k
    raise TypeError(f"reference_math does not restate {type(pdf).__name__}")


def _ld(s):
    """mpmath number -> longdouble, through 25 significant digits (more than the 64-bit significand holds)."""
    return LD(mpmath.nstr(s, 25))


def flatten(pdf, weight=1.0):
    """[(component, weight as a Python float or longdouble)] with nested mixtures expanded and the weights of every level
    normalised to one."""
    if _kind(pdf) != "MixtureModel":
        return [(pdf, LD(weight))]
    w = np.asarray(pdf.weights, dtype=LD)
    w = w / w.sum()
    out = []
    for p, wk in zip(pdf.pdfs, w):
        out += flatten(p, LD(weight) * wk)
    return out


# ------------------------------------------------------------------------------------------ longdouble path
def _rows(X):
    X = np.asarray(X, dtype=np.float64)
    return X.ndim == 1, np.atleast_2d(X).astype(LD)


def _vmf_norm_ld(mu):
    """|mu| in longdouble and log(2 pi) + log I0(|mu|): the Bessel function at the longdouble norm, from mpmath."""
    with mpmath.workdps(MP_DIGITS):
        m = [mpmath.mpf(float(v)) for v in np.asarray(mu, dtype=np.float64)]
        kappa = mpmath.sqrt(mpmath.fsum(v * v for v in m))
        return _ld(mpmath.log(2 * mpmath.pi) + mpmath.log(mpmath.besseli(0, kappa)))


def curve_candidates(pdf, X):
    """Every segment's candidate for rows X (n, d): (x.y (n, S), y (n, S, d)) in longdouble, S = knots - 1."""
    _, x = _rows(X)
    knots = np.asarray(pdf.curve.knots, dtype=np.float64).astype(LD)
    a, b = knots[:-1], knots[1:]
    theta = np.arccos(np.clip(np.sum(a * b, axis=-1), LD(-1), LD(1)))            # (S,)
    ax, bx = x @ a.T, x @ b.T                                                    # (n, S)
    t = np.clip(np.arctan2(bx - ax * np.cos(theta), ax * np.sin(theta)), LD(0), theta)
    y = (np.sin(theta - t)[..., None] * a + np.sin(t)[..., None] * b) / (np.sin(theta) + LD(1e-10))[:, None]
    xy = np.sum(x[:, None, :] * y, axis=-1)
    return xy, y


def _curve_ld(pdf, x):
    xy, y = curve_candidates(pdf, x)
    dist = np.arccos(np.clip(xy, LD(-1), LD(1)))
    best = np.argmin(dist, axis=1)                                               # the first of least distance
    r = np.arange(len(best))
    kappa = LD(float(pdf.kappa))
    return kappa * xy[r, best], kappa * y[r, best]


def _single_ld(pdf, x, want_grad):
    """(log_prob (n,), gradient (n, d) or None) of one non-mixture component at longdouble rows x."""
    kind = _kind(pdf)
    n, d = x.shape
    if kind == "VonMisesFisher":
        mu = np.asarray(pdf.mu, dtype=np.float64).astype(LD)
        return x @ mu - _vmf_norm_ld(pdf.mu), (np.broadcast_to(mu, x.shape).copy() if want_grad else None)
    if kind == "Uniform":
        return np.zeros(n, dtype=LD), (np.zeros_like(x) if want_grad else None)
    if kind in ("Bingham", "BinghamFisher"):
        A = np.asarray(pdf.A, dtype=np.float64).astype(LD)
        Ax = np.einsum("ij,nj->ni", A, x)                                        # x^T A x = x . (A x), whatever A
        lp = np.sum(Ax * x, axis=-1)
        if kind == "BinghamFisher":
            lp = lp + x @ np.asarray(pdf.b, dtype=np.float64).astype(LD)
        return lp, (2 * Ax if want_grad else None)
    if kind == "CurvedVonMisesFisher":
        lp, g = _curve_ld(pdf, x)
        return lp, (g if want_grad else None)
    raise TypeError(kind)


def _eval_ld(pdf, X, want_grad):
    single, x = _rows(X)
    if _kind(pdf) != "MixtureModel":
        lp, g = _single_ld(pdf, x, want_grad)
    else:
        terms = [(p, w) for p, w in flatten(pdf) if w > 0]                      # a zero weight adds no term
        vals, grads = [], []
        for p, w in terms:
            lp, g = _single_ld(p, x, want_grad)
            vals.append(lp + np.log(w))
            grads.append(g)
        v = np.stack(vals, axis=-1)                                              # (n, T)
        m = np.max(v, axis=-1)
        e = np.exp(v - m[:, None])
        s = e.sum(axis=-1)
        lp = m + np.log(s)
        g = None
        if want_grad:
            soft = e / s[:, None]
            g = np.zeros_like(x)
            for k, gk in enumerate(grads):
                g += soft[:, k:k + 1] * gk
    if single:
        return lp[0], (g[0] if want_grad else None)
    return lp, g


# ------------------------------------------------------------------------------------------ mpmath path
def _mpv(v):
    return [mpmath.mpf(float(t)) for t in np.asarray(v, dtype=np.float64)]


def _dot_mp(a, b):
    return mpmath.fsum(p * q for p, q in zip(a, b))


def _clip_mp(v, lo, hi):
    return lo if v < lo else (hi if v > hi else v)


def _single_mp(pdf, x):
    """(log_prob, gradient list) of one non-mixture component at one point x (list of mpf)."""
    kind = _kind(pdf)
    d = len(x)
    if kind == "VonMisesFisher":
        mu = _mpv(pdf.mu)
        kappa = mpmath.sqrt(_dot_mp(mu, mu))
        return _dot_mp(x, mu) - mpmath.log(2 * mpmath.pi) - mpmath.log(mpmath.besseli(0, kappa)), mu
    if kind == "Uniform":
        return mpmath.mpf(0), [mpmath.mpf(0)] * d
    if kind in ("Bingham", "BinghamFisher"):
        A = [_mpv(r) for r in np.asarray(pdf.A, dtype=np.float64)]
        Ax = [_dot_mp(r, x) for r in A]
        lp = _dot_mp(Ax, x)
        if kind == "BinghamFisher":
            lp += _dot_mp(_mpv(pdf.b), x)
        return lp, [2 * v for v in Ax]
    if kind == "CurvedVonMisesFisher":
        knots = [_mpv(r) for r in np.asarray(pdf.curve.knots, dtype=np.float64)]
        best, out = None, None
        for a, b in zip(knots[:-1], knots[1:]):
            theta = mpmath.acos(_clip_mp(_dot_mp(a, b), -1, 1))
            ax, bx = _dot_mp(a, x), _dot_mp(b, x)
            t = _clip_mp(mpmath.atan2(bx - ax * mpmath.cos(theta), ax * mpmath.sin(theta)), mpmath.mpf(0), theta)
            den = mpmath.sin(theta) + mpmath.mpf(1e-10)
            y = [(mpmath.sin(theta - t) * p + mpmath.sin(t) * q) / den for p, q in zip(a, b)]
            xy = _dot_mp(x, y)
            dist = mpmath.acos(_clip_mp(xy, -1, 1))
            if best is None or dist < best:
                best, out = dist, (xy, y)
        kappa = mpmath.mpf(float(pdf.kappa))
        return kappa * out[0], [kappa * v for v in out[1]]
    raise TypeError(kind)


def _flatten_mp(pdf, weight):
    if _kind(pdf) != "MixtureModel":
        return [(pdf, weight)]
    w = _mpv(pdf.weights)
    tot = mpmath.fsum(w)
    out = []
    for p, wk in zip(pdf.pdfs, w):
        out += _flatten_mp(p, weight * wk / tot)
    return out


def _point_mp(pdf, x):
    if _kind(pdf) != "MixtureModel":
        return _single_mp(pdf, x)
    vals, grads = [], []
    for p, w in _flatten_mp(pdf, mpmath.mpf(1)):
        if w > 0:
            lp, g = _single_mp(p, x)
            vals.append(lp + mpmath.log(w))
            grads.append(g)
    m = max(vals)
    e = [mpmath.exp(v - m) for v in vals]
    s = mpmath.fsum(e)
    g = [mpmath.fsum(ek * gk[i] for ek, gk in zip(e, grads)) / s for i in range(len(x))]
    return m + mpmath.log(s), g


def _eval_mp(pdf, X):
    X = np.asarray(X, dtype=np.float64)
    with mpmath.workdps(MP_DIGITS):
        res = [_point_mp(pdf, _mpv(r)) for r in np.atleast_2d(X)]
    lp = np.array([r[0] for r in res], dtype=object)
    g = np.array([r[1] for r in res], dtype=object)
    return (lp[0], g[0]) if X.ndim == 1 else (lp, g)


def log_prob_mp(pdf, X):
    """log_prob in mpmath at 50 digits: an object array of mpf (or one mpf for a point)."""
    return _eval_mp(pdf, X)[0]


def gradient_mp(pdf, X):
    return _eval_mp(pdf, X)[1]


def _mp_to_ld(a):
    if isinstance(a, np.ndarray):
        return np.array([_ld(v) for v in a.ravel()], dtype=LD).reshape(a.shape)
    return _ld(a)


# ------------------------------------------------------------------------------------------ the reference
def log_prob(pdf, X):
    """log_prob of rows X (n, d) or a point (d,), as longdouble."""
    if HAVE_LONGDOUBLE:
        return _eval_ld(pdf, X, False)[0]
    return _mp_to_ld(log_prob_mp(pdf, X))


def gradient(pdf, X):
    """The class's gradient at rows X (n, d) or a point (d,), as longdouble."""
    if HAVE_LONGDOUBLE:
        return _eval_ld(pdf, X, True)[1]
    return _mp_to_ld(gradient_mp(pdf, X))


def log_prob_and_gradient(pdf, X):
    """Both at once (one pass over the parameters)."""
    if HAVE_LONGDOUBLE:
        return _eval_ld(pdf, X, True)
    lp, g = _eval_mp(pdf, X)
    return _mp_to_ld(lp), _mp_to_ld(g)


def curve_gradient_candidates(pdf, X):
    """For a CurvedVonMisesFisher: (x.y (n, S), kappa y (n, S, d)) of every segment, for the near-tie rule of the tests."""
    xy, y = curve_candidates(pdf, X)
    return xy, LD(float(pdf.kappa)) * y

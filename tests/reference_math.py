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
    registration    GaussianMixtureModel / CoherentPointDrift on a quaternion q (x, y, z, w): R the rotation matrix of q / |q|,
                    T(x) = R x or, for a RotationProjection source, its first two rows;  per target point y_l the k smallest
                    d^2 = |y_l - T x_i|^2 over ALL source points (a full sort), terms log w_i - d^2 / (2 sigma^2) + log_const with
                    log_const = -dim / 2 log(2 pi sigma^2) [+ log(1 - omega) for CPD], CPD's outlier column
                    log(omega + 1e-308) - sum log ptp(target);  log_prob = beta sum_l tw_l logsumexp_l;  gradient: gamma =
                    exp(clip(term - lse, -20, 0)), G = sum tw_l gamma / sigma^2 (y_l - T x_i)(padded) (x) x_i contracted with
                    d(M / r)/dq at q AS GIVEN, r = |q|^2 + 1e-300 (`registration` below returns the values' scales too)

Vector work (dots, quadratic forms) and the scalar transcendentals run in np.longdouble where it carries a 64-bit significand
(x87 extended precision); `log_prob_mp` / `gradient_mp` evaluate the same definitions in mpmath at 50 digits -- the measure of
the longdouble path's own error (tests/test_reference_math.py), and the path taken where longdouble is only a double."""
import functools

import mpmath
import numpy as np

LD = np.longdouble
HAVE_LONGDOUBLE = np.finfo(LD).nmant >= 63
MP_DIGITS = 50


def _names(pdf):
    return [c.__name__ for c in type(pdf).__mro__]


def _kind(pdf):
    n = _names(pdf)
    for k in ("CoherentPointDrift", "GaussianMixtureModel", "MixtureModel", "CurvedVonMisesFisher", "Uniform", "BinghamFisher", "Bingham", "VonMisesFisher"):
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


@functools.lru_cache(maxsize=16384)
def _vmf_norm_of(mu_bytes):
    with mpmath.workdps(MP_DIGITS):
        m = [mpmath.mpf(float(v)) for v in np.frombuffer(mu_bytes, dtype=np.float64)]
        kappa = mpmath.sqrt(mpmath.fsum(v * v for v in m))
        return _ld(mpmath.log(2 * mpmath.pi) + mpmath.log(mpmath.besseli(0, kappa)))


def _vmf_norm_ld(mu):
    """|mu| in longdouble and log(2 pi) + log I0(|mu|): the Bessel function at the longdouble norm, from mpmath.  A function of
    the parameters alone, so the reference chains (layout_cases.mh_chain), which evaluate a target hundreds of times, form it
    once per mu."""
    return _vmf_norm_of(np.ascontiguousarray(mu, dtype=np.float64).tobytes())


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


_MATRICES = {}


def _matrix_ld(A):
    """A as longdouble; the conversion of the few large matrices last used is kept (a reference chain evaluates its target at
    every step), keyed by the array itself."""
    if A.size < 1 << 16:
        return A.astype(LD)
    hit = _MATRICES.get(id(A))
    if hit is None or hit[0] is not A:
        while len(_MATRICES) >= 4:
            _MATRICES.pop(next(iter(_MATRICES)))
        hit = _MATRICES[id(A)] = (A, A.astype(LD))
    return hit[1]


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
        A64 = np.asarray(pdf.A, dtype=np.float64)
        if d > 64 and np.count_nonzero(A64) == np.count_nonzero(A64.diagonal()):  # a diagonal A: the sum's zero terms left out
            Ax = A64.diagonal().astype(LD) * x
        else:
            AL = _matrix_ld(A64)                                                 # x^T A x = x . (A x), whatever A
            # (by blocks of rows that stay in cache while every point meets them: the same sums, sooner)
            Ax = np.concatenate([np.einsum("ij,nj->ni", AL[i:i + 256], x) for i in range(0, d, 256)], axis=1)
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
    if _kind(pdf) in REGISTRATION:
        res = _registration_ld(pdf, X, want_grad)
        lp, g = res["lp"], (res["gr"] if want_grad else None)
    elif _kind(pdf) != "MixtureModel":
        lp, g = _single_ld(pdf, x, want_grad)
    else:
        terms = [(p, w) for p, w in flatten(pdf) if w > 0]                      # a zero weight adds no term
        vals, grads = [], []
        if len(terms) > 64 and all(_kind(p) == "VonMisesFisher" for p, _ in terms):
            # thousands of vMF terms: the same terms, formed for all components at once (grads[k] below is then mu_k)
            mus = np.array([p.mu for p, _ in terms], dtype=np.float64).astype(LD)
            norms = np.array([_vmf_norm_ld(p.mu) for p, _ in terms], dtype=LD)
            vals = list((x @ mus.T - norms + np.log(np.array([w for _, w in terms], dtype=LD))).T)
            grads = None
        for p, w in (terms if grads is not None else []):
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
            g = np.zeros_like(x) if grads is not None else soft @ mus
            for k, gk in enumerate(grads or []):
                g += soft[:, k:k + 1] * gk
    if single:
        return lp[0], (g[0] if want_grad else None)
    return lp, g


# ------------------------------------------------------------------------------------------ registration, longdouble
REGISTRATION = ("CoherentPointDrift", "GaussianMixtureModel")
TIE_GAP = 1e-11  # the k-th and (k+1)-th squared distances must differ by more than TIE_GAP (1 + d^2[k]): 10^4 double roundings
LOG_EPS = 1e-308  # CoherentPointDrift's guard inside the outlier column's logarithm


def _reg_params(pdf, conv):
    """The objects' parameters through `conv` (array -> the arithmetic's own type)."""
    cpd = _kind(pdf) == "CoherentPointDrift"
    projected = "RotationProjection" in _names(pdf.source)
    src, tgt = np.asarray(pdf.source.positions, dtype=np.float64), np.asarray(pdf.target.positions, dtype=np.float64)
    assert src.ndim == 2 and src.shape[1] == 3 and tgt.ndim == 2 and tgt.shape[1] == (2 if projected else 3)
    k = int(pdf.k)
    assert 1 <= k <= len(src)
    return dict(cpd=cpd, dt=tgt.shape[1], k=k, src=conv(src), sw=conv(np.asarray(pdf.source.weights, dtype=np.float64)),
                tgt=conv(tgt), tw=conv(np.asarray(pdf.target.weights, dtype=np.float64)), ptp=conv(np.ptp(tgt, axis=0)),
                sigma=float(pdf.sigma), beta=float(pdf.beta), omega=float(pdf.omega) if cpd else 0.0)


def _rotation(x, y, z, w):
    """The rotation matrix of the unit quaternion (x, y, z, w), scalar last, as nested lists of whatever type the entries are."""
    return [[x * x - y * y - z * z + w * w, 2 * (x * y - z * w), 2 * (x * z + y * w)],
            [2 * (x * y + z * w), -x * x + y * y - z * z + w * w, 2 * (y * z - x * w)],
            [2 * (x * z - y * w), 2 * (y * z + x * w), -x * x - y * y + z * z + w * w]]


def _d_rotation(x, y, z, w):
    """d M / d q_c, c = x, y, z, w, of the entries M above (the same polynomial at an unnormalised quaternion)."""
    return [[[2 * x, 2 * y, 2 * z], [2 * y, -2 * x, -2 * w], [2 * z, 2 * w, -2 * x]],
            [[-2 * y, 2 * x, 2 * w], [2 * x, 2 * y, 2 * z], [-2 * w, 2 * z, -2 * y]],
            [[-2 * z, -2 * w, 2 * x], [2 * w, -2 * z, 2 * y], [2 * x, 2 * y, 2 * z]],
            [[2 * w, -2 * z, 2 * y], [2 * z, 2 * w, -2 * x], [-2 * y, 2 * x, 2 * w]]]


def _registration_ld(pdf, X, want_grad):
    """-> dict(lp (n,), lp_scale (n,), gr (n, 4), gr_scale (n, 4), gap: the smallest relative gap between the k-th and the
    (k+1)-th squared distance, term: the largest of |log w_i|, d^2 / (2 sigma^2), |log_const| that entered a term) in longdouble,
    rows X (n, 4)."""
    p = _reg_params(pdf, lambda a: a.astype(LD))
    x = np.atleast_2d(np.asarray(X, dtype=np.float64)).astype(LD)
    n, ns, nt, dt, k = len(x), len(p["src"]), len(p["tgt"]), p["dt"], p["k"]
    s2 = LD(p["sigma"]) ** 2
    with mpmath.workdps(MP_DIGITS):
        pi = _ld(+mpmath.pi)                                # (np.pi is the double: 4e-17 short of what the mpmath twin takes)
    log_const = -LD(dt) / 2 * np.log(2 * pi * s2) + (np.log(1 - LD(p["omega"])) if p["cpd"] else LD(0))
    log_out = np.log(LD(p["omega"]) + LD(LOG_EPS)) - np.sum(np.log(p["ptp"])) if p["cpd"] else None
    beta, tw, log_sw = LD(p["beta"]), p["tw"], np.log(p["sw"])
    out = dict(lp=np.empty(n, dtype=LD), lp_scale=np.empty(n, dtype=LD), gr=np.zeros((n, 4), dtype=LD),
               gr_scale=np.zeros((n, 4), dtype=LD), gap=np.inf, term=0.0)
    step = max(1, 400_000 // (ns * nt))
    for lo in range(0, n, step):
        q = x[lo:lo + step]
        u = q / np.sqrt(np.sum(q * q, axis=1))[:, None]
        R = np.array(_rotation(u[:, 0], u[:, 1], u[:, 2], u[:, 3]), dtype=LD).transpose(2, 0, 1)        # (m, 3, 3)
        moved = np.einsum("mji,si->msj", R[:, :dt, :], p["src"])                                        # T x_i: (m, ns, dt)
        diff = p["tgt"][None, :, None, :] - moved[:, None, :, :]                                        # (m, nt, ns, dt)
        d2 = np.sum(diff * diff, axis=-1)
        order = np.argsort(d2, axis=-1, kind="stable")                                                  # the full sort
        d2s = np.take_along_axis(d2, order, axis=-1)
        if k < ns:
            gaps = (d2s[..., k] - d2s[..., k - 1]) / (1 + d2s[..., k])
            out["gap"] = min(out["gap"], float(gaps.min()))
            assert gaps.min() > TIE_GAP, f"near-tie of the k-th neighbour: relative gap {float(gaps.min()):.2e}"
        near = order[..., :k]                                                                           # (m, nt, k)
        terms = log_sw[near] - d2s[..., :k] / (2 * s2) + log_const
        every = np.concatenate([terms, np.full(terms.shape[:2] + (1,), log_out, dtype=LD)], axis=-1) if p["cpd"] else terms
        out["term"] = max(out["term"], float(np.abs(log_sw[near]).max()), float(d2s[..., :k].max() / (2 * s2)), float(abs(log_const)))
        top = every.max(axis=-1)
        lse = top + np.log(np.sum(np.exp(every - top[..., None]), axis=-1))                             # (m, nt)
        out["lp"][lo:lo + step] = beta * np.sum(tw * lse, axis=-1)
        out["lp_scale"][lo:lo + step] = beta * np.sum(tw * np.abs(lse), axis=-1)
        if not want_grad:
            continue
        gamma = np.exp(np.clip(terms - lse[..., None], LD(-20), LD(0)))
        coeff = tw[None, :, None] * gamma / s2                                                          # (m, nt, k)
        resid = np.zeros(near.shape + (3,), dtype=LD)                                                   # y_l - T x_i, padded
        resid[..., :dt] = np.take_along_axis(diff, near[..., None], axis=2)
        xs = p["src"][near]                                                                             # (m, nt, k, 3)
        each = coeff[..., None, None] * resid[..., :, None] * xs[..., None, :]                          # (m, nt, k, j, i)
        G, A = each.sum(axis=(1, 2)), np.abs(each).sum(axis=(1, 2))                                     # (m, 3, 3)
        r = np.sum(q * q, axis=1) + LD(1e-300)
        M = np.array(_rotation(q[:, 0], q[:, 1], q[:, 2], q[:, 3]), dtype=LD).transpose(2, 0, 1)
        dM = np.array(_d_rotation(q[:, 0], q[:, 1], q[:, 2], q[:, 3]), dtype=LD).transpose(3, 0, 1, 2)  # (m, c, 3, 3)
        first = dM / r[:, None, None, None]
        second = -2 * q[:, :, None, None] * M[:, None, :, :] / (r * r)[:, None, None, None]
        out["gr"][lo:lo + step] = beta * np.sum((first + second) * G[:, None], axis=(2, 3))
        out["gr_scale"][lo:lo + step] = beta * np.sum((np.abs(first) + np.abs(second)) * A[:, None], axis=(2, 3))
    return out


def registration(pdf, X, want_grad=True):
    """log_prob and gradient of a registration target at rows X (n, 4) with their scales, in longdouble: dict(lp, lp_scale =
    beta sum_l tw_l |lse_l|, gr, gr_scale = per component the sum of the absolute values of every accumulated term -- near a good
    pose the gradient is a cancelling sum --, gap, term).  Asserts of every (row, target point) that the k-th neighbour is no
    near-tie."""
    if HAVE_LONGDOUBLE:
        return _registration_ld(pdf, X, want_grad)
    lp, gr, lp_scale, gr_scale = _registration_mp(pdf, np.atleast_2d(np.asarray(X, dtype=np.float64)))
    return dict(lp=_mp_to_ld(lp), lp_scale=_mp_to_ld(lp_scale), gr=_mp_to_ld(gr), gr_scale=_mp_to_ld(gr_scale), gap=np.nan, term=np.nan)


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


def _registration_point_mp(p, q):
    """(log_prob, gradient, log_prob's scale, gradient's scales) of a registration target with parameters p (lists of mpf) at
    one quaternion q (list of mpf): the definition of the module docstring, term by term."""
    mpf = mpmath.mpf
    dt, k, s2 = p["dt"], p["k"], mpf(p["sigma"]) ** 2
    nq = mpmath.sqrt(_dot_mp(q, q))
    R = _rotation(*[v / nq for v in q])
    log_const = -mpf(dt) / 2 * mpmath.log(2 * mpmath.pi * s2) + (mpmath.log(1 - mpf(p["omega"])) if p["cpd"] else 0)
    log_out = mpmath.log(mpf(p["omega"]) + mpf(LOG_EPS)) - mpmath.fsum(mpmath.log(v) for v in p["ptp"]) if p["cpd"] else None
    moved = [[_dot_mp(R[j], xi) for j in range(dt)] for xi in p["src"]]
    lp, lp_scale = mpf(0), mpf(0)
    G = [[mpf(0)] * 3 for _ in range(3)]
    A = [[mpf(0)] * 3 for _ in range(3)]
    for y, twl in zip(p["tgt"], p["tw"]):
        diff = [[y[j] - m[j] for j in range(dt)] for m in moved]
        d2 = [_dot_mp(v, v) for v in diff]
        order = sorted(range(len(d2)), key=lambda i: d2[i])
        if k < len(order):
            gap = (d2[order[k]] - d2[order[k - 1]]) / (1 + d2[order[k]])
            assert gap > TIE_GAP, f"near-tie of the k-th neighbour: relative gap {float(gap):.2e}"
        near = order[:k]
        terms = [mpmath.log(p["sw"][i]) - d2[i] / (2 * s2) + log_const for i in near]
        every = terms + ([log_out] if p["cpd"] else [])
        top = max(every)
        lse = top + mpmath.log(mpmath.fsum(mpmath.exp(v - top) for v in every))
        lp += twl * lse
        lp_scale += twl * abs(lse)
        for i, t in zip(near, terms):
            coeff = twl * mpmath.exp(_clip_mp(t - lse, mpf(-20), mpf(0))) / s2
            resid = diff[i] + [mpf(0)] * (3 - dt)
            for a in range(3):
                for b in range(3):
                    G[a][b] += coeff * resid[a] * p["src"][i][b]
                    A[a][b] += abs(coeff * resid[a] * p["src"][i][b])
    r = _dot_mp(q, q) + mpf(1e-300)
    M, dM = _rotation(*q), _d_rotation(*q)
    beta = mpf(p["beta"])
    gr, gr_scale = [], []
    for c in range(4):
        J = [[dM[c][a][b] / r - 2 * q[c] * M[a][b] / (r * r) for b in range(3)] for a in range(3)]
        Jabs = [[abs(dM[c][a][b] / r) + abs(2 * q[c] * M[a][b] / (r * r)) for b in range(3)] for a in range(3)]
        gr.append(beta * mpmath.fsum(J[a][b] * G[a][b] for a in range(3) for b in range(3)))
        gr_scale.append(beta * mpmath.fsum(Jabs[a][b] * A[a][b] for a in range(3) for b in range(3)))
    return beta * lp, gr, beta * lp_scale, gr_scale


def _registration_mp(pdf, X):
    """(lp (n,), gr (n, 4), lp_scale (n,), gr_scale (n, 4)) as object arrays of mpf."""
    with mpmath.workdps(MP_DIGITS):
        p = _reg_params(pdf, lambda a: [_mpv(r) for r in a] if a.ndim == 2 else _mpv(a))
        res = [_registration_point_mp(p, _mpv(r)) for r in X]
    return tuple(np.array([r[i] for r in res], dtype=object) for i in range(4))


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
    if _kind(pdf) in REGISTRATION:
        p = _reg_params(pdf, lambda a: [_mpv(r) for r in a] if a.ndim == 2 else _mpv(a))
        return _registration_point_mp(p, x)[:2]
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

"""C++ sources of DeviceDistribution targets used by the tests: restatements of built-in targets (so that their chains can be
held to the reference's recorded ones) and the angular central Gaussian, which the library lacks.  Plain C++, evaluated op by op
as the built-in policies of geosss_amd/csrc/gsss_device.h evaluate theirs."""
import math

import numpy as np

# README mixture of vMF terms: p = [K, mu (K x d, kappa * direction), logc (K: log w - log 2 pi - log i0(kappa))]
VMF_MIXTURE = r"""
__device__ double gsss_user_log_prob(const double *x, int d, const double *p) {
    const int K = (int)p[0];
    const double *mu = p + 1, *lc = p + 1 + K * d;
    double amax = -INFINITY;
    for (int k = 0; k < K; ++k) {
        double s = 0.0;
        for (int i = 0; i < d; ++i) s = fma(x[i], mu[k * d + i], s);
        amax = fmax(amax, s + lc[k]);
    }
    if (!(amax > -INFINITY) || amax == INFINITY) return amax;
    double t = 0.0;
    for (int k = 0; k < K; ++k) {
        double s = 0.0;
        for (int i = 0; i < d; ++i) s = fma(x[i], mu[k * d + i], s);
        t += exp(s + lc[k] - amax);
    }
    return amax + log(t);
}
"""

# Bingham: log_prob = x^T A x, gradient 2 A x; p = A (d x d, symmetric, row-major)
BINGHAM = r"""
__device__ double gsss_user_log_prob(const double *x, int d, const double *p) {
    double s = 0.0;
    for (int j = 0; j < d; ++j) {
        double xa = 0.0;
        for (int i = 0; i < d; ++i) xa = fma(x[i], p[i * d + j], xa);
        s = fma(xa, x[j], s);
    }
    return s;
}
__device__ void gsss_user_gradient(const double *x, int d, const double *p, double *g) {
    for (int j = 0; j < d; ++j) {
        double xa = 0.0;
        for (int i = 0; i < d; ++i) xa = fma(p[j * d + i], x[i], xa);
        g[j] = 2.0 * xa;
    }
}
"""

# curve-vMF: kappa * (x . nearest point of the slerp curve); p = [K, kappa, knots (K x d), per segment theta, cos, sin, sin + 1e-10]
CURVE_VMF = r"""
__device__ double gsss_user_log_prob(const double *x, int d, const double *p) {
    const int K = (int)p[0];
    const double kappa = p[1];
    const double *kn = p + 2, *seg = p + 2 + K * d;
    double best = INFINITY, best_dot = 0.0;
    double ay = 0.0;
    for (int i = 0; i < d; ++i) ay = fma(kn[i], x[i], ay);
    for (int s = 0; s + 1 < K; ++s) {
        const double *a = kn + s * d, *b = a + d;
        double by = 0.0;
        for (int i = 0; i < d; ++i) by = fma(b[i], x[i], by);
        const double theta = seg[4 * s], ct = seg[4 * s + 1], st = seg[4 * s + 2], den = seg[4 * s + 3];
        double t = atan2(by - ay * ct, ay * st);
        t = fmin(fmax(t, 0.0), theta);
        const double sa = sin(theta - t), sb = sin(t);
        double xy = 0.0;
        for (int i = 0; i < d; ++i) xy = fma(x[i], (sa * a[i] + sb * b[i]) / den, xy);
        const double dist = acos(fmin(fmax(xy, -1.0), 1.0));
        if (dist < best) {
            best = dist;
            best_dot = xy;
        }
        ay = by;
    }
    return kappa * best_dot;
}
"""

# angular central Gaussian: -(d / 2) log(x^T C^-1 x), gradient -d C^-1 x / (x^T C^-1 x); p = C^-1 (row-major)
ACG = r"""
__device__ double gsss_user_log_prob(const double *x, int d, const double *p) {
    double q = 0.0;
    for (int i = 0; i < d; ++i) {
        double r = 0.0;
        for (int j = 0; j < d; ++j) r = fma(p[i * d + j], x[j], r);
        q = fma(x[i], r, q);
    }
    return -0.5 * d * log(q);
}
__device__ void gsss_user_gradient(const double *x, int d, const double *p, double *g) {
    double q = 0.0;
    for (int i = 0; i < d; ++i) {
        double r = 0.0;
        for (int j = 0; j < d; ++j) r = fma(p[i * d + j], x[j], r);
        g[i] = r;
        q = fma(x[i], r, q);
    }
    for (int i = 0; i < d; ++i) g[i] = -d * g[i] / q;
}
"""

# the ACG without its gradient
ACG_NO_GRADIENT = ACG[: ACG.index("__device__ void")]


def vmf_mixture_params(mu, weights):
    from geosss_amd.distributions import log_bessel_i0
    mu = np.asarray(mu, dtype=np.float64)
    w = np.asarray(weights, dtype=np.float64)
    w = w / w.sum()
    kappa = np.linalg.norm(mu, axis=1)
    logc = np.log(w) - np.log(2 * np.pi) - log_bessel_i0(kappa)
    return np.concatenate([[len(mu)], mu.ravel(), logc])


def curve_params(knots, kappa):
    """The x-independent segment quantities the library packs for its curve target (std::acos / cos / sin: Python's math)."""
    knots = np.asarray(knots, dtype=np.float64)
    seg = []
    for a, b in zip(knots[:-1], knots[1:]):
        ab = min(max(float(sum(float(u) * float(v) for u, v in zip(a, b))), -1.0), 1.0)
        th = math.acos(ab)
        seg += [th, math.cos(th), math.sin(th), math.sin(th) + 1e-10]
    return np.concatenate([[len(knots), float(kappa)], knots.ravel(), seg])


def user_target(gs, z, cache_dir):
    """The DeviceDistribution restating the target of golden fixture z (vMF mixture, Bingham or curve-vMF)."""
    kind = str(z["target_kind"])
    d = int(z["x0"].shape[0])
    if kind == "vmf_mixture":
        return gs.DeviceDistribution(d, VMF_MIXTURE, vmf_mixture_params(z["target_mu"], z["target_weights"]), cache_dir=cache_dir)
    if kind == "bingham":
        return gs.DeviceDistribution(d, BINGHAM, z["target_A"], cache_dir=cache_dir)
    if kind == "curve_vmf":
        return gs.DeviceDistribution(d, CURVE_VMF, curve_params(z["target_knots"], z["target_kappa"]), cache_dir=cache_dir)
    raise ValueError(kind)

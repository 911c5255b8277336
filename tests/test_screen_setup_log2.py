"""The single-precision pack of the vMF-mixture screen (ScreenVmf, geosss_amd/csrc/gsss_screen.h) formed from rows staged in
log2 units (setup32_log2) against the one formed by multiplying every coefficient by log2 e (make32).  Everything is restated
here in IEEE float64 / float32 (fused multiply-adds exactly, through rationals); nothing runs on a device.

* q_new and q_old are neighbouring floats at most.  Both are roundings of double-precision values that differ by the few
  double-precision roundings of their sums: (2 D + 2) 2^-53 sum_j |mu_kj x_j| L for the dot products.  Two such values round to
  the same or to adjacent floats while that distance is below a float ulp of the value, i.e. while the sum has not cancelled
  more than 26 of its bits; an entry that HAS (x perpendicular to a mean to 1e-8) is held to that absolute distance instead --
  it is what the margin's derivation takes as exact, 2^-29 of the 2^-24 it counts per coefficient.  Every random case, and
  nearly every entry of the adversarial ones, is held to the one-ulp bound.
* b is max_k (|q_k| + |q_K+k| + |q_2K+k|) + |t2| over the real components, bit for bit the maximum of the sums with |t2| in, and
  the margin formed from it is finite only below 0.25 and then at least the 1e-7 + 1.25 (v_exp_f32 + K roundings) of its formula.
  (An affine upper bound of the margin in b was built, measured and taken out -- DESIGN.md section 11 -- and is not tested.)
* No certain verdict is wrong: tries evaluated as the kernel evaluates them, with correctly rounded single-precision functions
  in place of the hardware's (their errors are inside the constants), against the level and threshold in extended precision.
"""
import os
import re
from fractions import Fraction

import numpy as np

F32, F64 = np.float32, np.float64
L = 1.4426950408889634074
K_LOG_ZERO = -1.0e5
README_MUS = 80.0 * np.array([[0.87, -0.37, 0.33], [-0.20, -0.89, -0.40], [0.19, 0.22, -0.96]])


def _consts():
    path = os.path.join(os.path.dirname(__file__), "..", "geosss_amd", "csrc", "gsss_screen_consts.h")
    txt = open(path).read()
    return {n: float(F32(float(v))) for n, v in re.findall(r"constexpr float (k\w+) = ([0-9.eE+-]+)f;", txt)}


C = _consts()
SINCOS, UNIT, EXP2, LOG2 = (F32(C[k]) for k in ("kSinCosErr32", "kUnit32", "kExp2Err32", "kLog2Err32"))


def fma(a, b, c):
    """the correctly rounded a b + c of finite doubles"""
    return float(Fraction(float(a)) * Fraction(float(b)) + Fraction(float(c)))


def dot_fma(row, v):
    acc = 0.0
    for m, x in zip(row, v):
        acc = fma(m, x, acc)
    return acc


def stage(mus, logc, kc):
    """FastVmf::stage: zero rows and kLogZero beyond K, -inf clamped"""
    k, d = mus.shape
    mu = np.zeros((kc, d))
    mu[:k] = mus
    lc = np.full(kc, K_LOG_ZERO)
    lc[:k] = np.maximum(logc, K_LOG_ZERO)
    return mu, lc


def pack_old(mu, lc, x, u):
    ax = np.array([dot_fma(r, x) for r in mu])
    au = np.array([dot_fma(r, u) for r in mu])
    m = np.max(ax + lc)
    return np.concatenate([F32(ax * L), F32(au * L), F32((lc - m) * L)]), (ax, au, m)


def pack_new(mu, lc, x, u):
    mul, lcl = mu * L, lc * L  # the scaled copy, formed once
    ax = np.array([dot_fma(r, x) for r in mul])
    au = np.array([dot_fma(r, u) for r in mul])
    m = np.max(ax + lcl)
    return np.concatenate([F32(ax), F32(au), F32(lcl - m)])


def ordered(f):
    """float32 -> integers in the order of the floats (neighbouring floats differ by one)"""
    i = np.asarray(f, F32).view(np.int32).astype(np.int64)
    return np.where(i < 0, -(i & 0x7FFFFFFF), i)


def log2_32(v):
    m, e = np.frexp(F64(v))
    return F32(F32(e) + F32(np.log2(F64(F32(m)))))


def margin_old(b, kc):
    """the margin of finish32, operation for operation in float32"""
    b = np.asarray(b, F32)
    kcf = F32(kc)
    c1 = F32(SINCOS + F32(F32(7.0) * UNIT))
    e3 = F32(EXP2 + F32(kcf * UNIT))
    c2 = F32(F32(F32(F32(1.4427) * e3) + F32(6.0e-8)) + LOG2)
    e_a = F32(F32(b * c1) + c2)
    t = F32(F32(F32(0.69315) * e_a) * F32(F32(1.0) + e_a))
    return F32(F32(F32(1.25) * F32(F32(t + EXP2) + F32(kcf * UNIT))) + F32(1.0e-7))


def finish(q, k, kc, u_thr):
    """finish32: s0, t2, the shifted third block, b and the margin; returns the finished pack, b, t2"""
    q = q.copy()
    s0 = None
    for i in range(kc):
        t = F32(np.exp2(F64(F32(q[i] + q[2 * kc + i]))))
        s0 = t if s0 is None else F32(s0 + t)
    m0, e = np.frexp(s0)
    t2 = F32(F32(F32(e) + F32(np.log2(F64(m0)))) + log2_32(u_thr))
    b = F32(0.0)
    sums_with_t2 = []
    for i in range(kc):
        q[2 * kc + i] = F32(q[2 * kc + i] - t2)
        if i < k:
            s = F32(F32(abs(q[i]) + abs(q[kc + i])) + abs(q[2 * kc + i]))
            b = max(b, s)
            sums_with_t2.append(F32(s + abs(t2)))
    b = F32(b + abs(t2))
    assert b == max(sums_with_t2)  # "= max_k (... + |t2|) bit for bit"
    margin = margin_old(b, kc)
    if not (u_thr > 1e-290) or not (margin < F32(0.25)):
        margin = F32(np.inf)
    return q, b, t2, margin


def tangent(rng, x):
    v = rng.standard_normal(x.shape)
    v -= np.dot(v, x) * x
    return v / np.linalg.norm(v)


def vmf_logc(kappa, w):
    with np.errstate(divide="ignore"):
        return np.log(w) + np.log(kappa) - np.log(2.0 * np.pi) - kappa - np.log1p(-np.exp(-2.0 * kappa))


def _targets():
    rng = np.random.default_rng(3)
    def unit(n, d):
        v = rng.standard_normal((n, d))
        return v / np.linalg.norm(v, axis=1, keepdims=True)
    yield "readme", README_MUS, vmf_logc(np.full(3, 80.0), np.full(3, 1 / 3)), 3
    yield "k1_in_3", 80.0 * unit(1, 3), vmf_logc(np.full(1, 80.0), np.ones(1)), 3
    yield "k2_in_3", 40.0 * unit(2, 3), vmf_logc(np.full(2, 40.0), np.array([0.3, 0.7])), 3
    yield "zero_weight", README_MUS, vmf_logc(np.full(3, 80.0), np.array([0.5, 0.0, 0.5])), 3
    yield "k5_in_6", 60.0 * unit(5, 3), vmf_logc(np.full(5, 60.0), np.full(5, 0.2)), 6
    yield "kappa500", 500.0 * unit(3, 3), vmf_logc(np.full(3, 500.0), np.full(3, 1 / 3)), 3
    yield "flat", 1.0e-3 * unit(3, 3), vmf_logc(np.full(3, 1.0e-3), np.full(3, 1 / 3)), 3


def _states(rng, mus, n_random):
    """(x, u, kind): random points with random tangents; then the adversarial ones -- at and opposite every mean, the tangent
    towards another mean; next to the poles (tangent3's branch); on the axes; and exactly perpendicular to a mean (the dot
    product cancels completely)"""
    d = mus.shape[1]
    for _ in range(n_random):
        x = rng.standard_normal(d)
        x /= np.linalg.norm(x)
        yield x, tangent(rng, x), "random"
    units = mus / np.linalg.norm(mus, axis=1, keepdims=True)
    for i, m in enumerate(units):
        for sgn in (1.0, -1.0):
            x = sgn * m
            o = units[(i + 1) % len(units)] if len(units) > 1 else np.roll(m, 1)
            u = o - np.dot(o, x) * x
            if np.linalg.norm(u) < 1e-8:
                u = tangent(rng, x)
            yield x, u / np.linalg.norm(u), "adversarial"
        p = np.cross(m, np.array([0.3, -0.5, 0.8]))
        p /= np.linalg.norm(p)
        yield p, tangent(rng, p), "perpendicular"  # mu . x cancels completely
    for eps in (1e-3, 1e-8, 1e-15):
        for pole in (1.0, -1.0):
            x = np.array([eps, -eps, pole])
            x /= np.linalg.norm(x)
            yield x, tangent(rng, x), "adversarial"
    for j in range(d):
        x = np.zeros(d)
        x[j] = 1.0
        yield x, tangent(rng, x), "adversarial"


def _cases():
    rng = np.random.default_rng(5)
    for name, mus, logc, kc in _targets():
        mu, lc = stage(mus, logc, kc)
        for x, u, kind in _states(rng, mus, 1200 if name == "readme" else 400):
            yield name, mus.shape[0], kc, mu, lc, x, u, kind


CASES = list(_cases())


def test_new_pack_is_the_old_one_to_a_float():
    n_strict = n_abs = 0
    for name, k, kc, mu, lc, x, u, kind in CASES:
        d = len(x)
        qo, (ax, au, m) = pack_old(mu, lc, x, u)
        qn = pack_new(mu, lc, x, u)
        assert np.all(np.isfinite(qn)) and np.all(np.isfinite(qo))
        sx, su = np.abs(mu) @ np.abs(x), np.abs(mu) @ np.abs(u)
        # distance of the two double-precision values an entry is rounded from (module docstring)
        dist = np.concatenate([(2 * d + 2) * sx, (2 * d + 2) * su,
                               (2 * d + 2) * sx.max() + 6.0 * (np.abs(lc) + abs(m) + np.abs(lc).max())]) * L * 2.0 ** -53
        val = np.maximum(np.abs(qo), np.abs(qn)).astype(F64)
        well = dist <= val * 2.0 ** -24
        ulps = np.abs(ordered(qn) - ordered(qo))
        assert np.all(ulps[well] <= 1), (name, x, u, qo, qn)
        assert np.all(np.abs(qn.astype(F64) - qo.astype(F64))[~well] <= dist[~well] + 2.0 ** -23 * val[~well]), (name, x, u, qo, qn)
        assert kind != "random" or well.all(), (name, x, u)  # every random case is held to the strict bound
        n_strict += int(well.sum())
        n_abs += int((~well).sum())
    assert n_strict > 20 * max(n_abs, 1)  # the strict bound is what nearly every entry is held to
    assert n_abs > 0                      # ... and the cancelled ones are among the cases


def test_padding_and_zero_weight_rows_of_the_scaled_copy():
    mu, lc = stage(README_MUS[:2], vmf_logc(np.full(2, 80.0), np.array([1.0, 0.0])), 3)
    assert lc[1] == K_LOG_ZERO and lc[2] == K_LOG_ZERO and not mu[2].any()
    x = np.array([0.6, 0.0, 0.8])
    qn = pack_new(mu, lc, x, np.array([0.8, 0.0, -0.6]))
    assert qn[2] == 0.0 and qn[5] == 0.0                    # a padded row: +0 coefficients
    assert qn[7] < -1.0e5 and qn[8] < -1.0e5                # exponent -1e5 L and below: 2^q is +0 in every sum
    assert F32(np.exp2(F64(qn[7]))) == 0.0


def _try_sum(q, kc, theta):
    t = F32(theta * 0.15915494309189535)
    s, c = F32(np.sin(2.0 * np.pi * F64(t))), F32(np.cos(2.0 * np.pi * F64(t)))
    total = None
    for i in range(kc):
        e = F32(F64(c) * F64(q[i]) + F64(F32(F64(s) * F64(q[kc + i]) + F64(q[2 * kc + i]))))
        with np.errstate(over="ignore"):
            v = F32(np.exp2(F64(e)))  # (a try far above the threshold may overflow to +inf: certainly accepted)
        total = v if total is None else F32(total + v)
    return total


def test_b_margin_and_certain_verdicts():
    rng = np.random.default_rng(9)
    LD = np.longdouble
    certain_new = certain_old = tries = 0
    for idx, (name, k, kc, mu, lc, x, u, kind) in enumerate(CASES):
        if idx % 3:
            continue
        u_thr = float(rng.uniform()) if idx % 7 else float(rng.uniform() * 1e-6)
        qn, b, t2, margin = finish(pack_new(mu, lc, x, u), k, kc, u_thr)
        qo, bo, _, margin_o = finish(pack_old(mu, lc, x, u)[0], k, kc, u_thr)
        assert margin < F32(0.25) or margin == np.inf
        assert margin >= F32(1.0e-7) + F32(1.25) * (EXP2 + F32(kc) * UNIT) * F32(0.999)
        # b moves with q by a few float ulps of its terms at the most, and the margin with it
        assert abs(float(b) - float(bo)) <= 8.0 * 2.0 ** -23 * float(bo)
        assert margin == margin_o or abs(float(margin) - float(margin_o)) <= 1.0e-5 * float(margin_o)
        ax, au = LD(mu) @ LD(x), LD(mu) @ LD(u)
        m = np.max(ax + LD(lc))
        thr = np.sum(np.exp(ax + LD(lc) - m)) * LD(u_thr)
        for theta in rng.uniform(-2.0 * np.pi, 2.0 * np.pi, 12):
            level = np.sum(np.exp(LD(np.cos(LD(theta))) * ax + LD(np.sin(LD(theta))) * au + LD(lc) - m))
            tries += 1
            for q, mg, which in ((qn, margin, "new"), (qo, margin_o, "old")):
                dev = F32(_try_sum(q, kc, theta) - F32(1.0))
                if dev < -mg:
                    assert level < thr, (name, which, theta)
                elif dev > mg:
                    assert level > thr, (name, which, theta)
                else:
                    continue
                if which == "new":
                    certain_new += 1
                else:
                    certain_old += 1
    assert tries > 5000
    assert certain_new > 0.9 * tries          # the screen still decides nearly every try
    assert abs(certain_new - certain_old) <= 0.001 * tries  # ... as the old pack does: the verdicts move only next to the margin

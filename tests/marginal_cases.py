"""The cases that hold gsss_target_marginals to a host reference, shared by the host tests (which assert the cases' conditions
on the CPU) and the device tests (which compare counts, exactly).  No device is touched here.

Inputs: seeded random walks on the sphere from numpy (not from the sampler), steps uniform in 0.05 .. pi - 0.05 so that acos is
evaluated away from its ends, every target with its own seeded directions.

The reference.  For coordinate-axis directions (directions=None) no margin is needed: u = x . e_j is x_j bit for bit, because
fma(x_i, 0, acc) = acc, so the host bin is floor((x_j + 1.0) * (0.5 * B)) in double arithmetic, clamped to 0 .. B - 1.  For
general directions u is taken in longdouble, and theta by longdouble arccos of the longdouble product; a value is "on an edge"
if its t lies within EDGE = 1e-9 of an integer.  The seeds are chosen so that NO value of any case is on an edge
(`Reference.on_edge == 0`, asserted by the host tests for every case): the counts are then the same in double and in longdouble
provided the device's t lies within 1e-9 of the exact one, which `Reference.t_error` bounds from the number formats:

    u      a chain of d fused multiply-adds errs by at most (d + 1) 2^-52 sum_j |x_j v_j| <= (d + 1) 2^-52 |v| for a unit x (|v|
           the Euclidean norm); t = (u + 1) B / 2 adds two roundings of a number below B:
           |dt| <= (B / 2) (d + 1) 2^-52 max(|v|, 1) + 2 B 2^-52;
    theta  the product errs by delta = (d + 1) 2^-52, acos has the slope 1 / sin(theta): |dtheta| <= delta / sin_min + 4 2^-52 pi
           (four ulp of pi allowed to the device's acos, the assumption of tests/test_hip_target_mixing.py), sin_min the smallest
           sin(theta) of the case's pairs; |dt| <= (B / pi) |dtheta| + 2 B 2^-52."""
import functools

import numpy as np

LD = np.longdouble
EPS = 2.0 ** -52
EDGE = 1e-9

# name: (M, m, rows, d, directions, P, bins, steps, n_hist, specials)
#   directions  "axes": None, the d coordinate axes | "own": (M, P, d), every target its own, with -e_0, a direction of norm 0.5
#               and one of norm 2 (the clamp at both ends) among them | "shared": (P, d), broadcast
#   specials    draws placed at x_j = +-1 and x_j = 0 exactly (last bin, first bin, the middle edge)
CASES = {
    # every lane another target | two chunks of 36 and 4 targets, targets inside a wavefront | the LDS cap cuts the chunk to one
    # target of one lane
    "d2_m1_axes":          (40, 1, 5, 2, "axes", 2, 64, True, 1, True),
    "d3_m7_own":           (40, 7, 5, 3, "own", 3, 64, True, 0, False),
    "d5_m1_lds_cap":       (40, 1, 1, 5, "axes", 5, 1024, False, 0, True),
    # S B = 8192: 32 KiB of counters and the staged directions, wave-aligned targets, one per workgroup
    "d16_m64_full_lds":    (3, 64, 5, 16, "own", 7, 1024, True, 1, False),
    # a target spans two workgroups, the second ragged; 70 rows over 6 chunks: the rows are split, pairs cross the split
    "d16_m259_split":      (3, 259, 70, 16, "axes", 16, 64, True, 1, True),
    "d3_m256_split":       (3, 256, 70, 3, "own", 3, 64, True, 0, False),
    # the build with a run-time d
    "d17_m600_own":        (3, 600, 70, 17, "own", 5, 64, True, 1, False),
    "d17_m7_axes_b2":      (5, 7, 5, 17, "axes", 17, 2, False, 0, True),
    "d600_m7_global":      (3, 7, 5, 600, "own", 8, 256, True, 1, False),   # 38 KB of directions and 9 KB of counters: global reads
    # one row behind its history row: one pair per chain; two bins
    "d3_m256_one_row":     (4, 256, 1, 3, "shared", 2, 2, True, 1, False),
    "d2_m64_axes":         (3, 64, 5, 2, "axes", 2, 64, True, 0, True),
    "d5_m40_b100":         (6, 40, 5, 5, "own", 5, 100, False, 0, False),
    "d3_m7_steps_alone":   (3, 7, 5, 3, "shared", 0, 64, True, 1, False),
}


def _seed(name):
    return sum((i + 1) * ord(c) for i, c in enumerate(name))


def walk(rows, d, n, seed):
    """(rows, d, n): random walks on the sphere, steps uniform in 0.05 .. pi - 0.05."""
    g = np.random.default_rng(seed)
    x = np.empty((rows, n, d))
    x[0] = g.standard_normal((n, d))
    x[0] /= np.linalg.norm(x[0], axis=1, keepdims=True)
    for r in range(1, rows):
        t = g.standard_normal((n, d))
        t -= (t * x[r - 1]).sum(1, keepdims=True) * x[r - 1]
        t /= np.linalg.norm(t, axis=1, keepdims=True)
        th = g.uniform(0.05, np.pi - 0.05, (n, 1))
        x[r] = np.cos(th) * x[r - 1] + np.sin(th) * t
        x[r] /= np.linalg.norm(x[r], axis=1, keepdims=True)
    return np.ascontiguousarray(x.transpose(0, 2, 1))


def place_specials(x):
    """Draws at +-e_0, +-e_{d-1} and with x_0 = 0, x_{d-1} = 0 exactly, in different chains where there are enough."""
    R, d, n = x.shape
    g = np.random.default_rng(R + d + n)
    for s, (j, v) in enumerate([(0, 1.0), (0, -1.0), (d - 1, 1.0), (d - 1, -1.0), (0, 0.0), (d - 1, 0.0)]):
        r, c = (3 * s) % R, (5 * s + 1) % n
        if v:
            x[r, :, c] = 0.0
            x[r, j, c] = v
        else:
            y = g.standard_normal(d)
            y[j] = 0.0
            x[r, :, c] = y / np.linalg.norm(y)
            assert x[r, j, c] == 0.0
    return x


def own_directions(M, P, d, seed):
    """(M, P, d): seeded unit directions, every target its own; target 0 has -e_0 first, target 1 (and 0 where M = 1) a direction
    of norm 0.5 and target M - 1 one of norm 2 last."""
    g = np.random.default_rng(seed)
    v = g.standard_normal((M, P, d))
    v /= np.linalg.norm(v, axis=-1, keepdims=True)
    if P:
        v[0, 0] = 0.0
        v[0, 0, 0] = -1.0
        v[min(1, M - 1), P - 1] *= 0.5
        v[M - 1, P // 2] *= 2.0
    return v


def inputs(name):
    """(x (rows, d, n), hist (n_hist, d, n), directions: None | (P, d) | (M, P, d)) of a case: the walk's first row is the history."""
    M, m, rows, d, kind, P, bins, steps, n_hist, specials = CASES[name]
    seed = _seed(name)
    full = walk(rows + n_hist, d, M * m, seed)
    hist, x = full[:n_hist].copy(), full[n_hist:].copy()
    if specials:
        place_specials(x)
    if kind == "axes":
        assert P == d
        dirs = None
    elif kind == "own":
        dirs = own_directions(M, P, d, seed + 1)
    else:
        dirs = own_directions(1, P, d, seed + 1)[0] if P else np.zeros((0, d))
    return x, hist, dirs


def axis_bins(v, bins):
    """The bin of u = x_j by the device's own double arithmetic; -1 for NaN."""
    t = (v + 1.0) * (0.5 * bins)
    with np.errstate(invalid="ignore"):
        b = np.where(t < 0, 0.0, np.minimum(bins - 1.0, np.floor(t)))
    return np.where(np.isnan(t), -1, b).astype(np.int64)


class Reference:
    """counts (M, S, B) int64 of the draws x (R, d, n) behind hist (h <= 1, d, n), target t owning the chains [t m, (t + 1) m),
    against directions None | (P, d) | (M, P, d); on_edge: how many values lie within EDGE of a bin edge (axis directions: not
    counted, they are exact); t_error: the bound of the module's docstring on the device's error in t."""

    def __init__(self, x, hist, m, dirs, bins, steps):
        R, d, n = x.shape
        M = n // m
        target = np.arange(n) // m
        self.on_edge, self.t_error = 0, 0.0
        if dirs is None:
            P = d
            b = axis_bins(x.transpose(0, 2, 1), bins)                                   # (R, n, P)
        else:
            dirs = np.broadcast_to(dirs, (M,) + dirs.shape[-2:]) if np.ndim(dirs) == 2 else dirs
            P = dirs.shape[1]
            vl = np.repeat(dirs.astype(LD), m, axis=0)                                  # (n, P, d)
            u = np.einsum("rdn,npd->rnp", x.astype(LD), vl)
            t = (u + 1) * (LD(bins) / 2)
            b = self._bins(t, bins)
            if P:
                self.t_error = bins / 2 * (d + 1) * EPS * max(1.0, float(np.linalg.norm(dirs, axis=-1).max())) + 2 * bins * EPS
        S = P + (1 if steps else 0)
        self.counts = np.zeros((M, S, bins), dtype=np.int64)
        tt, pp = np.broadcast_to(target[None, :, None], b.shape), np.broadcast_to(np.arange(P)[None, None, :], b.shape)
        ok = b >= 0
        np.add.at(self.counts, (tt[ok], pp[ok], b[ok]), 1)
        self.pairs = 0
        if steps:
            xl = np.concatenate([hist, x]).astype(LD)
            dot = (xl[1:] * xl[:-1]).sum(1)                                             # (pairs per chain, n)
            theta = np.arccos(np.clip(dot, LD(-1), LD(1)))
            b = self._bins(theta * LD(bins / np.pi), bins)
            ok = b >= 0
            np.add.at(self.counts, (np.broadcast_to(target[None, :], b.shape)[ok], P, b[ok]), 1)
            self.pairs = int(ok.sum())
            if ok.any():
                sin_min = float(np.sqrt(np.maximum(1 - dot[ok] * dot[ok], 0)).min())
                err = (d + 1) * EPS / max(sin_min, 1e-300) + 4 * EPS * np.pi
                self.t_error = max(self.t_error, bins / np.pi * err + 2 * bins * EPS)

    def _bins(self, t, bins):
        """Bins of longdouble t, -1 for NaN; counts the values on an edge."""
        nan = np.isnan(t)
        t = np.where(nan, LD(0.5), t)
        self.on_edge += int((np.abs(t - np.rint(t)) < EDGE).sum())
        b = np.where(t < 0, LD(0), np.minimum(LD(bins - 1), np.floor(t)))
        return np.where(nan, -1, b.astype(np.int64))


@functools.lru_cache(maxsize=None)
def case(name):
    """(x, hist, dirs, Reference) of a case, computed once; treat them as read-only."""
    M, m, rows, d, kind, P, bins, steps, n_hist, specials = CASES[name]
    x, hist, dirs = inputs(name)
    for a in (x, hist) + (() if dirs is None else (dirs,)):
        a.setflags(write=False)
    return x, hist, dirs, Reference(x, hist, m, dirs, bins, steps)


def quantile_rule(counts, edges, q):
    """The quantile rule of diagnostics.marginal_quantile restated for ONE row of counts, in plain numpy doubles."""
    counts = np.asarray(counts, dtype=np.float64)
    N, B = counts.sum(), len(counts)
    if N == 0:
        return np.nan
    cum = np.cumsum(counts)
    want = N * q
    b = next(i for i in range(B) if cum[i] >= want and cum[i] > 0)
    before = cum[b - 1] if b else 0.0
    return edges[b] + (edges[-1] - edges[0]) / B * (want - before) / counts[b]

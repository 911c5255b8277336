"""Log normalising constants along ladders of a TargetBatch (gsss_batch_ladder; diagnostics.target_ladder, from_target_ladder,
summarize(log_z=)): the cases and the host restatement (test_ladder_host.py, test_hip_ladder.py, test_exchange_layouts_host.py,
test_hip_exchange_layouts.py).  Building a case touches no device; check_accumulators, which the two GPU modules share, holds
the device to a case.

The cases: two ladders of R = 3 -- the middle rung has both neighbours, the end rungs one -- of M = 6 members that really differ
(batch_layout_cases.members; a global-row case: its two members three times over), at the smallest shapes that reach every code
path of the evaluation kernel: a full chunk, a ragged chunk and a workgroup boundary inside every member, in each of the four
layout families and with the rows in global memory; the layout sweep (both ends of every one of the fifteen layouts) and the
tempered ladders with a flat hottest rung share exchange_cases' dims and members.

The restatement: the fold of include/gsss.h (gsss_batch_ladder) and the estimators of diagnostics.from_target_ladder in
np.longdouble, from a table of log-densities.  host_fold walks the rows with the stated recurrence; direct_sums takes the same
quantities without a recurrence (a maximum and one sum over the used rows), which is what host_fold itself is held to."""
import functools

import numpy as np

import layout_cases as lc

LD = np.longdouble
SLOTS = 10
R, G = 3, 2
N_ROWS = 5
FAMILIES = ("vmf1", "vmf3", "bingham_dense", "binghamfisher", "bingham_diag")
GLOBAL = "bingham_d129"      # dense Bingham d = 129: d^2 doubles exceed a workgroup's rows, read from global memory
TOL = 1e-10     # device against host, the project's tolerance (batch_layout_cases.TOL): only exp differs


def _coop16_d():
    """batch_layout_cases' first d of the sixteen-lane family."""
    import batch_layout_cases as bc
    return next(d for d in bc.DIMS if bc.layout_family(bc.natural_layout(d)) == "coop16")


# layout family -> (d, chains per target)
def shapes():
    return {"lane": (5, 259), "coop4": (17, 67), "coop16": (_coop16_d(), 19), "coop64": (130, 7)}


def cases():
    """Every (family, layout family) and the global-row case."""
    return [(f, name) for name in ("lane", "coop4", "coop16", "coop64") for f in FAMILIES] + [GLOBAL]


def layout_cases():
    """The layout sweep, ("layout", family, d): exchange_cases' dims (both ends of every one of the fifteen layouts) and
    families (one per target policy)."""
    import exchange_cases as ec
    return [("layout", f, d) for d in ec.layout_dims() for f in ec.LAYOUT_FAMILIES]


def flat_cases():
    """("flat", family, d): exchange_cases.flat_batch, two tempered ladders of three whose hottest rung is flat."""
    import exchange_cases as ec
    return [("flat", f, d) for d in ec.flat_dims() for f in ec.LAYOUT_FAMILIES]


def case_id(key):
    return key if isinstance(key, str) else "-".join(map(str, key))


def case_members(key):
    import batch_layout_cases as bc
    if isinstance(key, str):
        a, b = bc.global_members(key)
        return (a, b, a, b, a, b)
    if key[0] == "flat":
        import exchange_cases as ec
        return tuple(ec.flat_batch(*key[1:]).pdfs)
    if key[0] == "layout":
        return bc.members(key[1], key[2], R * G)
    return bc.members(key[0], shapes()[key[1]][0], R * G)


def case_m(key):
    import batch_layout_cases as bc
    if not isinstance(key, str) and len(key) == 3:
        return bc.chains_per_target(bc.natural_layout(key[2]))
    return 7 if isinstance(key, str) else shapes()[key[1]][1]


@functools.lru_cache(maxsize=None)
def case_rows(key):
    """-> (members, m, rows (N_ROWS, M m, d)): seeded unit vectors near one another, so that the differences u, v are of order
    one to ten and the sums have terms of both signs."""
    import batch_layout_cases as bc
    pdfs, m = case_members(key), case_m(key)
    d = pdfs[0].d
    if not isinstance(key, str) and len(key) == 2:     # the shape is the one that puts the case into its layout family
        assert bc.layout_family(bc.layout_of((key[0], d, R * G))) == key[1] and bc.chains_per_target(bc.layout_of((key[0], d, R * G))) == m
    rng = lc._rng("ladder", case_id(key))
    centre = lc._unit(rng.standard_normal(d))
    x = lc._unit(centre + 0.35 * rng.standard_normal((N_ROWS, len(pdfs) * m, d)) / np.sqrt(d))
    return pdfs, m, x


# ------------------------------------------------------------------------------------------ the host restatement
def pair_values(lp3, ladder):
    """lp3 (rows, M, m, 3): l_t at the member's own, its lower neighbour's (t - 1) and its upper neighbour's (t + 1) columns;
    slots of neighbours that do not exist are never read.  -> (la_a, la_b, lb_b, lb_a), each (rows, G, R - 1, m): the four
    values of every pair (a, b = a + 1) of neighbouring rungs."""
    rows, M, m, _ = lp3.shape
    assert M % ladder == 0 and ladder >= 2
    t = lp3.reshape(rows, M // ladder, ladder, m, 3)
    return t[:, :, :-1, :, 0], t[:, :, :-1, :, 2], t[:, :, 1:, :, 0], t[:, :, 1:, :, 1]


def host_fold(lp3, ladder, acc=None):
    """The fold, row by row, in longdouble: -> acc (G, R - 1, m, 10), continued from `acc` if given.  M starts at -inf and S
    at 0; the first used draw sets M = u, S = 1."""
    la_a, la_b, lb_b, lb_a = (np.asarray(v, dtype=LD) for v in pair_values(np.asarray(lp3), ladder))
    rows = la_a.shape[0]
    if acc is None:
        acc = np.zeros(la_a.shape[1:] + (SLOTS,), dtype=LD)
        acc[..., 1] = acc[..., 5] = -np.inf
    acc = np.array(acc, dtype=LD)
    for r in range(rows):
        ok = np.isfinite(la_a[r]) & np.isfinite(la_b[r]) & np.isfinite(lb_b[r]) & np.isfinite(lb_a[r])
        with np.errstate(all="ignore"):
            u, v = la_b[r] - lb_b[r], lb_a[r] - la_a[r]
        first = acc[..., 0] == 0
        for (iM, iS, i1, i2), w in (((1, 2, 3, 4), u), ((5, 6, 7, 8), v)):
            M, S = acc[..., iM], acc[..., iS]
            with np.errstate(all="ignore"):
                Mn = np.maximum(M, w)
                Sn = S * np.exp(M - Mn) + np.exp(w - Mn)
            Mn, Sn = np.where(first, w, Mn), np.where(first, LD(1), Sn)
            acc[..., iM], acc[..., iS] = np.where(ok, Mn, M), np.where(ok, Sn, S)
            acc[..., i1] = np.where(ok, acc[..., i1] + np.where(ok, w, 0), acc[..., i1])
            acc[..., i2] = np.where(ok, acc[..., i2] + np.where(ok, w * w, 0), acc[..., i2])
        acc[..., 0] += ok
        acc[..., 9] += ~ok
    return acc


def direct_sums(lp3, ladder):
    """Without a recurrence: -> dict of (G, R - 1, m) longdouble arrays: used, skipped, lse_u = log sum exp u over the used rows
    (a maximum, then one sum), sum_u, sum_uu, lse_v, sum_v, sum_vv."""
    la_a, la_b, lb_b, lb_a = (np.asarray(v, dtype=LD) for v in pair_values(np.asarray(lp3), ladder))
    ok = np.isfinite(la_a) & np.isfinite(la_b) & np.isfinite(lb_b) & np.isfinite(lb_a)
    out = {"used": ok.sum(0).astype(LD), "skipped": (~ok).sum(0).astype(LD)}
    with np.errstate(all="ignore"):
        for name, w in (("u", la_b - lb_b), ("v", lb_a - la_a)):
            top = np.max(np.where(ok, w, -np.inf), axis=0)
            safe = np.where(np.isfinite(top), top, 0)
            out["lse_" + name] = np.where(np.isfinite(top), safe + np.log(np.sum(np.where(ok, np.exp(w - safe), 0), axis=0)), -np.inf)
            out["sum_" + name] = np.sum(np.where(ok, w, 0), axis=0)
            out["sum_" + name * 2] = np.sum(np.where(ok, w * w, 0), axis=0)
    return out


def _lse(a, axis):
    top = np.max(a, axis=axis, keepdims=True)
    safe = np.where(np.isfinite(top), top, 0)
    with np.errstate(all="ignore"):
        return np.squeeze(safe, axis) + np.log(np.sum(np.exp(a - safe), axis=axis))


def host_estimates(acc, hot_log_z=None):
    """diagnostics.from_target_ladder restated in longdouble from acc (G, R - 1, m, 10)."""
    acc = np.asarray(acc, dtype=LD)
    m = acc.shape[2]
    n_i = acc[..., 0]
    used = n_i.sum(-1)
    with np.errstate(all="ignore"):
        lse_u = np.where(n_i > 0, acc[..., 1] + np.log(acc[..., 2]), -np.inf)
        lse_v = np.where(n_i > 0, acc[..., 5] + np.log(acc[..., 6]), -np.inf)
        forward = _lse(lse_u, -1) - np.log(used)
        backward = -(_lse(lse_v, -1) - np.log(used))
        per_chain = lse_u - np.log(n_i)
        se = per_chain.std(axis=-1, ddof=1) / np.sqrt(LD(m)) if m > 1 else np.full(forward.shape, np.nan)
        hot = np.zeros(acc.shape[0], dtype=LD) if hot_log_z is None else np.broadcast_to(np.asarray(hot_log_z, dtype=LD), acc.shape[:1])
        hot = np.where(np.isnan(hot), 0, hot)           # (a ladder without a flat hottest rung: relative to that rung)
        down = np.cumsum(forward[:, ::-1], axis=1)[:, ::-1]
        log_z = np.concatenate([down, np.zeros((acc.shape[0], 1), dtype=LD)], axis=1) + hot[:, None]
        return {"log_z_ratio_forward": forward, "log_z_ratio_backward": backward, "log_z_ratio": forward,
                "log_z_lower": acc[..., 3].sum(-1) / used, "log_z_upper": -acc[..., 7].sum(-1) / used, "log_z_ratio_se": se,
                "used": used, "skipped": acc[..., 9].sum(-1), "log_z": log_z}


def synthetic_table(seed, rows=40, ladders=2, ladder=4, m=5):
    """A table lp3 (rows, M, m, 3) of log-densities of order ten, with what the skip rule and the recurrence have to survive:
    NaN, +inf and -inf entries in slots that are read, a chain whose every row is skipped, a chain whose FIRST used draw is
    its maximum by far, one whose maximum comes last, and garbage (NaN) in the slots of neighbours that do not exist."""
    rng = np.random.default_rng(seed)
    M = ladders * ladder
    lp3 = 10.0 * rng.standard_normal((rows, M, m, 3))
    lp3[3, 1, 2, 0] = np.nan            # member 1's own value: pairs (0, 1) and (1, 2), chain 2, row 3
    lp3[5, 0, 1, 2] = np.inf            # l_0 at member 1's columns: pair (0, 1), chain 1
    lp3[7, 2, 0, 1] = -np.inf           # l_2 at member 1's columns: pair (1, 2), chain 0
    lp3[0, 5, 3, 0] = np.nan            # the first row of a chain: the first USED draw is then row 1
    lp3[:, ladder + 1, 4, 1] = np.nan   # pair (R, R + 1), chain 4: never used
    lp3[0, 2, 1, 2] += 400.0            # pair (2, 3), chain 1: u of the first draw exceeds every later one by hundreds
    lp3[-1, 2, 3, 2] += 400.0           # pair (2, 3), chain 3: the maximum comes last
    for g in range(ladders):            # never read
        lp3[:, g * ladder, :, 1] = np.nan
        lp3[:, g * ladder + ladder - 1, :, 2] = np.nan
    return lp3


def release():
    """Drop every cached case, and exchange_cases' and batch_layout_cases' with them."""
    import exchange_cases as ec
    case_rows.cache_clear()
    ec.release()


# ------------------------------------------------------------------------------------------ device against host restatement
# (device_rows, table and check_accumulators are the functions of this module that touch a device; test_hip_ladder.py and
# test_hip_exchange_layouts.py share them)
def device_rows(x):
    """(rows, N, d) numpy -> the component-major (rows, d, N) CUDA tensor"""
    import torch
    return torch.from_numpy(np.ascontiguousarray(np.transpose(x, (0, 2, 1)))).cuda()


def table(batch, x, m, ladder):
    """lp3 (rows, M, m, 3) from TargetBatch.log_prob: every member at its own rows, at its lower neighbour's and at its upper
    neighbour's, re-indexed; NaN where the neighbour does not exist (never read)."""
    rows, N, d = x.shape
    M = N // m
    xm = np.ascontiguousarray(x.reshape(rows, M, m, d).transpose(1, 0, 2, 3)).reshape(M, rows * m, d)
    t = np.arange(M)
    out = np.full((rows, M, m, 3), np.nan)
    for w, src, exists in ((0, t, np.ones(M, bool)), (1, t - 1, t % ladder != 0), (2, t + 1, t % ladder != ladder - 1)):
        lp = batch.log_prob(np.ascontiguousarray(xm[np.where(exists, src, t)])).reshape(M, rows, m).transpose(1, 0, 2)
        out[..., w][:, exists] = lp[:, exists]
    return out


def rel(got, want):
    got, want = np.asarray(got, dtype=LD), np.asarray(want, dtype=LD)
    return float(np.max(np.abs(got - want) / np.maximum(1, np.abs(want))))


def check_accumulators(key):
    """diagnostics.target_ladder on case_rows(key) against host_fold fed with TargetBatch.log_prob's values of the same rows:
    the counts (slots 0 and 9) equal, every row used, the four plain sums and the two S e^M products within TOL, and
    chain_major=True the same bits.  -> (the accumulators as a CUDA tensor, {quantity: worst deviation})."""
    import geosss_amd as gs
    import torch
    from geosss_amd import diagnostics
    pdfs, m, x = case_rows(key)
    batch = gs.TargetBatch(list(pdfs))
    acc = diagnostics.target_ladder(batch, device_rows(x), R)
    assert tuple(acc.shape) == (G, R - 1, m, 10) and acc.is_cuda
    got = acc.cpu().numpy()
    want = host_fold(table(batch, x, m, R), R)
    assert np.array_equal(got[..., 0], want[..., 0]) and np.array_equal(got[..., 9], want[..., 9])
    assert np.all(got[..., 0] == N_ROWS) and not got[..., 9].any()
    worst = {}
    for name, i in (("sum u", 3), ("sum u^2", 4), ("sum v", 7), ("sum v^2", 8)):
        worst[name] = rel(got[..., i], want[..., i])
    for name, (iM, iS) in (("S e^M (u)", (1, 2)), ("S e^M (v)", (5, 6))):
        g = got[..., iS].astype(LD) * np.exp(got[..., iM].astype(LD))
        w = want[..., iS] * np.exp(want[..., iM])
        assert np.all(np.isfinite(w)) and np.all(w > 0)
        worst[name] = float(np.max(np.abs(g - w) / w))
    print(case_id(key), {k: f"{v:.1e}" for k, v in worst.items()}, "max |u|", float(np.max(np.abs(got[..., 1]))))
    assert max(worst.values()) < TOL, worst
    # chain_major: the same draws as (N, rows, d), the same bits
    again = diagnostics.target_ladder(batch, torch.from_numpy(np.ascontiguousarray(np.transpose(x, (1, 0, 2)))).cuda(), R,
                                      chain_major=True)
    assert torch.equal(acc, again)
    return acc, worst

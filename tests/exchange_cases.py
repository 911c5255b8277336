"""Replica exchange along ladders of a TargetBatch: the reference and the cases (test_exchange_host.py, test_hip_exchange.py,
test_exchange_layouts_host.py, test_hip_exchange_layouts.py).

reference_sweep restates one sweep (include/gsss.h, gsss_batch_exchange) in numpy: the members' log-densities from
reference_math in longdouble, the uniform from the CPU oracle's stream.  Building a case touches no device; check_sweep, which
the two GPU modules share, holds the device to a case.

THE DECISION MARGIN IS A CONDITION, NOT A MEASUREMENT.  The device forms log alpha from double-precision values and its own
log(u); a pair whose |log u - log alpha| is at or below MARGIN could be decided either way by the last bits.  Such a pair is left
out of every comparison of decisions, and no case of the GPU tests may contain one: the seeds below were chosen on the CPU so that
the reference alone shows none (test_exchange_host.py asserts it).  At the test sizes one is expected about once in 10^5 seeds.

The d = 10 case (ladder_case): two orthogonal modes, equal weights, kappa = 1000, betas = 0.6 ** r for r = 0 .. 11, m = 64 chains
per rung, every chain started at mode 1, a sweep every 2 steps.  Settled on the CPU with run_ladder (the oracle's shrinkage chains
plus reference_sweep): the coldest member's occupancy of mode 2 over windows of 200 steps climbs 0.01, 0.11, 0.26, 0.30, 0.36, 0.37,
0.46 and reaches 0.5 after 1400 steps (the rungs accept 45 to 70 % of their pairs, so a state needs about a thousand steps from
the hot end to the cold one) -- hence N_STEPS = 2400 steps of which the first BURNIN = 1400 are dropped.  OCC_TOL has the figures.
"""
import functools

import numpy as np

import layout_cases as lc
import reference_math as rm

LD = np.longdouble
EXCHANGE_BLOCK = 0xFFFFFFFF   # kExchangeBlock, gsss_exchange.h
MARGIN = 1e-9


def _oracle():
    from oracle import oracle as orc
    orc.build()
    return orc


def uniforms(seed, chains, step):
    """The exchange uniform of every global chain id of `chains` at `step`."""
    orc = _oracle()
    return np.array([orc.stream_block(seed, int(c), step, EXCHANGE_BLOCK)[0] for c in chains])


def reference_sweep(batch_pdfs, x, err, m, R, parity, seed, step, chain_offset=0):
    """One sweep over the rows x (M m, d), target-major, of the members batch_pdfs.  -> dict: x (the permuted rows), replica
    (the permutation: row c of the result is row replica[c] of x), swap (M m,) bool at the LOWER chain of a pair, lower (M m,)
    bool, log_alpha (M m,) longdouble at the lower chains (nan elsewhere), margin (M m,) |log u - log alpha| at the lower chains
    that may swap (inf elsewhere: a refused pair is decided by the rule, not by the draw), attempts and accepts (M,) per
    lower member, scale (M m,) the largest magnitude of the pair's four values."""
    x = np.asarray(x, dtype=np.float64)
    n, d = x.shape
    M = n // m
    assert M == len(batch_pdfs) and n == M * m and M % R == 0 and parity in (0, 1)
    err = np.zeros(n, dtype=np.int32) if err is None else np.asarray(err)
    out, replica = x.copy(), np.arange(n)
    swap, lower = np.zeros(n, dtype=bool), np.zeros(n, dtype=bool)
    log_alpha, margin, scale = np.full(n, np.nan, dtype=LD), np.full(n, np.inf), np.zeros(n)
    attempts, accepts = np.zeros(M, dtype=np.int64), np.zeros(M, dtype=np.int64)
    for g in range(M // R):
        for k in range((R - parity) // 2):
            a = g * R + 2 * k + parity
            ia, ib = np.arange(a * m, (a + 1) * m), np.arange((a + 1) * m, (a + 2) * m)
            with np.errstate(all="ignore"):
                la_a, la_b = rm.log_prob(batch_pdfs[a], x[ia]), rm.log_prob(batch_pdfs[a], x[ib])
                lb_a, lb_b = rm.log_prob(batch_pdfs[a + 1], x[ia]), rm.log_prob(batch_pdfs[a + 1], x[ib])
                la = (la_b - la_a) + (lb_a - lb_b)
                may = (np.isfinite(la_a) & np.isfinite(la_b) & np.isfinite(lb_a) & np.isfinite(lb_b)
                       & (err[ia] == 0) & (err[ib] == 0))
                log_u = np.log(uniforms(seed, chain_offset + ia, step).astype(LD))   # u = 0: -inf, a swap
                s = may & (log_u < la)
                margin[ia] = np.where(may, np.abs(np.where(np.isfinite(log_u), log_u - la, LD(np.inf))).astype(np.float64), np.inf)
                scale[ia] = np.max(np.abs(np.stack([la_a, la_b, lb_a, lb_b]).astype(np.float64)), axis=0)
            lower[ia], swap[ia], log_alpha[ia] = True, s, la
            out[ia[s]], out[ib[s]] = x[ib[s]], x[ia[s]]
            replica[ia[s]], replica[ib[s]] = ib[s], ia[s]
            attempts[a] += m
            accepts[a] += int(s.sum())
    return {"x": out, "replica": replica, "swap": swap, "lower": lower, "log_alpha": log_alpha, "margin": margin,
            "attempts": attempts, "accepts": accepts, "scale": scale}


# ------------------------------------------------------------------------------------------ one sweep on the device: the cases
SWEEP_R, SWEEP_G = 3, 2       # two ladders of three: one member sits out under each parity
SWEEP_SEED, SWEEP_STEP = 777, 40
# (family, d) of batch_layout_cases, one d per layout family (lane, four, sixteen and sixty-four lanes a chain), and the two
# batches whose rows stay in global memory
SWEEP_CASES = [(f, d) for d in (5, 17, 40, 130) for f in ("vmf1", "vmf3", "bingham_dense", "binghamfisher", "bingham_diag")]
SWEEP_GLOBAL = ["vmf_k7000_d3", "bingham_d129"]

# The layout sweep (test_exchange_layouts_host.py, test_hip_exchange_layouts.py): every one of the fifteen layouts, at the
# smallest and the largest d of layout_cases.DIMS that the layout serves, one family per target policy (layout_cases.MH_FORCED's
# choice).  The keys are (family, d) like SWEEP_CASES', so sweep_case serves them as they are.
LAYOUT_FAMILIES = ("vmf3", "binghamfisher")
# a flat hottest rung: TargetBatch.tempered(p, FLAT_BETAS) of two members p -- two ladders of three whose last member has every
# mu = 0 (A = 0 and b = 0); keys ("flat", family, d), one d per layout family
FLAT_BETAS = (1.0, 0.5, 0.0)
# non-zero high words of the stream's counter: the second ladder of a SWEEP_CASES case alone, target0 = R.
# The low words are those of chain_offset = 0 and SWEEP_STEP, so that a sweep that dropped the high words would repeat that
# sweep's draws -- whose decisions differ (test_exchange_layouts_host.py asserts it on the reference).
HIGH_KEY = ("vmf3", 5)
HIGH_CHAIN_OFFSET = 5 << 32
HIGH_STEP = (0xBEEF << 32) | SWEEP_STEP


def case_id(key):
    return key if isinstance(key, str) else "-".join(map(str, key))


@functools.lru_cache(maxsize=None)
def layout_dims():
    """For each layout of batch_layout_cases.LAYOUTS the smallest and the largest d of layout_cases.DIMS whose natural layout
    it is (a lane layout that serves one d of DIMS gives that d once) -> the sorted dims."""
    import batch_layout_cases as bc
    by = {}
    for d in bc.DIMS:
        by.setdefault(bc.natural_layout(d), []).append(d)
    assert set(by) == set(bc.LAYOUTS), sorted(set(bc.LAYOUTS) - set(by))
    return tuple(sorted({d for name in bc.LAYOUTS for d in (min(by[name]), max(by[name]))}))


def layout_cases():
    return [(f, d) for d in layout_dims() for f in LAYOUT_FAMILIES]


def flat_dims():
    """One d per layout family: 5, 17, batch_layout_cases' first d of the sixteen-lane family, 130."""
    import batch_layout_cases as bc
    return (5, 17, next(d for d in bc.DIMS if bc.layout_family(bc.natural_layout(d)) == "coop16"), 130)


def flat_cases():
    return [("flat", f, d) for d in flat_dims() for f in LAYOUT_FAMILIES]


@functools.lru_cache(maxsize=None)
def flat_batch(family, d):
    """TargetBatch.tempered of the first two of batch_layout_cases.members(family, d) along FLAT_BETAS: the batch whose
    members the ("flat", family, d) cases of this module and of ladder_cases share."""
    import batch_layout_cases as bc
    import geosss_amd as gs
    return gs.TargetBatch.tempered(list(bc.members(family, d)[:SWEEP_G]), FLAT_BETAS)


def sweep_members(key):
    """The 6 members of a sweep case: (family, d) -> batch_layout_cases.members(family, d, 6); ("flat", family, d) -> the
    members of flat_batch; a global-row case -> its two members three times over (a ladder of members that differ, twice)."""
    import batch_layout_cases as bc
    if isinstance(key, str):
        a, b = bc.global_members(key)
        return (a, b, a, b, a, b)
    if key[0] == "flat":
        return tuple(flat_batch(*key[1:]).pdfs)
    return bc.members(key[0], key[1], SWEEP_R * SWEEP_G)


def sweep_m(key):
    import batch_layout_cases as bc
    if not isinstance(key, str) and key[0] == "flat":
        return bc.chains_per_target(bc.natural_layout(key[2]))
    if isinstance(key, str):
        import geosss_amd  # noqa: F401  (the members are the package's objects)
        pdfs = bc.global_members(key)
        d = pdfs[0].d
        layout = bc.natural_layout(d)
        dpad = bc.DPAD.get(layout, d)
        if dpad < 256 and bc.row_doubles(pdfs, dpad) * 8 > bc.ROWS_LDS_BYTES:
            layout = next(name for name in bc.LAYOUTS[11:] if d <= bc.DPAD[name])
        return bc.chains_per_target(layout)
    return bc.chains_per_target(bc.natural_layout(key[1]))


@functools.lru_cache(maxsize=None)
def sweep_case(key):
    """-> (members, m, rows (6 m, d), err (6 m,), the reference sweeps of parity 0 and 1).  The rows are seeded unit vectors near
    one another (so that log alpha is of order one and both decisions occur); one chain carries an error bit and one column a
    NaN, in members that take part under both parities."""
    pdfs, m = sweep_members(key), sweep_m(key)
    d = pdfs[0].d
    rng = lc._rng("exchange", key if isinstance(key, str) else "-".join(map(str, key)))
    n = len(pdfs) * m
    centre = lc._unit(rng.standard_normal(d))
    x = lc._unit(centre + 0.35 * rng.standard_normal((n, d)) / np.sqrt(d))
    err = np.zeros(n, dtype=np.int32)
    err[1 * m + 2] = 1                  # ladder 0, member 1: the upper chain under parity 0, the lower under parity 1
    x[4 * m + 1, d // 2] = np.nan       # ladder 1, member 1
    refs = tuple(reference_sweep(pdfs, x, err, m, SWEEP_R, p, SWEEP_SEED, SWEEP_STEP) for p in (0, 1))
    return pdfs, m, x, err, refs


@functools.lru_cache(maxsize=None)
def high_case():
    """The second ladder of sweep_case(HIGH_KEY) alone -> (all 6 members, m, its rows (3 m, d), its err (3 m,), the reference
    sweeps of parity 0 and 1 at chain_offset = HIGH_CHAIN_OFFSET and step = HIGH_STEP, the same at chain_offset = 0 and
    SWEEP_STEP).  The ladder holds the case's NaN column (member 1, chain 1) and no error bit."""
    pdfs, m, x, err, _ = sweep_case(HIGH_KEY)
    n = SWEEP_R * m
    sub, sub_err = x[n:].copy(), err[n:].copy()
    high = tuple(reference_sweep(pdfs[SWEEP_R:], sub, sub_err, m, SWEEP_R, p, SWEEP_SEED, HIGH_STEP, chain_offset=HIGH_CHAIN_OFFSET)
                 for p in (0, 1))
    low = tuple(reference_sweep(pdfs[SWEEP_R:], sub, sub_err, m, SWEEP_R, p, SWEEP_SEED, SWEEP_STEP) for p in (0, 1))
    return pdfs, m, sub, sub_err, high, low


def release():
    """Drop every cached case (dense members at d >= 1025 are 33 MB each) and batch_layout_cases' with them."""
    import batch_layout_cases as bc
    for cache in (sweep_case, high_case, flat_batch):
        cache.cache_clear()
    bc.release()


# ------------------------------------------------------------------------------------------ one sweep on the device: the checks
# (check_sweep and log_prob_pairs are the functions of this module that touch a device; test_hip_exchange.py and
# test_hip_exchange_layouts.py share them)
def log_prob_pairs(batch, x, m, lower):
    """The four values of every pair from TargetBatch.log_prob: own[c] = l_t(x_c), and across[c] = l_t(x_partner(c))."""
    M, d = len(batch), x.shape[1]
    xm = x.reshape(M, m, d)
    own = batch.log_prob(xm)
    partner = np.arange(M)
    lo = np.flatnonzero(lower.reshape(M, m)[:, 0])
    partner[lo], partner[lo + 1] = lo + 1, lo
    across = batch.log_prob(xm[partner])
    return own.reshape(-1), across.reshape(-1)


def check_sweep(key):
    """One sweep of either parity of sweep_case(key) on the device against reference_sweep: log alpha (the stated combination
    of TargetBatch.log_prob values bit for bit, the reference's to 1e-10 of the pair's scale, written at the lower chains only),
    the permuted rows bit for bit, replica, counts; errors and try counts untouched.  -> per parity dict(la: the device's
    log alpha (n,), own, across: log_prob_pairs' values, rel: the worst deviation of log alpha from the reference)."""
    import geosss_amd as gs
    import torch
    pdfs, m, x, err, refs = sweep_case(key)
    n = len(x)
    out = []
    for parity, ref in enumerate(refs):
        assert ref["margin"].min() > MARGIN
        s = gs.ShrinkageSphericalSliceSampler(gs.TargetBatch(list(pdfs)), x, seed=SWEEP_SEED, mode="exact", step_offset=SWEEP_STEP)
        s._err.copy_(torch.from_numpy(err))
        before = s.state_rows().cpu().numpy()
        assert np.array_equal(before, x, equal_nan=True)
        log_alpha = torch.full((n,), 7.25, dtype=torch.float64, device="cuda")
        s.exchange(SWEEP_R, parity, log_alpha=log_alpha)
        after = s.state_rows().cpu().numpy()
        la = log_alpha.cpu().numpy()
        lower, swap = ref["lower"], ref["swap"]
        # log alpha: the stated combination of TargetBatch.log_prob values bit for bit, the reference's to 1e-10 of their scale
        own, across = log_prob_pairs(s.target, x, m, lower)
        lo = np.flatnonzero(lower)
        with np.errstate(invalid="ignore"):
            want = (across[lo] - own[lo]) + (across[lo + m] - own[lo + m])
        assert np.array_equal(la[lo], want, equal_nan=True)
        assert np.all(la[~lower] == 7.25)                                        # written at the lower chains only
        fin = np.isfinite(ref["log_alpha"][lo].astype(np.float64))
        rel = np.abs(la[lo][fin] - ref["log_alpha"][lo][fin]).astype(np.float64) / ref["scale"][lo][fin]
        print(f"{case_id(key)} parity {parity}: {int(swap.sum())} of {int(lower.sum())} swap, log alpha within {rel.max():.1e}, "
              f"margin {ref['margin'].min():.1e}")
        assert rel.max() < 1e-10
        # decisions: a swapped column is the partner's old column bit for bit, every other column is untouched bit for bit
        # (members that sit out, the pair with the error bit, the pair with the NaN column, pairs the draw refused)
        moved = np.any((after != before) & ~(np.isnan(after) & np.isnan(before)), axis=1)
        assert np.array_equal(after, ref["x"], equal_nan=True)
        assert np.array_equal(after, before[ref["replica"]], equal_nan=True)
        assert not moved[~(np.isin(np.arange(n), lo[swap[lo]]) | np.isin(np.arange(n), lo[swap[lo]] + m))].any()
        assert np.array_equal(s.replica.cpu().numpy(), ref["replica"])
        st = s.exchange_stats()
        assert np.array_equal(st["attempts"].cpu().numpy(), ref["attempts"]) and np.array_equal(st["accepts"].cpu().numpy(), ref["accepts"])
        assert not swap[1 * m + 2] and not swap[0 * m + 2] and not swap[4 * m + 1] and not swap[3 * m + 1]   # err, NaN
        # counters and errors stay with the slot
        assert np.array_equal(s.errors, err) and not s.n_tries_per_chain.any()
        out.append({"la": la, "own": own, "across": across, "rel": float(rel.max())})
    return out


# ------------------------------------------------------------------------------------------ the d = 10 ladder
LADDER_D, LADDER_R, LADDER_M, LADDER_EVERY, LADDER_KAPPA = 10, 12, 64, 2, 1000.0
LADDER_BETAS = 0.6 ** np.arange(LADDER_R)
N_STEPS, BURNIN = 2400, 1400
LADDER_SEED = 101
TOL_SEEDS = (102, 103, 104, 105, 106)
# |occupancy of mode 2 by the coldest member - 0.5| over the retained steps (BURNIN .. N_STEPS, 64 chains), run_ladder with
# exchange, the five seeds of TOL_SEEDS: see OCC_DEVIATIONS; the tolerance is three times the largest.
OCC_DEVIATIONS = (0.0104, 0.0309, 0.0348, 0.0318, 0.0759)   # (seed 101 itself: 0.0144)
OCC_TOL = 3 * max(OCC_DEVIATIONS)                            # 0.2277


def ladder_modes():
    mu = np.zeros((2, LADDER_D))
    mu[0, 0] = mu[1, 1] = 1.0
    return mu


@functools.lru_cache(maxsize=None)
def ladder_case():
    """-> (the density, the tempered batch of 12 members, the start rows (768, 10): every chain at mode 1)."""
    import geosss_amd as gs
    mu = ladder_modes()
    pdf = gs.MixtureModel([gs.VonMisesFisher(LADDER_KAPPA * v) for v in mu], [0.5, 0.5])
    batch = gs.TargetBatch.tempered(pdf, LADDER_BETAS)
    x0 = np.tile(mu[0], (LADDER_R * LADDER_M, 1))
    return pdf, batch, x0


def run_ladder(pdfs, x0, m, R, every, n_steps, seed, exchange=True, keep_member=0):
    """The CPU reference of advance(n_steps, exchange=dict(ladder=R, every=every)) from step 0: the oracle's shrinkage chains of
    every member on the library stream (chain_offset = t m), cut at the sweep points, and reference_sweep between them.  ->
    dict: draws (n_steps, m, d) the states of member keep_member after every step (before the sweep that follows it), lp
    (n_steps, M) every member's mean log-density over its chains after every `every`-th step (before the sweep), state,
    attempts, accepts, min_margin."""
    orc = _oracle()
    targets = [lc.oracle_target(orc, p) for p in pdfs]
    M = len(pdfs)
    x = np.array(x0, dtype=np.float64)
    draws, lps = [], []
    attempts, accepts, min_margin = np.zeros(M, dtype=np.int64), np.zeros(M, dtype=np.int64), np.inf
    s = 0
    while s < n_steps:
        seg = min(every - s % every, n_steps - s)
        for t in range(M):
            r = orc.run(targets[t], x[t * m:(t + 1) * m], seg, seed=seed, chain_offset=t * m, step_offset=s, sampler=orc.SHRINK,
                        keep_samples=(t == keep_member))
            assert not r["err"].any()
            x[t * m:(t + 1) * m] = r["state"]
            if t == keep_member:
                draws.append(np.transpose(r["samples"], (1, 0, 2)))
        s += seg
        if s % every == 0:
            lps.append([float(np.mean(rm.log_prob(p, x[t * m:(t + 1) * m]))) for t, p in enumerate(pdfs)])
            if exchange:
                ref = reference_sweep(pdfs, x, None, m, R, (s // every) % 2, seed, s)
                x = ref["x"]
                attempts += ref["attempts"]
                accepts += ref["accepts"]
                min_margin = min(min_margin, float(ref["margin"].min()))
    return {"draws": np.concatenate(draws), "lp": np.array(lps), "state": x, "attempts": attempts, "accepts": accepts,
            "min_margin": min_margin}


def occupancy(draws, modes):
    """Share of the draws (.., d) whose nearest mode (the first maximum of x . mode_k, like np.argmax) is k -> (K,)."""
    k = np.argmax(np.asarray(draws) @ np.asarray(modes).T, axis=-1)
    return np.bincount(k.ravel(), minlength=len(modes)) / k.size


def sample_vmf(mu, size, rng):
    """`size` i.i.d. draws of VonMisesFisher(mu) on the host -- the scheme of geosss_amd.rand.sample_vMF (Wood 1994: rejection
    from a transformed Beta envelope along the mean direction, a uniform direction across it, a Householder reflection), which
    itself generates on the device and so cannot serve a test that runs without one."""
    mu = np.asarray(mu, dtype=np.float64)
    d, kappa = mu.size, float(np.linalg.norm(mu))
    z = rng.standard_normal((size, d))
    if kappa < 1e-12:
        return z / np.linalg.norm(z, axis=1, keepdims=True)
    p = d - 1
    b0 = (-2.0 * kappa + np.sqrt(4.0 * kappa * kappa + p * p)) / p
    x0 = (1.0 - b0) / (1.0 + b0)
    c = kappa * x0 + p * np.log(1.0 - x0 * x0)
    w = np.empty(size)
    todo = np.arange(size)
    while todo.size:
        zb = rng.beta(0.5 * p, 0.5 * p, todo.size)
        u = rng.uniform(size=todo.size)
        cand = (1.0 - (1.0 + b0) * zb) / (1.0 - (1.0 - b0) * zb)
        ok = kappa * cand + p * np.log(1.0 - x0 * cand) - c >= np.log(u)
        w[todo[ok]] = cand[ok]
        todo = todo[~ok]
    v = z[:, :p] / np.linalg.norm(z[:, :p], axis=1, keepdims=True)
    y = np.concatenate([np.sqrt(np.clip(1.0 - w * w, 0.0, None))[:, None] * v, w[:, None]], axis=1)
    e = np.zeros(d)
    e[-1] = 1.0
    h = e - mu / kappa
    hh = float(h @ h)
    return y if hh < 1e-30 else y - (2.0 / hh) * (y @ h)[:, None] * h[None, :]


def sample_member(pdf, size, rng):
    """i.i.d. draws of a vMF mixture member: a component by its weight, then sample_vmf of that component."""
    comps = [p for p, _ in pdf._terms()]
    w = np.array([v for _, v in pdf._terms()])
    pick = rng.choice(len(comps), size=size, p=w / w.sum())
    out = np.empty((size, pdf.d))
    for k, p in enumerate(comps):
        out[pick == k] = sample_vmf(p.mu, int((pick == k).sum()), rng).reshape(-1, pdf.d)
    return out

"""The target batches of the exact-mode layout sweep (test_target_batch_layouts_host.py, test_hip_target_batch_layouts.py): M
members that really differ per (family, d) of layout_cases.DIMS, the batches whose rows stay in global memory, the chains per
target that put a workgroup boundary and a ragged chunk inside every target, and the CPU oracle's chains of every member -- the
reference the device is held to.  Building a case touches no device: the distribution objects are parameter carriers.  Everything
is seeded and cached, so the tests that share a case share its members, its start rows and its reference chains.  The one function
here that evaluates on the device is check_logprob, which the two GPU modules of TargetBatch.log_prob share."""
import functools

import numpy as np

import layout_cases as lc
import reference_math as rm

LAYOUTS = ["lane2", "lane3", "lane4", "lane5", "lane6", "lane8", "lane10", "coop4x4", "coop4x8", "coop16x4", "coop16x8", "coop64x4",
           "coop64x8", "coop64x16", "coop64x32"]  # GSSS_VEC_LIST ids 1 .. 15
# columns a row is padded to in LDS (a lane layout: d itself)
DPAD = {"coop4x4": 16, "coop4x8": 32, "coop16x4": 64, "coop16x8": 128, "coop64x4": 256, "coop64x8": 512, "coop64x16": 1024,
        "coop64x32": 2048}
ROWS_LDS_BYTES = 136 * 1024  # kRowsLdsBytes, gsss_device.h
BLOCK = 256                  # lanes of a workgroup

DIMS = lc.DIMS
FAMILIES = ["vmf1", "vmf3", "bingham_dense", "bingham_diag", "binghamfisher"]
VMF_FAMILIES = ["vmf1", "vmf3"]
GLOBAL_CASES = ["vmf_k7000_d3", "vmf_k40_d600", "bingham_d129", "bingham_d300"]
SWEEP = [(family, d) for d in DIMS for family in FAMILIES]
SAMPLERS = ["shrink", "reject"]
PLACEMENTS = {"auto": 0, "packed": 1, "spread": 2}

SEED, X0_SEED = 20250, 31            # the library stream's seed, and that of the start rows
N_STEPS, THIN, FIRST = 6, 2, 4       # six steps, every second kept, run as advance(4, thin=2) then advance(2, thin=2)
TOL = 1e-10                          # device against oracle, tests/test_hip_parity.py


def _unit(v):
    return lc._unit(v)


def is_vmf(key):
    return (key if isinstance(key, str) else key[0]).startswith("vmf")


# ------------------------------------------------------------------------------------------ members
def _member(gs, rng, family, d):
    """One member: a direction, concentration, spectrum and weights of its own.  Moderate concentration (what
    layout_cases.chain_target uses), so that the rejection sampler accepts within tens of tries."""
    if family == "vmf1":
        return gs.VonMisesFisher(rng.uniform(5.0, 25.0) * _unit(rng.standard_normal(d)))
    if family == "vmf3":
        dirs = _unit(rng.standard_normal((3, d)))
        return gs.MixtureModel([gs.VonMisesFisher(k * v) for k, v in zip(rng.uniform(5.0, 25.0, 3), dirs)], rng.uniform(0.5, 2.0, 3))
    if family == "bingham_dense":
        return lc._bingham(gs, lc._sym(rng, d, rng.uniform(4.0, 10.0)))
    if family == "bingham_diag":
        return lc._bingham(gs, np.diag(rng.permutation(np.linspace(-rng.uniform(2.0, 6.0), rng.uniform(4.0, 10.0), d))))
    if family == "binghamfisher":
        return lc._bingham(gs, lc._sym(rng, d, rng.uniform(4.0, 10.0)), rng.uniform(1.0, 4.0) * _unit(rng.standard_normal(d)))
    raise ValueError(family)


@functools.lru_cache(maxsize=8)
def members(family, d, M=3):
    """M members of a sweep family at d, drawn one after the other from _rng("batch", family, d): the first three of M = 4 are
    the M = 3 case's.  The same objects for every test of the case."""
    import geosss_amd as gs
    rng = lc._rng("batch", family, d)
    return tuple(_member(gs, rng, family, d) for _ in range(M))


@functools.lru_cache(maxsize=None)
def global_members(name):
    """Two members whose rows do not fit a workgroup's LDS: the kernels read them from the moved blob in global memory."""
    import geosss_amd as gs
    rng = lc._rng("batch", name)
    out = []
    for _ in range(2):
        if name in ("vmf_k7000_d3", "vmf_k40_d600"):
            K, d = (7000, 3) if name == "vmf_k7000_d3" else (40, 600)
            dirs = _unit(rng.standard_normal((K, d)))
            out.append(gs.MixtureModel([gs.VonMisesFisher(k * v) for k, v in zip(rng.uniform(10.0, 100.0, K), dirs)],
                                       rng.uniform(0.5, 2.0, K)))
        elif name in ("bingham_d129", "bingham_d300"):
            d = int(name.split("_d")[1])
            out.append(lc._bingham(gs, lc._sym(rng, d, rng.uniform(4.0, 10.0))))
        else:
            raise ValueError(name)
    return tuple(out)


def pdfs_of(key):
    """key: (family, d), (family, d, M) or the name of a global-row case."""
    return global_members(key) if isinstance(key, str) else members(*key)


def mixed_members(d=24):
    """Diagonal and dense Bingham members alternating: the batch of section (d)."""
    diag, dense = members("bingham_diag", d), members("bingham_dense", d)
    return (diag[0], dense[0], diag[1], dense[1])


# ------------------------------------------------------------------------------------------ layouts
def lanes(layout):
    """Lanes per chain of a layout: 1, 4, 16 or 64."""
    return 1 if layout.startswith("lane") else int(layout[4:].split("x")[0])


def layout_family(layout):
    return "lane" if layout.startswith("lane") else "coop" + str(lanes(layout))


def natural_layout(d):
    """The layout gsss_exact_layout(d) names (no device is needed for the call)."""
    from geosss_amd import _lib
    vec = _lib.load().gsss_exact_layout(int(d))
    assert 1 <= vec <= len(LAYOUTS), (d, vec)
    return LAYOUTS[vec - 1]


def row_doubles(pdfs, dpad):
    """The rows a member stages in a layout of `dpad` columns (vmf_row_doubles, bingham_row_doubles; gsss_device.h)."""
    p = pdfs[0]
    kind = rm._kind(p)
    if kind == "VonMisesFisher":
        return dpad + 1
    if kind == "MixtureModel":
        return len(p.pdfs) * dpad + len(p.pdfs)
    return (p.d + 1) * dpad


def layout_of(key):
    """The layout an exact-mode launch of the batch runs in, restated from DESIGN.md: the one gsss_exact_layout(d) names, unless
    that one has fewer than sixty-four lanes a chain and the member's rows exceed the LDS budget -- then the smallest
    sixty-four-lane layout, whose kernels read the rows from global memory."""
    pdfs = pdfs_of(key)
    layout = natural_layout(pdfs[0].d)
    dpad = DPAD.get(layout, pdfs[0].d)
    if dpad < 256 and row_doubles(pdfs, dpad) * 8 > ROWS_LDS_BYTES:
        return next(name for name in LAYOUTS[11:] if pdfs[0].d <= DPAD[name])
    return layout


def rows_in_lds(key):
    pdfs = pdfs_of(key)
    layout = layout_of(key)
    return row_doubles(pdfs, DPAD.get(layout, pdfs[0].d)) * 8 <= ROWS_LDS_BYTES


def chains_per_target(layout, placement="packed"):
    """The layout's chains per workgroup + 3: one full chunk and a ragged one per target, a workgroup boundary inside it.  259
    for a lane layout when packed, 7 when spread (a chain a wavefront); 67, 19 and 7 for four, sixteen and sixty-four lanes."""
    L = lanes(layout)
    per_workgroup = BLOCK // 64 if (L == 1 and placement == "spread") else BLOCK // L
    return per_workgroup + 3


def chains(key, placement="packed"):
    return chains_per_target(layout_of(key), placement)


def sweep_params():
    """(key, placement, sampler) of section (a): every (family, d) packed, the lane layouts spread as well; the tests of a case
    stand side by side, so that its members are built once."""
    out = []
    for key in SWEEP:
        for placement in ("packed", "spread") if lanes(natural_layout(key[1])) == 1 else ("packed",):
            out += [(key, placement, sampler) for sampler in SAMPLERS]
    return out


def case_id(p):
    return p if isinstance(p, str) else "-".join(str(v) for v in p)


# ------------------------------------------------------------------------------------------ start rows and the oracle's chains
def _oracle():
    from oracle import oracle as orc
    orc.build()
    return orc


@functools.lru_cache(maxsize=None)
def x0(key, placement="packed"):
    """(M m, d) start rows, target-major, from oracle.sample_sphere."""
    pdfs = pdfs_of(key)
    return _oracle().sample_sphere(X0_SEED, len(pdfs) * chains(key, placement), pdfs[0].d)


def _run_members(pdfs, X0, m, sampler):
    orc = _oracle()
    kind = orc.SHRINK if sampler == "shrink" else orc.REJECT
    parts = [orc.run(lc.oracle_target(orc, p), X0[t * m:(t + 1) * m], N_STEPS, seed=SEED, chain_offset=t * m, thin=THIN, sampler=kind,
                     n_threads=8) for t, p in enumerate(pdfs)]
    return {k: np.concatenate([q[k] for q in parts]) for k in ("samples", "state", "n_tries", "n_reject", "err")}


@functools.lru_cache(maxsize=None)
def oracle_chains(key, sampler, placement="packed"):
    """The CPU oracle on every member alone, chain_offset = t m, the library stream of SEED: samples (M m, 3, d), state (M m, d),
    n_tries, n_reject, err (M m,)."""
    return _run_members(pdfs_of(key), x0(key, placement), chains(key, placement), sampler)


@functools.lru_cache(maxsize=None)
def oracle_chains_of_wrong_member(key, sampler):
    """What a batch that read member 0's rows for target 1 would have to reproduce: member 0 on target 1's start rows and
    chain ids.  -> the samples (m, 3, d) to hold against oracle_chains(key, sampler)["samples"][m:2 m]."""
    pdfs, m = pdfs_of(key), chains(key)
    orc = _oracle()
    out = orc.run(lc.oracle_target(orc, pdfs[0]), x0(key)[m:2 * m], N_STEPS, seed=SEED, chain_offset=m, thin=THIN,
                  sampler=orc.SHRINK if sampler == "shrink" else orc.REJECT, n_threads=8)
    return out["samples"]


@functools.lru_cache(maxsize=None)
def mixed_case(sampler, d=24):
    """-> (members, m, start rows, oracle chains) of the mixed diagonal / dense batch."""
    pdfs = mixed_members(d)
    m = chains_per_target(natural_layout(d))
    X0 = _oracle().sample_sphere(X0_SEED + 1, len(pdfs) * m, d)
    return pdfs, m, X0, _run_members(pdfs, X0, m, sampler)


# ------------------------------------------------------------------------------------------ log_prob / gradient of a batch
def points(what, M, n, d):
    """(M, n, d) seeded unit rows."""
    return _unit(lc._rng("points", what, M, n).standard_normal((M, n, d)))


def check_logprob(gs, pdfs, what, sizes, device_tensors=True, xs=None):
    """TargetBatch.log_prob / .gradient of the members `pdfs` at (M, n, d) rows for every n of `sizes`:
    (a) the members' own values bit for bit (np.array_equal), with no member uploaded by the batch's calls;
    (b) within 1e-10 of the value's scale (layout_cases.rel / gradient_error) of reference_math.log_prob_and_gradient."""
    import torch
    M, d = len(pdfs), pdfs[0].d
    for p in pdfs:  # (cached members may carry a device copy from an earlier test: (a) is about this batch's calls)
        p._invalidate()
    batch = gs.TargetBatch(pdfs)
    xs = [points(what, M, n, d) for n in sizes] if xs is None else xs
    got = [(batch.log_prob(x), batch.gradient(x)) for x in xs]
    if device_tensors:  # device tensors in, device tensors out, the same bits
        for x, (lp, gr) in zip(xs, got):
            xt = torch.from_numpy(x).cuda()
            assert np.array_equal(batch.log_prob(xt).cpu().numpy(), lp) and np.array_equal(batch.gradient(xt).cpu().numpy(), gr)
    # (a) no member was uploaded for any of it ...
    assert not any("_targets" in p.__dict__ for p in pdfs), "the batch evaluated a member's own handle"
    # ... then the members' own values (which upload them) and (b) the independent reference, once for the rows of all sizes:
    # a point's value does not depend on the rows beside it
    rows = np.concatenate(xs, axis=1)                                   # (M, sum of sizes, d)
    own_lp = np.stack([p._log_prob_device(rows[t]) for t, p in enumerate(pdfs)])
    own_gr = np.stack([p._gradient_device(rows[t]) for t, p in enumerate(pdfs)])
    ref = [rm.log_prob_and_gradient(p, rows[t]) for t, p in enumerate(pdfs)]
    at = 0
    for n, x, (lp, gr) in zip(sizes, xs, got):
        assert lp.shape == (M, n) and gr.shape == (M, n, d)
        assert np.array_equal(lp, own_lp[:, at:at + n]), (what, M, n)
        assert np.array_equal(gr, own_gr[:, at:at + n]), (what, M, n)
        worst = [0.0, 0.0]
        for t, p in enumerate(pdfs):
            worst[0] = max(worst[0], lc.rel(lp[t], ref[t][0][at:at + n]))
            worst[1] = max(worst[1], lc.gradient_error(p, x[t], gr[t], ref[t][1][at:at + n], d))
        print(f"{what} M={M} n={n}: log_prob {worst[0]:.1e}, gradient {worst[1]:.1e}")
        assert worst[0] < TOL and worst[1] < TOL, (what, M, n, worst)
        at += n
    for p in pdfs:  # the members' own device copies go again: the next check of these members starts as this one did
        p._invalidate()


def release():
    """Drop every cached case, and with it the device copies of the members' parameters."""
    import gc
    for cache in (members, global_members, x0, oracle_chains, oracle_chains_of_wrong_member, mixed_case):
        cache.cache_clear()
    rm._MATRICES.clear()
    gc.collect()

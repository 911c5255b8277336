"""One GPU step of tests/test_hip_target_batch_shared.py, run in a process of its own under the test's timeout:
    python tests/batch_shared_worker.py '<json: {"step": ..., ...}>'
Prints what it measured and exits 0, or fails an assertion.  Nothing here is a test by itself."""
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import geosss_amd as gs  # noqa: E402

SEED = 20251
README_MUS = 80.0 * np.array([[0.87, -0.37, 0.33], [-0.20, -0.89, -0.40], [0.19, 0.22, -0.96]])


def members(family, d, M):
    """M members that really differ: "diag" / "dense" / "b" Bingham, "vmfK" mixtures of K terms (d = 3, K = 3: the README target first)."""
    g = np.random.default_rng(1000 * d + sum(family.encode()))
    if family.startswith("vmf"):
        K = int(family[3:])
        out = []
        for t in range(M):
            if d == 3 and K == 3 and t == 0:
                out.append(gs.MixtureModel([gs.VonMisesFisher(mu) for mu in README_MUS]))
                continue
            mus = g.standard_normal((K, d))
            mus *= (20.0 + 80.0 * g.random((K, 1))) / np.linalg.norm(mus, axis=1, keepdims=True)
            out.append(gs.MixtureModel([gs.VonMisesFisher(mu) for mu in mus], g.random(K) + 0.2) if K > 1 else gs.VonMisesFisher(mus[0]))
        return out
    out = []
    for _ in range(M):
        p = gs.random_bingham(d, vmax=10.0 + 40.0 * g.random(), vmin=0.0, eigensystem=family == "diag", seed=int(g.integers(1 << 30)))
        out.append(gs.BinghamFisher(p.A, (1.0 + 4.0 * g.random()) * g.standard_normal(d)) if family == "b" else p)
    return out


def outputs(s, launches, thin):
    draws = np.concatenate([s.advance(n, thin=thin).cpu().numpy() for n in launches])
    return {"draws": draws, "state": s.state, "tries": s.n_tries_per_chain, "reject": s.n_reject_per_chain, "errors": s.errors}


def separate(cls, pdfs, x0, m, launches, thin, **kw):
    if pdfs[0].d > 10:  # the member's lane kernel: packed and screened (tests/test_hip_target_batch.py, the module's docstring)
        kw["placement"], kw["screen"] = "packed", True
    parts = [outputs(cls(p, x0[i * m:(i + 1) * m], SEED, chain_offset=i * m, mode="fast", **kw), launches, thin) for i, p in enumerate(pdfs)]
    return {k: np.concatenate([q[k] for q in parts], axis=2 if k == "draws" else 0) for k in parts[0]}


def same(got, want, what):
    for k in want:
        assert got[k].shape == want[k].shape, (what, k)
        assert np.array_equal(got[k], want[k]), (what, k, int(np.sum(got[k] != want[k])))
    assert not got["errors"].any(), what


def step_loop(a):
    """batch == loop, bit for bit; launches of 7 + 6 steps at thin 2 end between kept rows"""
    cls = getattr(gs, a["sampler"])
    M, m, d = a["M"], a["m"], a["d"]
    pdfs = members(a["family"], d, M)
    batch = gs.TargetBatch(pdfs)
    plan = batch.launch_plan(m)
    x0 = gs.sample_sphere(d - 1, M * m, seed=11)
    got = outputs(cls(batch, x0, SEED, mode="fast", screen=a["screen"]), [7, 6], 2)
    want = separate(cls, pdfs, x0, m, [7, 6], 2, screen=a["screen"])
    same(got, want, a)
    print("same", a, plan)


def step_splits(a):
    """a sampler started at target t0, sample() in 1 / 2 / 7 blocks, a two-way shard: each is the one launch"""
    import torch
    from geosss_amd import ensemble
    cls = gs.ShrinkageSphericalSliceSampler
    M, m, d = a["M"], a["m"], a["d"]
    batch = gs.TargetBatch(members(a["family"], d, M))
    x0 = gs.sample_sphere(d - 1, M * m, seed=11)
    full = outputs(cls(batch, x0, SEED, mode="fast"), [12], 2)
    t0 = 3
    part = outputs(cls(batch, x0[t0 * m:], SEED, mode="fast", chain_offset=t0 * m, chains_per_target=m), [12], 2)
    for k in full:
        assert np.array_equal(part[k], full[k][..., t0 * m:] if k == "draws" else full[k][t0 * m:]), ("t0", k)
    ref = cls(batch, x0, SEED, mode="fast").sample(10, burnin=4, blocks=1)
    for blocks in (2, 7):
        assert np.array_equal(cls(batch, x0, SEED, mode="fast").sample(10, burnin=4, blocks=blocks), ref), blocks
    one = ensemble.sharded_sampler(cls, batch, M * m, SEED, mode="fast")
    one.advance(12)
    halves = []
    world = ensemble.world
    try:
        for rank in (0, 1):
            ensemble.world = lambda rank=rank: (rank, 2)
            s = ensemble.sharded_sampler(cls, batch, M * m, SEED, mode="fast")
            s.advance(12)
            halves.append(s.state_device)
    finally:
        ensemble.world = world
    assert halves[0].shape[1] % m == 0 and torch.equal(torch.cat(halves, dim=1), one.state_device)
    print("splits", a)


def step_plan(a):
    """the launch is the plan: grid (gsss_last_launch) and the LDS, chains and targets a workgroup the library reports on stderr
    (GSSS_DEBUG_OCCUPANCY, set by the test)"""
    cls = gs.ShrinkageSphericalSliceSampler
    M, m, d = a["M"], a["m"], a["d"]
    batch = gs.TargetBatch(members(a["family"], d, M))
    plan = batch.launch_plan(m)
    s = cls(batch, gs.sample_sphere(d - 1, M * m, seed=11), SEED, mode="fast", screen=a["screen"])
    s.advance(4)
    grid = C.c_int64()
    gs._lib.load().gsss_last_launch(C.byref(grid), None, None)
    assert grid.value == plan["grid"], (grid.value, plan)
    print("plan", json.dumps(plan))


def step_family(a):
    """step_loop over the issue's m for one (family, d).  M per m: workgroups straddle target boundaries and the last one is
    ragged; m = 1 at d = 3, 16 has more targets than a workgroup's chains.  The two samplers and screen on / off rotate over the
    m, shifted by `turn`, so that every m meets every combination somewhere in the (family, d) grid."""
    combos = [(s, sc) for s in ("ShrinkageSphericalSliceSampler", "RejectionSphericalSliceSampler") for sc in (True, False)]
    sizes = {1: 270 if a["d"] in (3, 16) else 40, 3: 100, 16: 19, 64: 5, 100: 3, 300: 2}
    for i, (m, M) in enumerate(sizes.items()):
        sampler, screen = combos[(i + a["turn"]) % 4]
        step_loop({"family": a["family"], "d": a["d"], "M": M, "m": m, "sampler": sampler, "screen": screen})


def step_mixed(a):
    """diagonal and dense A mixed, small m: the batch runs the dense kernels, its diagonal members alone the diagonal ones, another
    arithmetic -- the existing 1e-10 exception (tests/test_hip_target_batch.py::test_diagonal_and_dense_members_mixed); integers exact"""
    cls = gs.ShrinkageSphericalSliceSampler
    m, d = a["m"], 10
    diag, dense = members("diag", d, 9), members("dense", d, 9)
    pdfs = [p for pair in zip(diag, dense) for p in pair]
    x0 = gs.sample_sphere(d - 1, len(pdfs) * m, seed=11)
    s = cls(gs.TargetBatch(pdfs), x0, SEED, mode="fast")
    assert gs._lib.load().gsss_kernel_name(s._target_dev.handle, 1, 0, 0) == b"screened_kernel<10, ScreenBingham<10>, batch>"
    got, want = outputs(s, [20], 2), separate(cls, pdfs, x0, m, [20], 2)
    for k in ("draws", "state"):
        err = float(np.max(np.abs(got[k] - want[k])))
        print(f"mixed diagonal / dense batch, m = {m}, {k}: max |dx| = {err:.3e}")
        assert err < 1e-10, (k, err)
    for k in ("tries", "reject", "errors"):
        assert np.array_equal(got[k], want[k]), k


if __name__ == "__main__":
    args = json.loads(sys.argv[1])
    {"loop": step_loop, "family": step_family, "splits": step_splits, "mixed": step_mixed, "plan": step_plan}[args.pop("step")](args)

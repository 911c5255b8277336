#!/usr/bin/env python3
"""What does one launch for M targets (gs.TargetBatch) buy over the loop a user wrote before it -- M samplers, one launch per
target per advance?  chain-steps/s of (a) the batch launch and (b) that loop, for Bingham d = 5 and the README mixture,
M in {1, 64, 1024, 4096} targets x m in {256, 1024} chains each, 1000 steps per launch, thin 100, fast mode; both sides in this
process, timed with events on the launch stream after a warm-up launch.  The batch side is timed over 20 launches; a repetition
of the loop side is M launches, repeated until at least 20 launches are timed (LOOP_REPS overrides).  Last, what the batch
indexing itself costs: M = 1, m = 10^6 against the plain one-chain-per-lane launch of the same target.
    MS=1,64 SIZES=256 python tools/bench_target_batch.py      # a subset
SMALL=16,64,100,256,300,1024: instead, the shape the type is for -- many small targets, M m ~ 10^6 chains (M = 10^6 // m) -- the
batch launch alone (a loop of 10^4 .. 10^5 samplers is not a baseline anybody runs), with the launch plan where the library
reports one (TargetBatch.launch_plan): the rows of DESIGN.md section 5.6c, taken on the parent and on this tree on one box."""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np, torch
import geosss_amd as gs

STEPS, THIN, REPS = 1000, 100, 20
README_MUS = 80.0 * np.array([[0.87, -0.37, 0.33], [-0.20, -0.89, -0.40], [0.19, 0.22, -0.96]])


def members(name, M):
    g = np.random.default_rng(1)
    if name == "bingham_d5":
        return [gs.random_bingham(5, vmax=10.0 + 40.0 * g.random(), vmin=0.0, seed=int(g.integers(1 << 30))) for _ in range(M)]
    out = []
    for _ in range(M):
        q, _ = np.linalg.qr(g.standard_normal((3, 3)))
        out.append(gs.MixtureModel([gs.VonMisesFisher(v) for v in (0.5 + g.random()) * README_MUS @ q.T]))
    return out


def timed(fn, reps):
    """seconds per call of fn, events on the current stream"""
    fn()                                   # warm-up: first-launch costs, the LDS attribute, the allocator
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(reps):
        fn()
    t1.record()
    t1.synchronize()
    return t0.elapsed_time(t1) * 1e-3 / reps


def small_targets(sizes):
    cls = gs.ShrinkageSphericalSliceSampler
    for name in ("bingham_d5", "vmfmix_readme"):
        for m in sizes:
            M = 1_000_000 // m
            batch = gs.TargetBatch(members(name, M))
            d = batch.d
            x0 = gs.sample_sphere_device(d - 1, M * m, seed=1).T.contiguous()
            sb = cls(batch, x0, 3521, mode="fast")
            out = torch.empty((STEPS // THIN, d, M * m), dtype=torch.float64, device=x0.device)
            t = timed(lambda: sb.advance(STEPS, thin=THIN, out=out), REPS)
            plan = batch.launch_plan(m) if hasattr(batch, "launch_plan") else {}
            print(f"{name:14s} M={M:6d} m={m:5d}: batch {M * m * STEPS / t:.3e} chain-steps/s ({t * 1e3:9.3f} ms a launch)   {plan}", flush=True)
            del sb, out, x0, batch


def main():
    if os.environ.get("SMALL"):
        return small_targets([int(v) for v in os.environ["SMALL"].split(",")])
    Ms = [int(v) for v in os.environ.get("MS", "1,64,1024,4096").split(",")]
    sizes = [int(v) for v in os.environ.get("SIZES", "256,1024").split(",")]
    cls = gs.ShrinkageSphericalSliceSampler
    for name in ("bingham_d5", "vmfmix_readme"):
        for m in sizes:
            for M in Ms:
                pdfs = members(name, M)
                d = pdfs[0].d
                x0 = gs.sample_sphere_device(d - 1, M * m, seed=1).T.contiguous()
                sb = cls(gs.TargetBatch(pdfs), x0, 3521, mode="fast")
                out = torch.empty((STEPS // THIN, d, M * m), dtype=torch.float64, device=x0.device)
                t_batch = timed(lambda: sb.advance(STEPS, thin=THIN, out=out), REPS)
                loop = [cls(p, x0[t * m:(t + 1) * m], 3521, mode="fast", chain_offset=t * m) for t, p in enumerate(pdfs)]
                outs = torch.empty((M, STEPS // THIN, d, m), dtype=torch.float64, device=x0.device)

                def run_loop():
                    for t, s in enumerate(loop):
                        s.advance(STEPS, thin=THIN, out=outs[t])
                t_loop = timed(run_loop, int(os.environ.get("LOOP_REPS", max(1, -(-20 // M)))))
                cs = M * m * STEPS
                print(f"{name:14s} M={M:5d} m={m:5d}: batch {cs / t_batch:.3e} chain-steps/s ({t_batch * 1e3:9.3f} ms a launch)   "
                      f"loop of {M} samplers {cs / t_loop:.3e} ({t_loop * 1e3:9.3f} ms)   x{t_loop / t_batch:.1f}", flush=True)
                del loop, outs, out, sb
    if os.environ.get("SKIP_INDEXING"):
        return
    os.environ.pop("GSSS_RESIDENT_PER_CU", None)
    n = 1_000_000
    for name in ("bingham_d5", "vmfmix_readme"):
        (pdf,) = members(name, 1)
        x0 = gs.sample_sphere_device(pdf.d - 1, n, seed=1).T.contiguous()
        out = torch.empty((STEPS // THIN, pdf.d, n), dtype=torch.float64, device=x0.device)
        res = {}
        os.environ["GSSS_ONE_PER_LANE"] = "2"      # the plain launch with one chain per lane too (read by the library per launch)
        for what, target in (("batch of one", gs.TargetBatch([pdf])), ("plain", pdf)):
            s = cls(target, x0, 3521, mode="fast", placement="packed")
            res[what] = n * STEPS / timed(lambda: s.advance(STEPS, thin=THIN, out=out), REPS)
        os.environ.pop("GSSS_ONE_PER_LANE")
        print(f"{name:14s} M=1 m={n}: batch of one {res['batch of one']:.3e}   plain one-chain-per-lane launch {res['plain']:.3e} "
              f"chain-steps/s   batch / plain {res['batch of one'] / res['plain']:.3f}", flush=True)


if __name__ == "__main__":
    main()

"""What one fold of the per-target marginal histograms costs, on a flat and on a peaked posterior, beside its two neighbours.

    python tools/bench_marginals.py [--rows 32] [--repeats 20] [--passes 2]

One block of 10^6 chains (3906 targets of m = 256: 999 936) x 32 rows at d = 5, 1.28 GB, read once by every kernel timed:

  (i)   gsss_target_marginals (diagnostics.target_marginals) with B = 64 bins along the P = d coordinate axes, without and with
        the step series;
  (ii)  gsss_target_mixing with K = 5 mode directions (the same axes) on the same block: the yardstick for the contention
        question -- a lane adds 1 to one of its target's K mode counters in LDS per draw with the same plain atomic, so on a
        peaked posterior the 64 lanes of a wavefront hit one address there too;
  (iii) gsss_target_moments on the same block: a kernel that reads the block and keeps no counter at all.

Two inputs.  flat: draws uniform on the sphere -- the lanes of a wavefront spread over the bins.  peaked: every draw within
0.05 rad of e_0 -- along e_0 all lanes of a target hit the last bin, along the other axes the three bins about 0, and the step
series the first three: LDS atomics to one address serialise.

Warm-up calls first, then `repeats` timed launches, each bracketed by device events on the stream the work runs on; median,
minimum and maximum are reported, and the whole series is run `passes` times so that the run-to-run spread can be read beside
any difference.  The block is far larger than the caches, so every launch reads HBM: bytes / time is given as a share of the
6.3 TB/s a streaming read reaches on this chip.  No pass criterion: one JSON line per measurement."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from geosss_amd import diagnostics  # noqa: E402

HBM_STREAM_TBS = 6.3
M, M_CHAINS, D, BINS = 3906, 256, 5, 64


def timed(fn, repeats, warmup=3):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return float(np.median(ms)), float(np.min(ms)), float(np.max(ms))


def block(kind, rows, n):
    """(rows, d, n) on the device: uniform on the sphere, or within 0.05 rad of e_0."""
    g = torch.Generator(device="cuda").manual_seed(17)
    x = torch.randn((rows, D, n), dtype=torch.float64, device="cuda", generator=g)
    if kind == "peaked":
        x[:, 0] = 0.0
        x /= x.norm(dim=1, keepdim=True)
        theta = 0.05 * torch.rand((rows, 1, n), dtype=torch.float64, device="cuda", generator=g)
        x *= torch.sin(theta)
        x[:, 0:1] = torch.cos(theta)
    return x / x.norm(dim=1, keepdim=True)


def bench(kind, rows, repeats, pass_no):
    n = M * M_CHAINS
    x = block(kind, rows, n)
    nbytes = 8 * x.numel()
    axes = torch.eye(D, dtype=torch.float64, device="cuda")
    runs = {}
    for steps in (False, True):
        counts = torch.zeros((M, D + steps, BINS), dtype=torch.int64, device="cuda")
        runs["marginals_steps" if steps else "marginals"] = (
            lambda steps=steps, counts=counts: diagnostics.target_marginals(x, M_CHAINS, bins=BINS, directions=axes, steps=steps,
                                                                            counts=counts))
    step, mix = torch.zeros((M, 2), dtype=torch.float64, device="cuda"), torch.zeros((M, 3 + D), dtype=torch.int64, device="cuda")
    runs["mixing_K5"] = lambda: diagnostics.target_mixing(x, M_CHAINS, hop=axes[0], modes=axes, step=step, counts=mix)
    acc = torch.zeros((M, 1 + D + D * (D + 1) // 2), dtype=torch.float64, device="cuda")
    runs["moments"] = lambda: diagnostics.target_moments(x, M_CHAINS, acc=acc)
    out = {"bench": "marginals", "input": kind, "pass": pass_no, "M": M, "m": M_CHAINS, "d": D, "bins": BINS, "rows": rows,
           "bytes": nbytes}
    for name, fn in runs.items():
        med, lo, hi = timed(fn, repeats)
        out.update({name + "_ms": round(med, 4), name + "_ms_min": round(lo, 4), name + "_ms_max": round(hi, 4),
                    name + "_TBs": round(nbytes / med / 1e9, 3),
                    name + "_share_of_stream_peak": round(nbytes / med / 1e9 / HBM_STREAM_TBS, 3)})
    c = diagnostics.target_marginals(x, M_CHAINS, bins=BINS, directions=axes, steps=True)
    busiest = c.max(-1).values.to(torch.float64) / c.sum(-1).to(torch.float64)
    out["share_of_the_busiest_bin_per_series"] = [round(float(v), 3) for v in busiest.mean(0)]
    out["marginals_over_mixing"] = round(out["marginals_ms"] / out["mixing_K5_ms"], 3)
    out["marginals_steps_over_mixing"] = round(out["marginals_steps_ms"] / out["mixing_K5_ms"], 3)
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=32)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--passes", type=int, default=2)
    a = ap.parse_args()
    for p in range(a.passes):
        for kind in ("flat", "peaked"):
            bench(kind, a.rows, a.repeats, p)

"""What the per-target moments kernel costs, against what a user would do without it.

    python tools/bench_target_moments.py [--shape big|small|both] [--repeats 20] [--end-to-end]

Two shapes (d = 5, R = 100 retained rows): M = 4096 targets of m = 256 chains, and M = 65 536 of m = 16.  On each, on a
resident window of draws [R][d][n] (unit vectors, 4.2 GB):

  (i)   gsss_target_moments on the window (diagnostics.target_moments, chain sums included): median time, bytes read / time,
        and that as a fraction of the 6.3 TB/s a streaming kernel reaches on this chip;
  (ii)  the torch formulation on the same window -- x.view(R, d, M, m).sum((0, 3)) for the means, and the second moment by a
        permute-and-copy to (M, d, R m) and a bmm with its transpose -- the yardstick: its `sum` pass alone is reported too;
  (iii) with --end-to-end: Sampler.summarize() against advance(n, thin=thin, out=...) storing the same rows (a batch of Bingham
        targets, d = 5, fast mode, windows of R rows): the overhead of folding every window.

Warm-up calls first, then the median of `repeats` timed calls, each bracketed by device events on the stream the work runs on;
the window is far larger than the caches, so every call reads HBM.  One JSON line per measurement."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import geosss_amd as gs  # noqa: E402
from geosss_amd import diagnostics  # noqa: E402

HBM_STREAM_TBS = 6.3
SHAPES = {"big": (4096, 256), "small": (65536, 16)}
D, R = 5, 100


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
    return float(np.median(ms)), float(np.min(ms))


def torch_sum(x, M, m):
    return x.view(R, D, M, m).sum((0, 3))


def torch_moments(x, M, m):
    s = torch_sum(x, M, m)
    y = x.view(R, D, M, m).permute(2, 1, 0, 3).reshape(M, D, R * m)
    return s, torch.bmm(y, y.transpose(1, 2))


def window_bench(name, repeats):
    M, m = SHAPES[name]
    n = M * m
    x = torch.randn((R, D, n), dtype=torch.float64, device="cuda")
    x /= x.norm(dim=1, keepdim=True)
    nbytes = 8 * x.numel()
    acc = torch.zeros((M, 1 + D + D * (D + 1) // 2), dtype=torch.float64, device="cuda")
    cs = torch.zeros((D, n), dtype=torch.float64, device="cuda")
    med, best = timed(lambda: diagnostics.target_moments(x, m, acc=acc, chain_sum=cs), repeats)
    med0, _ = timed(lambda: diagnostics.target_moments(x, m, acc=acc), repeats)
    t_med, t_best = timed(lambda: torch_moments(x, M, m), repeats)
    s_med, _ = timed(lambda: torch_sum(x, M, m), repeats)
    # the two agree
    acc.zero_()
    diagnostics.target_moments(x, m, acc=acc)
    s, q = torch_moments(x, M, m)
    iu = torch.triu_indices(D, D, device="cuda")
    err = max(float((acc[:, 1:1 + D] - s.T).abs().max()), float((acc[:, 1 + D:] - q[:, iu[0], iu[1]]).abs().max()))
    print(json.dumps({"bench": "window", "shape": name, "M": M, "m": m, "d": D, "rows": R, "bytes": nbytes,
                      "kernel_ms": med, "kernel_ms_min": best, "kernel_no_chain_sum_ms": med0,
                      "kernel_TBs": nbytes / med / 1e9, "fraction_of_stream_peak": nbytes / med / 1e9 / HBM_STREAM_TBS,
                      "torch_ms": t_med, "torch_ms_min": t_best, "torch_sum_only_ms": s_med,
                      "torch_sum_only_TBs": nbytes / s_med / 1e9, "torch_over_kernel": t_med / med,
                      "max_abs_difference": err}), flush=True)


def end_to_end(name, repeats):
    M, m = SHAPES[name]
    n = M * m
    g = np.random.default_rng(0)
    pdfs = [gs.random_bingham(D, vmax=20.0, vmin=0.0, seed=int(g.integers(1 << 30))) for _ in range(64)]
    pdfs = [pdfs[t % 64] for t in range(M)]
    x0 = g.standard_normal((n, D))
    x0 /= np.linalg.norm(x0, axis=1, keepdims=True)
    thin, rows = 2, 20
    s = gs.ShrinkageSphericalSliceSampler(gs.TargetBatch(pdfs), x0, 1, mode="fast")
    buf = torch.empty((rows, D, n), dtype=torch.float64, device="cuda")
    adv, _ = timed(lambda: (s.advance(thin), s.advance(rows * thin, thin=thin, out=buf)), repeats, warmup=2)
    summ, _ = timed(lambda: s.summarize(rows + 1, burnin=thin, thin=thin, window=rows), repeats, warmup=2)
    print(json.dumps({"bench": "end_to_end", "shape": name, "M": M, "m": m, "d": D, "rows": rows, "thin": thin,
                      "advance_ms": adv, "summarize_ms": summ, "overhead": summ / adv - 1.0}), flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", default="both", choices=["big", "small", "both"])
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--end-to-end", action="store_true")
    a = ap.parse_args()
    for name in (("big", "small") if a.shape == "both" else (a.shape,)):
        window_bench(name, a.repeats)
        if a.end_to_end:
            end_to_end(name, max(3, a.repeats // 4))

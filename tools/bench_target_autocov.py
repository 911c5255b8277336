"""What the per-target lagged-products kernel costs, against what a user would do without it.

    python tools/bench_target_autocov.py [--lags 8 32 64] [--rows 100] [--repeats 20] [--end-to-end]

One shape, the regime the estimator is for: M = 65 536 targets of m = 16 chains, d = 5.  For every L:

  (i)   gsss_target_autocov on a resident window of draws [R][d][n] (diagnostics.target_autocov; R = 100: 4.2 GB): median time,
        bytes read / time and that as a fraction of the 6.3 TB/s a streaming kernel reaches on this chip, and the floating-point
        instructions the kernel issues per value -- one fused multiply-add and one add per lag, three for lag 0 -- over time,
        against the chip's 39 T double-precision instructions/s (78.6 TFLOP/s counted as fused multiply-adds);
  (ii)  the torch formulation of the same sums on the same window, lag by lag: (x[l:] * x[:R - l]).view(.., M, m).sum((0, 3)) and
        the two plain sums -- the yardstick the kernel must beat to be worth having;
  (iii) with --end-to-end: Sampler.summarize(100, lags=L) against summarize(100) on the same sampler, one after the other (a
        batch of Bingham targets, d = 5, fast mode): what folding the lags adds to a summary.  summarize() without lags launches
        what it launched before the lags existed.

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
FP64_TINSTR_S = 39.3
M, CHAINS, D = 65536, 16, 5


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


def torch_autocov(x, lags):
    R = x.shape[0]
    out = torch.empty((M, D, lags + 1, 3), dtype=torch.float64, device=x.device)
    for lag in range(lags + 1):
        lead, trail = x[lag:], x[:R - lag]
        out[:, :, lag, 0] = (lead * trail).view(R - lag, D, M, CHAINS).sum((0, 3)).T
        out[:, :, lag, 1] = lead.view(R - lag, D, M, CHAINS).sum((0, 3)).T
        out[:, :, lag, 2] = trail.view(R - lag, D, M, CHAINS).sum((0, 3)).T
    return out


def window_bench(x, lags, repeats):
    nbytes, values = 8 * x.numel(), x.numel()
    acc = torch.zeros((M, D, lags + 1, 3), dtype=torch.float64, device="cuda")
    med, best = timed(lambda: diagnostics.target_autocov(x, CHAINS, lags, acc=acc), repeats)
    t_med, t_best = timed(lambda: torch_autocov(x, lags), max(3, repeats // 4), warmup=1)
    acc.zero_()
    diagnostics.target_autocov(x, CHAINS, lags, acc=acc)
    err = float((acc - torch_autocov(x, lags)).abs().max())
    instr = values * (2 * lags + 3)
    print(json.dumps({"bench": "window", "M": M, "m": CHAINS, "d": D, "rows": int(x.shape[0]), "lags": lags, "bytes": nbytes,
                      "kernel_ms": med, "kernel_ms_min": best, "kernel_TBs": nbytes / med / 1e9,
                      "fraction_of_stream_peak": nbytes / med / 1e9 / HBM_STREAM_TBS,
                      "fp64_Tinstr_s": instr / med / 1e9, "fraction_of_fp64_peak": instr / med / 1e9 / FP64_TINSTR_S,
                      "torch_ms": t_med, "torch_ms_min": t_best, "torch_over_kernel": t_med / med,
                      "max_abs_difference": err}), flush=True)


def end_to_end(lags_list, repeats):
    n = M * CHAINS
    g = np.random.default_rng(0)
    pdfs = [gs.random_bingham(D, vmax=20.0, vmin=0.0, seed=int(g.integers(1 << 30))) for _ in range(64)]
    pdfs = [pdfs[t % 64] for t in range(M)]
    x0 = g.standard_normal((n, D))
    x0 /= np.linalg.norm(x0, axis=1, keepdims=True)
    s = gs.ShrinkageSphericalSliceSampler(gs.TargetBatch(pdfs), x0, 1, mode="fast")
    for lags in lags_list:
        plain, _ = timed(lambda: s.summarize(100, burnin=1), repeats, warmup=1)
        with_lags, _ = timed(lambda: s.summarize(100, burnin=1, lags=lags), repeats, warmup=1)
        # the default ring of 256 MiB holds 6 rows of this ensemble: windows of ONE row behind `lags` rows of history; a ring of
        # 2 `lags` rows (window=lags) reads every row of history once per `lags` rows of progress
        wide, _ = timed(lambda: s.summarize(100, burnin=1, lags=lags, window=lags), repeats, warmup=1)
        print(json.dumps({"bench": "end_to_end", "M": M, "m": CHAINS, "d": D, "n_samples": 100, "lags": lags,
                          "summarize_ms": plain, "summarize_lags_ms": with_lags, "overhead": with_lags / plain - 1.0,
                          "summarize_lags_window_eq_lags_ms": wide, "ring_bytes_window_eq_lags": 2 * lags * D * n * 8}), flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--lags", type=int, nargs="+", default=[8, 32, 64])
    ap.add_argument("--rows", type=int, default=100)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--end-to-end", action="store_true")
    a = ap.parse_args()
    window = 3.0 + torch.randn((a.rows, D, M * CHAINS), dtype=torch.float64, device="cuda")
    for L in a.lags:
        window_bench(window, L, a.repeats)
    del window
    if a.end_to_end:
        end_to_end(a.lags, max(3, a.repeats // 4))

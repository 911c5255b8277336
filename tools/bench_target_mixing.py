"""What the per-target mixing kernel costs, against what a user would do without it.

    python tools/bench_target_mixing.py [--rows 100] [--repeats 20] [--end-to-end]

Two shapes of 2^20 chains, d = 5, K = 3 mode directions per target: M = 65 536 targets of m = 16 chains, and M = 4096 of m = 256.

  (i)   gsss_target_mixing on a resident window of draws [R][d][n] (diagnostics.target_mixing; R = 100: 4.2 GB), without and with
        the K x K transitions: median time, bytes read / time and that as a fraction of the 6.3 TB/s a streaming kernel reaches
        on this chip;
  (ii)  the torch formulation of the same sums on the same window, with every target's own directions: the geodesic step
        arccos(clamp(sum_j x_r x_{r-1})) and its square, the signs of x . h_t, the argmax of x . mode_k and a scatter_add per
        target (diagnostics.distance, hopping_frequency and argmax + bincount, batched over the targets) -- the yardstick;
  (iii) with --end-to-end: Sampler.summarize(100, mixing=True) against summarize(100) and summarize(100, lags=1) -- the same ring
        of 1 + window rows -- on the same sampler, one after the other (a batch of vMF mixtures, d = 5, K = 3, fast mode): what
        folding the mixing metrics adds to a summary.  mixing=True collects the members' directions on the host at every call
        that begins a summary (a Python loop over the M members); mixing=dict(...) with directions held on the device shows
        the fold alone.  summarize() without mixing launches what it launched before.

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
N, D, K = 1 << 20, 5, 3
SHAPES = [(65536, 16), (4096, 256)]


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


def torch_mixing(x, m, hop, modes):
    """-> (step (M, 2), counts (M, 3 + K)) with torch alone; hop (M, d), modes (M, K, d)."""
    R, d, n = x.shape
    M = n // m
    theta = torch.arccos(torch.clamp((x[1:] * x[:-1]).sum(1), -1.0, 1.0)).view(R - 1, M, m)
    step = torch.stack([theta.sum((0, 2)), (theta * theta).sum((0, 2))], 1)
    xv = x.view(R, d, M, m)
    side = torch.sign(torch.einsum("rdtc,td->rtc", xv, hop))
    counts = torch.zeros((M, 3 + K), dtype=torch.int64, device=x.device)
    counts[:, 0], counts[:, 1] = m * R, m * (R - 1)
    counts[:, 2] = (side[1:] != side[:-1]).sum((0, 2))
    mode = torch.argmax(torch.einsum("rdtc,tkd->rtck", xv, modes), -1)                       # (R, M, m)
    cell = mode + 3 + (3 + K) * torch.arange(M, device=x.device)[None, :, None]
    counts.view(-1).scatter_add_(0, cell.reshape(-1), torch.ones(cell.numel(), dtype=torch.int64, device=x.device))
    return step, counts


def window_bench(x, M, m, repeats):
    g = torch.Generator(device="cuda").manual_seed(M)
    dirs = torch.randn((M, 1 + K, D), dtype=torch.float64, device="cuda", generator=g)
    dirs /= dirs.norm(dim=-1, keepdim=True)
    hop, modes = dirs[:, 0].contiguous(), dirs[:, 1:].contiguous()
    nbytes = 8 * x.numel()
    out = {"bench": "window", "M": M, "m": m, "d": D, "K": K, "rows": int(x.shape[0]), "bytes": nbytes}
    for transitions in (False, True):
        step = torch.zeros((M, 2), dtype=torch.float64, device="cuda")
        counts = torch.zeros((M, 3 + K + (K * K if transitions else 0)), dtype=torch.int64, device="cuda")
        med, best = timed(lambda: diagnostics.target_mixing(x, m, hop=hop, modes=modes, transitions=transitions, step=step,
                                                            counts=counts), repeats)
        key = "kernel_transitions" if transitions else "kernel"
        out.update({key + "_ms": med, key + "_ms_min": best, key + "_TBs": nbytes / med / 1e9,
                    key + "_fraction_of_stream_peak": nbytes / med / 1e9 / HBM_STREAM_TBS})
    t_med, t_best = timed(lambda: torch_mixing(x, m, hop, modes), max(3, repeats // 4), warmup=1)
    step, counts = diagnostics.target_mixing(x, m, hop=hop, modes=modes)
    t_step, t_counts = torch_mixing(x, m, hop, modes)
    out.update({"torch_ms": t_med, "torch_ms_min": t_best, "torch_over_kernel": t_med / out["kernel_ms"],
                "counts_differ": int((counts != t_counts).sum()),
                "max_rel_step_difference": float(((step - t_step).abs() / t_step.abs()).max())})
    print(json.dumps(out), flush=True)


def end_to_end(M, m, repeats):
    g = np.random.default_rng(0)
    base = []
    for _ in range(64):
        mu = g.standard_normal((K, D))
        mu *= (10.0 + 30.0 * g.random((K, 1))) / np.linalg.norm(mu, axis=1, keepdims=True)
        base.append(gs.MixtureModel([gs.VonMisesFisher(v) for v in mu], g.random(K) + 0.5))
    pdfs = [base[t % 64] for t in range(M)]
    x0 = g.standard_normal((M * m, D))
    x0 /= np.linalg.norm(x0, axis=1, keepdims=True)
    s = gs.ShrinkageSphericalSliceSampler(gs.TargetBatch(pdfs), x0, 1, mode="fast")
    plain, _ = timed(lambda: s.summarize(100, burnin=1), repeats, warmup=1)
    ring, _ = timed(lambda: s.summarize(100, burnin=1, lags=1), repeats, warmup=1)
    mixing, _ = timed(lambda: s.summarize(100, burnin=1, mixing=True), repeats, warmup=1)
    # mixing=True gathers the M members' directions on the host at every call that begins a summary; with the directions
    # already on the device what is left is the fold itself
    hop, modes, weights = (torch.from_numpy(v).cuda() for v in s.target.mixing_directions())
    held, _ = timed(lambda: s.summarize(100, burnin=1, mixing=dict(hop=hop, modes=modes, weights=weights)), repeats, warmup=1)
    print(json.dumps({"bench": "end_to_end", "M": M, "m": m, "d": D, "K": K, "n_samples": 100, "summarize_ms": plain,
                      "summarize_lags1_ms": ring, "summarize_mixing_true_ms": mixing, "summarize_mixing_held_directions_ms": held,
                      "overhead_over_plain": held / plain - 1.0, "overhead_over_ring": held / ring - 1.0}), flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=100)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--end-to-end", action="store_true")
    a = ap.parse_args()
    window = torch.randn((a.rows, D, N), dtype=torch.float64, device="cuda")
    window /= window.norm(dim=1, keepdim=True)
    for M, m in SHAPES:
        window_bench(window, M, m, a.repeats)
    del window
    if a.end_to_end:
        for M, m in SHAPES:
            end_to_end(M, m, max(3, a.repeats // 4))

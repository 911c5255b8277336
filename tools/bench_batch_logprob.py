"""What evaluating a TargetBatch in one launch saves over the member loop, and what the log-density trace costs summarize().

    python tools/bench_batch_logprob.py [--repeats 20] [--skip-summarize]

(i)   Bingham d = 5 and the README mixture (3 vMF terms on S^2) at M = 64 / 1024 / 4096 targets, n = 256 points per target,
      points resident on the device where the call takes device tensors:
        one_launch_ms   TargetBatch.log_prob(x) on a CUDA tensor (M, n, d): the Python call, its key check included;
        c_abi_ms        gsss_batch_logprob on the batch handle alone: the launch;
        loop_ms         np.stack([p.log_prob(x[t]) for t, p in enumerate(pdfs)]) on warm member handles -- what
                        TargetBatch.log_prob did before: M uploads of the points, M launches, M downloads;
        loop_device_ms  torch.stack([p._log_prob_device(xt[t]) ...]): the same loop without the host copies.
(ii)  The kernel against a streaming read: gsss_batch_logprob on M = 4096 targets x 4096 points (0.7 GB at d = 5), and
      gsss_batch_logprob_draws on a window [100][d][M x 256] (4.2 GB at d = 5): bytes read / time, and that over the 6.3 TB/s a
      streaming kernel reaches on this chip.  A label, not a target: Bingham at d = 5 does 2 d^2 flops per 8 d bytes read and need
      not be bandwidth-bound; the mixture evaluates K exponentials per point.
(iii) Sampler.summarize(log_prob=True) against summarize() on M = 4096 Bingham targets, m = 256 chains, d = 5, 100 draws.

Warm-up calls first, then the median of `repeats` timed calls (fewer for the member loops at large M: they take seconds), each
bracketed by device events on the stream the work runs on.  One JSON line per measurement."""
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
README_MUS = 80.0 * np.array([[0.87, -0.37, 0.33], [-0.20, -0.89, -0.40], [0.19, 0.22, -0.96]])
N_POINTS = 256


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


def members(family, M, g):
    """64 distinct members, repeated (every member is uploaded and staged as its own either way)."""
    if family == "bingham_d5":
        base = [gs.random_bingham(5, vmax=20.0, vmin=0.0, seed=int(g.integers(1 << 30))) for _ in range(min(M, 64))]
        return [gs.Bingham(base[t % len(base)].A) for t in range(M)]
    out = []
    for t in range(M):
        q, r = np.linalg.qr(np.random.default_rng(t % 64).standard_normal((3, 3)))
        out.append(gs.MixtureModel([gs.VonMisesFisher(m) for m in README_MUS @ (q * np.sign(np.diag(r))).T]))
    return out


def unit(shape, device="cuda"):
    x = torch.randn(shape, dtype=torch.float64, device=device)
    return x / x.norm(dim=-1, keepdim=True)


def one_launch_against_the_loop(family, M, repeats):
    g = np.random.default_rng(0)
    pdfs = members(family, M, g)
    d = pdfs[0].d
    batch = gs.TargetBatch(pdfs)
    xt = unit((M, N_POINTS, d))
    x = xt.cpu().numpy()
    lib, h = gs._lib.load(), batch._device_target().handle
    out = torch.empty((M, N_POINTS), dtype=torch.float64, device="cuda")
    one, one_min = timed(lambda: batch.log_prob(xt), repeats)
    raw, raw_min = timed(lambda: lib.gsss_batch_logprob(h, xt.data_ptr(), N_POINTS, out.data_ptr(), None), repeats)
    loop_repeats = max(3, min(repeats, 20 * 64 // M))
    loop, _ = timed(lambda: np.stack([p.log_prob(x[t]) for t, p in enumerate(pdfs)]), loop_repeats, warmup=1)
    loop_dev, _ = timed(lambda: torch.stack([p._log_prob_device(xt[t]) for t, p in enumerate(pdfs)]), loop_repeats, warmup=1)
    same = bool(np.array_equal(batch.log_prob(x), np.stack([p.log_prob(x[t]) for t, p in enumerate(pdfs)])))
    nbytes = 8 * xt.numel()
    print(json.dumps({"bench": "one_launch", "family": family, "M": M, "n": N_POINTS, "d": d, "one_launch_ms": one,
                      "one_launch_ms_min": one_min, "c_abi_ms": raw, "c_abi_ms_min": raw_min, "loop_ms": loop,
                      "loop_device_ms": loop_dev, "loop_repeats": loop_repeats, "loop_over_one_launch": loop / one,
                      "loop_device_over_one_launch": loop_dev / one, "bytes_read": nbytes, "c_abi_TBs": nbytes / raw / 1e9,
                      "bitwise_equal": same}), flush=True)


def against_a_streaming_read(family, repeats):
    M = 4096
    pdfs = members(family, M, np.random.default_rng(0))
    d = pdfs[0].d
    batch = gs.TargetBatch(pdfs)
    lib = gs._lib.load()
    n = 4096
    xt = unit((M, n, d))
    out = torch.empty((M, n), dtype=torch.float64, device="cuda")
    h = batch._device_target().handle
    rows, _ = timed(lambda: lib.gsss_batch_logprob(h, xt.data_ptr(), n, out.data_ptr(), None), repeats)
    nb_rows = 8 * xt.numel()
    del xt, out
    R, m = 100, 256
    win = unit((R, M * m, d)).permute(0, 2, 1).contiguous()                     # [R][d][N]
    out = torch.empty((R, M * m), dtype=torch.float64, device="cuda")
    hm = batch._device_target(chains_per_target=m).handle
    draws, _ = timed(lambda: lib.gsss_batch_logprob_draws(hm, win.data_ptr(), R, M * m, 0, out.data_ptr(), None), repeats)
    nb_draws = 8 * win.numel()
    print(json.dumps({"bench": "stream", "family": family, "M": M, "d": d, "rows_n": n, "rows_bytes_read": nb_rows, "rows_ms": rows,
                      "rows_TBs": nb_rows / rows / 1e9, "rows_fraction_of_stream_peak": nb_rows / rows / 1e9 / HBM_STREAM_TBS,
                      "draws_rows": R, "draws_m": m, "draws_bytes_read": nb_draws, "draws_ms": draws,
                      "draws_TBs": nb_draws / draws / 1e9, "draws_fraction_of_stream_peak": nb_draws / draws / 1e9 / HBM_STREAM_TBS}),
          flush=True)


def summarize_with_the_trace(repeats):
    M, m, d, draws = 4096, 256, 5, 100
    g = np.random.default_rng(0)
    pdfs = members("bingham_d5", M, g)
    x0 = g.standard_normal((M * m, d))
    x0 /= np.linalg.norm(x0, axis=1, keepdims=True)
    s = gs.ShrinkageSphericalSliceSampler(gs.TargetBatch(pdfs), x0, 1, mode="fast")
    plain, _ = timed(lambda: s.summarize(draws, burnin=1), repeats, warmup=1)
    trace, _ = timed(lambda: s.summarize(draws, burnin=1, log_prob=True), repeats, warmup=1)
    print(json.dumps({"bench": "summarize", "M": M, "m": m, "d": d, "draws": draws, "summarize_ms": plain,
                      "summarize_log_prob_ms": trace, "overhead": trace / plain - 1.0}), flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--skip-summarize", action="store_true")
    a = ap.parse_args()
    for family in ("bingham_d5", "vmfmix_readme"):
        for M in (64, 1024, 4096):
            one_launch_against_the_loop(family, M, a.repeats)
    for family in ("bingham_d5", "vmfmix_readme"):
        against_a_streaming_read(family, a.repeats)
    if not a.skip_summarize:
        summarize_with_the_trace(max(3, a.repeats // 4))

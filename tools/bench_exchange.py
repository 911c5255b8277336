"""What a replica-exchange sweep costs beside the sampling it sits between.

    python tools/bench_exchange.py [--repeats 20] [--steps 100] [--every 10]

M = 4096 targets in ladders of R = 8, m = 256 chains per target (2^20 chains), fast mode, for two ladders: a Bingham target at
d = 5 (betas 0.7^r, exact powers) and the README mixture (3 vMF terms on S^2, kappa = 80; a ladder, not a power).
    sweep_ms            one sampler.exchange(R) at the current step: the evaluation launch and the swap launch;
    sweep_c_abi_ms      gsss_batch_exchange alone, replica and counts given;
    advance_ms          sampler.advance(steps): what the same call costs on the parent commit (exchange=None takes its code path);
    advance_exchange_ms sampler.advance(steps, exchange=dict(ladder=R, every=every)): the launches cut at the sweep points, a
                        sweep after each;
and per sweep the bytes it must move, 4 d 8 per chain that takes part (both columns read by the evaluation, read and written
by the swap where it is accepted) plus 4 x 8 of scratch, against the time -- a label, not a target.
Warm-up calls first, then the median of `repeats` timed calls, each bracketed by device events on the stream the work runs on.
One JSON line per ladder."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import geosss_amd as gs  # noqa: E402

README_MUS = 80.0 * np.array([[0.87, -0.37, 0.33], [-0.20, -0.89, -0.40], [0.19, 0.22, -0.96]])
M, R, CHAINS = 4096, 8, 256


def timed(fn, repeats, warmup=2):
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
    return float(np.median(ms))


def ladders(family):
    g = np.random.default_rng(0)
    betas = 0.7 ** np.arange(R)
    if family == "bingham_d5":
        base = [gs.Bingham(gs.random_bingham(5, vmax=20.0, vmin=0.0, seed=int(g.integers(1 << 30))).A) for _ in range(M // R)]
    else:
        base = []
        for t in range(M // R):
            q, r = np.linalg.qr(np.random.default_rng(t % 64).standard_normal((3, 3)))
            base.append(gs.MixtureModel([gs.VonMisesFisher(m) for m in README_MUS @ (q * np.sign(np.diag(r))).T]))
    return gs.TargetBatch.tempered(base, betas)


def run(family, repeats, steps, every):
    batch = ladders(family)
    d, n = batch.d, M * CHAINS
    x0 = np.random.default_rng(1).standard_normal((n, d))
    x0 /= np.linalg.norm(x0, axis=1, keepdims=True)
    s = gs.ShrinkageSphericalSliceSampler(batch, x0, 1, mode="fast")
    s.advance(20)
    ex = dict(ladder=R, every=every)
    sweep = timed(lambda: s.exchange(R), repeats)
    x = s._exchange_buffers()
    lib, h = gs._lib.load(), s._target_dev.handle
    raw = timed(lambda: lib.gsss_batch_exchange(h, s.state_device.data_ptr(), s._err.data_ptr(), n, 0, R, 0, s.seed, 0, s._step,
                                                x["scratch"].data_ptr(), x["replica"].data_ptr(), x["counts"].data_ptr(), None, None),
                repeats)
    plain = timed(lambda: s.advance(steps), max(3, repeats // 4), warmup=1)
    with_x = timed(lambda: s.advance(steps, exchange=ex), max(3, repeats // 4), warmup=1)
    st = s.exchange_stats()
    taking_part = n // R * (R // 2) * 2                       # chains of a parity-0 sweep
    nbytes = taking_part * (4 * d * 8 + 4 * 8)
    print(json.dumps({"bench": "exchange", "family": family, "M": M, "R": R, "m": CHAINS, "d": d, "sweep_ms": sweep,
                      "sweep_c_abi_ms": raw, "sweep_bytes": nbytes, "sweep_TBs": nbytes / raw / 1e9, "steps": steps, "every": every,
                      "advance_ms": plain, "advance_exchange_ms": with_x, "overhead": with_x / plain - 1.0,
                      "ms_per_sweep_in_advance": (with_x - plain) / max(1, steps // every),
                      "mean_rate": float(np.nanmean(st["rate"].cpu().numpy()))}), flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--every", type=int, default=10)
    a = ap.parse_args()
    for family in ("bingham_d5", "vmfmix_readme"):
        run(family, a.repeats, a.steps, a.every)

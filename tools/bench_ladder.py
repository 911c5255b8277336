"""What the log normalising constants along a ladder cost beside the run they summarise.

    python tools/bench_ladder.py [--repeats 10] [--steps 100] [--every 10] [--rows 16]

M = 4096 targets in ladders of R = 8, m = 256 chains per target (2^20 chains), fast mode, for two ladders: a Bingham target at
d = 5 (betas 0.7^r, exact powers) and the README mixture (3 vMF terms on S^2, kappa = 80; a ladder, not a power).
    summarize_ms        sampler.summarize(steps, exchange=dict(ladder=R, every=every)): what the same call costs on the parent
                        commit (log_z=False takes its code path);
    summarize_log_z_ms  the same with log_z=True: every window also goes through gsss_batch_ladder;
    ladder_ms           gsss_batch_ladder alone on a block of `rows` retained rows: the evaluation launch (every member at its
                        own and at its two neighbours' columns, its rows staged once) and the fold launch;
    per_row_eval_ms     what it replaces: rows x 2 calls of gsss_batch_exchange on the same rows, one per row and parity, with
                        log_alpha_out given -- the per-row evaluation that stages every member's rows per call (each call also
                        runs the swap kernel, which is part of the figure);
and the bytes gsss_batch_ladder must move -- the three column sets read, 3 x 8 of scratch written and read per draw, the
accumulators read and written -- against ladder_ms: a label, not a target.
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
from bench_exchange import CHAINS, M, R, ladders, timed  # noqa: E402


def run(family, repeats, steps, every, rows):
    batch = ladders(family)
    d, n = batch.d, M * CHAINS
    x0 = np.random.default_rng(1).standard_normal((n, d))
    x0 /= np.linalg.norm(x0, axis=1, keepdims=True)
    s = gs.ShrinkageSphericalSliceSampler(batch, x0, 1, mode="fast")
    s.advance(20)
    ex = dict(ladder=R, every=every)
    few = max(3, repeats // 3)
    out = {"bench": "ladder", "family": family, "M": M, "R": R, "m": CHAINS, "d": d, "steps": steps, "every": every, "rows": rows}
    out["summarize_ms"] = timed(lambda: s.summarize(steps, exchange=ex), few, warmup=1)
    if hasattr(gs.diagnostics, "target_ladder"):        # (the parent commit runs up to here)
        out["summarize_log_z_ms"] = timed(lambda: s.summarize(steps, exchange=ex, log_z=True), few, warmup=1)
        out["log_z_overhead"] = out["summarize_log_z_ms"] / out["summarize_ms"] - 1.0
        lib, h = gs._lib.load(), s._target_dev.handle
        block = s.advance(rows, thin=1)                                        # (rows, d, n), component-major
        scratch = torch.empty(int(lib.gsss_ladder_scratch_doubles(rows, n)), dtype=torch.float64, device=block.device)
        acc = torch.zeros(int(lib.gsss_ladder_acc_doubles(n, CHAINS, R)), dtype=torch.float64, device=block.device)
        out["ladder_ms"] = timed(lambda: gs._lib.check(lib.gsss_batch_ladder(h, block.data_ptr(), rows, n, 0, R, scratch.data_ptr(),
                                                                             acc.data_ptr(), None)), repeats)
        nbytes = rows * n * (3 * d * 8 + 2 * 3 * 8) + 2 * acc.numel() * 8
        out.update(ladder_bytes=nbytes, ladder_TBs=nbytes / out["ladder_ms"] / 1e9)
        x = s._exchange_buffers()
        err = torch.zeros(n, dtype=torch.int32, device=block.device)
        log_alpha = torch.empty(n, dtype=torch.float64, device=block.device)
        copy = block.clone()                                                   # (the swaps move columns of the copy)

        def per_row():
            for r in range(rows):
                for parity in (0, 1):
                    gs._lib.check(lib.gsss_batch_exchange(h, copy[r].data_ptr(), err.data_ptr(), n, 0, R, parity, s.seed, 0, s._step,
                                                          x["scratch"].data_ptr(), None, None, log_alpha.data_ptr(), None))
        out["per_row_eval_ms"] = timed(per_row, repeats)
        out["per_row_over_ladder"] = out["per_row_eval_ms"] / out["ladder_ms"]
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--every", type=int, default=10)
    ap.add_argument("--rows", type=int, default=16)
    a = ap.parse_args()
    for family in ("bingham_d5", "vmfmix_readme"):
        run(family, a.repeats, a.steps, a.every, a.rows)

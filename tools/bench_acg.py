#!/usr/bin/env python3
"""The angular central Gaussian as a native target (gs.AngularCentralGaussian, GSSS_ACG): chain-steps/s of the shrinkage sampler,
packed placement, nothing kept, at d = 5 and d = 10 for
    native fast     fast_kernel<D, FastAcg<D>>: a try is three FMAs and a comparison
    native exact    run_kernel<laneD, Acg>
    user target     the same density as a DeviceDistribution (tests/user_sources.py::ACG), exact mode only
Lambda = Q diag(linspace(1, 1 + 40 / sqrt(d), d)) Q^T, the targets of tests/acg_cases.py.  Prints the tries per step too: the
three variants run the same chains.
GPU box: python tools/bench_acg.py [n_chains] [steps]"""
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import geosss_amd as gs  # noqa: E402
from acg_cases import precision  # noqa: E402
from user_sources import ACG  # noqa: E402


def rate(pdf, x0, steps, mode):
    s = gs.ShrinkageSphericalSliceSampler(pdf, x0, 3521, mode=mode, placement="packed")
    name = s._lib.gsss_kernel_name(s._target_dev.handle, 1 if mode == "fast" else 0, 0, 1).decode()
    s.advance(20)  # warm-up
    torch.cuda.synchronize()
    best = 0.0
    for _ in range(3):
        t0 = time.perf_counter()
        s.advance(steps)
        torch.cuda.synchronize()
        best = max(best, x0.shape[0] * steps / (time.perf_counter() - t0))
    assert not np.any(s.errors)
    return best, name, float(s._n_tries.sum().item()) / (x0.shape[0] * (20 + 3 * steps))


n = int(sys.argv[1]) if len(sys.argv) > 1 else 1_000_000
steps = int(sys.argv[2]) if len(sys.argv) > 2 else 200
with tempfile.TemporaryDirectory() as cache:
    for d in (5, 10):
        native = gs.AngularCentralGaussian(precision(d))
        user = gs.DeviceDistribution(d, ACG, native.precision, cache_dir=cache)
        x0 = gs.sample_sphere_device(d - 1, n, seed=1).T
        rf, nf, tf = rate(native, x0, steps, "fast")
        re, ne, te = rate(native, x0, steps, "exact")
        ru, nu, tu = rate(user, x0, steps, "exact")
        print(f"ACG d={d}, {n} chains x {steps} steps, {tf:.2f} / {te:.2f} / {tu:.2f} tries per step: native fast {rf:.3e} "
              f"chain-steps/s ({nf}), native exact {re:.3e} ({ne}), user target {ru:.3e} ({nu}); fast / exact = {rf / re:.2f}, "
              f"native exact / user = {re / ru:.2f}", flush=True)

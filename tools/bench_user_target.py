#!/usr/bin/env python3
"""User-defined targets (DeviceDistribution, GSSS_USER) against the built-in ones: chain-steps/s of the shrinkage sampler in
exact mode, packed placement, keep=False, on the same layout and kernel template -- the user C++ of tests/user_sources.py:
    README mixture of three vMF terms (d = 3, kappa = 80)          vs gs.MixtureModel of gs.VonMisesFisher
    Bingham d = 10, random_bingham(vmax = 30)                       vs gs.Bingham
Prints the compile time of each module too (a fresh cache directory: every module is compiled).
GPU box: python tools/bench_user_target.py [n_chains] [steps]"""
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
from user_sources import BINGHAM, VMF_MIXTURE, vmf_mixture_params  # noqa: E402


def cases(cache):
    mus = 80.0 * np.array([[0.87, -0.37, 0.33], [-0.20, -0.89, -0.40], [0.19, 0.22, -0.96]])
    t0 = time.perf_counter()
    user = gs.DeviceDistribution(3, VMF_MIXTURE, vmf_mixture_params(mus, np.ones(3)), cache_dir=cache)
    yield "README vMF mixture d=3", user, gs.MixtureModel([gs.VonMisesFisher(m) for m in mus]), time.perf_counter() - t0
    A = gs.random_bingham(d=10, vmax=30.0, vmin=0.0, seed=7).A
    t0 = time.perf_counter()
    user = gs.DeviceDistribution(10, BINGHAM, A, cache_dir=cache)
    yield "Bingham d=10", user, gs.Bingham(A), time.perf_counter() - t0


def rate(pdf, x0, steps):
    s = gs.ShrinkageSphericalSliceSampler(pdf, x0, 3521, mode="exact", placement="packed")
    name = s._lib.gsss_kernel_name(s._target_dev.handle, 0, 0, 1).decode()
    s.advance(20)  # warm-up
    torch.cuda.synchronize()
    best = 0.0
    for _ in range(3):
        t0 = time.perf_counter()
        s.advance(steps)
        torch.cuda.synchronize()
        best = max(best, x0.shape[0] * steps / (time.perf_counter() - t0))
    return best, name


n = int(sys.argv[1]) if len(sys.argv) > 1 else 1_000_000
steps = int(sys.argv[2]) if len(sys.argv) > 2 else 200
with tempfile.TemporaryDirectory() as cache:
    for label, user, builtin, t_compile in cases(cache):
        x0 = gs.sample_sphere_device(user.d - 1, n, seed=1).T
        ru, nu = rate(user, x0, steps)
        rb, nb = rate(builtin, x0, steps)
        print(f"{label}, {n} chains x {steps} steps, exact: user {ru:.3e} chain-steps/s ({nu}), built-in {rb:.3e} ({nb}), "
              f"user / built-in = {ru / rb:.3f}; module compiled in {t_compile:.1f} s", flush=True)

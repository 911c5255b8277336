#!/usr/bin/env python3
"""MixtureModel targets of vMF / Bingham / Fisher-Bingham / Uniform terms (GSSS_MIXTURE): chain-steps/s at 10^6 chains, fast
(FastMixture) against exact (Mixture) kernels, keep=False, the two cases of tests/golden/make_golden_mixtures.py:
    d = 3: VonMisesFisher(50 m) + Bingham(A) + Uniform, weights (.5, .3, .2)
    d = 5: two dense random_bingham + one BinghamFisher, weights (.4, .4, .2)
GPU box: python tools/bench_mixture.py [n_chains] [steps]"""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import geosss_amd as gs  # noqa: E402


def unit(v):
    v = np.asarray(v, dtype=float)
    return v / np.linalg.norm(v)


def cases():
    A = np.array([[4.0, 1.0, 0.0], [1.0, -2.0, 0.5], [0.0, 0.5, 3.0]])
    yield "d3 vMF+Bingham+Uniform", gs.MixtureModel([gs.VonMisesFisher(50.0 * unit([0.3, -0.5, 0.8])), gs.Bingham(A), gs.Uniform()],
                                                    [0.5, 0.3, 0.2])
    B1 = gs.random_bingham(d=5, vmax=20.0, vmin=0.0, seed=11).A
    B2 = gs.random_bingham(d=5, vmax=15.0, vmin=0.0, seed=12).A
    A3 = gs.random_bingham(d=5, vmax=10.0, vmin=0.0, seed=13).A
    yield "d5 2 Bingham+Fisher-Bingham", gs.MixtureModel([gs.Bingham(B1), gs.Bingham(B2), gs.BinghamFisher(A3, 4.0 * unit(np.arange(1.0, 6.0)))],
                                                         [0.4, 0.4, 0.2])


n = int(sys.argv[1]) if len(sys.argv) > 1 else 1_000_000
steps = int(sys.argv[2]) if len(sys.argv) > 2 else 200
for label, pdf in cases():
    x0 = gs.sample_sphere_device(pdf.d - 1, n, seed=1).T
    row = []
    for mode in ("fast", "exact"):
        s = gs.ShrinkageSphericalSliceSampler(pdf, x0, 3521, mode=mode, placement="packed")
        name = s._lib.gsss_kernel_name(s._target_dev.handle, 1 if mode == "fast" else 0, 0, 1).decode()
        s.advance(20, keep=False)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        s.advance(steps, keep=False)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        row.append(f"{mode} {n * steps / dt:.3e} ({name})")
    print(f"{label}, {n} chains x {steps} steps: " + "   ".join(row), flush=True)

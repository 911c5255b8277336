#!/usr/bin/env python3
"""What the service phases of the lane kernel serve, from the A/B counter build (GSSS_COUNT_SERVICE, gsss_screen.h).

    tools/build_variant.sh count gsss_fast_vmf_d3.hip -DGSSS_COUNT_SERVICE     # -> geosss_amd/libgsss_count.so
    python tools/count_service.py [--lib geosss_amd/libgsss_count.so] [--workload vmfmix_readme] [--chains N]

Runs bench.py (one warm-up launch, one timed launch) under that library and sums the counter line every launch of the
instrumented kernel prints: the share of service phases that carry a double-precision decision, how many of the decisions
accept, lanes served per phase, and the phases in which every lane that set up a step held a certain accept that had sat idle
through a try iteration.
"""
import argparse
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYS = ["phases", "decide_phases", "decides", "decide_accepts", "finalised", "setups", "try_iters", "all_idle_accept_phases"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib", default=os.path.join(ROOT, "geosss_amd", "libgsss_count.so"))
    ap.add_argument("--workload", default="vmfmix_readme")
    ap.add_argument("--chains", type=int, default=1_000_000)
    ap.add_argument("--inner", type=int, default=1000)
    a = ap.parse_args()
    env = dict(os.environ, GSSS_HIP_LIB=os.path.abspath(a.lib))
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--workload", a.workload, "--chains", str(a.chains), "--inner",
           str(a.inner), "--steps", "1", "--warmup", "1"]
    out = subprocess.run(cmd, env=env, capture_output=True, text=True, check=True).stdout
    tot = dict.fromkeys(KEYS, 0)
    launches = 0
    for line in out.splitlines():
        if line.startswith("gsss-svc "):
            f = line.split()[1:]
            vals = dict(zip(f[0::2], map(int, f[1::2])))
            for k in KEYS:
                tot[k] += vals[k]
            launches += 1
    if launches == 0:
        sys.exit("no counter lines: is the library the GSSS_COUNT_SERVICE build?")
    steps = launches * a.chains * a.inner
    print(f"{a.workload}: {launches} launches, {steps:.3e} chain-steps, " + ", ".join(f"{k} {v}" for k, v in tot.items()))
    p = max(tot["phases"], 1)
    print(f"  service phases per chain-step          {tot['phases'] / steps:.4f}")
    print(f"  lanes finalised per phase              {tot['finalised'] / p:.2f}")
    print(f"  lanes set up per phase                 {tot['setups'] / p:.2f}")
    print(f"  phases with a decision                 {tot['decide_phases'] / p:.4f}")
    print(f"  decisions per chain-step               {tot['decides'] / steps:.5f}")
    print(f"  decisions that accept                  {tot['decide_accepts'] / max(tot['decides'], 1):.4f}")
    print(f"  phases whose set-ups all sat idle      {tot['all_idle_accept_phases'] / p:.4f}")
    print(f"  try iterations per service phase       {tot['try_iters'] / p:.3f}")


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Measure mcd_posterior_predictive on one GPU: one JSON line per workload, for profiles/.

    python tools/predictive_probe.py [--calls 10] [--cases all|small]

Each case builds a synthetic catalogue and draws S samples around the truth exactly as tools/posterior_probe.py does (its
`catalogue` and `samples`), and times the fused call: wall-clock median of `--calls` blocking calls after two warm-up
calls, and the HIP-event time of its kernels (option "timing", median of five calls).  Beside it, from the same run on the
same catalogue and samples, the kernel time of mcd_pointwise_posterior (membership on for the background models): the
summaries kernel whose decomposition this one shares.  `mixture` is on for the two models with a Gaussian background.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from mcmc_dynamics_amd import _native                 # noqa: E402
import posterior_probe as pp                           # noqa: E402

# (label, model, free centre, N, S)
CASES = [
    ("C3 catalogue (CONST_BGFIXED)", 1, False, 1000000, 4096),
    ("CONST_BGGAUSS", 2, False, 1000000, 1024),
    ("small catalogue, sliced (PROFILE_BGGAUSS, free centre)", 4, True, 10000, 4096),
]
MIX_MODELS = (2, 4)


def kernel_ms(gpu, call, repeats=5):
    gpu.set_option("timing", 1)
    ms = []
    for _ in range(repeats):
        call()
        ms.append(gpu.last_kernel_ms)
    gpu.set_option("timing", 0)
    return float(np.median(ms))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--cases", default="all", choices=["all", "small"])
    args = ap.parse_args()
    ctx = _native.default_context()
    cases = CASES if args.cases == "all" else [c for c in CASES if c[3] <= 100000]
    for label, model, free, n, S in cases:
        cat, truth, kw, centre = pp.catalogue(model, free, n)
        table = pp.samples(model, free, truth, S)
        gpu = _native.Catalog(ctx, cat["ra"], cat["dec"], cat["v"], cat["verr"], model=model, centre=centre, **kw)
        mix, mem = model in MIX_MODELS, model in pp.BG_MODELS

        def predictive():
            return gpu.posterior_predictive(table, mixture=mix)

        def pointwise():
            return gpu.pointwise_posterior(table, membership=mem)

        for _ in range(2):
            out = predictive()
            pointwise()
        wall = []
        for _ in range(args.calls):
            t0 = time.perf_counter()
            predictive()
            wall.append((time.perf_counter() - t0) * 1e3)
        k_pred, k_point = kernel_ms(gpu, predictive), kernel_ms(gpu, pointwise)
        terms = float(n) * S
        row = {"case": label, "model": pp.MODEL_NAMES[model], "free_centre": free, "mixture": mix, "n_stars": n,
               "n_samples": S, "ms": round(float(np.median(wall)), 3), "kernel_ms": round(k_pred, 3),
               "kernel_terms_per_s": terms / (k_pred * 1e-3), "pointwise_posterior_kernel_ms": round(k_point, 3),
               "pointwise_posterior_membership": mem, "kernel_ms_ratio": round(k_pred / k_point, 3),
               "finite_outputs": bool(all(np.all(np.isfinite(v)) for v in out.values())),
               "tail_fraction_of_pit": float(np.mean((out["pit"] < 0.025) | (out["pit"] > 0.975)))}
        print(json.dumps(row), flush=True)
        gpu.close()


if __name__ == "__main__":
    sys.exit(main())

#!/usr/bin/env python3
"""Measure mcd_psis_loo_expect on one GPU: one JSON line per workload, for profiles/.

    python tools/loo_expect_probe.py [--calls 5] [--cases all|small]

Each case builds a synthetic catalogue and draws S samples around the truth as tools/posterior_probe.py does, and times
the call with all outputs (the four predictive rows, pit_mix where the model has one, and the standardised parameters as
functions): two warm-up calls, then the median of the HIP-event kernel time (option "timing") and of the wall time of
`--calls` calls.  The baseline is the two calls it replaces on the same catalogue and samples, mcd_psis_loo and
mcd_posterior_predictive, and beside them the call with the functions only (one row per star: mcd_psis_loo's tiles).
`tiles` counts the term tiles of the default scratch budget by the plan of csrc/mcd_psis.h (psis_tile_stars_rows).
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
    ("CONST_BGGAUSS", 2, False, 10000, 16384),
]
MIX_MODELS = (2, 4)
KD = 20                                                # derived values per sample row (csrc/mcd_math.h)


def timed(gpu, call, calls):
    for _ in range(2):
        call()
    gpu.set_option("timing", 1)
    kernel, wall = [], []
    for _ in range(calls):
        t0 = time.perf_counter()
        call()
        wall.append((time.perf_counter() - t0) * 1e3)
        kernel.append(gpu.last_kernel_ms)
    gpu.set_option("timing", 0)
    return float(np.median(kernel)), float(np.median(wall))


def tiles(n, S, rows, k, n_func, budget_mb=2048, pass_len=65536):
    """Term tiles of one shard of n stars (psis_tile_stars_rows of csrc/mcd_psis.h with the driver's fixed part)."""
    fixed = min(S, pass_len) * k * 8 + S * KD * 8 + S * n_func * 8
    t = (budget_mb * 1048576 - fixed) // (S * 8 * rows)
    if t >= 64:
        t -= t % 64
    t = min(t, n)
    return -(-n // t)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--cases", default="all", choices=["all", "small"])
    args = ap.parse_args()
    ctx = _native.default_context()
    cases = CASES if args.cases == "all" else [c for c in CASES if c[3] <= 100000]
    for label, model, free, n, S in cases:
        cat, truth, kw, centre = pp.catalogue(model, free, n)
        table = pp.samples(model, free, truth, S)
        gpu = _native.Catalog(ctx, cat["ra"], cat["dec"], cat["v"], cat["verr"], model=model, centre=centre, **kw)
        mix = model in MIX_MODELS
        std = table.std(axis=0)
        func = np.where(std > 0, (table - table.mean(axis=0)) / np.where(std > 0, std, 1.0), 0.0)
        k_all, w_all = timed(gpu, lambda: gpu.psis_loo_expect(table, func=func, mixture=mix), args.calls)
        k_func, _ = timed(gpu, lambda: gpu.psis_loo_expect(table, func=func, predictive=False), args.calls)
        k_loo, w_loo = timed(gpu, lambda: gpu.psis_loo(table), args.calls)
        k_pred, w_pred = timed(gpu, lambda: gpu.posterior_predictive(table, mixture=mix), args.calls)
        out = gpu.psis_loo_expect(table, func=func, mixture=mix)
        rows = 6 if mix else 5
        row = {"case": label, "model": pp.MODEL_NAMES[model], "n_stars": n, "n_samples": S, "mixture": mix,
               "n_func": int(func.shape[1]), "rows_per_star": rows, "kernel_ms": round(k_all, 3), "ms": round(w_all, 3),
               "functions_only_kernel_ms": round(k_func, 3), "psis_loo_kernel_ms": round(k_loo, 3),
               "posterior_predictive_kernel_ms": round(k_pred, 3), "baseline_kernel_ms": round(k_loo + k_pred, 3),
               "baseline_ms": round(w_loo + w_pred, 3), "kernel_ms_ratio": round(k_all / (k_loo + k_pred), 3),
               "tiles": tiles(n, S, rows, table.shape[1], func.shape[1]), "tiles_psis_loo": tiles(n, S, 1, table.shape[1], 0),
               "finite_pit": bool(np.all(np.isfinite(out["pit"]))),
               "tail_fraction_of_loo_pit": float(np.mean((out["pit"] < 0.025) | (out["pit"] > 0.975)))}
        print(json.dumps(row), flush=True)
        gpu.close()


if __name__ == "__main__":
    sys.exit(main())

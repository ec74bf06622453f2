#!/usr/bin/env python
"""Times mcd_loglike_grad_batch against mcd_loglike_batch (option "fast_path" = 0: the plain kernels the gradient shares
its term with) on the C3 and m1 catalogues of bench.py: 1e6 synthetic stars x 256 walkers, ConstantFit + fixed Gaussian
background (K = 4) and the ModelFit profile (K = 6), fixed centre.

Protocol: untimed warm-up calls until the clocks have ramped, then the median (and min / max) over --calls >= 20 blocking
calls of two HIP-event intervals (option "timing"), which mean the same for both entry points:
    kernel_ms   mcd_last_kernel_ms: the main kernel alone (loglike_kernel / loglike_grad_kernel), no reduction
    device_ms   mcd_last_device_ms: the device sequence behind the staged table -- main kernel and fixed-order reduction;
                the gradient call's also holds the copy of its (1 + K) x W results to the host, the value call writes its W
                results through mapped memory inside the reduction
kernel_ratio and device_ratio are the gradient's median over the value's.  Prints one JSON line per workload; the
generators and catalogue builders are bench.py's own (imported, not copied).

    python tools/grad_probe.py [--stars N] [--walkers W] [--calls 25] [--warmup 10]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench                                                         # noqa: E402
from mcmc_dynamics_amd import _native as native, synthetic           # noqa: E402


def walkers_of(workload, n_walkers, truth):
    _, _, _, model, _, config = bench.WORKLOADS[workload]
    pos = synthetic.make_walkers(n_walkers, bench.NAMES4, truth, config=config)
    if model == "profile":               # a (30 arcsec) and r_peak (60 arcsec) balls, as bench.py draws them
        rng = np.random.default_rng(synthetic.WALKER_SEED_BASE + 100 + config)
        a_col = 30.0 * (1.0 + 0.05 * rng.normal(size=n_walkers))
        rp_col = 60.0 * (1.0 + 0.05 * rng.normal(size=n_walkers))
        pos = np.column_stack([pos[:, 0], pos[:, 1], a_col, pos[:, 2], pos[:, 3], rp_col])
    return np.ascontiguousarray(pos)


def timed(call, cat, warmup, calls):
    for _ in range(warmup):
        call()
    kernel, device = [], []
    for _ in range(calls):
        call()
        kernel.append(cat.last_kernel_ms)
        device.append(cat.last_device_ms)
    stats = lambda a: {"median": float(np.median(a)), "min": float(np.min(a)), "max": float(np.max(a))}
    return stats(kernel), stats(device)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--stars", type=int, default=None)
    ap.add_argument("--walkers", type=int, default=None)
    ap.add_argument("--calls", type=int, default=25)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--workloads", default="c3,m1")
    args = ap.parse_args()
    if args.calls < 20:
        ap.error("--calls must be at least 20")
    ctx = native.default_context()
    for workload in args.workloads.split(","):
        _, n_stars, n_walkers, model, _, config = bench.WORKLOADS[workload]
        n_stars, n_walkers = args.stars or n_stars, args.walkers or n_walkers
        cat = synthetic.make_catalog(n_stars, config=config, seed=synthetic.CATALOG_SEED_BASE + config,
                                     background=(model != "const"))
        pos = walkers_of(workload, n_walkers, cat["truth"])
        gpu = bench._build_catalog(native, ctx, synthetic, cat, model, "f64", None)
        gpu.set_option("fast_path", 0)
        gpu.set_option("timing", 1)
        k = pos.shape[1]
        value_k, value_d = timed(lambda: gpu.loglike(pos), gpu, args.warmup, args.calls)
        grad_k, grad_d = timed(lambda: gpu.loglike_grad(pos), gpu, args.warmup, args.calls)
        v, g = gpu.loglike_grad(pos)
        agree = float(np.max(np.abs(v - gpu.loglike(pos)) / np.maximum(np.abs(v), n_stars)))
        print(json.dumps({"probe": "grad_probe", "workload": workload, "model": model, "stars": n_stars, "walkers": n_walkers,
                          "k": k, "calls": args.calls, "warmup": args.warmup,
                          "value_kernel_ms": value_k, "grad_kernel_ms": grad_k, "value_device_ms": value_d,
                          "grad_device_ms": grad_d,
                          "kernel_ratio": grad_k["median"] / value_k["median"],
                          "device_ratio": grad_d["median"] / value_d["median"],
                          "finite_difference_value_calls": 2 * k, "value_agreement": agree,
                          "grad_finite": bool(np.all(np.isfinite(g)))}))
        gpu.close()


if __name__ == "__main__":
    main()

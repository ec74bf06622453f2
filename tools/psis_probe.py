#!/usr/bin/env python3
"""Measure mcd_psis_loo on one GPU: one JSON line per case.

    python tools/psis_probe.py [--calls 10] [--kernel-only] [--scratch-mb 256,2048]

Cases: the C3 catalogue (1e6 stars, CONST_BGFIXED, 4 096 samples) and 1e4 stars x 16 384 samples (CONST_BGGAUSS).  Each
is timed as a blocking call (median wall clock after two warm-up calls) and by the HIP events of its kernels (option
"timing": sample prep, term and tail kernels of every tile), for each scratch budget (option "loo_scratch_mb"), next to
mcd_pointwise_posterior on the same samples (the term arithmetic alone, section 3.7).  The per-kernel split of a run
comes from `rocprofv3 --kernel-trace --stats -- python tools/psis_probe.py --kernel-only --calls 3`.  The NumPy PSIS of
tests/psis_helper.py is timed on one core over a subset of the lnL matrix and scaled to all stars.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

from mcmc_dynamics_amd import _native     # noqa: E402
from posterior_probe import catalogue, samples, MODEL_NAMES     # noqa: E402

# (label, model, N, S)
CASES = [("C3 catalogue (CONST_BGFIXED)", 1, 1000000, 4096), ("small catalogue (CONST_BGGAUSS)", 2, 10000, 16384)]


def numpy_ms(gpu, table, n, n_stars=200):
    import psis_helper as psh
    lnl = np.array([gpu.loglike_per_star(row)[:n_stars] for row in table]).T
    t0 = time.perf_counter()
    psh.numpy_psis(lnl)
    return (time.perf_counter() - t0) * 1e3 * n / n_stars


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--kernel-only", action="store_true")
    ap.add_argument("--scratch-mb", default="256,2048")
    args = ap.parse_args()
    ctx = _native.default_context()
    for label, model, n, S in CASES:
        cat, truth, kw, centre = catalogue(model, False, n)
        table = samples(model, False, truth, S)
        gpu = _native.Catalog(ctx, cat["ra"], cat["dec"], cat["v"], cat["verr"], model=model, centre=centre, **kw)
        out = {"case": label, "model": MODEL_NAMES[model], "n_stars": n, "n_samples": S}
        for mb in (int(x) for x in args.scratch_mb.split(",")):
            gpu.set_option("loo_scratch_mb", mb)
            for _ in range(2):
                res = gpu.psis_loo(table)
            wall = []
            for _ in range(args.calls):
                t0 = time.perf_counter()
                gpu.psis_loo(table)
                wall.append((time.perf_counter() - t0) * 1e3)
            gpu.set_option("timing", 1)
            kms = []
            for _ in range(3):
                gpu.psis_loo(table)
                kms.append(gpu.last_kernel_ms)
            gpu.set_option("timing", 0)
            out["scratch_mb_{0}".format(mb)] = {"ms": round(float(np.median(wall)), 3),
                                               "kernel_ms": round(float(np.median(kms)), 3)}
        gpu.set_option("timing", 1)
        pk = []
        for _ in range(3):
            gpu.pointwise_posterior(table)
            pk.append(gpu.last_kernel_ms)
        gpu.set_option("timing", 0)
        out["pointwise_posterior_kernel_ms"] = round(float(np.median(pk)), 3)
        k = res["pareto_k"]
        out["pareto_k_median"] = float(np.median(k[np.isfinite(k)]))
        out["n_k_above_0.7"] = int(np.count_nonzero(k > 0.7))
        if not args.kernel_only:
            out["numpy_ms_extrapolated_one_core"] = round(numpy_ms(gpu, table, n), 0)
        print(json.dumps(out), flush=True)
        gpu.close()


if __name__ == "__main__":
    sys.exit(main())

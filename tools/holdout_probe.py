#!/usr/bin/env python3
"""Measurement instrument for the exact leave-out refits: what one mcd_holdout_loglike call costs for
E in {1, 8, 16} ensembles of 64 walkers, beside mcd_loglike_batch with the plain kernels (fast_path = 0) for the same
number of rows, and the wall time of a Runner.reloo of 16 stars.  No threshold is attached to any figure.

    python tools/holdout_probe.py --stars 100000
    python tools/holdout_probe.py --stars 1000000

One JSON line per run, printed and written to profiles/holdout_probe_<stars>.json.  The catalogue is bench.py's C3
(synthetic.make_catalog(config=3), CONST_BGFIXED, 4 free parameters = the kernel columns); the hold-out sets are the
singletons {0}, ..., {E - 1}.

Method.  Every timed shape is warmed up by two calls of its own (code objects loaded, plans and buffers built, pages
touched).  A timing is a host clock around one synchronous library call; each is repeated `--repeats` times alternating
the variants, and the line holds the median and the spread (min, max) in microseconds, and beside them the HIP-event time
of the main kernel alone (option "timing").  The reloo line times one Runner.reloo call -- sibling catalogue, E = 16
lock-stepped refits of `--reloo-steps` steps through the Python loop of BinnedSampler (two launches of 512 rows per step),
pointwise pass and diagnostics included -- after a short full-posterior chain and its loo()."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from mcmc_dynamics_amd import DataReader, _native as native, synthetic      # noqa: E402
from mcmc_dynamics_amd.analysis import ConstantFit                           # noqa: E402
from mcmc_dynamics_amd.background import Gaussian                            # noqa: E402

CENTRE = (synthetic.CENTER_RA_DEG, synthetic.CENTER_DEC_DEG)
NAMES = ["v_sys", "sigma_max", "v_maxx", "v_maxy"]


def spread(seconds):
    s = 1e6 * np.asarray(seconds)
    return {"us": round(float(np.median(s)), 1), "us_min": round(float(s.min()), 1), "us_max": round(float(s.max()), 1)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--stars", type=int, default=100000)
    ap.add_argument("--walkers", type=int, default=64)
    ap.add_argument("--repeats", type=int, default=15)
    ap.add_argument("--reloo-steps", type=int, default=200)
    ap.add_argument("--chain-steps", type=int, default=200)
    ap.add_argument("--no-reloo", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    w = a.walkers
    cols = synthetic.make_catalog(a.stars, config=3, background=True)
    tr = cols["truth"]
    bg = Gaussian(tr["v_back"], tr["sigma_back"])
    ctx = native.default_context()
    cat = native.Catalog(ctx, cols["ra"], cols["dec"], cols["v"], cols["verr"], model=native.MODEL_CONST_BGFIXED,
                         centre=CENTRE, lnlike_bg=bg(cols["v"], cols["verr"]), pmember=cols["pmember"])
    cat.set_option("timing", 1)
    line = {"tool": "tools/holdout_probe.py", "stars": a.stars, "walkers": w, "repeats": a.repeats, "shapes": {}}
    for n_sets in (1, 8, 16):
        rows = n_sets * w
        table = np.ascontiguousarray(synthetic.make_walkers(rows, NAMES, tr, config=3)).reshape(n_sets, w, 4)
        offs = np.arange(n_sets + 1, dtype=np.int64)

        def holdout():
            t0 = time.perf_counter()
            cat.holdout_loglike(offs, table, want_test=False)
            return time.perf_counter() - t0, cat.last_kernel_ms

        def plain():
            cat.set_option("fast_path", 0)
            t0 = time.perf_counter()
            cat.loglike(table.reshape(rows, 4))
            dt = time.perf_counter() - t0
            ms = cat.last_kernel_ms
            cat.set_option("fast_path", 1)
            return dt, ms

        for fn in (holdout, plain, holdout, plain):
            fn()
        times = {"holdout": [], "plain": []}
        for _ in range(a.repeats):
            times["holdout"].append(holdout())
            times["plain"].append(plain())
        shape = {"rows": rows}
        for name, t in times.items():
            shape[name] = dict(spread([x[0] for x in t]), kernel_us=round(1e3 * float(np.median([x[1] for x in t])), 1))
        shape["holdout_over_plain"] = round(shape["holdout"]["us"] / shape["plain"]["us"], 3)
        holdout()
        shape["launch"] = {k: v for k, v in cat.launch_info().items() if k in ("workgroups", "chunks")}
        line["shapes"]["{0}x{1}".format(n_sets, w)] = shape
    cat.close()

    if not a.no_reloo:
        fit = ConstantFit(DataReader({k: cols[k] for k in ("ra", "dec", "v", "verr", "pmember")}), background=bg, context=ctx)
        fit.parameters["ra_center"].set(value=CENTRE[0], fixed=True)
        fit.parameters["dec_center"].set(value=CENTRE[1], fixed=True)
        pos = synthetic.make_walkers(w, NAMES, tr, config=3)
        sampler = fit(n_walkers=w, n_steps=a.chain_steps, n_out=None, prefix=None, pos=pos)
        chain, n_burn = np.asarray(sampler.chain), a.chain_steps // 4
        loo = fit.loo(chain, n_burn)
        # the 16 largest FINITE k^ (a star whose term does not move with the parameters has no tail to fit and nothing to refit)
        k = np.where(np.isfinite(loo["pareto_k"]), loo["pareto_k"], -np.inf)
        stars = np.argsort(-k, kind="stable")[:16]
        t0 = time.perf_counter()
        re = fit.reloo(loo, chain, n_burn, stars=stars, n_walkers=w, n_steps=a.reloo_steps, refit_burn=a.reloo_steps // 4, seed=5)
        dt = time.perf_counter() - t0
        line["reloo"] = {"refits": int(stars.size), "walkers": w, "steps": a.reloo_steps, "seconds": round(dt, 3),
                         "ms_per_step": round(1e3 * dt / a.reloo_steps, 3), "n_bad_k_before": int(loo["n_bad_k"]),
                         "smallest_k_refitted": round(float(k[stars].min()), 3),
                         "n_bad_k_after": int(re["n_bad_k"]),
                         "largest_change_of_elpd_i": float("{0:.3e}".format(np.max(np.abs(re["pointwise"] - loo["pointwise"]))))}
        fit.close()
    text = json.dumps(line)
    print(text)
    out = a.out or os.path.join(ROOT, "profiles", "holdout_probe_{0}.json".format(a.stars))
    with open(out, "w") as fh:
        fh.write(text + "\n")


if __name__ == "__main__":
    main()

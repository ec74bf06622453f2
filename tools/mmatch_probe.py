#!/usr/bin/env python3
"""Measurement instrument for moment matching: the wall time of Runner.loo_moment_match for the 16 stars
with the largest finite Pareto k^ of bench.py's C3 catalogue at S = 4096 draws, the hold-out evaluations it makes, and
the wall time of a Runner.reloo of the same 16 stars beside it.  No threshold is attached to any figure.

    python tools/mmatch_probe.py --stars 100000

One JSON line, printed and written to profiles/mmatch_probe_<stars>.json (or --out).  The catalogue and the short
full-posterior chain are tools/holdout_probe.py's (synthetic.make_catalog(config=3), CONST_BGFIXED, 64 walkers); the
chain keeps 64 post-burn-in steps, i.e. S = 4096, so that the 16 stars are one lock-stepped group of 65536 rows.

Method.  Every timed call is warmed up once (code objects, plans, buffers), then repeated `--repeats` times; the line
holds the median and the spread of the host clock around the call.  On this catalogue the finite k^ lie below the
threshold, so the call as a user makes it ("default") stops after the baseline: one evaluation.  The loop is measured with
k_threshold = -inf ("forced"): every star then tries transforms until none lowers k^ or max_iters passes are made.  The
library does not count its launches; `rounds` is the HIP-event time of the hold-out main kernels of the whole call (option
"timing") over that of the one-evaluation call, i.e. the hold-out evaluations of the group, each of which evaluates the
rows of all 16 stars."""
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
    s = 1e3 * np.asarray(seconds)
    return {"ms": round(float(np.median(s)), 3), "ms_min": round(float(s.min()), 3), "ms_max": round(float(s.max()), 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--stars", type=int, default=100000)
    ap.add_argument("--walkers", type=int, default=64)
    ap.add_argument("--chain-steps", type=int, default=200)
    ap.add_argument("--kept-steps", type=int, default=64)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--max-iters", type=int, default=30)
    ap.add_argument("--reloo-steps", type=int, default=200)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    w = a.walkers
    cols = synthetic.make_catalog(a.stars, config=3, background=True)
    tr = cols["truth"]
    bg = Gaussian(tr["v_back"], tr["sigma_back"])
    ctx = native.default_context()
    fit = ConstantFit(DataReader({k: cols[k] for k in ("ra", "dec", "v", "verr", "pmember")}), background=bg, context=ctx)
    fit.parameters["ra_center"].set(value=CENTRE[0], fixed=True)
    fit.parameters["dec_center"].set(value=CENTRE[1], fixed=True)
    pos = synthetic.make_walkers(w, NAMES, tr, config=3)
    sampler = fit(n_walkers=w, n_steps=a.chain_steps, n_out=None, prefix=None, pos=pos)
    chain, n_burn = np.asarray(sampler.chain), a.chain_steps - a.kept_steps
    loo = fit.loo(chain, n_burn)
    k = np.where(np.isfinite(loo["pareto_k"]), loo["pareto_k"], -np.inf)
    stars = np.sort(np.argsort(-k, kind="stable")[:16])
    cat = fit._ensure_catalog()
    cat.set_option("timing", 1)
    line = {"tool": "tools/mmatch_probe.py", "stars": a.stars, "draws": int(loo["n_samples"]), "matched": int(stars.size),
            "repeats": a.repeats, "k_threshold": round(float(loo["k_threshold"]), 3),
            "k_of_the_matched": [round(float(k[stars].min()), 3), round(float(k[stars].max()), 3)]}
    results = {}
    for name, thr in (("default", None), ("forced", -np.inf)):
        def call():
            t0 = time.perf_counter()
            out = fit.loo_moment_match(loo, chain, n_burn, stars=stars, k_threshold=thr, max_iters=a.max_iters)
            return time.perf_counter() - t0, cat.last_kernel_ms, out
        call()
        runs = [call() for _ in range(a.repeats)]
        out = runs[-1][2]
        results[name] = dict(spread([r[0] for r in runs]), holdout_kernel_ms=round(float(np.median([r[1] for r in runs])), 3),
                             iterations=[int(i) for i in out["iterations"]],
                             accepted_per_level=[int(i) for i in out["accepted"].sum(axis=0)],
                             k_after=[round(float(out["pareto_k"][stars].min()), 3), round(float(out["pareto_k"][stars].max()), 3)],
                             largest_change_of_elpd_i=float("{0:.3e}".format(np.max(np.abs(out["pointwise"] - loo["pointwise"])))))
    one = results["default"]["holdout_kernel_ms"]
    for name in results:
        results[name]["rounds"] = round(results[name]["holdout_kernel_ms"] / one, 2)
    line["loo_moment_match"] = results
    cat.set_option("timing", 0)
    t0 = time.perf_counter()
    re = fit.reloo(loo, chain, n_burn, stars=stars, n_walkers=w, n_steps=a.reloo_steps, refit_burn=a.reloo_steps // 4, seed=5)
    dt = time.perf_counter() - t0
    line["reloo"] = {"refits": int(stars.size), "walkers": w, "steps": a.reloo_steps, "seconds": round(dt, 3),
                     "largest_change_of_elpd_i": float("{0:.3e}".format(np.max(np.abs(re["pointwise"] - loo["pointwise"]))))}
    fit.close()
    text = json.dumps(line)
    print(text)
    out = a.out or os.path.join(ROOT, "profiles", "mmatch_probe_{0}.json".format(a.stars))
    with open(out, "w") as fh:
        fh.write(text + "\n")


if __name__ == "__main__":
    main()

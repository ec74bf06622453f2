#!/usr/bin/env python3
"""Measurement instrument for the weighted value kernel and the bagged posterior: what one evaluation of
256 rows under per-row star weights costs through each route, and what a bagged run makes of it.  No threshold is attached
to any figure.

    python tools/bagged_probe.py --stars 100000
    python tools/bagged_probe.py --stars 1000000 --no-end-to-end

One JSON line per run, printed and written to profiles/bagged_probe_<stars>.json.  The catalogue is bench.py's C3
(synthetic.make_catalog(config=3), CONST_BGFIXED, 4 kernel columns), 256 parameter rows, one replicate per row.  Variants:

  a  grad_null     mcd_weighted_loglike_grad with grad = NULL, exponential weights: the gradient kernel, whose K extra sums
                   are computed and dropped -- the only route to these numbers before mcd_weighted_loglike
  b  exponential   mcd_weighted_loglike, Exp(1) weights
  c  poisson       mcd_weighted_loglike, Poisson(1) weights
  d  holdout       mcd_holdout_loglike with one empty set: the unweighted plain term over the same catalogue-order plan --
                   what the generator costs on top of the term

Method.  Every variant is warmed up by two calls of its own (code objects loaded, plans and buffers built, pages touched).
A timing is a host clock around one synchronous library call and, beside it, the HIP-event time of the main kernel alone
(option "timing"); each is repeated `--repeats` times, the variants taking turns, and the line holds the median and the
spread (min, max) of both in microseconds and the ratios of the medians b / a, c / a, b / d.

End to end (unless --no-end-to-end): Runner.bagged(64 bags, 64 walkers) on the same catalogue with ConstantFit and a fixed
Gaussian background, steps per second over `--steps` steps after a warm-up run, beside ConstantFit's own single-ensemble
run of 64 walkers (the `cf(...)` call of the examples) over the same number of steps: 64 such runs one after the other are
what the bags would cost without the lock step."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from mcmc_dynamics_amd import DataReader, _native as native, synthetic      # noqa: E402
from mcmc_dynamics_amd.background import Gaussian                            # noqa: E402

CENTRE = (synthetic.CENTER_RA_DEG, synthetic.CENTER_DEC_DEG)
NAMES = ["v_sys", "sigma_max", "v_maxx", "v_maxy"]


def spread(values, digits=1):
    s = np.asarray(values, dtype=np.float64)
    return {"us": round(float(np.median(s)), digits), "us_min": round(float(s.min()), digits), "us_max": round(float(s.max()), digits)}


def end_to_end(cols, bg, n_bags, n_walkers, n_steps, seed):
    from mcmc_dynamics_amd.analysis import ConstantFit
    data = DataReader({k: cols[k] for k in ("ra", "dec", "v", "verr", "pmember")})
    fit = ConstantFit(data, background=bg)
    fit.parameters["ra_center"].set(value=CENTRE[0], fixed=True)
    fit.parameters["dec_center"].set(value=CENTRE[1], fixed=True)
    try:
        pos = fit.get_initials(n_bags * n_walkers).reshape(n_bags, n_walkers, -1)
        fit.bagged(n_bags=n_bags, n_walkers=n_walkers, n_steps=8, n_burn=0, seed=seed, pos=pos)          # warm-up
        t0 = time.perf_counter()
        fit.bagged(n_bags=n_bags, n_walkers=n_walkers, n_steps=n_steps, n_burn=0, seed=seed, pos=pos)
        bagged_s = time.perf_counter() - t0
        fit(n_walkers=n_walkers, n_steps=8, n_out=None, prefix=None, pos=pos[0])                         # warm-up
        t0 = time.perf_counter()
        fit(n_walkers=n_walkers, n_steps=n_steps, n_out=None, prefix=None, pos=pos[0])
        single_s = time.perf_counter() - t0
    finally:
        fit.close()
    return {"bags": n_bags, "walkers": n_walkers, "steps": n_steps, "bagged_steps_per_s": round(n_steps / bagged_s, 1),
            "single_ensemble_steps_per_s": round(n_steps / single_s, 1),
            "sequential_equivalent_steps_per_s": round(n_steps / single_s / n_bags, 2),
            "bagged_over_sequential": round((n_steps / bagged_s) / (n_steps / single_s / n_bags), 2)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--stars", type=int, default=100000)
    ap.add_argument("--rows", type=int, default=256)
    ap.add_argument("--repeats", type=int, default=25)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--no-end-to-end", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    cols = synthetic.make_catalog(a.stars, config=3, background=True)
    tr = cols["truth"]
    bg = Gaussian(tr["v_back"], tr["sigma_back"])
    ctx = native.default_context()
    cat = native.Catalog(ctx, cols["ra"], cols["dec"], cols["v"], cols["verr"], model=native.MODEL_CONST_BGFIXED,
                         centre=CENTRE, lnlike_bg=bg(cols["v"], cols["verr"]), pmember=cols["pmember"])
    cat.set_option("timing", 1)
    table = np.ascontiguousarray(synthetic.make_walkers(a.rows, NAMES, tr, config=3))
    rep = np.arange(a.rows, dtype=np.int64)
    no_set = np.zeros(2, dtype=np.int64)

    def timed(call):
        t0 = time.perf_counter()
        call()
        return 1e6 * (time.perf_counter() - t0), 1e3 * cat.last_kernel_ms

    variants = {
        "grad_null": lambda: cat.weighted_loglike_grad(table, rep, scheme="exponential", seed=a.seed, want_grad=False),
        "exponential": lambda: cat.weighted_loglike(table, rep, scheme="exponential", seed=a.seed),
        "poisson": lambda: cat.weighted_loglike(table, rep, scheme="poisson", seed=a.seed),
        "holdout": lambda: cat.holdout_loglike(no_set, table[None, :, :], want_test=False),
    }
    for call in variants.values():
        call()
        call()
    times = {name: [] for name in variants}
    for _ in range(a.repeats):
        for name, call in variants.items():
            times[name].append(timed(call))
    line = {"tool": "tools/bagged_probe.py", "stars": a.stars, "rows": a.rows, "repeats": a.repeats, "model": "CONST_BGFIXED",
            "variants": {}}
    for name, t in times.items():
        line["variants"][name] = {"wall": spread([x[0] for x in t]), "kernel": spread([x[1] for x in t])}
    k = {name: v["kernel"]["us"] for name, v in line["variants"].items()}
    w = {name: v["wall"]["us"] for name, v in line["variants"].items()}
    line["kernel_ratios"] = {"exponential_over_grad_null": round(k["exponential"] / k["grad_null"], 3),
                             "poisson_over_grad_null": round(k["poisson"] / k["grad_null"], 3),
                             "exponential_over_holdout": round(k["exponential"] / k["holdout"], 3),
                             "poisson_over_holdout": round(k["poisson"] / k["holdout"], 3)}
    line["wall_ratios"] = {"exponential_over_grad_null": round(w["exponential"] / w["grad_null"], 3),
                           "poisson_over_grad_null": round(w["poisson"] / w["grad_null"], 3)}
    cat.close()
    if not a.no_end_to_end:
        line["end_to_end"] = end_to_end(cols, bg, 64, 64, a.steps, a.seed)
    text = json.dumps(line)
    print(text)
    out = a.out or os.path.join(ROOT, "profiles", "bagged_probe_{0}.json".format(a.stars))
    with open(out, "w") as fh:
        fh.write(text + "\n")


if __name__ == "__main__":
    main()

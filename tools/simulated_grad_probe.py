#!/usr/bin/env python3
"""Measurement instrument for the MAP fits of simulated catalogues: what the kernel of
csrc/mcd_simulated_grad.hip costs beside the plain gradient kernel and the simulated value kernel on the same rows, and what
`lrt` takes end to end.  No threshold is attached to any figure.

    python tools/simulated_grad_probe.py --stars 100000 --rows 256
    python tools/simulated_grad_probe.py --stars 2000 --rows 4096 --lrt 1024

One JSON line per run, printed and appended to profiles/simulated_grad_probe.txt.  The catalogue is bench.py's C3
(synthetic.make_catalog(config=3), CONST_BGFIXED with a fixed Gaussian background, 4 kernel columns); the rows are spread
over `--sims` simulations.  A timing is mcd_last_kernel_ms (option "timing": the HIP-event time of the main kernel alone);
every variant is warmed up by two calls of its own, then the variants take turns `--repeats` times and the line holds the
median and the spread (min, max) in microseconds.  `--lrt N`: the wall time of examples/run_lrt.py's lrt(n_sims=N) on its
rotating catalogue of 400 stars, warmed up by one lrt of 64 simulations."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from mcmc_dynamics_amd import _native as native, synthetic      # noqa: E402
from mcmc_dynamics_amd.background import Gaussian                # noqa: E402

CENTRE = (synthetic.CENTER_RA_DEG, synthetic.CENTER_DEC_DEG)
NAMES = ["v_sys", "sigma_max", "v_maxx", "v_maxy"]


def spread(values, digits=1):
    s = np.asarray(values, dtype=np.float64)
    return {"us": round(float(np.median(s)), digits), "us_min": round(float(s.min()), digits), "us_max": round(float(s.max()), digits)}


def lrt_wall(n_sims, seed):
    sys.path.insert(0, os.path.join(ROOT, "examples"))
    import run_lrt
    from mcmc_dynamics_amd.utils import calc_xy_offset
    cat = synthetic.make_catalog(400, config=2, background=False)
    truth = cat["truth"]
    rng = np.random.default_rng(3)
    dx, dy = calc_xy_offset(cat["ra"], cat["dec"], *CENTRE)
    theta = np.arctan2(dy, dx)
    noise = np.sqrt(np.asarray(cat["verr"]) ** 2 + truth["sigma_max"] ** 2) * rng.normal(size=400)
    cat = dict(cat, v=truth["v_sys"] + truth["v_maxx"] * np.sin(theta) - truth["v_maxy"] * np.cos(theta) + noise)
    full, null = run_lrt.make_fit(cat, True), run_lrt.make_fit(cat, False)
    try:
        full.lrt(null, n_sims=64, seed=seed)                                  # warm-up
        t0 = time.perf_counter()
        out = full.lrt(null, n_sims=n_sims, seed=seed)
        return {"n_sims": n_sims, "stars": 400, "wall_s": round(time.perf_counter() - t0, 3), "n_used": out["n_used"],
                "n_negative": out["n_negative"], "iterations_max": int(out["fits_full"]["n_iter"].max()),
                "p_value": round(out["p_value"], 5)}
    finally:
        full.close()
        null.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--stars", type=int, default=100000)
    ap.add_argument("--rows", type=int, default=256)
    ap.add_argument("--sims", type=int, default=16)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--lrt", type=int, default=0)
    ap.add_argument("--parent", default="")
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
    row_sim = np.arange(a.rows, dtype=np.int64) * a.sims // a.rows
    cat.simulate(table[:a.sims], a.seed, bg_mean=bg.mean, bg_sigma=bg.sigma, want_velocities=False)
    variants = {"simulated_grad": lambda: cat.simulated_loglike_grad(table, row_sim),
                "loglike_grad": lambda: cat.loglike_grad(table),
                "simulated_value": lambda: cat.simulated_loglike(table, row_sim)}
    times = {name: [] for name in variants}
    for call in variants.values():
        call()
        call()
    for _ in range(a.repeats):
        for name, call in variants.items():
            call()
            times[name].append(1e3 * cat.last_kernel_ms)
    line = {"tool": "tools/simulated_grad_probe.py", "parent": a.parent, "stars": a.stars, "rows": a.rows, "sims": a.sims,
            "repeats": a.repeats, "model": "CONST_BGFIXED", "kernel": {name: spread(t) for name, t in times.items()}}
    k = {name: v["us"] for name, v in line["kernel"].items()}
    line["kernel_ratios"] = {"simulated_grad_over_loglike_grad": round(k["simulated_grad"] / k["loglike_grad"], 3),
                             "simulated_grad_over_simulated_value": round(k["simulated_grad"] / k["simulated_value"], 3)}
    cat.close()
    if a.lrt > 0:
        line["lrt"] = lrt_wall(a.lrt, a.seed)
    text = json.dumps(line)
    print(text)
    with open(a.out or os.path.join(ROOT, "profiles", "simulated_grad_probe.txt"), "a") as fh:
        fh.write(text + "\n")


if __name__ == "__main__":
    main()

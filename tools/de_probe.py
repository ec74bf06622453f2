#!/usr/bin/env python3
"""Measurement instrument for the differential-evolution move: microseconds per step, acceptance, integrated
autocorrelation time of the slowest parameter and effective samples per second of the resident DE block against the
resident stretch block on the same catalogue, from the same start, over the same number of steps.  No threshold is attached
to any figure.

    python tools/de_probe.py --workload c3            # bench.py's C3 catalogue: CONST_BGFIXED, 4 parameters
    python tools/de_probe.py --workload m1            # bench.py's m1 catalogue: PROFILE, 6 parameters
    python tools/de_probe.py --workload free          # PROFILE_BGGAUSS with a free centre, 11 parameters (1e5 stars)

Per workload one JSON line, printed and written to profiles/de_probe_<workload>.json.  Catalogues, column orders, the MAP
and its Laplace ball (the start of both chains) and the autocorrelation estimator are tools/hmc_probe.py's.  Both moves run
`mcd_*_move_seeded` with 256 walkers: `--burn` steps that are dropped, then `--steps` timed steps whose rows are kept (default
3 000 / 5 000 / 6 000: fifty of the stretch chain's autocorrelation times as DESIGN 3.10 measured them).  DE runs with the
samplers' defaults, gamma0 = 2.38 / sqrt(2 P) and sigma = 1e-5.  ESS = walkers x steps / tau of the slowest parameter, per
second of the block's wall time."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from hmc_probe import autocorr_time, laplace, workload                 # noqa: E402
from mcmc_dynamics_amd import _native as native                        # noqa: E402
from mcmc_dynamics_amd.optimize import maximize_batch                  # noqa: E402
from mcmc_dynamics_amd.sampler import default_gamma0                   # noqa: E402

DEFAULT_STEPS = {"c3": 3000, "m1": 5000, "free": 6000}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="c3", choices=("c3", "m1", "free"))
    ap.add_argument("--stars", type=int, default=None)
    ap.add_argument("--walkers", type=int, default=256)
    ap.add_argument("--steps", type=int, default=None)
    ap.add_argument("--burn", type=int, default=500)
    ap.add_argument("--block", type=int, default=256, help="steps per library call")
    ap.add_argument("--seed", type=int, default=11)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    n_stars = a.stars if a.stars is not None else (100000 if a.workload == "free" else 1000000)
    steps = a.steps if a.steps is not None else DEFAULT_STEPS[a.workload]
    cols, kw, names, x_true, lo, hi, ball = workload(a.workload, n_stars)
    ctx = native.default_context()
    cat = native.Catalog(ctx, cols["ra"], cols["dec"], cols["v"], cols["verr"], **kw)
    p, w = len(names), a.walkers
    plan = {"col_source": np.arange(p, dtype=np.int32), "col_const": np.zeros(p), "col_factor": np.ones(p), "lo": lo,
            "hi": hi, "fixed_ok": True}

    def fn(rows):
        return cat.loglike_grad(np.ascontiguousarray(rows))

    rng = np.random.default_rng(a.seed)
    starts = np.clip(x_true + ball * rng.normal(size=(64, p)), lo, hi)
    res = maximize_batch(fn, starts, lo, hi, max_iter=200, gtol=1e-8)
    f = np.where(np.isfinite(res["f"]), res["f"], -np.inf)
    x_map = res["x"][int(np.argmax(f))]
    on_bound = bool(np.any(x_map <= lo) or np.any(x_map >= hi))
    hess = laplace(fn, np.clip(x_map, lo + 1e-9, hi - 1e-9) if on_bound else x_map, lo, hi)
    metric = "laplace"
    try:
        np.linalg.cholesky(-hess)
        cov = np.linalg.inv(-hess)
    except np.linalg.LinAlgError:
        metric = "diagonal 1/|H_jj| (-H not positive definite at the maximum found)"
        cov = np.diag(1.0 / np.maximum(np.abs(np.diag(hess)), 1e-300))
    pos0 = np.ascontiguousarray(np.clip(x_map + rng.normal(size=(w, p)) @ np.linalg.cholesky(cov).T, lo, hi))
    lnp0 = cat.loglike(pos0)
    g0 = float(default_gamma0(p))

    def block(move, pos, lnp, step0, n, chain, acc):
        if move == "de":
            cat.de_move_seeded(plan, pos, lnp, g0, 1e-5, a.seed, step0, n, chain, None, acc)
        else:
            cat.stretch_move_seeded(plan, pos, lnp, a.seed, step0, n, chain, None, acc)

    def run(move):
        pos, lnp = pos0.copy(), lnp0.copy()
        done = 0
        while done < a.burn:
            n = min(a.block, a.burn - done)
            block(move, pos, lnp, done, n, None, np.zeros(w, dtype=np.int64))
            done += n
        chain, acc = np.empty((steps, w, p)), np.zeros(w, dtype=np.int64)
        before = cat.de_info() if move == "de" else cat.stretch_info()
        t0 = time.perf_counter()
        at = 0
        while at < steps:
            n = min(a.block, steps - at)
            block(move, pos, lnp, a.burn + at, n, chain[at:at + n], acc)
            at += n
        seconds = time.perf_counter() - t0
        after = cat.de_info() if move == "de" else cat.stretch_info()
        tau = autocorr_time(chain, ctx)
        worst = float(np.nanmax(tau))
        return {"steps": steps, "burn": a.burn, "acceptance": round(float(acc.sum()) / (steps * w), 3),
                "us_per_step": round(1e6 * seconds / steps, 2),
                "blocks": {k: after[k] - before[k] for k in ("device_blocks", "host_blocks", "discarded_blocks")},
                "tau_steps": [round(float(v), 2) for v in tau], "slowest": names[int(np.nanargmax(tau))],
                "tau_slowest": round(worst, 2), "tau_reliable": bool(steps >= 50 * worst),
                "ess_per_s": round(w * steps / worst / seconds, 1)}

    run("stretch")                                                        # (arena sized, work set built, pages touched)
    line = {"tool": "tools/de_probe.py", "workload": a.workload, "stars": n_stars, "walkers": w, "parameters": names,
            "start": {"metric": metric, "on_bound": on_bound}, "gamma0": round(g0, 4), "sigma": 1e-5,
            "stretch": run("stretch"), "de": run("de")}
    line["tau_ratio_de_over_stretch"] = round(line["de"]["tau_slowest"] / line["stretch"]["tau_slowest"], 3)
    line["ess_per_s_ratio_de_over_stretch"] = round(line["de"]["ess_per_s"] / line["stretch"]["ess_per_s"], 3)
    text = json.dumps(line)
    print(text)
    out = a.out or os.path.join(ROOT, "profiles", "de_probe_{0}.json".format(a.workload))
    with open(out, "w") as fh:
        fh.write(text + "\n")
    cat.close()


if __name__ == "__main__":
    main()

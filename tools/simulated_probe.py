#!/usr/bin/env python3
"""Measurement instrument for the simulated catalogues: what the two kernels of csrc/mcd_simulated.hip cost, and
what the lock step makes of them.  No threshold is attached to any figure.

    python tools/simulated_probe.py --stars 100000 --parent <commit the comparison kernel is unchanged from>

One JSON line per run, printed and appended to profiles/simulated_probe.txt.  The catalogue is bench.py's C3
(synthetic.make_catalog(config=3), CONST_BGFIXED with a fixed Gaussian background, 4 kernel columns).

  value     mcd_simulated_loglike, 256 rows over 16 simulations, beside mcd_weighted_loglike with explicit weights at the
            same shape (16 replicates; csrc/mcd_weighted_value.hip, which this unit is modelled on line for line): the two
            differ by one subtraction and one gauss_lnl per term
  simulate  mcd_simulate, 256 simulations (no copy back), and its share of a 600-step sbc run of 256 catalogues x 32 walkers
            from the measured wall time per step of Runner.simulated_fits at that shape
  lockstep  the wall time per step of 16 lock-stepped simulated fits of 64 walkers beside 16 single-ensemble runs of 64
            walkers one after the other (the `cf(...)` call of the examples)

Method.  Every variant is warmed up by two calls of its own (code objects loaded, plans and buffers built, pages touched).
A kernel timing is the HIP-event time of the main kernel alone (option "timing") beside a host clock around the synchronous
library call; each is repeated `--repeats` times, the variants taking turns, and the line holds the median and the spread
(min, max) of both in microseconds."""
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


def make_fit(cols, bg):
    from mcmc_dynamics_amd.analysis import ConstantFit
    fit = ConstantFit(DataReader({k: cols[k] for k in ("ra", "dec", "v", "verr", "pmember")}), background=bg)
    fit.parameters["ra_center"].set(value=CENTRE[0], fixed=True)
    fit.parameters["dec_center"].set(value=CENTRE[1], fixed=True)
    return fit


def steps_per_second(fit, truths, n_walkers, n_steps, seed):
    fit.simulated_fits(truths, n_walkers=n_walkers, n_steps=8, n_burn=0, seed=seed)                       # warm-up
    t0 = time.perf_counter()
    fit.simulated_fits(truths, n_walkers=n_walkers, n_steps=n_steps, n_burn=0, seed=seed)
    return n_steps / (time.perf_counter() - t0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--stars", type=int, default=100000)
    ap.add_argument("--rows", type=int, default=256)
    ap.add_argument("--sims", type=int, default=16)
    ap.add_argument("--draw-sims", type=int, default=256)
    ap.add_argument("--repeats", type=int, default=25)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--parent", default="")
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
    truths = np.ascontiguousarray(synthetic.make_walkers(a.draw_sims, NAMES, tr, config=3))
    row_sim = np.repeat(np.arange(a.sims, dtype=np.int64), a.rows // a.sims)
    weights = np.random.default_rng(a.seed).exponential(size=(a.sims, a.stars))
    kw = dict(bg_mean=bg.mean, bg_sigma=bg.sigma)
    velocities = cat.simulate(truths[:a.sims], a.seed, **kw)

    def timed(call):
        t0 = time.perf_counter()
        call()
        return 1e6 * (time.perf_counter() - t0), 1e3 * cat.last_kernel_ms

    def draw():
        cat.simulate(truths, a.seed, want_velocities=False, **kw)

    def value():
        cat.simulated_loglike(table, row_sim)

    variants = {"weighted_explicit": lambda: cat.weighted_loglike(table, row_sim, scheme="explicit", weights=weights)}
    times = {"simulate": [], "simulated_value": [], "weighted_explicit": []}
    # (the draw replaces the resident set, so the value call gets its 16-simulation set back before its turn)
    for _ in range(2):
        draw()
        cat.simulated_set(velocities, **kw)
        value()
        variants["weighted_explicit"]()
    for _ in range(a.repeats):
        times["simulate"].append(timed(draw))
        cat.simulated_set(velocities, **kw)
        times["simulated_value"].append(timed(value))
        times["weighted_explicit"].append(timed(variants["weighted_explicit"]))
    line = {"tool": "tools/simulated_probe.py", "parent": a.parent, "stars": a.stars, "rows": a.rows, "sims": a.sims,
            "draw_sims": a.draw_sims, "repeats": a.repeats, "model": "CONST_BGFIXED", "variants": {}}
    for name, t in times.items():
        line["variants"][name] = {"wall": spread([x[0] for x in t]), "kernel": spread([x[1] for x in t])}
    k = {name: v["kernel"]["us"] for name, v in line["variants"].items()}
    line["kernel_ratios"] = {"simulated_value_over_weighted_explicit": round(k["simulated_value"] / k["weighted_explicit"], 3)}
    cat.close()
    if not a.no_end_to_end:
        fit = make_fit(cols, bg)
        try:
            sbc_rate = steps_per_second(fit, truths, 32, a.steps, a.seed)
            draw_s = 1e-6 * line["variants"]["simulate"]["wall"]["us"]
            line["sbc_600_steps"] = {"sims": a.draw_sims, "walkers": 32, "steps_per_s": round(sbc_rate, 2),
                                     "simulate_share": round(draw_s / (draw_s + 600.0 / sbc_rate), 6)}
            # (windows of about a second each: the lock step is some ten times slower per step than one ensemble)
            lock_steps, single_steps = 5 * a.steps, 50 * a.steps
            lock_rate = steps_per_second(fit, truths[:16], 64, lock_steps, a.seed)
            pos = fit.get_initials(64)
            fit(n_walkers=64, n_steps=8, n_out=None, prefix=None, pos=pos)                                # warm-up
            t0 = time.perf_counter()
            fit(n_walkers=64, n_steps=single_steps, n_out=None, prefix=None, pos=pos)
            single_rate = single_steps / (time.perf_counter() - t0)
            line["lockstep"] = {"sims": 16, "walkers": 64, "steps": lock_steps, "single_ensemble_steps": single_steps,
                                "lockstep_steps_per_s": round(lock_rate, 1),
                                "single_ensemble_steps_per_s": round(single_rate, 1),
                                "sequential_equivalent_steps_per_s": round(single_rate / 16, 2),
                                "lockstep_over_sequential": round(lock_rate / (single_rate / 16), 2)}
        finally:
            fit.close()
    text = json.dumps(line)
    print(text)
    with open(a.out or os.path.join(ROOT, "profiles", "simulated_probe.txt"), "a") as fh:
        fh.write(text + "\n")


if __name__ == "__main__":
    main()

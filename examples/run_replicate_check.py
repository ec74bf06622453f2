#!/usr/bin/env python3
"""Replicated-data predictive check per radial annulus: a synthetic cluster whose dispersion falls outwards (10 km/s
inside the median radius, 6 km/s outside) is fitted with `ConstantFit`, which has one dispersion for all stars.  The
pooled PIT histogram of `ppc` stays flat to within a few percent; `replicate_check` draws a replicated catalogue per
posterior sample on the device, compares the variance of the standardised residuals annulus by annulus, and shows the
inner annuli too hot and the outer ones too cold.  Needs an MI355X (gfx950) and the built library
(make -C mcmc_dynamics_amd/csrc).

    python examples/run_replicate_check.py [--stars 100000] [--walkers 64] [--steps 200] [--annuli 8]
"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mcmc_dynamics_amd import DataReader, synthetic                      # noqa: E402
from mcmc_dynamics_amd.analysis import ConstantFit                        # noqa: E402
from mcmc_dynamics_amd.utils import calc_xy_offset                        # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--stars", type=int, default=100000)
    ap.add_argument("--walkers", type=int, default=64)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--annuli", type=int, default=8)
    a = ap.parse_args()

    cat = synthetic.make_catalog(a.stars, config=3, background=False)    # truth: sigma = 10 km/s, v_max = 5 km/s
    dx, dy = calc_xy_offset(cat["ra"], cat["dec"], synthetic.CENTER_RA_DEG, synthetic.CENTER_DEC_DEG)
    r = np.hypot(dx, dy)
    outer = r > np.median(r)
    rng = np.random.default_rng(1)
    sigma = np.where(outer, 6.0, cat["truth"]["sigma_max"])
    # the outer stars' velocities are redrawn about the same rotation field with the smaller dispersion
    theta = np.arctan2(dy, dx)
    v_los = cat["truth"]["v_sys"] + cat["truth"]["v_maxx"] * np.sin(theta) - cat["truth"]["v_maxy"] * np.cos(theta)
    cat["v"] = np.where(outer, v_los + np.sqrt(cat["verr"] ** 2 + sigma ** 2) * rng.normal(size=a.stars), cat["v"])
    fit = ConstantFit(DataReader({k: cat[k] for k in ("ra", "dec", "v", "verr")}))
    fit.parameters["ra_center"].set(value=synthetic.CENTER_RA_DEG, fixed=True)
    fit.parameters["dec_center"].set(value=synthetic.CENTER_DEC_DEG, fixed=True)

    best = fit.maximize(n_starts=64)
    lap = fit.laplace(best["x"])
    pos = fit.get_initials_laplace(a.walkers, best["x"], lap["covariance"])
    sampler = fit(n_walkers=a.walkers, n_steps=a.steps, n_out=None, prefix=None, pos=pos)
    chain = np.asarray(sampler.chain)

    pooled = fit.ppc(chain, n_burn=a.steps // 4)
    print("pooled PIT histogram: chi2 = {0:.1f} over {1} bins, weight outside [0.025, 0.975]: {2:.4f}".format(
        pooled["chi2"], pooled["hist"].size, pooled["tail_fraction"]))
    t0 = time.perf_counter()
    out = fit.replicate_check(chain, n_burn=a.steps // 4, annuli=a.annuli, seed=7)
    dt = time.perf_counter() - t0
    print("replicate_check over {0} samples x {1} stars x {2} annuli in {3:.2f} s (seed {4})".format(
        out["n_samples"], int(out["n_stars"][0]), a.annuli, dt, out["seed"]))
    print("{0:>14s} {1:>8s} ".format("annulus", "stars") + " ".join("{0:>11s}".format(n) for n in out["names"]))
    labels = ["all"] + ["{0:.2f}-{1:.2f}'".format(lo, hi) for lo, hi in zip(out["edges"][:-1], out["edges"][1:])]
    for row, label in enumerate(labels):
        print("{0:>14s} {1:8d} ".format(label, int(out["n_stars"][row])) +
              " ".join("{0:11.3f}".format(p) for p in out["p_value"][row]))
    vi = out["names"].index("var_ratio")
    print("var_ratio, observed median against replicated 16 - 84 % band:")
    for row, label in enumerate(labels):
        b = out["bands"][row, vi]
        print("{0:>14s}  obs {1:.3f}   rep {2:.3f} .. {3:.3f}".format(label, b[0, 1], b[1, 0], b[1, 2]))
    fit.close()


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Weighted-likelihood bootstrap as a misspecification diagnostic: a synthetic cluster is fitted with `ConstantFit` twice,
once with the catalogue's honest velocity errors and once with a `verr` column understated by a factor (the velocities
scatter more than the catalogue admits).  `laplace()` gives the model-based width inv(-H) of the estimate; `bootstrap()`
refits the catalogue under random star weights -- all replicates as one lock-stepped optimisation on the device -- and
gives the width the estimate really has under resampling.  With honest errors the two agree (std_ratio about 1); with
understated errors the model-based width is too narrow and std_ratio rises well above 1 for the parameters that lean on
the error bars.  Needs an MI355X (gfx950) and the built library (make -C mcmc_dynamics_amd/csrc).

    python examples/run_bootstrap.py [--stars 20000] [--replicates 256] [--understate 3.0] [--scheme exponential]
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


def run(label, cat, verr, a):
    fit = ConstantFit(DataReader({"ra": cat["ra"], "dec": cat["dec"], "v": cat["v"], "verr": verr}))
    fit.parameters["ra_center"].set(value=synthetic.CENTER_RA_DEG, fixed=True)
    fit.parameters["dec_center"].set(value=synthetic.CENTER_DEC_DEG, fixed=True)
    best = fit.maximize(n_starts=64)
    t0 = time.perf_counter()
    out = fit.bootstrap(n_replicates=a.replicates, scheme=a.scheme, seed=a.seed, x_hat=best["x"])
    dt = time.perf_counter() - t0
    print("{0}: {1} replicates ({2}, seed {3}) in {4:.2f} s, {5} converged, at most {6} iterations".format(
        label, a.replicates, out["scheme"], out["seed"], dt, out["n_converged"], int(out["n_iter"].max())))
    lap_std = out["std"] / out["std_ratio"]
    print("{0:>12s} {1:>12s} {2:>12s} {3:>12s} {4:>10s} {5:>12s}".format("parameter", "estimate", "laplace std", "bootstrap std",
                                                                      "std_ratio", "bias"))
    for j, name in enumerate(out["names"]):
        print("{0:>12s} {1:12.4f} {2:12.4f} {3:12.4f} {4:10.3f} {5:12.4f}".format(name, best["x"][j], lap_std[j], out["std"][j],
                                                                                 out["std_ratio"][j], out["bias"][j]))
    fit.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--stars", type=int, default=20000)
    ap.add_argument("--replicates", type=int, default=256)
    ap.add_argument("--understate", type=float, default=3.0)
    ap.add_argument("--scheme", default="exponential", choices=["exponential", "poisson"])
    ap.add_argument("--seed", type=int, default=7)
    a = ap.parse_args()

    # Errors from well below to well above the dispersion (2 .. 50 km/s about sigma = 10 km/s), so that the error bars
    # matter to the fit; the velocities are redrawn about the catalogue's rotation field with exactly these errors.
    cat = synthetic.make_catalog(a.stars, config=3, background=False)
    truth = cat["truth"]
    rng = np.random.default_rng(2)
    dx, dy = calc_xy_offset(cat["ra"], cat["dec"], synthetic.CENTER_RA_DEG, synthetic.CENTER_DEC_DEG)
    theta = np.arctan2(dy, dx)
    v_los = truth["v_sys"] + truth["v_maxx"] * np.sin(theta) - truth["v_maxy"] * np.cos(theta)
    verr = 10.0 ** rng.uniform(0.3, 1.7, a.stars)
    cat["v"] = v_los + np.sqrt(verr ** 2 + truth["sigma_max"] ** 2) * rng.normal(size=a.stars)
    print("truth: v_sys {0:.2f}, sigma_max {1:.2f} km/s; {2} stars".format(truth["v_sys"], truth["sigma_max"], a.stars))
    honest = run("honest errors", cat, verr, a)
    wrong = run("errors understated by {0:g}".format(a.understate), cat, verr / a.understate, a)
    print("std_ratio, honest errors:      " + " ".join("{0:.3f}".format(r) for r in honest["std_ratio"]))
    print("std_ratio, understated errors: " + " ".join("{0:.3f}".format(r) for r in wrong["std_ratio"]))


if __name__ == "__main__":
    main()

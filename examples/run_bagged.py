#!/usr/bin/env python3
"""The bagged posterior ("BayesBag") against misspecification: a synthetic cluster is fitted with `ConstantFit` twice, once
with the catalogue's honest velocity errors and once with a `verr` column understated by a factor (the velocities scatter
more than the catalogue admits).  For each fit the script prints the standard posterior's intervals (one chain), the
bagged posterior's (`bagged()`: the same model on bootstrap-reweighted copies of the catalogue, all bags sampled in lock
step on the device and pooled) and `mismatch_ratio` = between-bag / within-bag variance, next to `bootstrap()`'s
`std_ratio` on the same catalogue.  With honest errors the ratio is about 1 and the bagged intervals are about sqrt(2)
times the standard ones; with understated errors the standard intervals are too narrow, the ratio rises well above 1 for
the parameters that lean on the error bars, and the bagged intervals widen with it.  Needs an MI355X (gfx950) and the
built library (make -C mcmc_dynamics_amd/csrc).

    python examples/run_bagged.py [--stars 20000] [--bags 64] [--walkers 64] [--steps 600] [--understate 3.0]
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
    burn = a.steps // 3
    best = fit.maximize(n_starts=64)
    lap = fit.laplace(best["x"])["covariance"]
    sampler = fit(n_walkers=a.walkers, n_steps=a.steps, n_out=None, prefix=None,
                  pos=fit.get_initials_laplace(a.walkers, best["x"], lap))
    draws = np.asarray(sampler.chain)[:, burn:, :].reshape(-1, len(best["x"]))
    t0 = time.perf_counter()
    bag = fit.bagged(n_bags=a.bags, n_walkers=a.walkers, n_steps=a.steps, n_burn=burn, scheme=a.scheme, seed=a.seed,
                     pos=fit.get_initials_laplace(a.bags * a.walkers, best["x"], lap).reshape(a.bags, a.walkers, -1))
    dt = time.perf_counter() - t0
    boot = fit.bootstrap(n_replicates=256, scheme=a.scheme, seed=a.seed, x_hat=best["x"])
    print("{0}: {1} bags x {2} walkers x {3} steps ({4}, seed {5}) in {6:.2f} s; {7} of {1} bags keep 50 tau".format(
        label, a.bags, a.walkers, a.steps, bag["scheme"], bag["seed"], dt, bag["n_converged"]))
    print("{0:>12s} {1:>22s} {2:>22s} {3:>10s} {4:>10s} {5:>10s}".format("parameter", "standard 16 .. 84 %", "bagged 16 .. 84 %",
                                                                      "std ratio", "mismatch", "bootstrap"))
    for j, name in enumerate(bag["names"]):
        lo, hi = np.percentile(draws[:, j], [16.0, 84.0])
        print("{0:>12s} {1:10.3f} ..{2:9.3f} {3:10.3f} ..{4:9.3f} {5:10.3f} {6:10.3f} {7:10.3f}".format(
            name, lo, hi, bag["percentiles"][16.0][j], bag["percentiles"][84.0][j], bag["std"][j] / draws[:, j].std(ddof=1),
            bag["mismatch_ratio"][j], boot["std_ratio"][j]))
    fit.close()
    return bag, boot


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--stars", type=int, default=20000)
    ap.add_argument("--bags", type=int, default=64)
    ap.add_argument("--walkers", type=int, default=64)
    ap.add_argument("--steps", type=int, default=600)
    ap.add_argument("--understate", type=float, default=3.0)
    ap.add_argument("--scheme", default="exponential", choices=["exponential", "poisson"])
    ap.add_argument("--seed", type=int, default=7)
    a = ap.parse_args()

    # Errors from well below to well above the dispersion (2 .. 50 km/s about sigma = 10 km/s), so that the error bars
    # matter to the fit; the velocities are redrawn about the catalogue's rotation field with exactly these errors
    # (the catalogue of examples/run_bootstrap.py).
    cat = synthetic.make_catalog(a.stars, config=3, background=False)
    truth = cat["truth"]
    rng = np.random.default_rng(2)
    dx, dy = calc_xy_offset(cat["ra"], cat["dec"], synthetic.CENTER_RA_DEG, synthetic.CENTER_DEC_DEG)
    theta = np.arctan2(dy, dx)
    v_los = truth["v_sys"] + truth["v_maxx"] * np.sin(theta) - truth["v_maxy"] * np.cos(theta)
    verr = 10.0 ** rng.uniform(0.3, 1.7, a.stars)
    cat["v"] = v_los + np.sqrt(verr ** 2 + truth["sigma_max"] ** 2) * rng.normal(size=a.stars)
    print("truth: v_sys {0:.2f}, sigma_max {1:.2f} km/s; {2} stars".format(truth["v_sys"], truth["sigma_max"], a.stars))
    honest, honest_boot = run("honest errors", cat, verr, a)
    wrong, wrong_boot = run("errors understated by {0:g}".format(a.understate), cat, verr / a.understate, a)
    fmt = lambda r: " ".join("{0:.3f}".format(x) for x in r)             # noqa: E731
    print("mismatch_ratio, honest errors:      " + fmt(honest["mismatch_ratio"]) + "   (bootstrap std_ratio^2: " +
          fmt(honest_boot["std_ratio"] ** 2) + ")")
    print("mismatch_ratio, understated errors: " + fmt(wrong["mismatch_ratio"]) + "   (bootstrap std_ratio^2: " +
          fmt(wrong_boot["std_ratio"] ** 2) + ")")


if __name__ == "__main__":
    main()

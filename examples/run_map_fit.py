#!/usr/bin/env python3
"""MAP fit, Laplace errors and a chain started from them: a synthetic cluster (rotation + dispersion, 20 % background
stars), `ConstantFit` with a fixed-Gaussian background and a fixed centre.  `maximize` climbs from 64 prior-ball starts on
the device gradient, `laplace` gives the covariance at the maximum, the walkers of a short chain start in that Gaussian
ball (no burn-in to speak of), and the two summaries are printed side by side.  Needs an MI355X (gfx950) and the built
library (make -C mcmc_dynamics_amd/csrc).

    python examples/run_map_fit.py [--stars 100000] [--walkers 64] [--steps 200]
"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mcmc_dynamics_amd import DataReader, Gaussian, synthetic          # noqa: E402
from mcmc_dynamics_amd.analysis import ConstantFit                      # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--stars", type=int, default=100000)
    ap.add_argument("--walkers", type=int, default=64)
    ap.add_argument("--steps", type=int, default=200)
    a = ap.parse_args()

    cat = synthetic.make_catalog(a.stars, config=3, background=True)     # truth: sigma = 10 km/s, v_max = 5 km/s
    data = DataReader({k: cat[k] for k in ("ra", "dec", "v", "verr", "pmember")})
    fit = ConstantFit(data, background=Gaussian(synthetic.TRUTH["v_back"], synthetic.TRUTH["sigma_back"]))
    fit.parameters["ra_center"].set(value=synthetic.CENTER_RA_DEG, fixed=True)
    fit.parameters["dec_center"].set(value=synthetic.CENTER_DEC_DEG, fixed=True)
    names = fit.fitted_parameters

    t0 = time.perf_counter()
    best = fit.maximize(n_starts=64)
    lap = fit.laplace(best["x"])
    dt = time.perf_counter() - t0
    sigma = np.sqrt(np.diag(lap["covariance"]))
    print("MAP from 64 starts ({0} converged, {1} iterations for the best) + Laplace in {2:.2f} s; lnprob = {3:.3f}".format(
        int(best["all_converged"].sum()), best["n_iter"], dt, best["lnprob"]))
    print("{0:>10s} {1:>12s} {2:>10s} {3:>10s}".format("parameter", "MAP", "sigma", "truth"))
    for n, x, s in zip(names, best["x"], sigma):
        print("{0:>10s} {1:12.4f} {2:10.4f} {3:10.4f}".format(n, x, s, cat["truth"][n]))

    pos = fit.get_initials_laplace(a.walkers, best["x"], lap["covariance"])
    t0 = time.perf_counter()
    sampler = fit(n_walkers=a.walkers, n_steps=a.steps, n_out=None, prefix=None, pos=pos)
    dt = time.perf_counter() - t0
    chain = np.asarray(sampler.chain)[:, a.steps // 4:, :].reshape(-1, len(names))
    lo, med, hi = np.percentile(chain, [16, 50, 84], axis=0)
    print("chain of {0} steps x {1} walkers started in the Laplace ball, {2:.2f} s, acceptance {3:.2f}".format(
        a.steps, a.walkers, dt, float(np.mean(sampler.acceptance_fraction))))
    print("{0:>10s} {1:>12s} {2:>10s} {3:>10s}".format("parameter", "median", "-", "+"))
    for n, m, l, h in zip(names, med, lo, hi):
        print("{0:>10s} {1:12.4f} {2:10.4f} {3:10.4f}".format(n, m, m - l, h - m))
    fit.close()


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""MAP -> Laplace -> Hamiltonian Monte Carlo -> best-fit table: a synthetic cluster (rotation + dispersion, 20 % background
stars), `ConstantFit` with a fixed-Gaussian background and a fixed centre.  `maximize` climbs from 64 prior-ball starts on
the device gradient, `laplace` gives the covariance at the maximum -- the metric of the sampler and the ball its chains
start in --, `Runner.hmc` adapts the step size during a short warm-up and samples, and the best-fit table of the chain is
printed beside the Laplace errors.  Needs an MI355X (gfx950) and the built library (make -C mcmc_dynamics_amd/csrc).

    python examples/run_hmc_fit.py [--stars 100000] [--walkers 64] [--steps 300] [--leap 8]
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
    ap.add_argument("--steps", type=int, default=300)
    ap.add_argument("--leap", type=int, default=8)
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
    sigma = np.sqrt(np.diag(lap["covariance"]))
    print("MAP from 64 starts ({0} converged) + Laplace in {1:.2f} s; lnprob = {2:.3f}".format(
        int(best["all_converged"].sum()), time.perf_counter() - t0, best["lnprob"]))

    pos = fit.get_initials_laplace(a.walkers, best["x"], lap["covariance"])
    t0 = time.perf_counter()
    sampler = fit.hmc(n_walkers=a.walkers, n_steps=a.steps, pos=pos, covariance=lap["covariance"], n_leap=a.leap)
    dt = time.perf_counter() - t0
    print("HMC: {0} chains x {1} steps x {2} leapfrog points in {3:.2f} s; step size {4:.3f} after warm-up, acceptance "
          "{5:.2f}, median |dH| {6:.3f}".format(a.walkers, a.steps, a.leap, dt, sampler.step_size,
                                                float(np.mean(sampler.acceptance_fraction)),
                                                float(np.median(sampler.energy_error))))
    table = fit.compute_bestfit_values(sampler.chain, n_burn=0)
    print(table)
    print("{0:>10s} {1:>12s} {2:>10s} {3:>12s} {4:>10s} {5:>10s}".format("parameter", "MAP", "Laplace", "median", "chain sd",
                                                                         "truth"))
    flat = sampler.flatchain
    for j, n in enumerate(names):
        print("{0:>10s} {1:12.4f} {2:10.4f} {3:12.4f} {4:10.4f} {5:10.4f}".format(
            n, best["x"][j], sigma[j], float(np.median(flat[:, j])), float(np.std(flat[:, j])), cat["truth"][n]))
    fit.close()


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""A run that stops itself when it has converged (emcee's documented pattern, here with the autocorrelation time computed
on the device beside the chain): a synthetic cluster, `ConstantFit` with a fixed centre, `Runner.run_converged`, and the
diagnostics table -- tau, effective sample size and split-R-hat per parameter.  Needs an MI355X (gfx950) and the built
library (make -C mcmc_dynamics_amd/csrc).

    python examples/run_convergence.py [--stars 100000] [--walkers 64] [--max-steps 20000] [--check-every 500]
"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mcmc_dynamics_amd import DataReader, synthetic                     # noqa: E402
from mcmc_dynamics_amd.analysis import ConstantFit                      # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--stars", type=int, default=100000)
    ap.add_argument("--walkers", type=int, default=64)
    ap.add_argument("--max-steps", type=int, default=20000)
    ap.add_argument("--check-every", type=int, default=500)
    ap.add_argument("--rtol", type=float, default=0.01)
    a = ap.parse_args()

    cat = synthetic.make_catalog(a.stars, config=3)                      # truth: sigma = 10 km/s, v_max = 5 km/s
    fit = ConstantFit(DataReader({k: cat[k] for k in ("ra", "dec", "v", "verr")}))
    fit.parameters["ra_center"].set(value=synthetic.CENTER_RA_DEG, fixed=True)
    fit.parameters["dec_center"].set(value=synthetic.CENTER_DEC_DEG, fixed=True)

    t0 = time.perf_counter()
    sampler, history = fit.run_converged(n_walkers=a.walkers, max_steps=a.max_steps, check_every=a.check_every, rtol=a.rtol)
    dt = time.perf_counter() - t0
    for steps, tau in history:
        print("{0:6d} steps: tau = {1}".format(steps, np.round(tau, 2)))
    steps, tau = history[-1]
    verdict = "converged" if steps < a.max_steps or steps > 50 * np.nanmax(tau) else "NOT converged at max_steps"
    print("{0} after {1} steps ({2:.2f} s, diagnostics included)".format(verdict, steps, dt))

    n_burn = int(2 * np.nanmax(tau))                                     # a few autocorrelation times of burn-in
    d = fit.chain_diagnostics(sampler.chain, n_burn=n_burn)
    print("{0:12s} {1:>8s} {2:>7s} {3:>10s} {4:>7s} {5:>12s} {6:>10s}".format("parameter", "tau", "window", "ess", "rhat", "mean", "std"))
    for i, name in enumerate(d["names"]):
        print("{0:12s} {1:8.2f} {2:7d} {3:10.0f} {4:7.4f} {5:12.5f} {6:10.5f}{7}".format(
            name, d["tau"][i], int(d["window"][i]), d["ess"][i], d["rhat"][i], d["mean"][i], d["std"][i],
            "" if d["converged"][i] else "   (chain shorter than 50 tau)"))
    print("truth:", {k: cat["truth"][k] for k in ("v_sys", "sigma_max", "v_maxx", "v_maxy")})
    fit.close()


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Informative priors on the device: a synthetic cluster fitted with `ModelFit` (Plummer dispersion profile, rotation, free
centre) under a log-normal prior on the scale radius `a` and normal priors on the centre -- what photometry would give --,
then MAP -> Laplace -> Hamiltonian Monte Carlo and the resident stretch move side by side.  The priors are evaluated by the
library (csrc/mcd_prior.h) inside the resident blocks; without them `a` is barely constrained by the kinematics and the
Laplace metric does not describe its marginal.  Needs an MI355X (gfx950) and the built library
(make -C mcmc_dynamics_amd/csrc).

    python examples/run_prior_fit.py [--stars 20000] [--walkers 64] [--steps 300]
"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mcmc_dynamics_amd import DataReader, synthetic                    # noqa: E402
from mcmc_dynamics_amd.analysis import ModelFit                          # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--stars", type=int, default=20000)
    ap.add_argument("--walkers", type=int, default=64)
    ap.add_argument("--steps", type=int, default=300)
    a = ap.parse_args()

    cat = synthetic.make_catalog(a.stars, config=3)
    fit = ModelFit(DataReader({k: cat[k] for k in ("ra", "dec", "v", "verr")}))
    pars = fit.parameters
    arcsec = 1.0 / 3600.0
    # the centre is known from photometry to 2 arcsec, the scale radius to a factor of 1.3
    pars["ra_center"].set(value=synthetic.CENTER_RA_DEG, prior=("normal", synthetic.CENTER_RA_DEG, 2.0 * arcsec / np.cos(np.radians(synthetic.CENTER_DEC_DEG))))
    pars["dec_center"].set(value=synthetic.CENTER_DEC_DEG, prior=("normal", synthetic.CENTER_DEC_DEG, 2.0 * arcsec))
    a_unit = pars["a"].unit
    a_guess = float(pars["a"].value)
    pars["a"].set(min=max(0.0, pars["a"].min), prior=("lognormal", float(np.log(a_guess)), float(np.log(1.3))))
    print("priors:", {n: p.prior for n, p in pars.items() if p.prior is not None}, "(a in {0})".format(a_unit))
    names = fit.fitted_parameters

    t0 = time.perf_counter()
    best = fit.maximize(n_starts=64)
    lap = fit.laplace(best["x"])
    sigma = np.sqrt(np.diag(lap["covariance"]))
    print("MAP from 64 starts ({0} converged) + Laplace in {1:.2f} s; lnprob = {2:.3f}".format(
        int(best["all_converged"].sum()), time.perf_counter() - t0, best["lnprob"]))

    pos = fit.get_initials_laplace(a.walkers, best["x"], lap["covariance"])
    t0 = time.perf_counter()
    hmc = fit.hmc(n_walkers=a.walkers, n_steps=a.steps, pos=pos, covariance=lap["covariance"])
    t_hmc = time.perf_counter() - t0
    fit.SAMPLER = "resident"
    t0 = time.perf_counter()
    stretch = fit(n_walkers=a.walkers, n_steps=4 * a.steps, pos=pos, prefix=None)
    t_stretch = time.perf_counter() - t0
    print("HMC: {0} steps in {1:.2f} s, acceptance {2:.2f}; resident stretch move: {3} steps in {4:.2f} s, acceptance {5:.2f}; "
          "blocks {6}".format(a.steps, t_hmc, float(np.mean(hmc.acceptance_fraction)), 4 * a.steps, t_stretch,
                              float(np.mean(stretch.acceptance_fraction)), fit._catalog.stretch_info()))
    flat_h = hmc.flatchain
    flat_s = np.asarray(stretch.chain)[:, a.steps:].reshape(-1, len(names))
    print("{0:>12s} {1:>14s} {2:>12s} {3:>14s} {4:>12s} {5:>14s} {6:>12s}".format("parameter", "MAP", "Laplace", "HMC median", "HMC sd",
                                                                                 "stretch median", "stretch sd"))
    for j, n in enumerate(names):
        print("{0:>12s} {1:14.6f} {2:12.6f} {3:14.6f} {4:12.6f} {5:14.6f} {6:12.6f}".format(
            n, best["x"][j], sigma[j], float(np.median(flat_h[:, j])), float(np.std(flat_h[:, j])),
            float(np.median(flat_s[:, j])), float(np.std(flat_s[:, j]))))
    fit.close()


if __name__ == "__main__":
    main()

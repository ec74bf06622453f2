#!/usr/bin/env python3
"""Posterior predictive check of a fitted model: a synthetic cluster (rotation + dispersion, 20 % background stars),
`ConstantFit` with a fixed-Gaussian background and a fixed centre.  A short chain is started in the Laplace ball of the
MAP fit; `ppc` then reduces its samples per star on the device -- standardised residuals, tail probabilities and the PIT
-- and the script prints the calibration summary (chi2 of the membership-weighted PIT histogram, the share of the weight
in the 5 % tails) and the ten members that contradict the model most (smallest tail_p): binary candidates and bad
measurements in a real catalogue.  Needs an MI355X (gfx950) and the built library (make -C mcmc_dynamics_amd/csrc).

    python examples/run_ppc.py [--stars 100000] [--walkers 64] [--steps 200]
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

    best = fit.maximize(n_starts=64)
    lap = fit.laplace(best["x"])
    pos = fit.get_initials_laplace(a.walkers, best["x"], lap["covariance"])
    sampler = fit(n_walkers=a.walkers, n_steps=a.steps, n_out=None, prefix=None, pos=pos)
    chain = np.asarray(sampler.chain)

    t0 = time.perf_counter()
    out = fit.ppc(chain, n_burn=a.steps // 4)
    dt = time.perf_counter() - t0
    print("ppc over {0} samples x {1} stars in {2:.2f} s".format(out["n_samples"], out["n_stars"], dt))
    print("chi2 of the PIT histogram ({0} bins, weight {1:.0f}): {2:.1f}; weight outside [0.025, 0.975]: {3:.4f} "
          "(0.05 when calibrated)".format(out["hist"].size, out["n"], out["chi2"], out["tail_fraction"]))
    print("{0} outliers with membership > 0.5 and tail_p < {1:.2e}".format(out["outliers"].size, out["outlier_p"]))
    members = np.flatnonzero(out["weight"] > 0.5)
    worst = members[np.argsort(out["tail_p"][members])[:10]]
    print("{0:>8s} {1:>10s} {2:>9s} {3:>9s} {4:>8s} {5:>8s} {6:>7s}".format("star", "tail_p", "z", "v", "v_los", "sigma", "p_mem"))
    for i in worst:
        print("{0:8d} {1:10.3e} {2:9.3f} {3:9.3f} {4:8.3f} {5:8.3f} {6:7.3f}".format(
            int(i), out["tail_p"][i], out["z_mean"][i], cat["v"][i], out["vlos_mean"][i], out["sigma_mean"][i],
            out["weight"][i]))
    fit.close()


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Simulation-based calibration and injection-recovery of `ConstantFit` on a synthetic cluster's positions and velocity
errors.  Three parts:

  1. `sbc()`: truths drawn from proper priors, one simulated catalogue each (drawn on the device, on the stars' own
     positions and errors), all fitted in lock step; the rank of every truth among its posterior draws must be uniform.
     The script prints the rank histogram, its chi2 and p-value per parameter.
  2. `recovery()` at v_rot = 0 and at v_rot = 0.1 sigma: bias, scatter and interval coverage of the fits, the bias of
     the rotation amplitude hypot(v_maxx, v_maxy) (positive by construction: the upper limit a non-detection supports),
     and how often rotation about the injected axis is "detected" (the 2.5 % quantile of v_maxx above its value at the
     null row, 0) -- the detection-power statement for these stars; at v_rot = 0 that share is the false-alarm rate.
  3. The same SBC with a deliberately broken fit: the fit is told a `verr` column half of what the simulations used (the
     catalogues come from the honest fit's `simulate`, the broken fit takes them through `velocities=`).  The histogram of
     sigma_max piles up at one end.

Needs an MI355X (gfx950) and the built library (make -C mcmc_dynamics_amd/csrc).

    python examples/run_sbc.py [--stars 2000] [--sims 256] [--walkers 32] [--steps 600]
"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mcmc_dynamics_amd import DataReader, synthetic                      # noqa: E402
from mcmc_dynamics_amd.analysis import ConstantFit                        # noqa: E402
from mcmc_dynamics_amd.analysis.runner import sbc_summary                 # noqa: E402


def make_fit(cat, verr):
    fit = ConstantFit(DataReader({"ra": cat["ra"], "dec": cat["dec"], "v": cat["v"], "verr": verr}))
    fit.parameters["ra_center"].set(value=synthetic.CENTER_RA_DEG, fixed=True)
    fit.parameters["dec_center"].set(value=synthetic.CENTER_DEC_DEG, fixed=True)
    # proper priors: what sbc() draws its truths from
    fit.parameters["v_sys"].set(min=-50.0, max=50.0, prior=("normal", 0.0, 10.0))
    fit.parameters["sigma_max"].set(min=0.5, max=60.0, prior=("lognormal", np.log(10.0), 0.4))
    fit.parameters["v_maxx"].set(min=-30.0, max=30.0, prior=("normal", 0.0, 3.0))
    fit.parameters["v_maxy"].set(min=-30.0, max=30.0, prior=("normal", 0.0, 3.0))
    return fit


def show_ranks(label, s, names):
    print("{0}: {1} catalogues, {2} draws per fit (thin {3}); uniform expectation {4:.1f} per bin".format(
        label, s["n_sims"], s["n_draws"], s["thin"], s["expected"][0]))
    for j, name in enumerate(names):
        print("{0:>12s}  {1}  chi2 {2:7.2f} (dof {3})  p {4:.4f}  max |ECDF - uniform| {5:.3f}  contraction {6:.3f}".format(
            name, " ".join("{0:4d}".format(int(h)) for h in s["hist"][j]), s["chi2"][j], s["dof"], s["p_value"][j], s["ecdf_max"][j],
            s["contraction"][j]))


def show_recovery(label, r):
    print("{0}: {1} catalogues".format(label, r["n_sims"]))
    for j, name in enumerate(r["names"]):
        print("{0:>12s}  truth {1:8.3f}  bias {2:8.3f}  scatter {3:7.3f}  rmse {4:7.3f}  coverage 68 % {5:.3f} +- {6:.3f}  95 % {7:.3f}"
              "  z {8:6.3f} +- {9:.3f}".format(name, r["truth"][j], r["bias"][j], r["scatter"][j], r["rmse"][j], r["coverage"][68][j],
                                               r["coverage_se"][68][j], r["coverage"][95][j], r["z_mean"][j], r["z_std"][j]))
    f, g = r["functions"]["v_rot"], r["functions"]["v_axis"]
    print("{0:>12s}  truth {1:8.3f}  bias {2:8.3f}  rmse {3:7.3f}".format("v_rot", f["truth"], f["bias"], f["rmse"]))
    print("{0:>12s}  truth {1:8.3f}  detected (2.5 % quantile above the null's {2:.2f}) in {3:.1%} of the fits".format(
        "v_axis", g["truth"], g["null"], g["exceeds"]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--stars", type=int, default=2000)
    ap.add_argument("--sims", type=int, default=256)
    ap.add_argument("--walkers", type=int, default=32)
    ap.add_argument("--steps", type=int, default=600)
    ap.add_argument("--seed", type=int, default=7)
    a = ap.parse_args()
    burn = a.steps // 3
    cat = synthetic.make_catalog(a.stars, config=3, background=False)
    verr = 10.0 ** np.random.default_rng(2).uniform(0.3, 1.3, a.stars)                    # 2 .. 20 km/s about sigma = 10 km/s
    fit = make_fit(cat, verr)
    names = fit.fitted_parameters

    # 1. calibration of the honest fit
    t0 = time.perf_counter()
    sbc = fit.sbc(n_sims=a.sims, n_walkers=a.walkers, n_steps=a.steps, n_burn=burn, seed=a.seed, n_bins=8)
    print("sbc: {0} catalogues x {1} walkers x {2} steps in {3:.2f} s; {4} fits keep 50 tau".format(
        a.sims, a.walkers, a.steps, time.perf_counter() - t0, int(sbc["fits"]["converged"].sum())))
    show_ranks("honest fit", sbc, names)

    # 2. recovery with and without rotation
    rot = {"v_rot": lambda t: np.hypot(t[:, names.index("v_maxx")], t[:, names.index("v_maxy")]),
           "v_axis": lambda t: t[:, names.index("v_maxx")]}
    null = np.array([0.0, 10.0, 0.0, 0.0])
    for v_rot in (0.0, 1.0):
        truth = np.array([0.0, 10.0, v_rot, 0.0])
        r = fit.recovery(truth, n_sims=min(a.sims, 64), n_walkers=a.walkers, n_steps=a.steps, n_burn=burn, seed=a.seed,
                         functions=rot, null=null)
        show_recovery("recovery at v_rot = {0:g} km/s (sigma = 10 km/s)".format(v_rot), r)

    # 3. the broken variant: the same catalogues, fitted with half the errors
    broken = make_fit(cat, 0.5 * verr)
    fits = broken.simulated_fits(sbc["truths"], n_walkers=a.walkers, n_steps=a.steps, n_burn=burn, seed=a.seed,
                                 velocities=sbc["fits"]["velocities"])
    show_ranks("fit told verr / 2", sbc_summary(fits["sampler"].chain, sbc["truths"], burn, n_bins=8,
                                                prior_variance=broken.prior_variance()), names)
    fit.close()
    broken.close()


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Leave-one-out checks of a fitted model: a small synthetic cluster (rotation + dispersion, no background) with one
star moved four sigma off the model, `ConstantFit` with a fixed centre, a short chain started in the Laplace ball of the
MAP fit.  `loo_pit` judges every star by the fit without it (the LOO-PIT histogram and its chi2, beside the posterior PIT
of `ppc`, which uses the data twice); `loo_influence` lists the stars the fit hinges on: by how many posterior standard
deviations every parameter, and the rotation amplitude, move when the star is removed.  Needs an MI355X (gfx950) and the
built library (make -C mcmc_dynamics_amd/csrc).

    python examples/run_loo_checks.py [--stars 300] [--walkers 64] [--steps 200]
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mcmc_dynamics_amd import DataReader, synthetic                     # noqa: E402
from mcmc_dynamics_amd.analysis import ConstantFit                      # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--stars", type=int, default=300)
    ap.add_argument("--walkers", type=int, default=64)
    ap.add_argument("--steps", type=int, default=200)
    a = ap.parse_args()

    cat = synthetic.make_catalog(a.stars, config=3)                      # truth: sigma = 10 km/s, v_max = 5 km/s
    planted = 7
    cat["v"][planted] += 4.0 * np.hypot(10.0, cat["verr"][planted])      # a binary candidate
    fit = ConstantFit(DataReader({k: cat[k] for k in ("ra", "dec", "v", "verr")}))
    fit.parameters["ra_center"].set(value=synthetic.CENTER_RA_DEG, fixed=True)
    fit.parameters["dec_center"].set(value=synthetic.CENTER_DEC_DEG, fixed=True)

    best = fit.maximize(n_starts=64)
    lap = fit.laplace(best["x"])
    pos = fit.get_initials_laplace(a.walkers, best["x"], lap["covariance"])
    sampler = fit(n_walkers=a.walkers, n_steps=a.steps, n_out=None, prefix=None, pos=pos)
    chain, n_burn = np.asarray(sampler.chain), a.steps // 4

    post, loo = fit.ppc(chain, n_burn, n_bins=10), fit.loo_pit(chain, n_burn, n_bins=10)
    print("{0} samples x {1} stars; {2} stars with k^ above {3:.2f}".format(loo["n_samples"], loo["n_stars"], loo["n_bad_k"],
                                                                           loo["k_threshold"]))
    for name, r in (("posterior PIT", post), ("LOO-PIT", loo)):
        print("{0:14s} chi2 ({1} bins) {2:6.1f}   weight outside [0.025, 0.975]: {3:.4f} (0.05 when calibrated)".format(
            name, r["hist"].size, r["chi2"], r["tail_fraction"]))

    names = list(fit.fitted_parameters)
    ix, iy = names.index("v_maxx"), names.index("v_maxy")
    functions = {n: (lambda t, q=q: t[:, q]) for q, n in enumerate(names)}
    functions["v_rot"] = lambda t: np.hypot(t[:, ix], t[:, iy])
    inf = fit.loo_influence(chain, n_burn, functions=functions)
    print("shift of the posterior mean when the star is removed, in posterior standard deviations:")
    print("{0:>6s} {1:>7s} ".format("star", "k^") + " ".join("{0:>10s}".format(n) for n in inf["names"]))
    for i in inf["ranking"][:8]:
        print("{0:6d} {1:7.2f} ".format(int(i), inf["pareto_k"][i]) + " ".join("{0:10.3f}".format(x) for x in inf["shift"][i]))
    print("planted star: {0}".format(planted))
    fit.close()


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Exact leave-out refits where PSIS-LOO gives up: a small synthetic cluster (rotation + dispersion, no background) with a
few stars moved many sigma off the model -- binaries, bad velocities -- and `ConstantFit` with a fixed centre.  `loo` flags
the planted stars by their Pareto k^; `reloo` refits without each of them, all refits in lock step on the device, and puts
the exact leave-one-out value in place of the PSIS estimate; `kfold` cross-validates every star by K refits.  Needs an
MI355X (gfx950) and the built library (make -C mcmc_dynamics_amd/csrc).

    python examples/run_reloo.py [--stars 300] [--walkers 64] [--steps 3000] [--folds 5]
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mcmc_dynamics_amd import DataReader, synthetic                     # noqa: E402
from mcmc_dynamics_amd.analysis import ConstantFit                      # noqa: E402
from mcmc_dynamics_amd.analysis.runner import elpd_compare              # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--stars", type=int, default=300)
    ap.add_argument("--walkers", type=int, default=64)
    ap.add_argument("--steps", type=int, default=3000)
    ap.add_argument("--folds", type=int, default=5)
    a = ap.parse_args()

    cat = synthetic.make_catalog(a.stars, config=3)                      # truth: sigma = 10 km/s, v_max = 5 km/s
    planted = {7: 9.0, 41: -8.0, 123: 7.0}                               # star -> offset in units of its own sigma
    for i, z in planted.items():
        cat["v"][i] += z * np.hypot(10.0, cat["verr"][i])
    fit = ConstantFit(DataReader({k: cat[k] for k in ("ra", "dec", "v", "verr")}))
    fit.parameters["ra_center"].set(value=synthetic.CENTER_RA_DEG, fixed=True)
    fit.parameters["dec_center"].set(value=synthetic.CENTER_DEC_DEG, fixed=True)

    best = fit.maximize(n_starts=64)
    pos = fit.get_initials_laplace(a.walkers, best["x"], fit.laplace(best["x"])["covariance"])
    sampler = fit(n_walkers=a.walkers, n_steps=a.steps, n_out=None, prefix=None, pos=pos)
    chain, n_burn = np.asarray(sampler.chain), a.steps // 4

    loo = fit.loo(chain, n_burn)
    print("PSIS-LOO: elpd {0:.2f} +- {1:.2f}, {2} stars with k^ above {3:.2f}".format(loo["elpd_loo"], loo["se"], loo["n_bad_k"],
                                                                                   loo["k_threshold"]))
    stars = np.argsort(-loo["pareto_k"], kind="stable")[:max(len(planted), loo["n_bad_k"])]
    re = fit.reloo(loo, chain, n_burn, stars=stars, n_walkers=a.walkers, n_steps=a.steps, refit_burn=n_burn, seed=1)
    print("reloo:    elpd {0:.2f} +- {1:.2f}, {2} stars still rely on PSIS".format(re["elpd_loo"], re["se"], re["n_bad_k"]))
    print("{0:>6s} {1:>7s} {2:>10s} {3:>10s} {4:>8s}".format("star", "k^", "psis", "exact", "planted"))
    for i in re["refit"]:
        print("{0:6d} {1:7.2f} {2:10.3f} {3:10.3f} {4:>8s}".format(int(i), loo["pareto_k"][i], loo["pointwise"][i],
                                                                  re["pointwise"][i], "yes" if int(i) in planted else ""))
    kf = fit.kfold(n_folds=a.folds, seed=2, n_walkers=a.walkers, n_steps=a.steps, n_burn=n_burn)
    print("{0}-fold:   elpd {1:.2f} +- {2:.2f}; refits converged: {3} of {0}".format(kf["n_folds"], kf["elpd_kfold"], kf["se"],
                                                                                  int(np.sum(kf["converged"]))))
    d = elpd_compare(kf, re)
    print("k-fold minus reloo: {0:.2f} +- {1:.2f} over {2} stars".format(d["elpd_diff"], d["se_diff"], d["n_stars"]))
    fit.close()


if __name__ == "__main__":
    main()

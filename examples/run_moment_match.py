#!/usr/bin/env python3
"""Moment matching before a refit: a small synthetic cluster (rotation + dispersion, no background) with a few stars moved
many sigma off the model, and `ConstantFit` with a fixed centre.  `loo` flags the planted stars by their Pareto k^;
`loo_moment_match` moves the posterior draws towards each flagged star's leave-one-out posterior on the device -- a few
hold-out evaluations per star instead of an MCMC run -- and `reloo` then refits only the stars whose k^ is still above the
threshold.  A full `reloo` of the same stars is run beside it for comparison.  Needs an MI355X (gfx950) and the built
library (make -C mcmc_dynamics_amd/csrc).

    python examples/run_moment_match.py [--stars 300] [--walkers 64] [--steps 3000]
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
    thin = max(1, (a.steps - n_burn) * a.walkers // 65536 + 1)           # moment matching takes at most 65536 draws

    loo = fit.loo(chain, n_burn, thin=thin)
    print("PSIS-LOO:        elpd {0:.2f} +- {1:.2f}, {2} stars with k^ above {3:.2f}".format(loo["elpd_loo"], loo["se"],
                                                                                          loo["n_bad_k"], loo["k_threshold"]))
    stars = np.argsort(-loo["pareto_k"], kind="stable")[:max(len(planted), loo["n_bad_k"])]
    # 0.5 is where PSIS starts to lose accuracy (Vehtari et al. 2017): match every star above it, not only the flagged ones
    mm = fit.loo_moment_match(loo, chain, n_burn, thin=thin, stars=stars, k_threshold=0.5)
    print("moment matching: elpd {0:.2f} +- {1:.2f}, {2} stars still above the threshold".format(mm["elpd_loo"], mm["se"],
                                                                                              mm["n_bad_k"]))
    exact = fit.reloo(loo, chain, n_burn, stars=stars, n_walkers=a.walkers, n_steps=a.steps, refit_burn=n_burn, seed=1)
    print("{0:>6s} {1:>7s} {2:>7s} {3:>6s} {4:>10s} {5:>10s} {6:>10s} {7:>8s}".format("star", "k^", "k^ mm", "passes", "psis",
                                                                                    "matched", "refit", "planted"))
    for e, i in enumerate(mm["matched"]):
        print("{0:6d} {1:7.2f} {2:7.2f} {3:6d} {4:10.3f} {5:10.3f} {6:10.3f} {7:>8s}".format(
            int(i), loo["pareto_k"][i], mm["pareto_k"][i], int(mm["iterations"][e]), loo["pointwise"][i], mm["pointwise"][i],
            exact["pointwise"][i], "yes" if int(i) in planted else ""))
    # the refits that moment matching leaves to do
    rest = fit.reloo(mm, chain, n_burn, n_walkers=a.walkers, n_steps=a.steps, refit_burn=n_burn, seed=1)
    print("reloo after moment matching refitted {0} stars; reloo alone {1}".format(rest["refit"].size, exact["refit"].size))
    d = elpd_compare(rest, exact)
    print("difference of the two totals: {0:.3f} +- {1:.3f} over {2} stars".format(d["elpd_diff"], d["se_diff"], d["n_stars"]))
    fit.close()


if __name__ == "__main__":
    main()

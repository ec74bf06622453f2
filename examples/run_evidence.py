#!/usr/bin/env python3
"""Does this cluster rotate?  A Bayes factor by parallel tempering: a synthetic cluster (rotation amplitude 5 km/s,
dispersion 10 km/s, no background), `ConstantFit` with a fixed centre and every free parameter in a finite box (a proper
prior: the ladder then ends at beta = 0 and anchors the evidence), once with the rotation components v_maxx, v_maxy free
and once with both fixed to zero.  `Runner.tempered` samples each model on a ladder of inverse temperatures,
`log_evidence` turns the rungs' log-likelihood series into log Z by the stepping-stone estimator, and `bayes_factor`
prints log Z(rotating) - log Z(non-rotating) with its error.  Needs an MI355X (gfx950) and the built library
(make -C mcmc_dynamics_amd/csrc).

    python examples/run_evidence.py [--stars 500] [--temps 20] [--walkers 64] [--steps 1500]
"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mcmc_dynamics_amd import DataReader, synthetic                     # noqa: E402
from mcmc_dynamics_amd.analysis import ConstantFit                      # noqa: E402
from mcmc_dynamics_amd.analysis.runner import bayes_factor              # noqa: E402

BOX = {"v_sys": (-20.0, 20.0), "sigma_max": (1.0, 30.0), "v_maxx": (-20.0, 20.0), "v_maxy": (-20.0, 20.0)}


def model(cat, rotating):
    fit = ConstantFit(DataReader({k: cat[k] for k in ("ra", "dec", "v", "verr")}))
    fit.parameters["ra_center"].set(value=synthetic.CENTER_RA_DEG, fixed=True)
    fit.parameters["dec_center"].set(value=synthetic.CENTER_DEC_DEG, fixed=True)
    for name, (lo, hi) in BOX.items():
        fit.parameters[name].set(min=lo, max=hi)
    if not rotating:
        fit.parameters["v_maxx"].set(value=0.0, fixed=True)
        fit.parameters["v_maxy"].set(value=0.0, fixed=True)
    return fit


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--stars", type=int, default=500)
    ap.add_argument("--temps", type=int, default=20)
    ap.add_argument("--walkers", type=int, default=64)
    ap.add_argument("--steps", type=int, default=1500)
    ap.add_argument("--seed", type=int, default=7)
    a = ap.parse_args()

    cat = synthetic.make_catalog(a.stars, config=3, background=False)    # truth: sigma = 10 km/s, v_max = 5 km/s
    results = {}
    for label, rotating in (("rotation free", True), ("rotation fixed to zero", False)):
        fit = model(cat, rotating)
        names = fit.fitted_parameters
        rng = np.random.default_rng(a.seed)
        centre = np.array([{"v_sys": 0.0, "sigma_max": 10.0}.get(n, 1.0) for n in names])
        pos = centre + 0.5 * rng.normal(size=(a.walkers, len(names)))
        t0 = time.perf_counter()
        sampler = fit.tempered(n_temps=a.temps, n_walkers=a.walkers, n_steps=a.steps, pos=pos, seed=a.seed)
        dt = time.perf_counter() - t0
        ev = sampler.log_evidence(discard=a.steps // 4)
        results[label] = ev
        print("{0}: {1} rungs x {2} walkers x {3} steps in {4:.2f} s; swap acceptance {5:.2f} .. {6:.2f}".format(
            label, sampler.ntemps, a.walkers, a.steps, dt, sampler.swap_acceptance_fraction.min(),
            sampler.swap_acceptance_fraction.max()))
        print("    log Z = {0:.3f} +- {1:.3f} (batch means: {2:.3f}); thermodynamic integral {3:.3f} +- {4:.3f}; smallest pair "
              "ESS {5:.0f}".format(ev["log_evidence"], ev["se"], ev["se_batch"], ev["log_evidence_ti"], ev["se_ti"],
                                   ev["pair_ess"].min()))
        flat = sampler.get_chain(discard=a.steps // 4, flat=True)
        print("    posterior: " + ", ".join("{0} = {1:.2f} +- {2:.2f}".format(n, flat[:, j].mean(), flat[:, j].std())
                                            for j, n in enumerate(names)))
        fit.close()
    bf = bayes_factor(results["rotation free"], results["rotation fixed to zero"])
    print("log Bayes factor (rotating over non-rotating) = {0:.2f} +- {1:.2f}".format(bf["log_bf"], bf["se"]))


if __name__ == "__main__":
    main()

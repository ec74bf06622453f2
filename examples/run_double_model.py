#!/usr/bin/env python3
"""A cluster with a counter-rotating core, fitted with both rotation-curve families: `synthetic.make_double_catalog`
plants a second, inner Lynden-Bell component turning against the outer one.  `ModelFit` has one component: its
`replicate_check` shows the rotation amplitude (`rot_amp`) of the inner annuli outside the replicated band, while
`DoubleModelFit` passes there.  `elpd_compare` of the two `loo` results and `bayes_factor` of two tempered runs then put
numbers on the nested-model question.  Needs an MI355X (gfx950) and the built library (make -C mcmc_dynamics_amd/csrc).

    python examples/run_double_model.py [--stars 20000] [--walkers 64] [--steps 300] [--annuli 8] [--temps 16]
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mcmc_dynamics_amd import DataReader, synthetic                                  # noqa: E402
from mcmc_dynamics_amd.analysis import DoubleModelFit, ModelFit                        # noqa: E402
from mcmc_dynamics_amd.analysis.runner import bayes_factor, elpd_compare              # noqa: E402

# proper priors for the evidence: finite boxes on every free parameter
BOX = {"v_sys": (-20.0, 20.0), "sigma_max": (1.0, 30.0), "a": (5.0, 300.0), "v_maxx": (-30.0, 30.0), "v_maxy": (-30.0, 30.0),
       "r_peak": (10.0, 300.0)}


def prepare(cls, cat):
    fit = cls(DataReader({k: cat[k] for k in ("ra", "dec", "v", "verr")}))
    fit.parameters["ra_center"].set(value=synthetic.CENTER_RA_DEG, fixed=True)
    fit.parameters["dec_center"].set(value=synthetic.CENTER_DEC_DEG, fixed=True)
    for name, (lo, hi) in BOX.items():
        fit.parameters[name].set(min=lo, max=hi)
    return fit


def start(fit, truth, n_walkers, rng):
    names = list(fit.fitted_parameters)
    pos = np.empty((n_walkers, len(names)))
    for j, name in enumerate(names):
        t = truth[name]
        pos[:, j] = t + (0.3 if t == 0.0 else 0.03 * abs(t)) * rng.normal(size=n_walkers)
        pos[:, j] = np.clip(pos[:, j], fit.parameters[name].min, fit.parameters[name].max)
    return pos


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--stars", type=int, default=20000)
    ap.add_argument("--walkers", type=int, default=64)
    ap.add_argument("--steps", type=int, default=300)
    ap.add_argument("--annuli", type=int, default=8)
    ap.add_argument("--temps", type=int, default=16)
    a = ap.parse_args()

    cat = synthetic.make_double_catalog(a.stars)
    truth = cat["truth"]
    rng = np.random.default_rng(3)
    results = {}
    for cls in (ModelFit, DoubleModelFit):
        fit = prepare(cls, cat)
        pos = start(fit, truth, a.walkers, rng)
        sampler = fit(n_walkers=a.walkers, n_steps=a.steps, n_out=None, prefix=None, pos=pos)
        chain = np.asarray(sampler.chain)
        n_burn = a.steps // 3
        rep = fit.replicate_check(chain, n_burn=n_burn, annuli=a.annuli, seed=7)
        loo = fit.loo(chain, n_burn=n_burn)
        tempered = fit.tempered(n_temps=a.temps, n_walkers=a.walkers, n_steps=a.steps, pos=pos, seed=11)
        results[cls.__name__] = {"rep": rep, "loo": loo, "evidence": tempered.log_evidence(discard=n_burn)}
        k = rep["names"].index("rot_amp")
        labels = ["all"] + ["{0:.2f}-{1:.2f}'".format(lo, hi) for lo, hi in zip(rep["edges"][:-1], rep["edges"][1:])]
        print("{0}: replicate_check p-values of rot_amp per annulus".format(cls.__name__))
        for row, label in enumerate(labels):
            flag = "  <-- outside" if min(rep["p_value"][row, k], 1.0 - rep["p_value"][row, k]) < 0.01 else ""
            print("  {0:>14s} {1:8d} stars  p = {2:.3f}{3}".format(label, int(rep["n_stars"][row]), rep["p_value"][row, k], flag))
        if cls is DoubleModelFit:
            rc = fit.r_peak_c(chain, n_burn)
            print("  r_peak_c = {0:.1f} (+{1:.1f} -{2:.1f}) arcsec, planted {3:.1f}".format(
                np.median(rc), np.percentile(rc, 84) - np.median(rc), np.median(rc) - np.percentile(rc, 16),
                truth["r_peak_ratio"] * truth["r_peak"]))
        fit.close()
    cmp_ = elpd_compare(results["DoubleModelFit"]["loo"], results["ModelFit"]["loo"])
    print("elpd_compare(double, single): elpd_diff = {0:.1f} +- {1:.1f}".format(cmp_["elpd_diff"], cmp_["se_diff"]))
    bf = bayes_factor(results["DoubleModelFit"]["evidence"], results["ModelFit"]["evidence"])
    print("bayes_factor(double, single): log BF = {0:.1f} +- {1:.1f}".format(bf["log_bf"], bf["se"]))


if __name__ == "__main__":
    main()

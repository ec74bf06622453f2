#!/usr/bin/env python3
"""Fitting the velocity-error scale: the synthetic cluster of examples/run_bootstrap.py with a `verr` column understated
twofold is fitted with `ConstantFit`, which takes the errors as stated, and with `ConstantFitES`, which fits the
dimensionless `err_scale` of variance = err_scale^2 verr^2 + sigma_max^2 along with the kinematics.  `ConstantFit` books the
missing error variance as dispersion (sigma_max too large); `ConstantFitES` recovers err_scale = 2 and the true sigma_max.
The two are nested (err_scale fixed at 1 IS ConstantFit), so `elpd_compare` of their PSIS-LOO and the simulated
likelihood-ratio test `lrt` against the null err_scale = 1 both say how much the data ask for the extra parameter.
Needs an MI355X (gfx950) and the built library (make -C mcmc_dynamics_amd/csrc).

    python examples/run_error_scale.py [--stars 20000] [--understate 2.0] [--walkers 64] [--steps 400] [--sims 256]
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mcmc_dynamics_amd import DataReader, synthetic                      # noqa: E402
from mcmc_dynamics_amd.analysis import ConstantFit, ConstantFitES          # noqa: E402
from mcmc_dynamics_amd.analysis.runner import elpd_compare                # noqa: E402
from mcmc_dynamics_amd.utils import calc_xy_offset                        # noqa: E402


def make(cls, cols):
    fit = cls(DataReader(cols))
    fit.parameters["ra_center"].set(value=synthetic.CENTER_RA_DEG, fixed=True)
    fit.parameters["dec_center"].set(value=synthetic.CENTER_DEC_DEG, fixed=True)
    return fit


def report(label, fit, a):
    best = fit.maximize(n_starts=64)
    sd = np.sqrt(np.diag(fit.laplace(best["x"])["covariance"]))
    names = list(fit.fitted_parameters)
    print("{0}: MAP (converged: {1})".format(label, best["converged"]))
    for j, name in enumerate(names):
        print("    {0:>10s} {1:10.4f} +- {2:.4f}".format(name, best["x"][j], sd[j]))
    rng = np.random.default_rng(a.seed)
    pos = best["x"] + sd * rng.normal(size=(a.walkers, len(names)))
    sampler = fit(n_walkers=a.walkers, n_steps=a.steps, n_out=None, prefix=None, pos=pos)
    chain = np.asarray(sampler.chain)
    pars = fit.convert_to_parameters(chain, a.steps // 2)
    for name in ("sigma_max", "err_scale"):
        if name in names:
            q = np.percentile(np.asarray(pars[name]), [16, 50, 84])
            print("    posterior {0}: {1:.4f} (+{2:.4f} / -{3:.4f})".format(name, q[1], q[2] - q[1], q[1] - q[0]))
    return fit.loo(chain, n_burn=a.steps // 2)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--stars", type=int, default=20000)
    ap.add_argument("--understate", type=float, default=2.0)
    ap.add_argument("--walkers", type=int, default=64)
    ap.add_argument("--steps", type=int, default=400)
    ap.add_argument("--sims", type=int, default=256)
    ap.add_argument("--seed", type=int, default=7)
    a = ap.parse_args()

    # run_bootstrap.py's cluster: errors from well below to well above the dispersion (2 .. 50 km/s about sigma = 10 km/s),
    # velocities redrawn about the catalogue's rotation field with exactly these errors
    cat = synthetic.make_catalog(a.stars, config=3, background=False)
    truth = cat["truth"]
    rng = np.random.default_rng(2)
    dx, dy = calc_xy_offset(cat["ra"], cat["dec"], synthetic.CENTER_RA_DEG, synthetic.CENTER_DEC_DEG)
    theta = np.arctan2(dy, dx)
    v_los = truth["v_sys"] + truth["v_maxx"] * np.sin(theta) - truth["v_maxy"] * np.cos(theta)
    verr = 10.0 ** rng.uniform(0.3, 1.7, a.stars)
    v = v_los + np.sqrt(verr ** 2 + truth["sigma_max"] ** 2) * rng.normal(size=a.stars)
    cols = {"ra": cat["ra"], "dec": cat["dec"], "v": v, "verr": verr / a.understate}
    print("truth: sigma_max {0:.2f} km/s, err_scale {1:g} (the catalogue states verr / {1:g}); {2} stars".format(
        truth["sigma_max"], a.understate, a.stars))

    plain, scaled = make(ConstantFit, cols), make(ConstantFitES, cols)
    loo_plain = report("ConstantFit", plain, a)
    loo_scaled = report("ConstantFitES", scaled, a)
    d = elpd_compare(loo_scaled, loo_plain)
    print("elpd_loo, ConstantFitES - ConstantFit: {0:.1f} +- {1:.1f}".format(d["elpd_diff"], d["se_diff"]))

    null = make(ConstantFitES, cols)
    null.parameters["err_scale"].set(value=1.0, fixed=True)             # the nested null: ConstantFit, bit for bit
    test = scaled.lrt(null, n_sims=a.sims, seed=a.seed)
    print("lrt against err_scale = 1: statistic {0:.1f}, simulated p = {1:.4f} +- {2:.4f} ({3} simulations, largest simulated "
          "statistic {4:.1f}), Wilks p = {5:.2e}".format(test["stat_obs"], test["p_value"], test["p_se"], test["n_used"],
                                                         float(np.max(test["stat"][test["used"]])), test["p_asymptotic"]))
    for fit in (plain, scaled, null):
        fit.close()


if __name__ == "__main__":
    main()

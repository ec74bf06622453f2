#!/usr/bin/env python3
"""Does this cluster rotate?  A likelihood-ratio test with a simulated null distribution, beside the parametric and the
weighted-likelihood bootstrap of the fit.  Two synthetic clusters of a few hundred stars are fitted with `ConstantFit`, one
with the catalogue's rotation amplitudes and one with none.  `lrt(null)` compares the fit with free (v_maxx, v_maxy)
against the fit with both fixed at zero; the null distribution of 2 (lnL_full - lnL_null) is not taken from chi2(2) but
simulated at the data's own positions and velocity errors -- `n_sims` catalogues drawn from the null fit, each refitted
under both models by a MAP fit on the device gradient, all of them in lock step.  `parametric_bootstrap()` refits
catalogues simulated at the full fit's own maximum (bias and covariance of the estimate under the model), `bootstrap()`
refits the observed catalogue under random star weights (the same without the model); their `std` side by side is the
model-based against the model-free width.  Needs an MI355X (gfx950) and the built library (make -C mcmc_dynamics_amd/csrc).

    python examples/run_lrt.py [--stars 400] [--sims 1024] [--replicates 256]
"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mcmc_dynamics_amd import DataReader, synthetic                      # noqa: E402
from mcmc_dynamics_amd.analysis import ConstantFit                        # noqa: E402
from mcmc_dynamics_amd.utils import calc_xy_offset                        # noqa: E402


def make_fit(cat, rotating):
    fit = ConstantFit(DataReader({k: cat[k] for k in ("ra", "dec", "v", "verr")}))
    fit.parameters["ra_center"].set(value=synthetic.CENTER_RA_DEG, fixed=True)
    fit.parameters["dec_center"].set(value=synthetic.CENTER_DEC_DEG, fixed=True)
    if not rotating:
        fit.parameters["v_maxx"].set(value=0.0, fixed=True)
        fit.parameters["v_maxy"].set(value=0.0, fixed=True)
    return fit


def run(label, cat, a):
    full, null = make_fit(cat, True), make_fit(cat, False)
    t0 = time.perf_counter()
    out = full.lrt(null, n_sims=a.sims, seed=a.seed)
    dt = time.perf_counter() - t0
    print("{0}: lrt of {1} simulated catalogues in {2:.2f} s ({3} used, {4} negative)".format(label, a.sims, dt, out["n_used"],
                                                                                           out["n_negative"]))
    print("    statistic {0:.3f}, simulated p = {1:.4f} +- {2:.4f}, chi2({3}) p = {4:.4g}".format(
        out["stat_obs"], out["p_value"], out["p_se"], out["df"], out["p_asymptotic"]))
    print("    null quantiles: " + ", ".join("{0:g} %: {1:.2f}".format(q, v) for q, v in sorted(out["quantiles"].items())))
    boot = full.parametric_bootstrap(n_sims=a.replicates, x_hat=out["x_full"], seed=a.seed)
    wlb = full.bootstrap(n_replicates=a.replicates, seed=a.seed, x_hat=out["x_full"])
    print("{0:>12s} {1:>10s} {2:>10s} {3:>12s} {4:>12s} {5:>10s}".format("parameter", "estimate", "bias", "parametric", "resampled",
                                                                      "ratio"))
    for j, name in enumerate(boot["names"]):
        print("{0:>12s} {1:10.4f} {2:10.4f} {3:12.4f} {4:12.4f} {5:10.3f}".format(name, out["x_full"][j], boot["bias"][j], boot["std"][j],
                                                                               wlb["std"][j], wlb["std"][j] / boot["std"][j]))
    full.close()
    null.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--stars", type=int, default=400)
    ap.add_argument("--sims", type=int, default=1024)
    ap.add_argument("--replicates", type=int, default=256)
    ap.add_argument("--seed", type=int, default=11)
    a = ap.parse_args()
    cat = synthetic.make_catalog(a.stars, config=2, background=False)
    truth = cat["truth"]
    rng = np.random.default_rng(3)
    dx, dy = calc_xy_offset(cat["ra"], cat["dec"], synthetic.CENTER_RA_DEG, synthetic.CENTER_DEC_DEG)
    theta = np.arctan2(dy, dx)
    noise = np.sqrt(np.asarray(cat["verr"]) ** 2 + truth["sigma_max"] ** 2) * rng.normal(size=a.stars)
    rotating = dict(cat, v=truth["v_sys"] + truth["v_maxx"] * np.sin(theta) - truth["v_maxy"] * np.cos(theta) + noise)
    still = dict(cat, v=truth["v_sys"] + np.sqrt(np.asarray(cat["verr"]) ** 2 + truth["sigma_max"] ** 2) * rng.normal(size=a.stars))
    print("truth: v_sys {0:.2f}, sigma_max {1:.2f}, v_maxx {2:.2f}, v_maxy {3:.2f} km/s; {4} stars".format(
        truth["v_sys"], truth["sigma_max"], truth["v_maxx"], truth["v_maxy"], a.stars))
    run("rotating cluster", rotating, a)
    run("non-rotating cluster", still, a)


if __name__ == "__main__":
    main()

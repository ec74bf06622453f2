#!/usr/bin/env python3
"""The two proposal rules of the ensemble sampler side by side: a synthetic cluster, `ConstantFit` with a fixed centre, the
stretch move (the default) and the differential-evolution move (`move="de"`) from the same start over the same
number of steps -- acceptance, the integrated autocorrelation time and the effective sample size per parameter, and the
posterior means of both.  Needs an MI355X (gfx950) and the built library (make -C mcmc_dynamics_amd/csrc).

    python examples/run_de_move.py [--stars 100000] [--walkers 64] [--steps 4000] [--burn 500]
"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mcmc_dynamics_amd import DataReader, synthetic                     # noqa: E402
from mcmc_dynamics_amd.analysis import ConstantFit                      # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--stars", type=int, default=100000)
    ap.add_argument("--walkers", type=int, default=64)
    ap.add_argument("--steps", type=int, default=4000)
    ap.add_argument("--burn", type=int, default=500)
    ap.add_argument("--seed", type=int, default=7)
    a = ap.parse_args()

    cat = synthetic.make_catalog(a.stars, config=3)                      # truth: sigma = 10 km/s, v_max = 5 km/s
    fit = ConstantFit(DataReader({k: cat[k] for k in ("ra", "dec", "v", "verr")}))
    fit.parameters["ra_center"].set(value=synthetic.CENTER_RA_DEG, fixed=True)
    fit.parameters["dec_center"].set(value=synthetic.CENTER_DEC_DEG, fixed=True)
    fit.SAMPLER = "builtin"                                              # both moves through the package's own sampler
    np.random.seed(a.seed)
    start = fit.get_initials(a.walkers)

    rows = {}
    for move in ("stretch", "de"):
        np.random.seed(a.seed)                                           # (the sampler's seed comes from NumPy's generator)
        t0 = time.perf_counter()
        sampler = fit(n_walkers=a.walkers, n_steps=a.steps, pos=start, move=move, prefix=None)
        seconds = time.perf_counter() - t0
        d = fit.chain_diagnostics(sampler.chain, n_burn=a.burn)
        rows[move] = (d, float(np.mean(sampler.acceptance_fraction)), seconds)
        print("{0:8s} {1:.2f} s, acceptance {2:.3f}".format(move, seconds, rows[move][1]))

    names = rows["de"][0]["names"]
    print("{0:12s} {1:>10s} {2:>10s} {3:>7s} {4:>10s} {5:>10s} {6:>12s} {7:>12s}".format(
        "parameter", "tau str.", "tau DE", "ratio", "ess str.", "ess DE", "mean str.", "mean DE"))
    for i, name in enumerate(names):
        s, d = rows["stretch"][0], rows["de"][0]
        print("{0:12s} {1:10.2f} {2:10.2f} {3:7.2f} {4:10.0f} {5:10.0f} {6:12.5f} {7:12.5f}".format(
            name, s["tau"][i], d["tau"][i], d["tau"][i] / s["tau"][i], s["ess"][i], d["ess"][i], s["mean"][i], d["mean"][i]))
    info = fit._catalog.de_info()
    print("DE blocks resident / host-driven / given back by the device: {device_blocks} / {host_blocks} / {discarded_blocks}".format(**info))
    print("truth:", {k: cat["truth"][k] for k in ("v_sys", "sigma_max", "v_maxx", "v_maxy")})
    fit.close()


if __name__ == "__main__":
    main()

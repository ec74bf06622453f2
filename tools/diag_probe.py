#!/usr/bin/env python3
"""What do the chain diagnostics cost beside the run that produced the chain?  

    python tools/diag_probe.py --shape c5      55 bins x 512 walkers x 4 parameters, 4 096 steps, max_lag 409
    python tools/diag_probe.py --shape c3      1 x 256 walkers x 4 parameters, 3 000 steps, max_lag 300

Per shape one JSON line, printed and written to profiles/diag_probe_<shape>.json (--out-dir).  The chain is the one the
package's resident sampler produces on bench.py's catalogue of that workload (synthetic.make_catalog with its configuration
number; C5: make_radial_bins(nstars=1000, dlogr=0.05)), after 256 discarded steps; its wall time is taken in this run.
Then, on that chain:
  * mcd_chain_diagnostics on the device -- wall time of the call (host to device copy of the chain included) and HIP-event
    time of its kernels: medians of --calls calls after --warmup;
  * the same call with ctx = NULL (the library's host loop, one thread) on --host-groups groups, scaled to all of them;
  * emcee's estimator restated in NumPy (tests/diag_helper.py: fft_tau, one FFT per walker and parameter), timed on
    --fft-groups groups and scaled to all of them;
and whether the device result equals the host loop's bit for bit."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import diag_helper as dh                                                # noqa: E402
from mcmc_dynamics_amd import DataReader, Gaussian, _native as native, synthetic   # noqa: E402
from mcmc_dynamics_amd.analysis import BinnedConstantFit, ConstantFit              # noqa: E402
from mcmc_dynamics_amd.sampler import _reserve                                     # noqa: E402

NAMES = ["v_sys", "sigma_max", "v_maxx", "v_maxy"]
BURN = 256


def _fix_centre(fit):
    fit.parameters["ra_center"].set(value=synthetic.CENTER_RA_DEG, fixed=True)
    fit.parameters["dec_center"].set(value=synthetic.CENTER_DEC_DEG, fixed=True)


def produce(shape, stars, steps, ctx):
    """(chain (T, G, W, P), seconds of the timed run, steps/s, description)"""
    if shape == "c5":
        cat = synthetic.make_catalog(stars, config=5, seed=synthetic.CATALOG_SEED_BASE + 5, background=False)
        reader = DataReader({k: cat[k] for k in ("ra", "dec", "v", "verr")})
        reader.make_radial_bins(synthetic.CENTER_RA_DEG, synthetic.CENTER_DEC_DEG, nstars=1000, dlogr=0.05)
        fit = BinnedConstantFit(reader, context=ctx)
        _fix_centre(fit)
        from mcmc_dynamics_amd.analysis.binned import BinnedSampler
        w = 512
        pos = synthetic.make_walkers(w, NAMES, cat["truth"], config=5)
        pos = np.ascontiguousarray(np.broadcast_to(pos, (fit.n_bins,) + pos.shape))
        sampler = BinnedSampler(fit.n_bins, w, 4, fit.lnprob_batch, seed=5, block_fn=fit._stretch_block, rng="device",
                                seeded_block_fn=fit._stretch_block_seeded)
        sampler.reserve(BURN + steps)
        state = sampler.run_mcmc(pos, BURN)
        t0 = time.perf_counter()
        sampler.run_mcmc(state[0], steps, log_prob0=state[1])
        dt = time.perf_counter() - t0
        chain = sampler.get_chain(discard=BURN)
        what = "BinnedSampler, mcd_stretch_move_seeded with n_bins = {0}".format(fit.n_bins)
    else:
        cat = synthetic.make_catalog(stars, config=3, seed=synthetic.CATALOG_SEED_BASE + 3, background=True)
        fit = ConstantFit(DataReader({k: cat[k] for k in ("ra", "dec", "v", "verr", "pmember")}),
                          background=Gaussian(synthetic.TRUTH["v_back"], synthetic.TRUTH["sigma_back"]), context=ctx)
        _fix_centre(fit)
        fit.SAMPLER = "resident"
        w = 256
        pos = synthetic.make_walkers(w, NAMES, cat["truth"], config=3)
        sampler = fit._make_sampler(w, seed=5)
        _reserve(sampler, BURN + steps)
        state = sampler.run_mcmc(pos, BURN)
        t0 = time.perf_counter()
        sampler.run_mcmc(state[0], steps, log_prob0=state[1])
        dt = time.perf_counter() - t0
        chain = sampler.get_chain(discard=BURN)[:, None]
        what = "EnsembleSampler, mcd_stretch_move_seeded"
    chain = np.ascontiguousarray(chain)
    fit.close()
    return chain, dt, steps / dt, what


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", choices=("c5", "c3"), default="c5")
    ap.add_argument("--stars", type=int, default=1000000)
    ap.add_argument("--steps", type=int, default=None)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--fft-groups", type=int, default=4)
    ap.add_argument("--host-groups", type=int, default=2, help="groups given to the ctx = NULL call (one thread: all 55 "
                                                                "of the C5 shape take minutes); 0: skip it")
    ap.add_argument("--out-dir", default=os.path.join(ROOT, "profiles"))
    a = ap.parse_args()
    steps = a.steps or (4096 if a.shape == "c5" else 3000)
    L = max(1, steps // 10)

    ctx = native.default_context()
    chain, run_s, rate, what = produce(a.shape, a.stars, steps, ctx)
    T, G, W, P = chain.shape

    wall, kern = [], []
    for i in range(a.warmup + a.calls):
        t0 = time.perf_counter()
        out = native.chain_diagnostics(chain, L, context=ctx)
        dt = time.perf_counter() - t0
        info = native.chain_diagnostics_info()
        if i >= a.warmup:
            wall.append(dt)
            kern.append(info["kernel_ms"] * 1e-3)

    # (a group's numbers depend on its own series only: the host loop on the first groups must reproduce their rows)
    host_s, same, hg = None, None, min(G, a.host_groups)
    if hg:
        part = np.ascontiguousarray(chain[:, :hg])
        t0 = time.perf_counter()
        ref = native.chain_diagnostics(part, L, context=None)
        host_s = (time.perf_counter() - t0) * G / hg
        same = all(np.array_equal(out[k][:hg], ref[k], equal_nan=True) for k in ref)

    ng = min(G, a.fft_groups)
    t0 = time.perf_counter()
    tau_fft = np.concatenate([dh.fft_tau(chain[:, g:g + 1]) for g in range(ng)])
    fft_s = (time.perf_counter() - t0) * G / ng
    found = out["found"][:ng] == 1

    line = {
        "tool": "tools/diag_probe.py", "shape": a.shape, "steps": T, "groups": G, "walkers": W, "parameters": P, "series": G * W * P,
        "max_lag": L, "chain_bytes": int(chain.nbytes),
        "sampler": {"what": what, "stars": a.stars, "seconds": round(run_s, 4), "steps_per_s": round(rate, 1)},
        "device": {"wall_s_median": round(float(np.median(wall)), 5), "kernel_s_median": round(float(np.median(kern)), 5),
                   "wall_s_min_max": [round(min(wall), 5), round(max(wall), 5)], "calls": a.calls, "warmup": a.warmup,
                   "tiles": info["n_tiles"], "groups_per_tile": info["tile_groups"],
                   "lag_fma_per_s": round(G * W * P * sum(T - k for k in range(L + 1)) / float(np.median(kern)), 0)},
        "host_loop_s": None if host_s is None else round(host_s, 3), "host_loop_groups_timed": hg,
        "device_equals_host_loop": same,
        "numpy_fft_s": round(fft_s, 3), "numpy_fft_groups_timed": ng,
        "numpy_fft_max_tau_difference": float(np.max(np.abs(tau_fft[found] - out["tau"][:ng][found]))) if found.any() else None,
        "tau_median": float(np.nanmedian(out["tau"])), "windows_found": int((out["found"] == 1).sum()), "of": int(out["found"].size),
        "rhat_max": float(np.nanmax(out["rhat"])),
        "diagnosis_over_run_wall": round(float(np.median(wall)) / run_s, 3),
        "diagnosis_over_run_kernel": round(float(np.median(kern)) / run_s, 4),
    }
    text = json.dumps(line)
    print(text)
    os.makedirs(a.out_dir, exist_ok=True)
    with open(os.path.join(a.out_dir, "diag_probe_{0}.json".format(a.shape)), "w") as f:
        f.write(text + "\n")


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Measure mcd_pointwise_posterior on one GPU: one JSON line per case.

    python tools/posterior_probe.py [--isa-json FILE] [--calls 20] [--host-samples 64] [--cases all|small]

Each case builds a synthetic catalogue (synthetic.make_catalog), draws S samples around the truth (make_walkers) and
times the fused call: wall-clock median of >= 20 blocking calls after two warm-up calls, and the HIP-event time of its
kernels (option "timing").  `frac_valu_f64` prices the kernel time with the VALU instructions per (star, sample) term of
the instantiation that ran (tools/posterior_isa.py; --isa-json reads a table written by `posterior_isa.py --json`) against
the f64 issue peak of DESIGN.md section 3.3 (256 CUs x 4 SIMDs x 2.4 GHz / 4 cycles = 6.144e11 wave-instructions/s).

The route that existed before, for the same S: one Catalog.loglike_per_star + Catalog.membership call per sample with the
running reduction on the host (background models), timed over `--host-samples` samples and scaled to S (the per-sample
cost does not depend on S); and the NumPy restatement on one core (tests/posterior_helper.py: the oracle's per-star
functions), timed on a subsample.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

from mcmc_dynamics_amd import _native, synthetic     # noqa: E402
from oracle import lnprob_numpy as oracle             # noqa: E402

PEAK_F64 = 256 * 4 * 2.4e9 / 4.0
MODEL_NAMES = {0: "CONST", 1: "BGFIXED", 2: "BGGAUSS", 3: "PROFILE", 4: "PROFILE_BGGAUSS", 5: "PROFILE_BGDENS",
               6: "PROFILE_BGFIXED"}
BG_MODELS = (1, 2, 4, 5, 6)
# (label, model, free centre, N, S)
CASES = [
    ("C3 catalogue (CONST_BGFIXED)", 1, False, 1000000, 4096),
    ("CONST_BGGAUSS", 2, False, 1000000, 1024),
    ("PROFILE_BGGAUSS", 4, False, 1000000, 1024),
    ("CONST free centre", 0, True, 100000, 4096),
    ("small catalogue, sliced (CONST_BGGAUSS)", 2, False, 10000, 16384),
]
EXTRA = {"a": 60.0, "r_peak": 90.0}


def abi_names(model, free):
    prof = model >= 3
    names = ["v_sys", "sigma_max"] + (["a"] if prof else []) + ["v_maxx", "v_maxy"] + (["r_peak"] if prof else [])
    if free:
        names += ["ra_center", "dec_center"]
    bg = {0: 0, 1: 1, 2: 2, 3: 0, 4: 2, 5: 3, 6: 1}[model]
    return names + {0: [], 1: [], 2: ["v_back", "sigma_back", "f_back"], 3: ["f_back"]}[bg]


def catalogue(model, free, n):
    cat = synthetic.make_catalog(n, config=3, background=True)
    truth = dict(cat["truth"], **EXTRA)
    kw = {}
    if model in (1, 6):
        kw = {"lnlike_bg": oracle.gaussian_background(cat["v"], cat["verr"], synthetic.TRUTH["v_back"],
                                                      synthetic.TRUTH["sigma_back"]), "pmember": cat["pmember"]}
    elif model in (2, 4):
        kw = {"density": cat["density"]}
    centre = None if free else (synthetic.CENTER_RA_DEG, synthetic.CENTER_DEC_DEG)
    return cat, truth, kw, centre


def samples(model, free, truth, S):
    names = abi_names(model, free)
    tr = {k: truth[k] for k in names}
    rows = np.empty((S, len(names)))
    for j, name in enumerate(names):       # make_walkers for the names it knows, the same ball for a and r_peak
        if name in synthetic.BOUNDS:
            rows[:, j] = synthetic.make_walkers(S, [name], tr, config=3, seed=100 + j)[:, 0]
        else:
            rows[:, j] = tr[name] * (1.0 + 0.05 * np.random.default_rng(100 + j).normal(size=S))
    return np.ascontiguousarray(rows)


def isa_rows(path):
    if path:
        with open(path) as f:
            return json.load(f)["rows"]
    import posterior_isa
    return posterior_isa.analyse()


def host_loop_ms(gpu, table, n_host):
    """ms per sample of the per-sample route: two per-star calls and a running (Welford / log-sum-exp) update on the host."""
    n = gpu.n_stars
    shift, sumexp = np.full(n, -np.inf), np.zeros(n)
    mean, m2, pm, pm2 = np.zeros(n), np.zeros(n), np.zeros(n), np.zeros(n)
    gpu.loglike_per_star(table[0])
    t0 = time.perf_counter()
    for j in range(n_host):
        x = gpu.loglike_per_star(table[j])
        p = gpu.membership(table[j])
        mx = np.maximum(shift, x)
        sumexp = sumexp * np.exp(shift - mx) + np.exp(x - mx)
        shift = mx
        d = x - mean
        mean += d / (j + 1)
        m2 += d * (x - mean)
        d = p - pm
        pm += d / (j + 1)
        pm2 += d * (p - pm)
    return (time.perf_counter() - t0) * 1e3 / n_host


def numpy_rate(cat, model, free, centre, table, n_stars=20000, n_samples=16):
    import posterior_helper as ph
    sub = {k: (v[:n_stars] if isinstance(v, np.ndarray) else v) for k, v in cat.items()}
    sub["lnlike_bg"] = oracle.gaussian_background(sub["v"], sub["verr"], synthetic.TRUTH["v_back"], synthetic.TRUTH["sigma_back"])
    t0 = time.perf_counter()
    ph.numpy_posterior(sub, table[:n_samples], model, centre)
    return n_stars * n_samples / (time.perf_counter() - t0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--isa-json", default=None)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--host-samples", type=int, default=64)
    ap.add_argument("--cases", default="all", choices=["all", "small"])
    ap.add_argument("--kernel-only", action="store_true", help="skip the host loop and NumPy baselines (profiler runs)")
    args = ap.parse_args()
    rows = isa_rows(args.isa_json)
    ctx = _native.default_context()
    cases = CASES if args.cases == "all" else [c for c in CASES if c[3] <= 100000]
    for label, model, free, n, S in cases:
        cat, truth, kw, centre = catalogue(model, free, n)
        table = samples(model, free, truth, S)
        gpu = _native.Catalog(ctx, cat["ra"], cat["dec"], cat["v"], cat["verr"], model=model, centre=centre, **kw)
        mem = model in BG_MODELS
        for _ in range(2):
            gpu.pointwise_posterior(table, membership=mem)
        wall = []
        for _ in range(args.calls):
            t0 = time.perf_counter()
            gpu.pointwise_posterior(table, membership=mem)
            wall.append((time.perf_counter() - t0) * 1e3)
        gpu.set_option("timing", 1)
        kms = []
        for _ in range(5):
            gpu.pointwise_posterior(table, membership=mem)
            kms.append(gpu.last_kernel_ms)
        gpu.set_option("timing", 0)
        ms, kernel_ms = float(np.median(wall)), float(np.median(kms))
        row = next(r for r in rows if r["model"] == MODEL_NAMES[model] and r["free_centre"] == free
                   and r["membership"] == mem and r["precision"] == "f64")
        terms = float(n) * S
        out = {"case": label, "model": MODEL_NAMES[model], "free_centre": free, "membership": mem, "n_stars": n,
               "n_samples": S, "ms": round(ms, 3), "kernel_ms": round(kernel_ms, 3),
               "terms_per_s": terms / (ms * 1e-3), "kernel_terms_per_s": terms / (kernel_ms * 1e-3),
               "valu_per_term": row["valu_per_term"],
               "frac_valu_f64": row["valu_per_term"] * terms / 64.0 / (kernel_ms * 1e-3) / PEAK_F64}
        if mem and not args.kernel_only:
            per = host_loop_ms(gpu, table, min(args.host_samples, S))
            out["host_loop_ms"] = round(per * S, 1)
            out["host_loop_ms_per_sample"] = round(per, 4)
            out["host_loop_samples_timed"] = min(args.host_samples, S)
            out["speedup_vs_host_loop"] = round(per * S / ms, 1)
        if not args.kernel_only:
            out["numpy_terms_per_s_one_core"] = numpy_rate(cat, model, free, centre, table)
            out["numpy_ms_extrapolated"] = round(terms / out["numpy_terms_per_s_one_core"] * 1e3, 0)
        print(json.dumps(out), flush=True)
        gpu.close()


if __name__ == "__main__":
    sys.exit(main())

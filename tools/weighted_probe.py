#!/usr/bin/env python3
"""Measurement instrument for the weighted value and gradient: what one mcd_weighted_loglike_grad call costs
for each of the three weight schemes, beside mcd_loglike_grad_batch -- the unweighted gradient kernel, which this feature
does not touch -- on the same rows.  No threshold is attached to any figure.

    python tools/weighted_probe.py --stars 100000
    python tools/weighted_probe.py --stars 1000000

One JSON line per run, printed and written to profiles/weighted_probe_<stars>.json.  The catalogue is bench.py's C3
(synthetic.make_catalog(config=3), CONST_BGFIXED, 4 kernel columns), 256 parameter rows, one replicate per row for the
generated schemes.  The explicit scheme is capped at 256 MiB of weights: min(256, cap) replicates, shared by the rows in
turn (row r reads replicate r mod that number); its wall time includes the host's check and fingerprint of the whole array
on every call (the transposed copy on the device is reused while the contents stand; `first_call_us` holds the call that
transposed and uploaded it), its kernel time does not.

Method.  Every variant is warmed up by two calls of its own (code objects loaded, plans and buffers built, pages touched).
A timing is a host clock around one synchronous library call and, beside it, the HIP-event time of the main kernel alone
(option "timing"); each is repeated `--repeats` times, the four variants taking turns, and the line holds the median and
the spread (min, max) of both in microseconds, and the ratios of the medians to the unweighted gradient's.  `launch` is
mcd_last_launch_info after the variant's warm-up (the gradient call does not fill it: zeros until a value launch has)."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from mcmc_dynamics_amd import _native as native, synthetic      # noqa: E402
from mcmc_dynamics_amd.background import Gaussian                # noqa: E402

CENTRE = (synthetic.CENTER_RA_DEG, synthetic.CENTER_DEC_DEG)
NAMES = ["v_sys", "sigma_max", "v_maxx", "v_maxy"]
EXPLICIT_CAP_BYTES = 256 << 20


def spread(values, digits=1):
    s = np.asarray(values, dtype=np.float64)
    return {"us": round(float(np.median(s)), digits), "us_min": round(float(s.min()), digits), "us_max": round(float(s.max()), digits)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--stars", type=int, default=100000)
    ap.add_argument("--rows", type=int, default=256)
    ap.add_argument("--repeats", type=int, default=25)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    cols = synthetic.make_catalog(a.stars, config=3, background=True)
    tr = cols["truth"]
    bg = Gaussian(tr["v_back"], tr["sigma_back"])
    ctx = native.default_context()
    cat = native.Catalog(ctx, cols["ra"], cols["dec"], cols["v"], cols["verr"], model=native.MODEL_CONST_BGFIXED,
                         centre=CENTRE, lnlike_bg=bg(cols["v"], cols["verr"]), pmember=cols["pmember"])
    cat.set_option("timing", 1)
    table = np.ascontiguousarray(synthetic.make_walkers(a.rows, NAMES, tr, config=3))
    rep = np.arange(a.rows, dtype=np.int64)
    n_explicit = int(max(1, min(a.rows, EXPLICIT_CAP_BYTES // (8 * a.stars))))
    weights = native.bootstrap_weights("exponential", a.seed, 0, n_explicit, 0, a.stars)

    def timed(call):
        t0 = time.perf_counter()
        call()
        return 1e6 * (time.perf_counter() - t0), 1e3 * cat.last_kernel_ms

    variants = {
        "unweighted": lambda: cat.loglike_grad(table),
        "exponential": lambda: cat.weighted_loglike_grad(table, rep, scheme="exponential", seed=a.seed),
        "poisson": lambda: cat.weighted_loglike_grad(table, rep, scheme="poisson", seed=a.seed),
        "explicit": lambda: cat.weighted_loglike_grad(table, rep % n_explicit, scheme="explicit", weights=weights),
    }
    launch, first_call_us = {}, {}
    for name, call in variants.items():
        first_call_us[name] = round(timed(call)[0], 1)          # (plans and buffers built; explicit: the transposed upload)
        call()
        launch[name] = {k: v for k, v in cat.launch_info().items() if k in ("workgroups", "chunks")}
    times = {name: [] for name in variants}
    for _ in range(a.repeats):
        for name, call in variants.items():
            times[name].append(timed(call))
    line = {"tool": "tools/weighted_probe.py", "stars": a.stars, "rows": a.rows, "repeats": a.repeats, "model": "CONST_BGFIXED",
            "explicit_replicates": n_explicit, "variants": {}}
    for name, t in times.items():
        line["variants"][name] = {"wall": spread([x[0] for x in t]), "kernel": spread([x[1] for x in t]), "launch": launch[name],
                                  "first_call_us": first_call_us[name]}
    base = line["variants"]["unweighted"]
    for name in ("exponential", "poisson", "explicit"):
        v = line["variants"][name]
        v["kernel_over_unweighted"] = round(v["kernel"]["us"] / base["kernel"]["us"], 3)
        v["wall_over_unweighted"] = round(v["wall"]["us"] / base["wall"]["us"], 3)
    cat.close()
    text = json.dumps(line)
    print(text)
    out = a.out or os.path.join(ROOT, "profiles", "weighted_probe_{0}.json".format(a.stars))
    with open(out, "w") as fh:
        fh.write(text + "\n")


if __name__ == "__main__":
    main()

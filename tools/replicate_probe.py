#!/usr/bin/env python3
"""Measurement instrument for the replicated-data predictive checks: what one mcd_replicate_check call costs,
beside mcd_posterior_predictive at the same shape in the same run.  No threshold is attached to any figure.

    python tools/replicate_probe.py [--out profiles/replicate_probe.json]

Shapes: bench.py's C3 catalogue (synthetic.make_catalog(config=3), CONST_BGFIXED) at 1e6 stars x 1024 samples x 8 annuli,
and CONST_BGGAUSS at 1e5 stars x 4096 samples x 8 annuli.  One JSON document, printed and written to --out.

Method.  Every timed call is warmed up by two calls of its own (code objects loaded, pages touched).  `wall_us`: a host
clock around one synchronous library call, the median of 10 (with min and max).  `kernel_us`: the HIP-event time of the
main kernel alone (option "timing"), the median of 5 further calls."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from mcmc_dynamics_amd import _native as native, synthetic      # noqa: E402
from mcmc_dynamics_amd.background import Gaussian               # noqa: E402
from mcmc_dynamics_amd.utils import calc_xy_offset               # noqa: E402

CENTRE = (synthetic.CENTER_RA_DEG, synthetic.CENTER_DEC_DEG)
NAMES = {"bgfixed": ["v_sys", "sigma_max", "v_maxx", "v_maxy"],
         "bggauss": ["v_sys", "sigma_max", "v_maxx", "v_maxy", "v_back", "sigma_back", "f_back"]}


def measure(cat, fn):
    for _ in range(2):
        fn()
    cat.set_option("timing", 0)
    wall = []
    for _ in range(10):
        t0 = time.perf_counter()
        fn()
        wall.append(1e6 * (time.perf_counter() - t0))
    cat.set_option("timing", 1)
    kernel = []
    for _ in range(5):
        fn()
        kernel.append(1e3 * cat.last_kernel_ms)
    cat.set_option("timing", 0)
    return {"wall_us": round(float(np.median(wall)), 1), "wall_us_min": round(min(wall), 1), "wall_us_max": round(max(wall), 1),
            "kernel_us": round(float(np.median(kernel)), 1)}


def shape(ctx, kind, n_stars, n_samples, n_annuli):
    cols = synthetic.make_catalog(n_stars, config=3, background=True)
    tr = cols["truth"]
    if kind == "bgfixed":
        bg = Gaussian(tr["v_back"], tr["sigma_back"])
        cat = native.Catalog(ctx, cols["ra"], cols["dec"], cols["v"], cols["verr"], model=native.MODEL_CONST_BGFIXED,
                             centre=CENTRE, lnlike_bg=bg(cols["v"], cols["verr"]), pmember=cols["pmember"])
        bg_args = (bg.mean, bg.sigma)
    else:
        cat = native.Catalog(ctx, cols["ra"], cols["dec"], cols["v"], cols["verr"], model=native.MODEL_CONST_BGGAUSS,
                             centre=CENTRE, density=cols["density"])
        bg_args = (float("nan"), float("nan"))
    table = np.ascontiguousarray(synthetic.make_walkers(n_samples, NAMES[kind], tr, config=3))
    dx, dy = calc_xy_offset(cols["ra"], cols["dec"], *CENTRE)
    order = np.argsort(np.hypot(dx, dy), kind="stable").astype(np.int64)
    offs = (np.arange(n_annuli + 1, dtype=np.int64) * n_stars) // n_annuli
    out = {"model": "CONST_" + kind.upper(), "stars": n_stars, "samples": n_samples, "annuli": n_annuli}
    out["replicate_check"] = measure(cat, lambda: cat.replicate_check(table, 1, offs, order, *bg_args))
    out["replicate_check"]["launch"] = {k: v for k, v in cat.launch_info().items() if k in ("workgroups", "chunks")}
    out["posterior_predictive"] = measure(cat, lambda: cat.posterior_predictive(table))
    terms = float(n_stars) * n_samples
    out["replicate_check"]["ns_per_term"] = round(1e3 * out["replicate_check"]["kernel_us"] / terms, 5)
    out["posterior_predictive"]["ns_per_term"] = round(1e3 * out["posterior_predictive"]["kernel_us"] / terms, 5)
    cat.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "replicate_probe.json"))
    a = ap.parse_args()
    ctx = native.default_context()
    doc = {"tool": "tools/replicate_probe.py",
           "shapes": [shape(ctx, "bgfixed", 1000000, 1024, 8), shape(ctx, "bggauss", 100000, 4096, 8)]}
    text = json.dumps(doc, indent=1, sort_keys=True)
    print(text)
    with open(a.out, "w") as fh:
        fh.write(text + "\n")


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Time per evaluation of the double Lynden-Bell models (7, 8) against their single-component counterparts (3, 4) on the
same catalogue: 1e6 stars x 256 walkers, fixed centre, fast path.  Measured, not gated.

    python tools/double_probe.py [--stars 1000000] [--walkers 256] [--rounds 25] [--per-round 20] [--out FILE]

Method (bench.py's): parameters staged once, a clock ramp of 0.4 s of launches, warm-up, then `rounds` timed rounds of
`per-round` pipelined launches between two synchronisations; the figure is the MEDIAN over the rounds of the wall time per
launch.  Every model sees the same stars, and rows that agree in their shared columns.  Prints one JSON line (and writes
it to --out).  Needs an MI355X (gfx950) and the built library."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mcmc_dynamics_amd import _native, synthetic                      # noqa: E402


def rows_for(model, truth, w, rng):
    names = ["v_sys", "sigma_max", "a", "v_maxx", "v_maxy", "r_peak"]
    if model in (_native.MODEL_DOUBLE, _native.MODEL_DOUBLE_BGGAUSS):
        names += ["v_maxx_c", "v_maxy_c", "r_peak_ratio"]
    if model in (_native.MODEL_PROFILE_BGGAUSS, _native.MODEL_DOUBLE_BGGAUSS):
        names += ["v_back", "sigma_back", "f_back"]
    pos = np.empty((w, len(names)))
    for j, name in enumerate(names):
        t = truth[name]
        pos[:, j] = t * (1.0 + 0.03 * rng.normal(size=w)) if t != 0.0 else 0.3 * rng.normal(size=w)
    if "r_peak_ratio" in names:
        pos[:, names.index("r_peak_ratio")] = np.clip(pos[:, names.index("r_peak_ratio")], 1e-3, 1.0)
    if "f_back" in names:
        pos[:, names.index("f_back")] = np.clip(pos[:, names.index("f_back")], 0.01, 0.99)
    return np.ascontiguousarray(pos)


def time_model(ctx, cat_cols, model, truth, w, rounds, per_round, ramp_seconds=0.4):
    kw = {"density": cat_cols["density"]} if model in (_native.MODEL_PROFILE_BGGAUSS, _native.MODEL_DOUBLE_BGGAUSS) else {}
    cat = _native.Catalog(ctx, cat_cols["ra"], cat_cols["dec"], cat_cols["v"], cat_cols["verr"], model=model,
                          centre=(synthetic.CENTER_RA_DEG, synthetic.CENTER_DEC_DEG), **kw)
    cat.set_option("fast_path", 2)                                    # the fast general form for every model: like for like
    params = rows_for(model, truth, w, np.random.default_rng(17))
    check = cat.loglike(params)
    level = cat.fast_level
    assert np.all(np.isfinite(check)) and level == 1, (model, level)
    cat.upload_params(params)
    t0 = time.perf_counter()
    for _ in range(8):
        cat.enqueue()
    cat.sync()
    per_step = max((time.perf_counter() - t0) / 8, 1e-6)
    for _ in range(int(min(20000, ramp_seconds / per_step))):
        cat.enqueue()
    cat.sync()
    times = []
    for _ in range(rounds):
        cat.enqueue()
        cat.sync()
        t0 = time.perf_counter()
        for _ in range(per_round):
            cat.enqueue()
        cat.sync()
        times.append((time.perf_counter() - t0) / per_round)
    cat.close()
    times = np.array(times) * 1e6
    return {"median_us": float(np.median(times)), "min_us": float(times.min()), "max_us": float(times.max()), "rounds": rounds,
            "launches_per_round": per_round, "columns": int(params.shape[1])}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--stars", type=int, default=1000000)
    ap.add_argument("--walkers", type=int, default=256)
    ap.add_argument("--rounds", type=int, default=25)
    ap.add_argument("--per-round", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.rounds < 20:
        ap.error("at least 20 rounds")
    cat = synthetic.make_catalog(a.stars, config=3, background=True)
    truth = dict(cat["truth"], a=60.0, r_peak=90.0, v_maxx_c=-4.0, v_maxy_c=2.5, r_peak_ratio=0.2)
    ctx = _native.default_context()
    out = {"stars": a.stars, "walkers": a.walkers, "centre": "fixed", "fast_path": "general (level 1)", "models": {}}
    for name, model in (("PROFILE", _native.MODEL_PROFILE), ("DOUBLE", _native.MODEL_DOUBLE),
                        ("PROFILE_BGGAUSS", _native.MODEL_PROFILE_BGGAUSS), ("DOUBLE_BGGAUSS", _native.MODEL_DOUBLE_BGGAUSS)):
        out["models"][name] = time_model(ctx, cat, model, truth, a.walkers, a.rounds, a.per_round)
    m = out["models"]
    out["ratio_double_over_profile"] = m["DOUBLE"]["median_us"] / m["PROFILE"]["median_us"]
    out["ratio_double_bggauss_over_profile_bggauss"] = m["DOUBLE_BGGAUSS"]["median_us"] / m["PROFILE_BGGAUSS"]["median_us"]
    isa = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "mcmc_dynamics_amd", "csrc", "isa_mix.json")
    with open(isa) as f:
        k = json.load(f)["kernels"]
    out["valu_per_term_prefetch"] = {key: k[key].get("valu_per_term_prefetch", k[key]["valu_per_term"])
                                     for key in ("profile_general", "double", "profile_bggauss", "double_bggauss")}
    out["slots_per_term_prefetch"] = {key: k[key].get("slots_per_term_prefetch", k[key]["slots_per_term"])
                                      for key in ("profile_general", "double", "profile_bggauss", "double_bggauss")}
    line = json.dumps(out, sort_keys=True)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Measurement instrument for the parallel-tempering block: tempered steps per second resident on the
device and host-driven, and beside them the plain resident stretch move at W = 64 on the same catalogue with the plain
kernels (fast_path = 0) and with the default -- what a tempered step costs relative to an un-tempered one, and what
guard level 0 gives up.  No threshold is attached to any figure.

    python tools/temper_probe.py --stars 100000 --temps 16 --walkers 64
    python tools/temper_probe.py --stars 1000000 --temps 8 --walkers 64

One JSON line per run, printed and written to profiles/temper_probe_<stars>_<T>x<W>.json.  The catalogue is bench.py's C3
(synthetic.make_catalog(config=3), CONST_BGFIXED, 4 free parameters = the kernel columns); the ladder is the default
geometric one with a final beta = 0 inside a box of +-20 posterior widths around the truth.

Method.  Every timed shape is warmed up by a block of its own (code objects loaded, arenas and work sets sized, pages
touched).  A timing is a host clock around one library call, which ends in the block's one stream synchronise; each is
repeated `--repeats` times alternating the variants, and the line holds the median and the spread (min, max).  Steps per
second = steps of the block / seconds of the call, the copies of the block's numbers and rows included."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from mcmc_dynamics_amd import _native as native, synthetic           # noqa: E402
from mcmc_dynamics_amd.sampler import default_ladder                 # noqa: E402

CENTRE = (synthetic.CENTER_RA_DEG, synthetic.CENTER_DEC_DEG)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--stars", type=int, default=100000)
    ap.add_argument("--temps", type=int, default=16)
    ap.add_argument("--walkers", type=int, default=64)
    ap.add_argument("--steps", type=int, default=256, help="steps of a timed resident block")
    ap.add_argument("--host-steps", type=int, default=32, help="steps of a timed host-driven block")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--seed", type=int, default=11)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    t_n, w = a.temps, a.walkers
    cols = synthetic.make_catalog(a.stars, config=3, background=True)
    from mcmc_dynamics_amd.background import Gaussian
    tr = cols["truth"]
    lnbg = Gaussian(tr["v_back"], tr["sigma_back"])(cols["v"], cols["verr"])
    ctx = native.default_context()
    cat = native.Catalog(ctx, cols["ra"], cols["dec"], cols["v"], cols["verr"], model=native.MODEL_CONST_BGFIXED,
                         centre=CENTRE, lnlike_bg=lnbg, pmember=cols["pmember"])
    names = ["v_sys", "sigma_max", "v_maxx", "v_maxy"]
    x = np.array([tr[k] for k in names])
    width = 10.0 / np.sqrt(0.75 * a.stars) * np.array([1.0, 0.7, 1.4, 1.4])
    lo, hi = x - 20.0 * width, x + 20.0 * width
    lo[1] = max(lo[1], 0.0)
    plan = {"col_source": np.arange(4, dtype=np.int32), "col_const": np.zeros(4), "col_factor": np.ones(4), "lo": lo, "hi": hi,
            "fixed_ok": True}
    betas = default_ladder(t_n, 0.5)
    rng = np.random.default_rng(a.seed)
    pos0 = np.ascontiguousarray(np.clip(x + width * rng.normal(size=(t_n, w, 4)), lo, hi))
    cat.set_option("fast_path", 0)
    rows = t_n * (w // 2)
    ll0 = np.concatenate([cat.loglike(np.ascontiguousarray(pos0.reshape(-1, 4)[i:i + rows])) for i in (0, rows)]).reshape(t_n, w)
    cat.set_option("fast_path", 1)

    state = {"step": 0}

    def tempered(n, resident):
        cat.set_option("device_chain", 1 if resident else 0)
        pos, ll, lp = pos0.copy(), ll0.copy(), np.zeros((t_n, w))
        chain, llc = np.empty((n, 1, w, 4)), np.empty((n, t_n, w))
        acc, swp, swa = np.zeros((t_n, w), dtype=np.int64), np.zeros(t_n - 1, dtype=np.int64), np.zeros(t_n - 1, dtype=np.int64)
        t0 = time.perf_counter()
        cat.temper_block(plan, betas, pos, ll, lp, a.seed, state["step"], n, chain, llc, acc, swp, swa)
        dt = time.perf_counter() - t0
        state["step"] += n
        cat.set_option("device_chain", 1)
        return dt, float(acc.sum()) / (n * t_n * w), (swa / np.maximum(swp, 1)).round(3).tolist()

    def stretch(n, fast):
        cat.set_option("fast_path", fast)
        cat.set_option("device_chain", 1)                        # (forgets the kernel family the last resident block ran)
        pos = np.ascontiguousarray(pos0[0])
        lnp = cat.loglike(pos)
        chain, lnpc = np.empty((n, w, 4)), np.empty((n, w))
        acc = np.zeros(w, dtype=np.int64)
        t0 = time.perf_counter()
        cat.stretch_move_seeded(plan, pos, lnp, a.seed, state["step"], n, chain, lnpc, acc)
        dt = time.perf_counter() - t0
        state["step"] += n
        cat.set_option("fast_path", 1)
        cat.set_option("device_chain", 1)
        return dt

    variants = [("tempered_resident", lambda: tempered(a.steps, True)[0], a.steps),
                ("tempered_host_driven", lambda: tempered(a.host_steps, False)[0], a.host_steps),
                ("stretch_resident_plain", lambda: stretch(a.steps, 0), a.steps),
                ("stretch_resident_default", lambda: stretch(a.steps, 1), a.steps)]
    for _, fn, _ in variants:                                    # warm-up: every timed shape once
        fn()
    before_t, before_s = cat.temper_info(), cat.stretch_info()
    times = {name: [] for name, _, _ in variants}
    for _ in range(a.repeats):
        for name, fn, _ in variants:
            times[name].append(fn())
    after_t, after_s = cat.temper_info(), cat.stretch_info()
    _, acc_rate, swap_rate = tempered(a.steps, True)

    def rate(name, n):
        s = np.array(times[name])
        return {"steps": n, "steps_per_s": round(n / float(np.median(s)), 1), "steps_per_s_min": round(n / float(s.max()), 1),
                "steps_per_s_max": round(n / float(s.min()), 1), "us_per_step": round(1e6 * float(np.median(s)) / n, 2)}

    line = {"tool": "tools/temper_probe.py", "stars": a.stars, "temps": t_n, "walkers": w, "rows_per_launch": rows,
            "betas": [float(b) for b in betas], "repeats": a.repeats}
    for name, _, n in variants:
        line[name] = rate(name, n)
    line["tempered_step_over_plain_stretch_step"] = round(line["tempered_resident"]["us_per_step"] /
                                                          line["stretch_resident_plain"]["us_per_step"], 3)
    line["plain_over_default_stretch_step"] = round(line["stretch_resident_plain"]["us_per_step"] /
                                                    line["stretch_resident_default"]["us_per_step"], 3)
    line["acceptance"] = round(acc_rate, 3)
    line["swap_acceptance"] = swap_rate
    line["temper_blocks"] = {k: after_t[k] - before_t[k] for k in after_t}
    line["stretch_blocks"] = {k: after_s[k] - before_s[k] for k in ("device_blocks", "host_blocks", "discarded_blocks")}
    text = json.dumps(line)
    print(text)
    out = a.out or os.path.join(ROOT, "profiles", "temper_probe_{0}_{1}x{2}.json".format(a.stars, t_n, w))
    with open(out, "w") as fh:
        fh.write(text + "\n")
    cat.close()


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Measurement instrument for the Hamiltonian Monte Carlo block: what a leapfrog point costs resident on
the device and host-driven, and effective samples per second of the slowest-mixing parameter against the resident stretch
move on the same catalogue.  No threshold is attached to any figure.

    python tools/hmc_probe.py --workload c3            # bench.py's C3 catalogue: CONST_BGFIXED, 4 parameters
    python tools/hmc_probe.py --workload m1            # bench.py's m1 catalogue: PROFILE, 6 parameters
    python tools/hmc_probe.py --workload free          # PROFILE_BGGAUSS with a free centre, 11 parameters (1e5 stars)

Per workload one JSON line, printed and written to profiles/hmc_probe_<workload>.json.  The catalogues and column orders
are those of bench.py (synthetic.make_catalog with its configuration numbers); every kernel column is a free parameter.

Method.  MAP by optimize.maximize_batch on the device gradient from a ball around the truth, Laplace covariance from
central differences of the gradient (what Runner.maximize / Runner.laplace do, on the kernel columns directly); when -H
is not positive definite the metric falls back to diag(1 / |H_jj|) and the line says so.  HMC: warm-up blocks of 10 steps
with eps *= exp(acceptance - 0.8), then the timed production blocks.  Stretch move: mcd_stretch_move_seeded, the walkers
started in the same Laplace ball.  Integrated autocorrelation time: emcee's estimator as the library has it
(mcmc_dynamics_amd.diagnostics) -- every walker's normalised autocorrelation function, averaged over the walkers, tau(M) = 1 + 2 sum_{t=1..M} rho_t at
the smallest window M with M >= c tau(M), c = 5 (Sokal).  For HMC the walkers are independent chains, for the stretch move
one ensemble; both are treated alike.  ESS = walkers x steps / tau, per second of the sampler's wall time (warm-up and
burn-in not counted on either side)."""
import argparse
import json
import os
import sys
import time
import warnings

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from mcmc_dynamics_amd import _native as native, diagnostics, synthetic   # noqa: E402
from mcmc_dynamics_amd.optimize import maximize_batch                  # noqa: E402

CENTRE = (synthetic.CENTER_RA_DEG, synthetic.CENTER_DEC_DEG)
INF = np.inf


def autocorr_time(chain, ctx, c=5.0):
    """chain (steps, walkers, parameters) -> integrated autocorrelation times in steps, per parameter: the library's
    estimator (mcmc_dynamics_amd.diagnostics, on the device) over all lags, without its length test -- `tau_reliable` below
    is this tool's."""
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return [float(v) for v in diagnostics.integrated_time(chain, c=c, tol=0, max_lag=chain.shape[0] - 1, quiet=True,
                                                              context=ctx)]


def workload(name, n_stars):
    t = synthetic.TRUTH
    if name == "c3":
        cat = synthetic.make_catalog(n_stars, config=3, background=True)
        from mcmc_dynamics_amd.background import Gaussian
        lnbg = Gaussian(t["v_back"], t["sigma_back"])(cat["v"], cat["verr"])
        kw = dict(model=native.MODEL_CONST_BGFIXED, centre=CENTRE, lnlike_bg=lnbg, pmember=cat["pmember"])
        names = ["v_sys", "sigma_max", "v_maxx", "v_maxy"]
        x = np.array([cat["truth"][k] for k in names])
        lo, hi = np.array([-INF, 0.0, -INF, -INF]), np.full(4, INF)
        ball = np.array([0.05, 0.05, 0.05, 0.05])
    elif name == "m1":
        cat = synthetic.make_catalog(n_stars, config=3, background=False)
        kw = dict(model=native.MODEL_PROFILE, centre=CENTRE)
        names = ["v_sys", "sigma_max", "a", "v_maxx", "v_maxy", "r_peak"]
        tr = cat["truth"]
        x = np.array([tr["v_sys"], tr["sigma_max"], 600.0, tr["v_maxx"], tr["v_maxy"], 150.0])
        lo, hi = np.array([-INF, 0.0, 1.0, -INF, -INF, 1.0]), np.array([INF, INF, 1e5, INF, INF, 1e5])
        ball = np.array([0.05, 0.05, 20.0, 0.05, 0.05, 5.0])
    else:
        cat = synthetic.make_catalog(n_stars, config=3, background=True)
        kw = dict(model=native.MODEL_PROFILE_BGGAUSS, centre=None, density=cat["density"])
        names = ["v_sys", "sigma_max", "a", "v_maxx", "v_maxy", "r_peak", "ra_center", "dec_center", "v_back", "sigma_back",
                 "f_back"]
        tr = cat["truth"]
        x = np.array([tr["v_sys"], tr["sigma_max"], 600.0, tr["v_maxx"], tr["v_maxy"], 150.0, CENTRE[0], CENTRE[1],
                      tr["v_back"], tr["sigma_back"], tr["f_back"]])
        lo = np.array([-INF, 0.0, 1.0, -INF, -INF, 1.0, CENTRE[0] - 0.05, CENTRE[1] - 0.05, -INF, 0.0, 0.0])
        hi = np.array([INF, INF, 1e5, INF, INF, 1e5, CENTRE[0] + 0.05, CENTRE[1] + 0.05, INF, INF, 1.0])
        ball = np.array([0.05, 0.05, 20.0, 0.05, 0.05, 5.0, 1e-4, 1e-4, 0.5, 0.5, 0.01])
    return cat, kw, names, x, lo, hi, ball


def laplace(fn, x, lo, hi, rel_step=1e-4):
    n_p = x.size
    width = np.where(np.isfinite(hi - lo), (hi - lo) / 100.0, 0.0)
    h = rel_step * np.maximum(np.maximum(np.abs(x), width), 1e-3)
    h = np.minimum(h, 0.5 * np.minimum(x - lo, hi - x))
    rows = np.tile(x, (2 * n_p, 1))
    rows[np.arange(n_p), np.arange(n_p)] += h
    rows[n_p + np.arange(n_p), np.arange(n_p)] -= h
    step = rows[:n_p].diagonal() - rows[n_p:].diagonal()
    _, grad = fn(rows)
    hess = (grad[:n_p] - grad[n_p:]) / step[:, None]
    return 0.5 * (hess + hess.T)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="c3", choices=("c3", "m1", "free"))
    ap.add_argument("--stars", type=int, default=None)
    ap.add_argument("--walkers", type=int, default=256)
    ap.add_argument("--leap", type=int, default=8)
    ap.add_argument("--hmc-steps", type=int, default=300)
    ap.add_argument("--hmc-warmup", type=int, default=60)
    ap.add_argument("--stretch-steps", type=int, default=3000)
    ap.add_argument("--stretch-burn", type=int, default=500)
    ap.add_argument("--host-steps", type=int, default=8, help="steps of the host-driven block that is timed")
    ap.add_argument("--seed", type=int, default=11)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    n_stars = a.stars if a.stars is not None else (100000 if a.workload == "free" else 1000000)
    cols, kw, names, x_true, lo, hi, ball = workload(a.workload, n_stars)
    ctx = native.default_context()
    cat = native.Catalog(ctx, cols["ra"], cols["dec"], cols["v"], cols["verr"], **kw)
    p = len(names)
    w = a.walkers
    plan = {"col_source": np.arange(p, dtype=np.int32), "col_const": np.zeros(p), "col_factor": np.ones(p), "lo": lo,
            "hi": hi, "fixed_ok": True}

    def fn(rows):
        return cat.loglike_grad(np.ascontiguousarray(rows))

    rng = np.random.default_rng(a.seed)
    starts = np.clip(x_true + ball * rng.normal(size=(64, p)), lo, hi)
    t0 = time.perf_counter()
    res = maximize_batch(fn, starts, lo, hi, max_iter=200, gtol=1e-8)
    f = np.where(np.isfinite(res["f"]), res["f"], -INF)
    best = int(np.argmax(f))
    x_map = res["x"][best]
    metric = "laplace"
    on_bound = bool(np.any(x_map <= lo) or np.any(x_map >= hi))
    hess = laplace(fn, np.clip(x_map, lo + 1e-9, hi - 1e-9) if on_bound else x_map, lo, hi)
    try:
        np.linalg.cholesky(-hess)
        cov = np.linalg.inv(-hess)
    except np.linalg.LinAlgError:
        metric = "diagonal 1/|H_jj| (-H not positive definite at the maximum found)"
        cov = np.diag(1.0 / np.maximum(np.abs(np.diag(hess)), 1e-300))
    chol = np.linalg.cholesky(cov)
    map_s = time.perf_counter() - t0
    pos0 = np.ascontiguousarray(np.clip(x_map + rng.normal(size=(w, p)) @ chol.T, lo, hi))

    # ---- HMC: warm-up (step-size adaptation), production (timed), a host-driven block (timed)
    def hmc(pos, eps, step0, n, resident, keep=True):
        cat.set_option("device_chain", 1 if resident else 0)
        chain = np.empty((n, w, p)) if keep else None
        acc, lnp, err = np.zeros(w, dtype=np.int64), np.empty(w), np.empty((n, w))
        t = time.perf_counter()
        cat.hmc_block(plan, chol, eps, a.leap, pos, lnp, a.seed, step0, n, chain, None, acc, err)
        return time.perf_counter() - t, chain, acc, err

    eps = 1.5 * p ** -0.25
    pos = pos0.copy()
    done = 0
    while done < a.hmc_warmup:
        _, _, acc, _ = hmc(pos, eps, done, 10, True, keep=False)
        eps *= float(np.exp(acc.sum() / (10.0 * w) - 0.8))
        done += 10
    hmc(pos.copy(), eps, done, 2, True, keep=False)                       # (scratch sized, pages touched)
    hmc_s, chain_h, acc_h, err_h = hmc(pos, eps, done, a.hmc_steps, True)
    host_pos = pos.copy()
    host_s, _, _, _ = hmc(host_pos, eps, done + a.hmc_steps, a.host_steps, False, keep=False)
    res_pos = pos.copy()
    res_s, _, _, _ = hmc(res_pos, eps, done + a.hmc_steps, a.host_steps, True, keep=False)
    info = cat.hmc_info()
    cat.set_option("device_chain", 1)
    tau_h = autocorr_time(chain_h, ctx)

    # ---- the resident stretch move on the same catalogue
    pos = pos0.copy()
    lnp = cat.loglike(np.ascontiguousarray(pos))
    acc = np.zeros(w, dtype=np.int64)
    cat.stretch_move_seeded(plan, pos, lnp, a.seed, 0, a.stretch_burn, None, None, acc)
    chain_s = np.empty((a.stretch_steps, w, p))
    acc = np.zeros(w, dtype=np.int64)
    t0 = time.perf_counter()
    cat.stretch_move_seeded(plan, pos, lnp, a.seed, a.stretch_burn, a.stretch_steps, chain_s, None, acc)
    stretch_s = time.perf_counter() - t0
    sinfo = cat.stretch_info()
    tau_s = autocorr_time(chain_s, ctx)

    def ess(tau, steps, seconds):
        worst = float(np.nanmax(tau))
        return {"tau_steps": [round(float(v), 2) for v in tau], "slowest": names[int(np.nanargmax(tau))],
                "tau_slowest": round(worst, 2), "tau_reliable": bool(steps >= 50 * worst),
                "ess_per_s": round(w * steps / worst / seconds, 1)}

    line = {
        "tool": "tools/hmc_probe.py", "workload": a.workload, "stars": n_stars, "walkers": w, "parameters": names,
        "map": {"converged": int(res["converged"].sum()), "of": 64, "seconds": round(map_s, 2), "metric": metric,
                "on_bound": on_bound},
        "hmc": dict({"n_leap": a.leap, "step_size": round(eps, 4), "steps": a.hmc_steps, "warmup_steps": a.hmc_warmup,
                     "acceptance": round(float(acc_h.sum()) / (a.hmc_steps * w), 3),
                     "median_energy_error": float(np.median(err_h)),
                     "us_per_leapfrog_resident": round(1e6 * hmc_s / (a.hmc_steps * a.leap), 2),
                     "us_per_leapfrog_resident_short_block": round(1e6 * res_s / (a.host_steps * a.leap + 1), 2),
                     "us_per_leapfrog_host_driven": round(1e6 * host_s / (a.host_steps * a.leap + 1), 2),
                     "blocks": info}, **ess(tau_h, a.hmc_steps, hmc_s)),
        "stretch": dict({"steps": a.stretch_steps, "burn": a.stretch_burn,
                         "acceptance": round(float(acc.sum()) / (a.stretch_steps * w), 3),
                         "us_per_step": round(1e6 * stretch_s / a.stretch_steps, 2), "blocks": sinfo},
                        **ess(tau_s, a.stretch_steps, stretch_s)),
    }
    line["ess_per_s_ratio_hmc_over_stretch"] = round(line["hmc"]["ess_per_s"] / line["stretch"]["ess_per_s"], 3)
    text = json.dumps(line)
    print(text)
    out = a.out or os.path.join(ROOT, "profiles", "hmc_probe_{0}.json".format(a.workload))
    with open(out, "w") as fh:
        fh.write(text + "\n")
    cat.close()


if __name__ == "__main__":
    main()

"""Test helper of moment matching for PSIS-LOO: the CPU build of csrc/mcd_mmatch.h (tests/emul/mmatch_emul.cpp), a NumPy
restatement of the algorithm on top of psis_helper (PSIS on given log weights, moments, the three transforms, the loop,
the split step), and the closed-form case the end-to-end tests share.

Closed form: ``ConstantFit`` without background and with a fixed centre, sigma_max fixed at SIGMA, v_sys / v_maxx / v_maxy
free in wide boxes.  v_los = v_sys + v_maxx sin(theta) - v_maxy cos(theta) is linear in the three parameters, so with
x_i = (1, sin theta_i, -cos theta_i) and n_i = verr_i^2 + SIGMA^2 the posterior is N(mu, Sigma), Sigma^-1 = sum x x^T / n,
and star i's exact leave-one-out density is log N(v_i; x_i^T mu_-i, n_i + x_i^T Sigma_-i x_i).

Test infrastructure only."""
import ctypes
import os
import subprocess

import numpy as np

import psis_helper as psh

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "emul", "mmatch_emul.cpp")
INC = os.path.join(ROOT, "mcmc_dynamics_amd", "csrc")
OUT = os.path.join(ROOT, "tests", "emul", "libmmatch_emul.so")
_lib = None
L = np.longdouble
SHIFT, SCALE, COV = 1, 2, 3
_p = ctypes.c_void_p


def lib():
    global _lib
    if _lib is None:
        deps = [SRC] + [os.path.join(INC, h) for h in ("mcd_mmatch.h", "mcd_prior.h", "mcd_rng.h", "mcd_math.h")]
        if not os.path.exists(OUT) or any(os.path.getmtime(d) > os.path.getmtime(OUT) for d in deps):
            subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-Wno-unknown-pragmas", "-I", INC,
                            SRC, "-o", OUT], check=True)
        lb = ctypes.CDLL(OUT)
        lb.emul_mm_moments.argtypes = [ctypes.c_int, ctypes.c_int64, _p, _p, _p]
        lb.emul_mm_moments.restype = None
        lb.emul_mm_trial.argtypes = [ctypes.c_int, ctypes.c_int, _p, _p, _p]
        lb.emul_mm_cholesky.argtypes = [ctypes.c_int, _p, _p]
        lb.emul_mm_compose.argtypes = [ctypes.c_int] + [_p] * 6
        lb.emul_mm_compose.restype = None
        lb.emul_mm_apply.argtypes = [ctypes.c_int, ctypes.c_int64] + [_p] * 4
        lb.emul_mm_apply.restype = None
        lb.emul_mm_inverse.argtypes = [ctypes.c_int] + [_p] * 5
        lb.emul_mm_rows_inside.argtypes = [ctypes.c_int, ctypes.c_int64, _p, _p, _p, ctypes.c_int32, _p, _p]
        lb.emul_mm_rows_inside.restype = None
        lb.emul_mm_lw_trial.argtypes = [ctypes.c_int64] + [_p] * 5
        lb.emul_mm_lw_trial.restype = None
        lb.emul_mm_lw_split.argtypes = [ctypes.c_int64] + [_p] * 4 + [ctypes.c_double, _p]
        lb.emul_mm_lw_split.restype = None
        lb.emul_mm_loop.argtypes = [ctypes.c_double, ctypes.c_double, ctypes.c_int, ctypes.c_int, ctypes.c_int] + [_p] * 7
        lb.emul_mm_max_level.argtypes = [ctypes.c_int, ctypes.c_int64, ctypes.c_int]
        lb.emul_mm_ranges.argtypes = [ctypes.c_int64, _p, ctypes.c_int64, _p, _p]
        lb.emul_mm_ranges.restype = ctypes.c_int64
        lb.emul_mm_stars_error.argtypes = [ctypes.c_int64, _p, ctypes.c_int64]
        lb.emul_mm_stars_error.restype = ctypes.c_char_p
        _lib = lb
    return _lib


def _c(a, dtype=np.float64):
    return np.ascontiguousarray(a, dtype=dtype)


# ---- the emulated header ----------------------------------------------------------------------------------------------
def emul_moments(rows, w):
    rows, w = _c(rows), _c(w)
    S, P = rows.shape
    mom = np.empty(3 * P + 2 * P * P)
    lib().emul_mm_moments(P, S, rows.ctypes.data, w.ctypes.data, mom.ctypes.data)
    return {"mu": mom[:P], "mu_w": mom[P:2 * P], "v_w": mom[2 * P:3 * P], "C": mom[3 * P:3 * P + P * P].reshape(P, P),
            "C_w": mom[3 * P + P * P:].reshape(P, P), "raw": mom}


def emul_trial(level, mom_raw, P):
    At, bt = np.empty((P, P)), np.empty(P)
    ok = lib().emul_mm_trial(P, level, _c(mom_raw).ctypes.data, At.ctypes.data, bt.ctypes.data)
    return bool(ok), At, bt


def emul_cholesky(a):
    a = _c(a)
    l = np.empty_like(a)
    return bool(lib().emul_mm_cholesky(a.shape[0], a.ctypes.data, l.ctypes.data)), l


def emul_compose(At, bt, A, b):
    P = len(b)
    A2, b2 = np.empty((P, P)), np.empty(P)
    lib().emul_mm_compose(P, _c(At).ctypes.data, _c(bt).ctypes.data, _c(A).ctypes.data, _c(b).ctypes.data, A2.ctypes.data,
                          b2.ctypes.data)
    return A2, b2


def emul_apply(A, b, x):
    x = _c(x)
    y = np.empty_like(x)
    lib().emul_mm_apply(x.shape[1], x.shape[0], _c(A).ctypes.data, _c(b).ctypes.data, x.ctypes.data, y.ctypes.data)
    return y


def emul_inverse(A, b):
    P = len(b)
    Ai, bi, lad = np.empty((P, P)), np.empty(P), np.zeros(1)
    ok = lib().emul_mm_inverse(P, _c(A).ctypes.data, _c(b).ctypes.data, Ai.ctypes.data, bi.ctypes.data, lad.ctypes.data)
    return bool(ok), Ai, bi, float(lad[0])


def emul_rows_inside(x, lo, hi, kind=None, fixed_ok=1):
    x = _c(x)
    S, P = x.shape
    kind = _c(np.zeros(P) if kind is None else kind, np.int32)
    out = np.empty(S, dtype=np.int32)
    lib().emul_mm_rows_inside(P, S, _c(lo).ctypes.data, _c(hi).ctypes.data, kind.ctypes.data, int(fixed_ok), x.ctypes.data,
                              out.ctypes.data)
    return out.astype(bool)


def emul_lw_trial(inside, train, lnprior, lp0):
    out = np.empty(len(train))
    lib().emul_mm_lw_trial(len(train), _c(inside, np.int32).ctypes.data, _c(train).ctypes.data, _c(lnprior).ctypes.data,
                           _c(lp0).ctypes.data, out.ctypes.data)
    return out


def emul_lw_split(num, lpf, inv_inside, lp_inv, lad):
    out = np.empty(len(num))
    lib().emul_mm_lw_split(len(num), _c(num).ctypes.data, _c(lpf).ctypes.data, _c(inv_inside, np.int32).ctypes.data,
                           _c(lp_inv).ctypes.data, float(lad), out.ctypes.data)
    return out


def emul_loop(k0, thr, max_iters, max_level, k_trial, usable):
    """The header's decision loop fed a script of trial results -> dict."""
    kt, us = _c(k_trial), _c(usable, np.int32)
    n = kt.size
    k, it, acc = np.zeros(1), np.zeros(1, np.int32), np.zeros(3, np.int32)
    lev, accs = np.zeros(n, np.int32), np.zeros(n, np.int32)
    used = lib().emul_mm_loop(float(k0), float(thr), int(max_iters), int(max_level), n, kt.ctypes.data, us.ctypes.data,
                              k.ctypes.data, it.ctypes.data, acc.ctypes.data, lev.ctypes.data, accs.ctypes.data)
    running = used < 0
    used = -used - 1 if running else used
    return {"k": float(k[0]), "iterations": int(it[0]), "accepted": acc, "levels": lev[:used], "accepts": accs[:used],
            "running": running}


def emul_ranges(n_stars, stars):
    stars = _c(stars, np.int64)
    r, sr = np.empty(2 * stars.size + 2, np.int64), np.empty(stars.size, np.int64)
    n = lib().emul_mm_ranges(int(n_stars), stars.ctypes.data, stars.size, r.ctypes.data, sr.ctypes.data)
    return r[:n + 1], sr


def emul_stars_error(stars, n_stars):
    stars = _c(stars, np.int64)
    msg = lib().emul_mm_stars_error(stars.size, stars.ctypes.data if stars.size else None, int(n_stars))
    return None if msg is None else msg.decode()


# ---- NumPy oracle ---------------------------------------------------------------------------------------------------
def psis_lw(lw, r_eff=1.0):
    """PSIS of given log ratios (-inf allowed): (smoothed, truncated log weights shifted so that the raw maximum is 0, k^):
    psis_helper.psis_star with the ratios as input."""
    lw = np.asarray(lw, dtype=np.float64)
    S = lw.size
    M = psh.tail_len(S, r_eff)
    with np.errstate(invalid="ignore"):
        lw = lw - np.max(lw)
    k_hat = np.inf
    if M >= 5:
        order = np.argsort(lw, kind="stable")
        tail = order[S - M:]
        cutoff = lw[order[S - M - 1]]
        vals = lw[tail]
        with np.errstate(all="ignore"):
            if vals.max() - vals.min() < np.finfo(np.float64).eps / 100.0:
                k_hat = -np.inf
            else:
                x = np.exp(vals) - np.exp(cutoff)
                k_hat, sigma = psh.gpdfit(x)
                if np.isfinite(k_hat):
                    p = (np.arange(1, M + 1) - 0.5) / M
                    q = -sigma * np.log1p(-p) if k_hat == 0.0 else sigma * np.expm1(-k_hat * np.log1p(-p)) / k_hat
                    lw = lw.copy()
                    lw[tail] = np.log(q + np.exp(cutoff))
    return np.minimum(lw, 0.0), float(k_hat)


def weights_summary(lw_s, li, r_eff=1.0):
    """(elpd, n_eff, normalised weights) of smoothed log weights and the star's own terms."""
    w = np.exp(lw_s - psh._lse(lw_s))
    with np.errstate(divide="ignore"):
        terms = np.where(w > 0, np.log(np.where(w > 0, w, 1.0)) + li, -np.inf)
    return psh._lse(terms), r_eff / np.sum(w * w), w


def moments(rows, w):
    """w: normalised weights."""
    S = rows.shape[0]
    mu, mu_w = rows.mean(axis=0), w @ rows
    d, dw = rows - mu, rows - mu_w
    C = d.T @ d / (S - 1)
    sw = (dw * w[:, None]).T @ dw
    return {"mu": mu, "mu_w": mu_w, "v_w": np.diag(sw) * S / (S - 1), "C": C, "C_w": sw / (1.0 - np.sum(w * w))}


def trial(level, m):
    """(At, bt) of the level from the moments, or None when T3 is skipped."""
    P = m["mu"].size
    if level == SHIFT:
        return np.eye(P), m["mu_w"] - m["mu"]
    if level == SCALE:
        v = np.diag(m["C"])
        with np.errstate(all="ignore"):
            s = np.sqrt(m["v_w"] / v)
        s = np.where((v > 0) & np.isfinite(s) & (s > 0), s, 1.0)
        return np.diag(s), m["mu_w"] - s * m["mu"]
    try:
        l, lw = np.linalg.cholesky(m["C"]), np.linalg.cholesky(m["C_w"])
    except np.linalg.LinAlgError:
        return None
    M = lw @ np.linalg.inv(l)
    return M, m["mu_w"] - M @ m["mu"]


def moment_match(draws, evaluate, inside, lnprior, k_threshold, max_iters=30, cov=True, split=True, r_eff=1.0, fixed_map=None):
    """One star.  ``evaluate(theta (n, P)) -> (train (n,), test (n,))`` for rows inside the prior, ``inside(theta) -> bool
    (n,)``, ``lnprior(theta) -> (n,)``.  ``fixed_map`` = (A, b): skip the loop and take this total map (what a device
    run returned), so that only the final weights are recomputed."""
    draws = np.asarray(draws, dtype=np.float64)
    S, P = draws.shape

    def ev(theta):
        ok = inside(theta)
        rows = np.where(ok[:, None], theta, theta[np.flatnonzero(ok)[0]] if ok.any() else draws)
        tr, te = evaluate(rows)
        return ok, tr, te, np.where(ok, lnprior(rows), 0.0)

    ok, tr, te, pr = ev(draws)
    assert ok.all(), "a draw outside the prior"
    lp0 = tr + te + pr
    lw_raw = -te
    lw_s, k = psis_lw(lw_raw, r_eff)
    A, b = np.eye(P), np.zeros(P)
    out = {"k_before": k, "iterations": 0, "accepted": np.zeros(3, dtype=int)}
    rows, li = draws, te
    max_level = COV if cov and S > 10 * P else SCALE
    if fixed_map is not None:
        A, b = np.asarray(fixed_map[0], dtype=np.float64), np.asarray(fixed_map[1], dtype=np.float64)
        if not (np.array_equal(A, np.eye(P)) and not b.any()):
            rows = draws @ A.T + b
            ok, tr, te, pr = ev(rows)
            with np.errstate(invalid="ignore"):
                lw_raw = np.where(ok, tr + pr - lp0, -np.inf)
            lw_s, k = psis_lw(lw_raw, r_eff)
            li = te
            out["accepted"][0] = 1
    else:
        while k > k_threshold and out["iterations"] < max_iters:
            out["iterations"] += 1
            w = np.exp(lw_s - psh._lse(lw_s))
            m = moments(rows, w)
            hit = False
            for level in range(SHIFT, max_level + 1):
                t = trial(level, m)
                if t is None:
                    continue
                A2, b2 = t[0] @ A, t[0] @ b + t[1]
                rows2 = draws @ A2.T + b2
                ok, tr, te, pr = ev(rows2)
                if not ok.any():
                    continue
                with np.errstate(invalid="ignore"):
                    raw2 = np.where(ok, tr + pr - lp0, -np.inf)
                lw2, k2 = psis_lw(raw2, r_eff)
                if k2 < k:
                    A, b, rows, li, lw_s, lw_raw, k, hit = A2, b2, rows2, te, lw2, raw2, k2, True
                    out["accepted"][level - 1] += 1
                    break
            if not hit:
                break
    out["k_loop"] = k
    if split and out["accepted"].sum() > 0:
        h = S // 2
        fwd = np.vstack([(draws @ A.T + b)[:h], draws[h:]])
        Ai = np.linalg.inv(A)
        back = np.vstack([draws[:h], (draws[h:] - b) @ Ai.T])
        ok_f, tr_f, te_f, pr_f = ev(fwd)
        ok_i, tr_i, te_i, pr_i = ev(back)
        lad = np.linalg.slogdet(A)[1]
        with np.errstate(invalid="ignore"):
            lp_i = np.where(ok_i, tr_i + te_i + pr_i - lad, -np.inf)
            lw = np.where(ok_f, tr_f + pr_f - np.logaddexp(tr_f + te_f + pr_f, lp_i), -np.inf)
        lw_raw = lw
        lw_s, k = psis_lw(lw, r_eff)
        li = te_f
    elpd, n_eff, w = weights_summary(lw_s, li, r_eff)
    out.update({"elpd": elpd, "pareto_k": k, "n_eff": n_eff, "A": A, "b": b, "weights": w, "lw_raw": lw_raw, "li": li})
    return out


# ---- the closed-form case -------------------------------------------------------------------------------------------
SIGMA, N_STARS, N_DRAWS, OUTLIER = 5.0, 20, 4096, 8.0
TRUTH = np.array([2.0, 3.0, -1.5])                                   # v_sys, v_maxx, v_maxy


def closed_form_columns(seed, outlier=OUTLIER):
    """20 stars round the synthetic centre, verr in U(0.5, 2), star 0 moved `outlier` sigma off."""
    from mcmc_dynamics_amd import synthetic
    rng = np.random.default_rng(1000 + seed)
    ang, rad = rng.uniform(0, 2 * np.pi, N_STARS), rng.uniform(20.0, 200.0, N_STARS) / 3600.0
    dec = synthetic.CENTER_DEC_DEG + rad * np.sin(ang)
    ra = synthetic.CENTER_RA_DEG + rad * np.cos(ang) / np.cos(np.deg2rad(synthetic.CENTER_DEC_DEG))
    verr = rng.uniform(0.5, 2.0, N_STARS)
    cols = {"ra": ra, "dec": dec, "verr": verr, "v": np.zeros(N_STARS)}
    X = design(cols)
    n = verr ** 2 + SIGMA ** 2
    v = X @ TRUTH + np.sqrt(n) * rng.normal(size=N_STARS)
    v[0] = X[0] @ TRUTH + outlier * np.sqrt(n[0])
    cols["v"] = v
    return cols


def design(cols):
    """x_i = (1, sin theta_i, -cos theta_i) with the position angle of the oracle (oracle/lnprob_numpy.py)."""
    from mcmc_dynamics_amd import synthetic
    from oracle import lnprob_numpy as oracle
    sin_t, cos_t = oracle.star_geometry_fixed(cols["ra"], cols["dec"], synthetic.CENTER_RA_DEG, synthetic.CENTER_DEC_DEG)
    return np.stack([np.ones(sin_t.size), sin_t, -cos_t], axis=1)


def posterior(cols, X, leave=None):
    """(mu, Sigma) in long double of all stars, or without star `leave`."""
    n = (cols["verr"].astype(L)) ** 2 + L(SIGMA) ** 2
    keep = np.ones(n.size, dtype=bool)
    if leave is not None:
        keep[leave] = False
    Xl = X.astype(L)[keep]
    prec = (Xl / n[keep, None]).T @ Xl
    cov = np.linalg.inv(prec.astype(np.float64)).astype(L)
    cov = cov @ (2 * np.eye(3, dtype=L) - prec @ cov)                 # one Newton step in long double
    mu = cov @ ((Xl / n[keep, None]).T @ cols["v"].astype(L)[keep])
    return mu, cov


def exact_loo(cols, X, i):
    mu, cov = posterior(cols, X, leave=i)
    x = X[i].astype(L)
    var = L(cols["verr"][i]) ** 2 + L(SIGMA) ** 2 + x @ cov @ x
    return float(-0.5 * (np.log(2 * L(np.pi) * var) + (L(cols["v"][i]) - x @ mu) ** 2 / var))


def exact_draws(cols, X, seed, n=N_DRAWS):
    mu, cov = posterior(cols, X)
    return np.random.default_rng(2000 + seed).multivariate_normal(mu.astype(np.float64), cov.astype(np.float64), size=n)


def numpy_evaluate(cols, X, i):
    """evaluate() of moment_match for star i by the Gaussian terms in NumPy."""
    n = cols["verr"] ** 2 + SIGMA ** 2

    def fn(theta):
        terms = -0.5 * (np.log(2 * np.pi * n) + (cols["v"] - theta @ X.T) ** 2 / n)       # (rows, stars)
        return terms.sum(axis=1) - terms[:, i], terms[:, i]
    return fn


def closed_form_fit(cols, **kwargs):
    """ConstantFit with v_sys, v_maxx, v_maxy free in wide boxes."""
    from mcmc_dynamics_amd import DataReader, synthetic
    from mcmc_dynamics_amd.analysis import ConstantFit
    fit = ConstantFit(DataReader(dict(cols)), **kwargs)
    for name in ("v_sys", "v_maxx", "v_maxy"):
        fit.parameters[name].set(min=-1000.0, max=1000.0, fixed=False)
    fit.parameters["sigma_max"].set(value=SIGMA, fixed=True)
    fit.parameters["ra_center"].set(value=synthetic.CENTER_RA_DEG, fixed=True)
    fit.parameters["dec_center"].set(value=synthetic.CENTER_DEC_DEG, fixed=True)
    return fit

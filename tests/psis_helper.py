"""Test helper: CPU build of the per-star PSIS-LOO arithmetic (tests/emul/psis_emul.cpp + csrc/mcd_psis.h + csrc/mcd_math.h)
and the NumPy oracle it is checked against, written from the definition of PSIS in psis() / loo() of the R package loo
(Vehtari, Gelman & Gabry 2017; Zhang & Stephens 2009 for the generalized Pareto fit), with one deliberate deviation: a
constant tail gets k^ = -inf (loo: +inf).  Test infrastructure only."""
import ctypes
import math
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "emul", "psis_emul.cpp")
INC = os.path.join(ROOT, "mcmc_dynamics_amd", "csrc")
OUT = os.path.join(ROOT, "tests", "emul", "libpsis_emul.so")
_lib = None


def lib():
    global _lib
    if _lib is None:
        deps = [SRC] + [os.path.join(INC, f) for f in ("mcd_psis.h", "mcd_math.h", "mcd_exp_table.h")]
        if not os.path.exists(OUT) or any(os.path.getmtime(d) > os.path.getmtime(OUT) for d in deps):
            subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-I", INC, SRC,
                            "-o", OUT], check=True)
        L = ctypes.CDLL(OUT)
        L.emul_psis.argtypes = [ctypes.c_int64, ctypes.c_int64, ctypes.c_void_p, ctypes.c_double, ctypes.c_void_p]
        L.emul_gpd_fit.argtypes = [ctypes.c_void_p, ctypes.c_int64, ctypes.POINTER(ctypes.c_double)]
        L.emul_gpd_fit.restype = ctypes.c_double
        L.emul_psis_tail_len.argtypes = [ctypes.c_int64, ctypes.c_double]
        L.emul_psis_tail_len.restype = ctypes.c_int64
        L.emul_psis_tile_stars.argtypes = [ctypes.c_int64] * 4
        L.emul_psis_tile_stars.restype = ctypes.c_int64
        L.emul_psis_key.argtypes = [ctypes.c_double]
        L.emul_psis_key.restype = ctypes.c_uint64
        _lib = L
    return _lib


FIELDS = ("elpd_loo", "pareto_k", "lppd", "n_eff")


def emul_psis(lnl, r_eff=1.0):
    """Emulated per-star routine: lnl (n, S) -> dict of (n,) arrays."""
    x = np.ascontiguousarray(lnl, dtype=np.float64)
    n, S = x.shape
    out = np.empty((4, n))
    assert lib().emul_psis(n, S, x.ctypes.data, float(r_eff), out.ctypes.data) == 0
    return dict(zip(FIELDS, out))


def emul_gpd_fit(x):
    x = np.ascontiguousarray(np.sort(x), dtype=np.float64)
    sigma = ctypes.c_double(0.0)
    k = lib().emul_gpd_fit(x.ctypes.data, x.size, ctypes.byref(sigma))
    return k, sigma.value


# ---- NumPy oracle ------------------------------------------------------------------------------------------------
def tail_len(S, r_eff=1.0):
    return int(min(math.ceil(0.2 * S), math.ceil(3.0 * math.sqrt(S / r_eff))))


def gpdfit(x):
    """Zhang & Stephens (2009) as loo's gpdfit states it; x ascending.  Returns (k^ adjusted, sigma)."""
    M = x.size
    m = 30 + int(np.floor(np.sqrt(M)))
    x_star = x[int(np.floor(M / 4.0 + 0.5)) - 1]
    j = np.arange(1, m + 1, dtype=np.float64)
    with np.errstate(all="ignore"):
        theta = 1.0 / x[-1] + (1.0 - np.sqrt(m / (j - 0.5))) / (3.0 * x_star)
        k = np.array([np.mean(np.log1p(-t * x)) for t in theta])
        l_theta = M * (np.log(-theta / k) - k - 1.0)
        mx = np.max(l_theta)
        lse = mx + np.log(np.sum(np.exp(l_theta - mx)))
        w = np.exp(l_theta - lse)
        theta_hat = np.sum(theta * w)
        k = np.mean(np.log1p(-theta_hat * x))
        sigma = -k / theta_hat
        k_hat = (M * k + 5.0) / (M + 10.0)
    if np.isnan(k_hat):
        k_hat = np.inf
    return float(k_hat), float(sigma)


def _lse(a):
    mx = np.max(a)
    return mx + np.log(np.sum(np.exp(a - mx)))


def psis_star(lnl, r_eff=1.0):
    """One star's (elpd_loo, k^, lppd, n_eff) from its S values of lnL."""
    lnl = np.asarray(lnl, dtype=np.float64)
    S = lnl.size
    M = tail_len(S, r_eff)
    r = -lnl
    lw = r - r.max()
    k_hat = np.inf
    if M >= 5:
        order = np.argsort(lw, kind="stable")                        # ascending, ties by sample index
        tail = order[S - M:]
        cutoff = lw[order[S - M - 1]]
        vals = lw[tail]
        if vals.max() - vals.min() < np.finfo(np.float64).eps / 100.0:
            k_hat = -np.inf
        else:
            x = np.exp(vals) - np.exp(cutoff)
            k_hat, sigma = gpdfit(x)
            if np.isfinite(k_hat):
                p = (np.arange(1, M + 1) - 0.5) / M
                if k_hat == 0.0:
                    q = -sigma * np.log1p(-p)
                else:
                    q = sigma * np.expm1(-k_hat * np.log1p(-p)) / k_hat
                lw = lw.copy()
                lw[tail] = np.log(q + np.exp(cutoff))
    lw = np.minimum(lw, 0.0)
    elpd = _lse(lw + lnl) - _lse(lw)
    lppd = _lse(lnl) - np.log(S)
    w = np.exp(lw - _lse(lw))
    return elpd, k_hat, lppd, r_eff / np.sum(w * w)


def numpy_psis(lnl, r_eff=1.0):
    """Oracle over an (n, S) matrix of lnL."""
    rows = [psis_star(row, r_eff) for row in np.atleast_2d(lnl)]
    a = np.array(rows).T
    return dict(zip(FIELDS, a))


def k_threshold(S):
    return min(1.0 - 1.0 / np.log10(S), 0.7)


def k_noise(lnl, r_eff=1.0, seed=0):
    """Per star, how far the oracle's own k^ moves when every lnL_is moves by one ulp: x = exp(tail) - exp(cutoff)
    cancels for tail values next to the cutoff, so k^ can only be as close as its inputs allow.  Terms from two device
    kernels (mcd_psis_loo's and loglike_per_star's) may differ in the last bit."""
    lnl = np.asarray(lnl, dtype=np.float64)
    sign = np.where(np.random.default_rng(seed).uniform(size=lnl.shape) < 0.5, -1.0, 1.0)
    moved = lnl + sign * np.spacing(lnl)
    a, b = numpy_psis(lnl, r_eff)["pareto_k"], numpy_psis(moved, r_eff)["pareto_k"]
    with np.errstate(invalid="ignore"):
        d = np.abs(a - b)
    return np.where(np.isfinite(d), d, 0.0)


def assert_matches(got, want, elpd_tol=1e-11, k_tol=1e-10, lppd_tol=1e-12):
    """The issue's tolerances: |d elpd_i| <= 1e-11 max(1, |elpd_i|), |d k^| <= 1e-10 (infinities equal).  ``k_tol`` may
    be an array (per star)."""
    e, we = np.asarray(got["elpd_loo"]), np.asarray(want["elpd_loo"])
    assert np.all(np.abs(e - we) <= elpd_tol * np.maximum(1.0, np.abs(we))), float(np.max(np.abs(e - we)))
    k, wk = np.asarray(got["pareto_k"]), np.asarray(want["pareto_k"])
    fin = np.isfinite(wk)
    assert np.array_equal(np.isfinite(k), fin) and np.array_equal(k[~fin], wk[~fin])
    k_tol = np.broadcast_to(np.asarray(k_tol, dtype=np.float64), wk.shape)[fin]
    assert np.all(np.abs(k[fin] - wk[fin]) <= k_tol), float(np.max(np.abs(k[fin] - wk[fin]) - k_tol))
    l, wl = np.asarray(got["lppd"]), np.asarray(want["lppd"])
    assert np.all(np.abs(l - wl) <= lppd_tol * np.maximum(1.0, np.abs(wl)))
    ne, wn = np.asarray(got["n_eff"]), np.asarray(want["n_eff"])
    assert np.all(np.abs(ne - wn) <= 1e-9 * np.abs(wn))


# ---- synthetic lnL matrices --------------------------------------------------------------------------------------
def near_gaussian(n, S, seed=1):
    rng = np.random.default_rng(seed)
    return -3.0 + rng.normal(scale=0.3, size=(n, 1)) + rng.normal(scale=0.2, size=(n, S))


def heavy_tailed(n, S, seed=2):
    """lnL whose importance ratios exp(-lnL) are Pareto with tail index 1/k, k in [0.8, 1.2] per star (k^ > 0.7)."""
    rng = np.random.default_rng(seed)
    k = rng.uniform(0.8, 1.2, size=(n, 1))
    return -2.0 + k * np.log(rng.uniform(size=(n, S))) + rng.normal(scale=0.01, size=(n, S))


def repeated_rows(n, S, seed=3):
    """Runs of exactly repeated samples, as rejected moves leave them in a chain."""
    rng = np.random.default_rng(seed)
    x = -4.0 + rng.normal(scale=0.5, size=(n, S))
    reps = rng.integers(1, 12, size=S)
    idx = np.repeat(np.arange(S), reps)[:S]
    return np.ascontiguousarray(x[:, idx])

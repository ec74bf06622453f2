"""Test helper: the NumPy oracle of the chain diagnostics (``mcd_chain_diagnostics``, csrc/mcd_diag.h) and the CPU build of
that header (tests/emul/diag_emul.cpp).  Test infrastructure only.

The definitions are those of emcee's ``autocorr.integrated_time`` (emcee is not installed where the tests run: they are
restated here, and this file is what the library is held to):

* a series is one walker's samples of one parameter; ``y = x - mean(x)``;
* ``a_k = sum_t y_t y_{t+k}`` (no ``1 / (T - k)``), ``rho_k = a_k / a_0`` per walker, then the mean over the walkers;
* ``tau_k = 2 sum_{j <= k} rho_j - 1``; the window is the smallest ``k`` with ``k >= c tau_k``.

The oracle takes every sum in ``np.longdouble`` (direct lag sums, no FFT); ``fft_rho`` is emcee's FFT route in float64, kept
as a cross-check of the definition.  Split-R-hat is BDA3's (Gelman et al. 2013, section 11.4)."""
import ctypes
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "emul", "diag_emul.cpp")
INC = os.path.join(ROOT, "mcmc_dynamics_amd", "csrc")
OUT = os.path.join(ROOT, "tests", "emul", "libdiag_emul.so")
_lib = None

LD = np.longdouble
EPS = 2.0 ** -53


def lib():
    global _lib
    if _lib is None:
        deps = [SRC, os.path.join(INC, "mcd_diag.h"), os.path.join(INC, "mcd_math.h")]
        if not os.path.exists(OUT) or any(os.path.getmtime(d) > os.path.getmtime(OUT) for d in deps):
            subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-I", INC, SRC, "-o", OUT],
                           check=True)
        _lib = ctypes.CDLL(OUT)
        _lib.emul_diag_groups.argtypes = [ctypes.c_int64, ctypes.c_int64, ctypes.c_int64, ctypes.c_int, ctypes.c_int64,
                                          ctypes.c_double, ctypes.c_int64, ctypes.c_int64] + [ctypes.c_void_p] * 8
        _lib.emul_diag_lag_sums.argtypes = [ctypes.c_void_p, ctypes.c_int64, ctypes.c_int64, ctypes.c_int64, ctypes.c_void_p]
        _lib.emul_diag_lag_sums.restype = None
        _lib.emul_diag_tile_groups.argtypes = [ctypes.c_int64, ctypes.c_int64, ctypes.c_int64, ctypes.c_int, ctypes.c_int64,
                                               ctypes.c_int64]
        _lib.emul_diag_tile_groups.restype = ctypes.c_int64
    return _lib


def empty_outputs(G, P, L, want_rho=True):
    out = {"tau": np.full((G, P), -7.0), "window": np.full((G, P), -7, dtype=np.int64),
           "found": np.full((G, P), -7, dtype=np.int32), "rhat": np.full((G, P), -7.0), "mean": np.full((G, P), -7.0),
           "var": np.full((G, P), -7.0)}
    if want_rho:
        out["rho"] = np.full((G, P, L + 1), -7.0)
    return out


def emul(chain, L, c=5.0, tiles=None, want_rho=True):
    """The header's host loop on chain (T, G, W, P); ``tiles``: a list of (g0, ng) to run it in pieces."""
    chain = np.ascontiguousarray(chain, dtype=np.float64)
    T, G, W, P = chain.shape
    out = empty_outputs(G, P, L, want_rho)
    for g0, ng in (tiles or [(0, G)]):
        rc = lib().emul_diag_groups(T, G, W, P, L, c, g0, ng, chain.ctypes.data, out["tau"].ctypes.data,
                                    out["window"].ctypes.data, out["found"].ctypes.data, out["rhat"].ctypes.data,
                                    out["mean"].ctypes.data, out["var"].ctypes.data,
                                    out["rho"].ctypes.data if want_rho else None)
        assert rc == 0
    return out


def emul_lag_sums(x, L):
    x = np.ascontiguousarray(x, dtype=np.float64)
    a = np.empty(L + 1)
    lib().emul_diag_lag_sums(x.ctypes.data, 1, x.size, L, a.ctypes.data)
    return a


def tile_groups(T, G, W, P, L, budget_bytes):
    return int(lib().emul_diag_tile_groups(T, G, W, P, L, int(budget_bytes)))


# ---- the oracle -----------------------------------------------------------------------------------------------------
def exact_rho(chain, L):
    """rho (G, P, L + 1) in longdouble: per walker a_k / a_0 by direct sums, then the mean over the walkers."""
    x = np.asarray(chain, dtype=LD)
    T = x.shape[0]
    d = x - x[:1]                          # exact in longdouble for a float64 series: y below is x - mean(x) to 2^-64 of the
    y = d - d.mean(axis=0)                 # series' WIDTH; without it a column at 56.3 +- 1e-8 leaves the oracle 6e-12 off
    a0 = (y * y).sum(axis=0)
    rho = np.empty(x.shape[1:2] + x.shape[3:] + (L + 1,), dtype=LD)
    with np.errstate(invalid="ignore", divide="ignore"):
        for k in range(L + 1):
            ak = (y[:T - k] * y[k:]).sum(axis=0)                       # (G, W, P)
            rho[..., k] = (ak / a0).mean(axis=1)
    return rho


def window_of(rho, c):
    """(tau, window, found, margin) of one rho row (longdouble); margin = min_k |k - c tau_k|."""
    taus = 2 * np.cumsum(rho) - 1
    k = np.arange(rho.size)
    if not np.all(np.isfinite(taus.astype(np.float64))):
        return np.nan, rho.size - 1, 0, np.inf
    hit = np.nonzero(k >= c * taus)[0]
    margin = float(np.min(np.abs(k - c * taus)))
    if hit.size:
        return taus[hit[0]], int(hit[0]), 1, margin
    return taus[-1], rho.size - 1, 0, margin


def exact(chain, L, c=5.0):
    """Every output of mcd_chain_diagnostics for chain (T, G, W, P), in longdouble, plus ``margin`` (G, P)."""
    x = np.asarray(chain, dtype=LD)
    T, G, W, P = x.shape
    rho = exact_rho(chain, L)
    out = {"rho": rho, "tau": np.empty((G, P), dtype=LD), "window": np.empty((G, P), dtype=np.int64),
           "found": np.empty((G, P), dtype=np.int32), "margin": np.empty((G, P))}
    for g in range(G):
        for p in range(P):
            out["tau"][g, p], out["window"][g, p], out["found"][g, p], out["margin"][g, p] = window_of(rho[g, p], c)
    ref = x[:1, :, :1, :]                                             # (as in exact_rho: exact, and no change of definition)
    x = x - ref
    flat = np.moveaxis(x, 0, 1).reshape(G, T * W, P)
    mean = flat.mean(axis=1)
    out["mean"] = mean + ref[0, :, 0, :]
    out["var"] = ((flat - mean[:, None, :]) ** 2).sum(axis=1) / (T * W - 1)
    n = T // 2
    rhat = np.full((G, P), np.nan, dtype=LD)
    if T >= 4:
        halves = np.concatenate([x[:n], x[T - n:]], axis=2)           # (n, G, 2 W, P)
        m = 2 * W
        hm = halves.mean(axis=0)                                      # (G, m, P)
        hv = ((halves - hm) ** 2).sum(axis=0) / (n - 1)
        B = LD(n) / (m - 1) * ((hm - hm.mean(axis=1, keepdims=True)) ** 2).sum(axis=1)
        Wv = hv.mean(axis=1)
        still = np.any(np.all(x == x[:1], axis=0), axis=1)            # (G, P): a walker that never moves
        with np.errstate(invalid="ignore", divide="ignore"):
            r = np.sqrt((LD(n - 1) / n * Wv + B / n) / Wv)
        rhat = np.where((Wv > 0) & ~still, r, np.nan)
    out["rhat"] = rhat
    return out


def fft_rho(chain, L):
    """emcee's route in float64: per walker the autocorrelation by a zero-padded FFT, normalised, then the walkers' mean."""
    x = np.asarray(chain, dtype=np.float64)
    T = x.shape[0]
    n = 1 << int(np.ceil(np.log2(2 * T)))
    f = np.fft.fft(x - x.mean(axis=0), n=n, axis=0)
    acf = np.fft.ifft(f * np.conjugate(f), axis=0)[:T].real
    acf = acf / acf[0]
    return np.moveaxis(acf[:L + 1].mean(axis=2), 0, -1)              # (G, P, L + 1)


def fft_tau(chain, c=5.0):
    """emcee's integrated_time in NumPy float64 (all lags by FFT, automatic window): tau (G, P).  What tools/diag_probe.py
    times beside the library."""
    x = np.asarray(chain, dtype=np.float64)
    rho = fft_rho(x, x.shape[0] - 1)
    taus = 2.0 * np.cumsum(rho, axis=-1) - 1.0
    m = np.arange(rho.shape[-1]) < c * taus
    window = np.where(np.any(~m, axis=-1), np.argmin(m, axis=-1), rho.shape[-1] - 1)
    return np.take_along_axis(taus, window[..., None], axis=-1)[..., 0]


def ar1(rng, phi, shape, T):
    """Stationary AR(1) series of unit marginal variance: (T,) + shape."""
    x = np.empty((T,) + tuple(shape))
    x[0] = rng.standard_normal(shape)
    e = rng.standard_normal((T,) + tuple(shape)) * np.sqrt(1.0 - phi * phi)
    for t in range(1, T):
        x[t] = phi * x[t - 1] + e[t]
    return x

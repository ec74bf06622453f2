"""Test helper: CPU build of the series reciprocal root and the verr-sorted record array of the main kernel
(tests/emul/root_series_emul.cpp + csrc/mcd_math.h: RootSeries, csrc/mcd_chunks.h).  Test infrastructure only."""
import ctypes
import os
import subprocess

import numpy as np

import emul_helper as emul

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "emul", "root_series_emul.cpp")
INC = os.path.join(ROOT, "mcmc_dynamics_amd", "csrc")
OUT = os.path.join(ROOT, "tests", "emul", "libroot_series_emul.so")
_lib = None


def lib():
    global _lib
    if _lib is None:
        deps = [SRC] + [os.path.join(INC, f) for f in ("mcd_math.h", "mcd_guard.h", "mcd_chunks.h", "mcd_exp_table.h")]
        if not os.path.exists(OUT) or any(os.path.getmtime(d) > os.path.getmtime(OUT) for d in deps):
            subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-I", INC, SRC,
                            "-o", OUT], check=True)
        _lib = ctypes.CDLL(OUT)
    return _lib


# ---- verr-sorted records and the series reciprocal root (csrc/mcd_math.h: RootSeries) ----------------------------
def series_root(eb, half, s2, e, seed_err=0.0):
    """(g, ok, newton): the series root about centre ``eb`` for sigma^2 ``s2`` at verr^2 ``e``, the lane's verdict for a
    band of half-width ``half``, and rsqrt2_newton(8 e + 8 s2) -- all (2 (e + s2))^(-1/2).  ``seed_err``: relative error
    put on the Newton form's seed (0: the host build's 1 / sqrt; the device's v_rsq_f64 is off by up to 2^-24.2)."""
    a = [np.ascontiguousarray(np.broadcast_to(x, np.broadcast(eb, half, s2, e).shape).ravel(), dtype=np.float64)
         for x in (eb, half, s2, e, seed_err)]
    n = a[0].size
    g, nw, ok = np.empty(n), np.empty(n), np.empty(n, np.uint8)
    L = lib()
    L.emul_series_root.argtypes = [ctypes.c_int64] + [ctypes.c_void_p] * 8
    L.emul_series_root.restype = None
    L.emul_series_root(n, *[x.ctypes.data for x in a[:4]], g.ctypes.data, ok.ctypes.data, nw.ctypes.data, a[4].ctypes.data)
    return g, ok.astype(bool), nw


def series_vote(e_first, e_last, s2_lanes):
    s2 = np.ascontiguousarray(s2_lanes, dtype=np.float64)
    L = lib()
    L.emul_series_vote.argtypes = [ctypes.c_double, ctypes.c_double, ctypes.c_int64, ctypes.c_void_p]
    return bool(L.emul_series_vote(float(e_first), float(e_last), s2.size, s2.ctypes.data))


def verr_order(records):
    rec = np.ascontiguousarray(records, dtype=np.float64)
    perm = np.empty(rec.shape[0], np.int64)
    L = lib()
    L.emul_verr_order.argtypes = [ctypes.c_int64, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p]
    L.emul_verr_order.restype = None
    L.emul_verr_order(rec.shape[0], rec.shape[1], rec.ctypes.data, perm.ctypes.data)
    return perm


def permuted_exceptions(exceptions, perm, star_begin=0):
    exc = np.ascontiguousarray(exceptions, dtype=np.int64)
    perm = np.ascontiguousarray(perm, dtype=np.int64)
    out = np.empty(max(1, exc.size), np.int64)
    L = lib()
    L.emul_permuted_exceptions.restype = ctypes.c_int64
    L.emul_permuted_exceptions.argtypes = [ctypes.c_int64, ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p, ctypes.c_int64,
                                           ctypes.c_void_p]
    m = L.emul_permuted_exceptions(exc.size, exc.ctypes.data, perm.size, perm.ctypes.data, int(star_begin), out.ctypes.data)
    return out[:m].copy()


def series_plan(sorted_e2, n_walkers, s2_min, target_waves=10240, tail_split=1, exceptions=(), balance=0):
    """{chunks, counted (planning-time thresholds), voted (the kernel's own test at s2_min), stars (in the voted chunks)}"""
    e2 = np.ascontiguousarray(sorted_e2, dtype=np.float64)
    exc = np.ascontiguousarray(exceptions, dtype=np.int64)
    info = np.zeros(4, np.int64)
    L = lib()
    L.emul_series_plan.restype = None
    L.emul_series_plan.argtypes = [ctypes.c_int64, ctypes.c_void_p, ctypes.c_int64, ctypes.c_int64, ctypes.c_int, ctypes.c_int64,
                                   ctypes.c_void_p, ctypes.c_int, ctypes.c_double, ctypes.c_void_p]
    L.emul_series_plan(e2.size, e2.ctypes.data, int(n_walkers), int(target_waves), int(tail_split), exc.size, exc.ctypes.data,
                       int(balance), float(s2_min), info.ctypes.data)
    return {"chunks": int(info[0]), "counted": int(info[1]), "voted": int(info[2]), "stars": int(info[3])}


def series_loglike(records, params, chunk_len, series):
    """Level-2 BGFIXED fixed-centre evaluation of packed ``records`` (in the given order) with 64-walker tiles voting per
    chunk: (lnL per walker, (chunk, tile) pairs that took the series)."""
    rec = np.ascontiguousarray(records, dtype=np.float64)
    wp = emul.pack_walkers(params, 1, False)
    out = np.empty(wp.shape[0])
    ns = ctypes.c_int64(0)
    L = lib()
    L.emul_series_loglike.restype = None
    L.emul_series_loglike.argtypes = [ctypes.c_int64, ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p, ctypes.c_int64, ctypes.c_int,
                                      ctypes.c_void_p, ctypes.c_void_p]
    L.emul_series_loglike(rec.shape[0], rec.ctypes.data, wp.shape[0], wp.ctypes.data, int(chunk_len), int(series), out.ctypes.data,
                          ctypes.byref(ns))
    return out, ns.value

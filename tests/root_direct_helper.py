"""Test helper: CPU build of the direct form of the series reciprocal root of the main kernel
(tests/emul/root_direct_emul.cpp + csrc/mcd_math.h: RootDirect, csrc/mcd_chunks.h).  Test infrastructure only."""
import ctypes
import os
import subprocess

import numpy as np

import emul_helper as emul

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "emul", "root_direct_emul.cpp")
INC = os.path.join(ROOT, "mcmc_dynamics_amd", "csrc")
OUT = os.path.join(ROOT, "tests", "emul", "libroot_direct_emul.so")
_lib = None


def lib():
    global _lib
    if _lib is None:
        deps = [SRC] + [os.path.join(INC, f) for f in ("mcd_math.h", "mcd_guard.h", "mcd_chunks.h", "mcd_exp_table.h")]
        if not os.path.exists(OUT) or any(os.path.getmtime(d) > os.path.getmtime(OUT) for d in deps):
            subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-I", INC, SRC,
                            "-o", OUT], check=True)
        _lib = ctypes.CDLL(OUT)
        _lib.emul_direct_rho_max.restype = ctypes.c_double
        _lib.emul_direct_error_bound.restype = ctypes.c_double
    return _lib


def rho_max():
    return lib().emul_direct_rho_max()


def error_bound():
    """the worst-case relative error derived in the comment of mcd_math.h: RootDirect"""
    return lib().emul_direct_error_bound()


def direct_root(eb, s2, e):
    """(g, ok, delta): the direct form about centre ``eb`` for sigma^2 ``s2`` at verr^2 ``e``, the lane's verdict on the
    direct form, and RootSeries::g on the same inputs -- both (2 (e + s2))^(-1/2)."""
    a = [np.ascontiguousarray(np.broadcast_to(x, np.broadcast(eb, s2, e).shape).ravel(), dtype=np.float64) for x in (eb, s2, e)]
    n = a[0].size
    g, dl, ok = np.empty(n), np.empty(n), np.empty(n, np.uint8)
    L = lib()
    L.emul_direct_root.argtypes = [ctypes.c_int64] + [ctypes.c_void_p] * 6
    L.emul_direct_root.restype = None
    L.emul_direct_root(n, *[x.ctypes.data for x in a], g.ctypes.data, ok.ctypes.data, dl.ctypes.data)
    return g, ok.astype(bool), dl


def direct_vote(e_first, e_last, s2_lanes):
    """0 the rsq loops, 1 the delta series, 2 the direct series"""
    s2 = np.ascontiguousarray(s2_lanes, dtype=np.float64)
    L = lib()
    L.emul_direct_vote.argtypes = [ctypes.c_double, ctypes.c_double, ctypes.c_int64, ctypes.c_void_p]
    return int(L.emul_direct_vote(float(e_first), float(e_last), s2.size, s2.ctypes.data))


def direct_plan(sorted_e2, n_walkers, s2_min, target_waves=10240, tail_split=1, exceptions=(), balance=0):
    """{chunks, counted (planning-time thresholds), voted (the kernel's own tests at s2_min), stars (in the voted chunks),
    series (planning-time count of the series chunks)}"""
    e2 = np.ascontiguousarray(sorted_e2, dtype=np.float64)
    exc = np.ascontiguousarray(exceptions, dtype=np.int64)
    info = np.zeros(5, np.int64)
    L = lib()
    L.emul_direct_plan.restype = None
    L.emul_direct_plan.argtypes = [ctypes.c_int64, ctypes.c_void_p, ctypes.c_int64, ctypes.c_int64, ctypes.c_int, ctypes.c_int64,
                                   ctypes.c_void_p, ctypes.c_int, ctypes.c_double, ctypes.c_void_p]
    L.emul_direct_plan(e2.size, e2.ctypes.data, int(n_walkers), int(target_waves), int(tail_split), exc.size, exc.ctypes.data,
                       int(balance), float(s2_min), info.ctypes.data)
    return {"chunks": int(info[0]), "counted": int(info[1]), "voted": int(info[2]), "stars": int(info[3]), "series": int(info[4])}


def direct_loglike(records, params, chunk_len, mode):
    """Level-2 BGFIXED fixed-centre evaluation of packed ``records`` (in the given order) with 64-walker tiles voting per
    chunk; ``mode`` 0 the rsq loops, 1 the series in its delta form only, 2 the direct form where the second vote passes:
    (lnL per walker, (chunk, tile) pairs in the delta form, ... in the direct form)."""
    rec = np.ascontiguousarray(records, dtype=np.float64)
    wp = emul.pack_walkers(params, 1, False)
    out = np.empty(wp.shape[0])
    counts = np.zeros(2, np.int64)
    L = lib()
    L.emul_direct_loglike.restype = None
    L.emul_direct_loglike.argtypes = [ctypes.c_int64, ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p, ctypes.c_int64, ctypes.c_int,
                                      ctypes.c_void_p, ctypes.c_void_p]
    L.emul_direct_loglike(rec.shape[0], rec.ctypes.data, wp.shape[0], wp.ctypes.data, int(chunk_len), int(mode), out.ctypes.data,
                          counts.ctypes.data)
    return out, int(counts[0]), int(counts[1])

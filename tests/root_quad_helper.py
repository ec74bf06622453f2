"""Test helper: CPU build of the quadratic series root on 32-star bands of the main kernel (tests/emul/root_quad_emul.cpp +
csrc/mcd_math.h: RootQuad, csrc/mcd_exp_split.h, csrc/mcd_chunks.h).  Test infrastructure only."""
import ctypes
import os
import subprocess

import numpy as np

import emul_helper as emul

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "emul", "root_quad_emul.cpp")
INC = os.path.join(ROOT, "mcmc_dynamics_amd", "csrc")
OUT = os.path.join(ROOT, "tests", "emul", "libroot_quad_emul.so")
_lib = None


def lib():
    global _lib
    if _lib is None:
        deps = [SRC] + [os.path.join(INC, f) for f in ("mcd_math.h", "mcd_guard.h", "mcd_chunks.h", "mcd_exp_table.h",
                                                       "mcd_exp_split.h")]
        if not os.path.exists(OUT) or any(os.path.getmtime(d) > os.path.getmtime(OUT) for d in deps):
            subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-I", INC, SRC,
                            "-o", OUT], check=True)
        _lib = ctypes.CDLL(OUT)
        for name in ("emul_quad_max_t", "emul_quad_error_bound", "emul_quad_scale"):
            getattr(_lib, name).restype = ctypes.c_double
    return _lib


def max_t():
    return lib().emul_quad_max_t()


def error_bound():
    """the worst-case relative error derived in the comment of mcd_math.h: RootQuad"""
    return lib().emul_quad_error_bound()


def scale():
    """c = sqrt(N / ln 2), the factor the split loops' root carries"""
    return lib().emul_quad_scale()


def _f64(*arrays):
    shape = np.broadcast(*arrays).shape
    return [np.ascontiguousarray(np.broadcast_to(a, shape).ravel(), dtype=np.float64) for a in arrays]


def quad_root(eb, s2, e_lo, e_hi, e):
    """(quadratic, cubic): the scaled root c (2 (e + s2))^(-1/2) of a chunk centred on ``eb`` at verr^2 ``e`` inside the block
    [e_lo, e_hi], from RootQuad and from RootDirectSplit"""
    a = _f64(eb, s2, e_lo, e_hi, e)
    quad, cubic = np.empty(a[0].size), np.empty(a[0].size)
    L = lib()
    L.emul_quad_root.restype = None
    L.emul_quad_root.argtypes = [ctypes.c_int64] + [ctypes.c_void_p] * 7
    L.emul_quad_root(a[0].size, *[x.ctypes.data for x in a], quad.ctypes.data, cubic.ctypes.data)
    return quad, cubic


def quad_ok(H, eb, s2):
    L = lib()
    L.emul_quad_ok.restype = ctypes.c_int
    L.emul_quad_ok.argtypes = [ctypes.c_double] * 3
    return bool(L.emul_quad_ok(float(H), float(eb), float(s2)))


def blocks(e2):
    """(n_blocks, 4) array of {a2, a1, a0, h} of the sorted verr^2 column"""
    e2 = np.ascontiguousarray(e2, dtype=np.float64)
    out = np.empty((max(1, e2.size // 32), 4))
    L = lib()
    L.emul_quad_blocks.restype = ctypes.c_int64
    L.emul_quad_blocks.argtypes = [ctypes.c_int64, ctypes.c_void_p, ctypes.c_void_p]
    return out[:L.emul_quad_blocks(e2.size, e2.ctypes.data, out.ctypes.data)]


def slots(e2):
    """(n, 2): slots 6 and 7 of the split records made for the sorted verr^2 column"""
    e2 = np.ascontiguousarray(e2, dtype=np.float64)
    out = np.empty((e2.size, 2))
    L = lib()
    L.emul_quad_slots.restype = None
    L.emul_quad_slots.argtypes = [ctypes.c_int64, ctypes.c_void_p, ctypes.c_void_p]
    L.emul_quad_slots(e2.size, e2.ctypes.data, out.ctypes.data)
    return out


def plan(e2, cuts):
    """per chunk [cuts[c], cuts[c + 1]): dict of H, the quad and direct thresholds, and the plan's two sorted vectors"""
    e2 = np.ascontiguousarray(e2, dtype=np.float64)
    cuts = np.ascontiguousarray(cuts, dtype=np.int64)
    n = cuts.size - 1
    out = [np.empty(n) for _ in range(5)]
    L = lib()
    L.emul_quad_plan.restype = None
    L.emul_quad_plan.argtypes = [ctypes.c_int64, ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p] + [ctypes.c_void_p] * 5
    L.emul_quad_plan(e2.size, e2.ctypes.data, n, cuts.ctypes.data, *[o.ctypes.data for o in out])
    return dict(zip(("H", "need_quad", "need_direct", "sorted_quad", "sorted_direct"), out))


def chunk(records, begin, count, params, rescale_iters=4):
    """((W, 4) sums of log y of ONE chunk of the sorted ``records``: 4-star, 8-star and bounded loop with the quadratic form
    offered, the 8-star split loop; (W,) whether chunk_loglike took the quadratic loop for the lane, observed from a call
    on NaN block constants)"""
    rec = np.ascontiguousarray(records, dtype=np.float64)
    wp = emul.pack_walkers(params, 1, False)
    out = np.empty((wp.shape[0], 4))
    took = np.zeros(wp.shape[0], np.int32)
    L = lib()
    L.emul_quad_chunk.restype = None
    L.emul_quad_chunk.argtypes = [ctypes.c_int64, ctypes.c_void_p, ctypes.c_int64, ctypes.c_int64, ctypes.c_int64, ctypes.c_void_p,
                                  ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p]
    L.emul_quad_chunk(rec.shape[0], rec.ctypes.data, int(begin), int(count), wp.shape[0], wp.ctypes.data, int(rescale_iters),
                      out.ctypes.data, took.ctypes.data)
    return out, took.astype(bool)

"""Test helper: CPU build of the split exponent offset of the direct BGFIXED loops (tests/emul/exp_split_emul.cpp +
csrc/mcd_math.h: BgFixedAcc::add_gs, csrc/mcd_exp_split.h, csrc/mcd_guard.h: exp_split_admitted).  Test infrastructure only."""
import ctypes
import os
import subprocess

import numpy as np

import emul_helper as emul

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "emul", "exp_split_emul.cpp")
INC = os.path.join(ROOT, "mcmc_dynamics_amd", "csrc")
OUT = os.path.join(ROOT, "tests", "emul", "libexp_split_emul.so")
MAGIC = 1.5 * 2.0 ** 52
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
        _lib.emul_split_c.restype = ctypes.c_double
        _lib.emul_split_log2_kappa_max.restype = ctypes.c_double
    return _lib


def constants():
    L = lib()
    return {"c": L.emul_split_c(), "N": L.emul_split_table_size(), "shift": L.emul_split_shift(),
            "k_min_table": L.emul_split_k_min_table(), "k_min_bounded": L.emul_split_k_min_bounded(),
            "log2_kappa_max": L.emul_split_log2_kappa_max()}


def _f64(*arrays):
    shape = np.broadcast(*arrays).shape
    return [np.ascontiguousarray(np.broadcast_to(a, shape).ravel(), dtype=np.float64) for a in arrays]


def record(nbp, omp):
    """(M, omp', nbf, |(nbi + nbf) ln2/N - nbp| in long double) of the record split"""
    nbp, omp = _f64(nbp, omp)
    out = [np.empty(nbp.size) for _ in range(4)]
    L = lib()
    L.emul_split_record.restype = None
    L.emul_split_record.argtypes = [ctypes.c_int64] + [ctypes.c_void_p] * 6
    L.emul_split_record(nbp.size, nbp.ctypes.data, omp.ctypes.data, *[o.ctypes.data for o in out])
    return out


def reduce(dgs, M):
    """(k, rv) of exp_split_reduce"""
    dgs, M = _f64(dgs, M)
    k, rv = np.empty(dgs.size, np.int32), np.empty(dgs.size)
    L = lib()
    L.emul_split_reduce.restype = None
    L.emul_split_reduce.argtypes = [ctypes.c_int64] + [ctypes.c_void_p] * 4
    L.emul_split_reduce(dgs.size, dgs.ctypes.data, M.ctypes.data, k.ctypes.data, rv.ctypes.data)
    return k, rv


def term_error(eb, s2, e, d, nbp, omp):
    """relative error of one mixture value against long double: (the parent's direct form, the split form with kappa
    divided out)"""
    a = _f64(eb, s2, e, d, nbp, omp)
    ep, es = np.empty(a[0].size), np.empty(a[0].size)
    L = lib()
    L.emul_split_term_error.restype = None
    L.emul_split_term_error.argtypes = [ctypes.c_int64] + [ctypes.c_void_p] * 8
    L.emul_split_term_error(a[0].size, *[x.ctypes.data for x in a], ep.ctypes.data, es.ctypes.data)
    return ep, es


def chunk_consts(nbp, cuts):
    """(per-chunk constants of the stars' offsets cut at ``cuts``, the stars' nbf)"""
    nbp = np.ascontiguousarray(nbp, dtype=np.float64)
    cuts = np.ascontiguousarray(cuts, dtype=np.int64)
    consts, nbf = np.empty(cuts.size - 1), np.empty(nbp.size)
    L = lib()
    L.emul_split_chunk_consts.restype = None
    L.emul_split_chunk_consts.argtypes = [ctypes.c_int64, ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p, ctypes.c_void_p,
                                          ctypes.c_void_p]
    L.emul_split_chunk_consts(nbp.size, nbp.ctypes.data, cuts.size - 1, cuts.ctypes.data, consts.ctypes.data, nbf.ctypes.data)
    return consts, nbf


def chunk(records, params, rescale_iters=4):
    """sum of log y of ONE chunk per walker, every lane in the direct form: columns (level-2 prefetch loop, the same with
    the split offset, bounded loop, the same with the split offset)"""
    rec = np.ascontiguousarray(records, dtype=np.float64)
    wp = emul.pack_walkers(params, 1, False)
    out = np.empty((wp.shape[0], 4))
    L = lib()
    L.emul_split_chunk.restype = None
    L.emul_split_chunk.argtypes = [ctypes.c_int64, ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p]
    L.emul_split_chunk(rec.shape[0], rec.ctypes.data, wp.shape[0], wp.ctypes.data, int(rescale_iters), out.ctypes.data)
    return out


def guard(cat, params, r_hi2=0.0):
    """(R of bounded_rescale, split admitted in that loop, split admitted in the loops that keep the clamp); ``r_hi2`` > 0:
    the catalogue's nbp_max replaced so that 32 hi2 of bounded_rescale equals it"""
    cols = [np.ascontiguousarray(cat[k], dtype=np.float64) for k in ("v", "verr", "lnlike_bg", "pmember")]
    params = np.ascontiguousarray(params, dtype=np.float64)
    out = np.zeros(3, np.int32)
    L = lib()
    L.emul_split_guard.restype = None
    L.emul_split_guard.argtypes = [ctypes.c_int64] + [ctypes.c_void_p] * 5 + [ctypes.c_int64, ctypes.c_double, ctypes.c_void_p]
    L.emul_split_guard(len(cols[0]), *[c.ctypes.data for c in cols], params.ctypes.data, len(params), float(r_hi2), out.ctypes.data)
    return int(out[0]), bool(out[1]), bool(out[2])

"""Test helper: CPU build of the block step of the bounded quadratic loop (tests/emul/block_step_emul.cpp + csrc/mcd_math.h:
chunk_bgfixed_fast<.., BOUNDED, BLOCK>, csrc/mcd_guard.h: block_step_admitted), and the catalogue the CPU and the GPU test
share.  Test infrastructure only."""
import ctypes
import os
import subprocess

import numpy as np

import emul_helper as emul
from mcmc_dynamics_amd import synthetic
from oracle import lnprob_numpy as oracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "emul", "block_step_emul.cpp")
INC = os.path.join(ROOT, "mcmc_dynamics_amd", "csrc")
NAMES4 = ["v_sys", "sigma_max", "v_maxx", "v_maxy"]
CENTRE = (synthetic.CENTER_RA_DEG, synthetic.CENTER_DEC_DEG)
N = 4000
N_TIGHT = 3200                  # stars with verr in 1 .. 1.0005: chunks that pass all three votes


def build(directory):
    out = os.path.join(str(directory), "libblock_step_emul.so")
    subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-I", INC, SRC, "-o", out], check=True)
    return ctypes.CDLL(out)


def catalogue():
    """4 000 stars of the C3 catalogue with a tight verr band in front (as tests/test_gpu_root_quad.py makes one), so that
    most chunks pass the three votes of the quadratic form"""
    cat = synthetic.make_catalog(N, config=3, seed=synthetic.CATALOG_SEED_BASE + 3, background=True)
    cat["verr"] = cat["verr"].copy()
    cat["verr"][:N_TIGHT] = 1.0 + 5e-4 * np.random.default_rng(14).random(N_TIGHT)
    cat["lnlike_bg"] = oracle.gaussian_background(cat["v"], cat["verr"], 20.0, 40.0)
    cat["lnlike_bg"][0] = -15.15         # one star the background all but rules out: it sets the largest mixture value
    return cat


def walkers(n):
    return synthetic.make_walkers(n, NAMES4, synthetic.make_catalog(8, config=3, background=True)["truth"], config=3)


def refused_table(pos):
    """``pos`` with its last walker at sigma_max = 4.5: the smallest total variance of the table falls from 70 to 21, the
    largest mixture value y_hi = 1 + e^14 / sqrt(n_min) rises from 2^17.1 to 2^18.0, and 56 (log2 y_hi + 0.265) <= 1000 fails
    where the bounded loop's 32 still hold (mcd_guard.h: block_step_admitted) -- for the catalogue above, whose star 0
    has lnL_bg = -15.15"""
    out = np.array(pos, dtype=np.float64)
    out[-1, 1] = 4.5
    return out


def verdict(lib, cat, params):
    """(R of bounded_rescale, block_step_admitted) for the catalogue and the parameter table"""
    cols = [np.ascontiguousarray(cat[k], dtype=np.float64) for k in ("v", "verr", "lnlike_bg", "pmember")]
    params = np.ascontiguousarray(params, dtype=np.float64)
    out = np.zeros(2, np.int32)
    lib.emul_block_verdict.restype = None
    lib.emul_block_verdict.argtypes = [ctypes.c_int64] + [ctypes.c_void_p] * 5 + [ctypes.c_int64, ctypes.c_void_p]
    lib.emul_block_verdict(len(cols[0]), *[c.ctypes.data for c in cols], params.ctypes.data, len(params), out.ctypes.data)
    return int(out[0]), bool(out[1])


def chunk(lib, records, begin, count, params, rescale_iters=4):
    """((W, 2) sums of log y of ONE chunk of the sorted ``records`` with the quadratic form offered: the bounded loop, the
    bounded loop with the block step; (W,) whether the block-step call took the quadratic loop for the lane)"""
    rec = np.ascontiguousarray(records, dtype=np.float64)
    wp = emul.pack_walkers(params, 1, False)
    out = np.empty((wp.shape[0], 2))
    took = np.zeros(wp.shape[0], np.int32)
    lib.emul_block_chunk.restype = None
    lib.emul_block_chunk.argtypes = [ctypes.c_int64, ctypes.c_void_p, ctypes.c_int64, ctypes.c_int64, ctypes.c_int64,
                                     ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p]
    lib.emul_block_chunk(rec.shape[0], rec.ctypes.data, int(begin), int(count), wp.shape[0], wp.ctypes.data, int(rescale_iters),
                         out.ctypes.data, took.ctypes.data)
    return out, took.astype(bool)

"""Test helper: CPU build of the parallel-tempering algebra (tests/emul/temper_emul.cpp + csrc/mcd_temper.h), with the
log-likelihood supplied as a Python callable, a block function for ``sampler.TemperedSampler`` on it, and the closed forms
the tests compare against.

Test infrastructure only."""
import ctypes
import math
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "emul", "temper_emul.cpp")
INC = os.path.join(ROOT, "mcmc_dynamics_amd", "csrc")
OUT = os.path.join(ROOT, "tests", "emul", "libtemper_emul.so")

TEMPER_OK, TEMPER_NAN, TEMPER_EVAL_FAILED, TEMPER_BAD_ARGS, TEMPER_OUTSIDE = 0, 1, 2, 3, 4
EVAL_FN = ctypes.CFUNCTYPE(ctypes.c_int, ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p)
_lib = None


def lib():
    global _lib
    if _lib is None:
        deps = [SRC] + [os.path.join(INC, h) for h in ("mcd_temper.h", "mcd_stretch.h", "mcd_prior.h", "mcd_rng.h", "mcd_math.h")]
        if not os.path.exists(OUT) or any(os.path.getmtime(d) > os.path.getmtime(OUT) for d in deps):
            subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-I", INC, SRC, "-o", OUT],
                           check=True)
        L = ctypes.CDLL(OUT)
        L.emul_temper_key.restype = ctypes.c_uint64
        L.emul_temper_numbers.argtypes = [ctypes.c_uint64, ctypes.c_int64, ctypes.c_int64, ctypes.c_int32, ctypes.c_int64,
                                          ctypes.c_void_p]
        L.emul_temper_numbers.restype = None
        L.emul_temper_block.argtypes = [ctypes.c_int32, ctypes.c_int64, ctypes.c_int, ctypes.c_int] + [ctypes.c_void_p] * 5 + \
            [ctypes.c_int] + [ctypes.c_void_p] * 4 + [ctypes.c_int64] + [ctypes.c_void_p] * 3 + \
            [ctypes.c_uint64, ctypes.c_int64, ctypes.c_int32] + [ctypes.c_void_p] * 5 + [EVAL_FN]
        L.emul_stretch_seeded.argtypes = [ctypes.c_int64, ctypes.c_int, ctypes.c_int] + [ctypes.c_void_p] * 5 + \
            [ctypes.c_int, ctypes.c_int64, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_int64] + \
            [ctypes.c_void_p] * 3 + [EVAL_FN]
        _lib = L
    return _lib


def key():
    return int(lib().emul_temper_key())


def numbers(seed, step0, n_steps, n_temps, n_walkers):
    """swap thresholds (steps, T - 1, W) from the host build of csrc/mcd_temper.h."""
    thr = np.empty((n_steps, max(n_temps - 1, 0), n_walkers))
    lib().emul_temper_numbers(seed, step0, n_steps, n_temps, n_walkers, thr.ctypes.data)
    return thr


def numpy_swap_thr(seed, step, t, w, det_log):
    """One swap threshold restated on ``numpy.random.Philox`` raw words (NumPy increments the counter before it generates
    a block, so the block of counter c is ``Philox(counter=c - 1)``'s first four words)."""
    value = sum(int(x) << (64 * i) for i, x in enumerate([step, t, w, 0]))
    before = (value - 1) % (1 << 256)
    c = [(before >> (64 * i)) & 0xFFFFFFFFFFFFFFFF for i in range(4)]
    bg = np.random.Philox(counter=np.array(c, dtype=np.uint64), key=np.array([int(seed), key()], dtype=np.uint64))
    u = float(int(bg.random_raw(4)[0]) >> 11) * (1.0 / 9007199254740992.0)
    return float(det_log(np.array([u]))[0])


def wrap_eval(fn, k):
    """``fn(table (n, K)) -> values (n,)`` as the C callback; a raised exception becomes status 1."""
    def call(table, n, out):
        try:
            t = np.ctypeslib.as_array(ctypes.cast(table, ctypes.POINTER(ctypes.c_double)), shape=(n, k))
            np.ctypeslib.as_array(ctypes.cast(out, ctypes.POINTER(ctypes.c_double)), shape=(n,))[:] = fn(t)
            return 0
        except Exception:                                    # noqa: BLE001 -- reported through the status
            return 1
    return EVAL_FN(call)


def identity_plan(n_dim, lo=None, hi=None, fixed_ok=True, prior=None):
    return {"col_source": np.arange(n_dim, dtype=np.int32), "col_const": np.zeros(n_dim), "col_factor": np.ones(n_dim),
            "lo": np.full(n_dim, -np.inf) if lo is None else np.asarray(lo, dtype=np.float64),
            "hi": np.full(n_dim, np.inf) if hi is None else np.asarray(hi, dtype=np.float64), "fixed_ok": fixed_ok,
            "prior": prior}


def _plan_arrays(plan):
    src = np.ascontiguousarray(plan["col_source"], dtype=np.int32)
    cols = [np.ascontiguousarray(plan[k], dtype=np.float64) for k in ("col_const", "col_factor", "lo", "hi")]
    return src, cols


def block(plan, betas, pos, lnlike, seed, step0, n_steps, fn, n_chain_temps=1, out=None):
    """The host-driven block on ``fn``.  ``out``: arrays to write the rows and counts into (a sampler's), else fresh ones.
    -> dict(status, pos, lnlike, lnprior, chain, lnlike_chain, accepted, swap_proposed, swap_accepted)"""
    pos = np.array(pos, dtype=np.float64)
    ll = np.array(lnlike, dtype=np.float64)
    T, W, P = pos.shape
    betas = np.ascontiguousarray(betas, dtype=np.float64)
    src, cols = _plan_arrays(plan)
    K = src.size
    lp = np.full((T, W), np.nan)
    o = out or {}
    chain = o.get("chain", np.full((n_steps, n_chain_temps, W, P), np.nan))
    llc = o.get("lnlike_chain", np.full((n_steps, T, W), np.nan))
    acc = o.get("accepted", np.zeros((T, W), dtype=np.int64))
    swp = o.get("swap_proposed", np.zeros(max(T - 1, 0), dtype=np.int64))
    swa = o.get("swap_accepted", np.zeros(max(T - 1, 0), dtype=np.int64))
    prior = plan.get("prior")
    keep = [None, None, None]
    if prior is not None:
        keep = [np.ascontiguousarray(prior[0], dtype=np.int32), np.ascontiguousarray(prior[1], dtype=np.float64),
                np.ascontiguousarray(prior[2], dtype=np.float64)]
    cb = wrap_eval(fn, K)
    rc = lib().emul_temper_block(T, W, P, K, src.ctypes.data, *[c.ctypes.data for c in cols],
                                 1 if plan.get("fixed_ok", True) else 0, betas.ctypes.data,
                                 *[a.ctypes.data if a is not None else None for a in keep], int(n_steps), pos.ctypes.data,
                                 ll.ctypes.data, lp.ctypes.data, seed, step0, n_chain_temps, chain.ctypes.data, llc.ctypes.data,
                                 acc.ctypes.data, swp.ctypes.data, swa.ctypes.data, cb)
    return {"status": rc, "pos": pos, "lnlike": ll, "lnprior": lp, "chain": chain, "lnlike_chain": llc, "accepted": acc,
            "swap_proposed": swp, "swap_accepted": swa}


def stretch_seeded(plan, pos, lnp, seed, step0, n_steps, fn):
    """The seeded stretch move of one ensemble (csrc/mcd_stretch.h fed chain_numbers_of_step) on ``fn``."""
    pos, lnp = np.array(pos, dtype=np.float64), np.array(lnp, dtype=np.float64)
    W, P = pos.shape
    src, cols = _plan_arrays(plan)
    chain, lnpc = np.full((n_steps, W, P), np.nan), np.full((n_steps, W), np.nan)
    acc = np.zeros(W, dtype=np.int64)
    cb = wrap_eval(fn, src.size)
    rc = lib().emul_stretch_seeded(W, P, src.size, src.ctypes.data, *[c.ctypes.data for c in cols],
                                   1 if plan.get("fixed_ok", True) else 0, int(n_steps), pos.ctypes.data, lnp.ctypes.data, seed,
                                   step0, chain.ctypes.data, lnpc.ctypes.data, acc.ctypes.data, cb)
    return {"status": rc, "pos": pos, "lnp": lnp, "chain": chain, "lnprob_chain": lnpc, "accepted": acc}


def emul_block_fn(fn, plan):
    """``block_fn`` of ``sampler.TemperedSampler`` on the CPU harness."""
    def block_fn(betas, pos, lnlike, lnprior, seed, step0, n_steps, chain, lnlike_chain, accepted, swap_proposed,
                 swap_accepted):
        out = block(plan, betas, pos, lnlike, seed, step0, n_steps, fn, n_chain_temps=chain.shape[1],
                    out={"chain": chain, "lnlike_chain": lnlike_chain, "accepted": accepted, "swap_proposed": swap_proposed,
                         "swap_accepted": swap_accepted})
        if out["status"] != TEMPER_OK:
            raise RuntimeError("temper_block status {0}".format(out["status"]))
        pos[:], lnlike[:], lnprior[:] = out["pos"], out["lnlike"], out["lnprior"]
    return block_fn


# ---- closed forms -------------------------------------------------------------------------------------------------------
def _phi(x):
    return math.exp(-0.5 * x * x) / math.sqrt(2.0 * math.pi)


def _Phi(x):
    return 0.5 * math.erfc(-x / math.sqrt(2.0))


def truncated_gaussian(mean, sd, lo, hi, beta):
    """Of exp(-beta (x - mean)^2 / (2 sd^2)) on [lo, hi]: (mean, variance, log of its integral, E[(x - mean)^2]).
    beta = 0: the uniform distribution."""
    if beta == 0.0:
        m, v = 0.5 * (lo + hi), (hi - lo) ** 2 / 12.0
        return m, v, math.log(hi - lo), v + (m - mean) ** 2
    s = sd / math.sqrt(beta)
    a, b = (lo - mean) / s, (hi - mean) / s
    z = _Phi(b) - _Phi(a)
    r = (_phi(a) - _phi(b)) / z
    m = mean + s * r
    v = s * s * (1.0 + (a * _phi(a) - b * _phi(b)) / z - r * r)
    return m, v, math.log(s * math.sqrt(2.0 * math.pi) * z), v + (m - mean) ** 2


def walker_means(x):
    """x (W, steps, ...) -> (mean, standard error) from the walkers' time averages (batch means)."""
    per_walker = x.mean(axis=1)
    return per_walker.mean(axis=0), per_walker.std(axis=0, ddof=1) / np.sqrt(x.shape[0])

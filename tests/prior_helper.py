"""Test helper: CPU build of the structured priors (tests/emul/prior_emul.cpp + csrc/mcd_prior.h, mcd_stretch.h, mcd_hmc.h)
with the likelihood supplied as a Python callable, and the priors' closed forms in numpy.longdouble.

Test infrastructure only."""
import ctypes
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "emul", "prior_emul.cpp")
INC = os.path.join(ROOT, "mcmc_dynamics_amd", "csrc")
OUT = os.path.join(ROOT, "tests", "emul", "libprior_emul.so")

FLAT, NORMAL, LOGNORMAL = 0, 1, 2
STRETCH_EVAL = ctypes.CFUNCTYPE(ctypes.c_int, ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p)
HMC_EVAL = ctypes.CFUNCTYPE(ctypes.c_int, ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p, ctypes.c_void_p)
_lib = None


def lib():
    global _lib
    if _lib is None:
        deps = [SRC] + [os.path.join(INC, h) for h in ("mcd_prior.h", "mcd_stretch.h", "mcd_hmc.h", "mcd_rng.h", "mcd_math.h")]
        if not os.path.exists(OUT) or any(os.path.getmtime(d) > os.path.getmtime(OUT) for d in deps):
            subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-I", INC, SRC, "-o", OUT],
                           check=True)
        L = ctypes.CDLL(OUT)
        L.emul_prior_eval.argtypes = [ctypes.c_int] + [ctypes.c_void_p] * 3 + [ctypes.c_int64] + [ctypes.c_void_p] * 3
        L.emul_prior_stretch_block.argtypes = [ctypes.c_int64, ctypes.c_int64, ctypes.c_int, ctypes.c_int] + \
            [ctypes.c_void_p] * 5 + [ctypes.c_int] + [ctypes.c_void_p] * 3 + [ctypes.c_int64] + [ctypes.c_void_p] * 9 + [STRETCH_EVAL]
        L.emul_prior_hmc_block.argtypes = [ctypes.c_int64, ctypes.c_int, ctypes.c_int] + [ctypes.c_void_p] * 5 + \
            [ctypes.c_int] + [ctypes.c_void_p] * 4 + [ctypes.c_double, ctypes.c_double, ctypes.c_int, ctypes.c_int64,
                                                     ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_int64] + \
            [ctypes.c_void_p] * 4 + [HMC_EVAL]
        _lib = L
    return _lib


def _prior_ptrs(prior):
    """prior: None or (kind, p0, p1) -> (three pointers or None, the arrays kept alive)"""
    if prior is None:
        return (None, None, None), ()
    kind = np.ascontiguousarray(prior[0], dtype=np.int32)
    p0, p1 = (np.ascontiguousarray(a, dtype=np.float64) for a in prior[1:])
    return (kind.ctypes.data, p0.ctypes.data, p1.ctypes.data), (kind, p0, p1)


def evaluate(prior, x, want_grad=False):
    """The header's value (n,) [and derivative (n, P)] of the rows x (n, P), host build."""
    x = np.ascontiguousarray(np.atleast_2d(x), dtype=np.float64)
    ptrs, keep = _prior_ptrs(prior)
    value = np.empty(x.shape[0])
    grad = np.empty(x.shape) if want_grad else None
    rc = lib().emul_prior_eval(x.shape[1], *ptrs, x.shape[0], x.ctypes.data, value.ctypes.data,
                               grad.ctypes.data if want_grad else None)
    assert rc == 0, rc
    return (value, grad) if want_grad else value


HALF_LOG_2PI = np.log(np.longdouble(2) * np.arccos(np.longdouble(-1))) / 2


def terms(kind, p0, p1, x):
    """n independent one-coordinate priors, element by element: (value (n,), derivative (n,)) from the host build."""
    kind = np.ascontiguousarray(kind, dtype=np.int32)
    p0, p1, x = (np.ascontiguousarray(a, dtype=np.float64) for a in (p0, p1, x))
    value, dx = np.empty(x.size), np.empty(x.size)
    L = lib()
    L.emul_prior_terms.argtypes = [ctypes.c_int64] + [ctypes.c_void_p] * 6
    rc = L.emul_prior_terms(x.size, kind.ctypes.data, p0.ctypes.data, p1.ctypes.data, x.ctypes.data, value.ctypes.data, dx.ctypes.data)
    assert rc == 0, rc
    return value, dx


def exact(kind, p0, p1, x):
    """One coordinate's closed form in numpy.longdouble (arrays broadcast)."""
    x, p0, p1 = (np.asarray(a, dtype=np.longdouble) for a in (x, p0, p1))
    if kind == NORMAL:
        return -np.log(p1) - HALF_LOG_2PI - ((x - p0) / p1) ** 2 / 2
    l = np.log(x)
    return -np.log(p1) - HALF_LOG_2PI - l - ((l - p0) / p1) ** 2 / 2


def exact_row(prior, x):
    """Sum over the coordinates of rows x (n, P) in longdouble; -inf where a log-normal coordinate is <= 0."""
    kind, p0, p1 = prior
    x = np.atleast_2d(np.asarray(x, dtype=np.longdouble))
    out = np.zeros(x.shape[0], dtype=np.longdouble)
    for c, k in enumerate(kind):
        if k == FLAT:
            continue
        with np.errstate(invalid="ignore", divide="ignore"):
            term = exact(int(k), p0[c], p1[c], np.where((k == LOGNORMAL) & (x[:, c] <= 0), 1, x[:, c]))
        out += np.where((k == LOGNORMAL) & (x[:, c] <= 0), -np.inf, term)
    return out


def stretch_block_fn(plan, prior, fn, n_bins=1):
    """block_fn of sampler.EnsembleSampler / BinnedSampler: the host-driven stretch block with priors on ``fn(table) -> (n,)``."""
    src = np.ascontiguousarray(plan["col_source"], dtype=np.int32)
    cols = [np.ascontiguousarray(plan[k], dtype=np.float64) for k in ("col_const", "col_factor", "lo", "hi")]
    ptrs, keep = _prior_ptrs(prior)
    k = src.size

    @STRETCH_EVAL
    def cb(tab, n, out):
        table = np.ctypeslib.as_array(ctypes.cast(tab, ctypes.POINTER(ctypes.c_double)), shape=(n_bins * n, k))
        np.ctypeslib.as_array(ctypes.cast(out, ctypes.POINTER(ctypes.c_double)), shape=(n_bins * n,))[:] = fn(table.copy())
        return 0

    def run(pos, lnp, order, zz, thr, pick, chain, lnprob_chain, accepted):
        p = lambda a: a.ctypes.data if a is not None else None
        rc = lib().emul_prior_stretch_block(n_bins, pos.shape[-2], pos.shape[-1], k, src.ctypes.data, *[c.ctypes.data for c in cols],
                                            1 if plan.get("fixed_ok", True) else 0, *ptrs, order.shape[0], p(pos), p(lnp),
                                            p(order), p(zz), p(thr), p(pick), p(chain), p(lnprob_chain), p(accepted), cb)
        assert rc == 0, rc
    run.keep = (cb, keep, cols, src)
    return run


def hmc_block(plan, prior, chol, step_size, n_leap, pos, seed, step0, n_steps, fn, jitter=0.1):
    """The host-driven HMC block with priors on ``fn(table) -> (values, grad)``; as hmc_helper.block."""
    pos = np.array(pos, dtype=np.float64)
    W, P = pos.shape
    src = np.ascontiguousarray(plan["col_source"], dtype=np.int32)
    K = src.size
    cols = [np.ascontiguousarray(plan[k], dtype=np.float64) for k in ("col_const", "col_factor", "lo", "hi")]
    ptrs, keep = _prior_ptrs(prior)
    chol = np.ascontiguousarray(chol, dtype=np.float64)
    lnp = np.full(W, np.nan)
    chain, lnpc, err = np.full((n_steps, W, P), np.nan), np.full((n_steps, W), np.nan), np.full((n_steps, W), np.nan)
    acc = np.zeros(W, dtype=np.int64)

    @HMC_EVAL
    def cb(table, n, out, grad):
        t = np.ctypeslib.as_array(ctypes.cast(table, ctypes.POINTER(ctypes.c_double)), shape=(n, K))
        v, g = fn(t.copy())
        np.ctypeslib.as_array(ctypes.cast(out, ctypes.POINTER(ctypes.c_double)), shape=(n,))[:] = v
        np.ctypeslib.as_array(ctypes.cast(grad, ctypes.POINTER(ctypes.c_double)), shape=(n, K))[:] = g
        return 0

    rc = lib().emul_prior_hmc_block(W, P, K, src.ctypes.data, *[c.ctypes.data for c in cols], 1 if plan.get("fixed_ok", True) else 0,
                                    *ptrs, chol.ctypes.data, float(step_size), float(jitter), int(n_leap), int(n_steps),
                                    pos.ctypes.data, lnp.ctypes.data, seed, step0, chain.ctypes.data, lnpc.ctypes.data,
                                    acc.ctypes.data, err.ctypes.data, cb)
    return {"status": rc, "pos": pos, "lnp": lnp, "chain": chain, "lnprob_chain": lnpc, "accepted": acc, "energy_error": err}

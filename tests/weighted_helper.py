"""Test helper of the weighted-likelihood bootstrap (tests/test_weights_cpu.py, tests/test_bootstrap_cpu.py,
tests/test_gpu_weighted.py).  Test infrastructure only.

  * the CPU build of the weighted gradient loop and of the weight generator (tests/emul/weighted_emul.cpp: csrc/mcd_weighted.h,
    csrc/mcd_weights.h);
  * the reference: sum_i w_i t_i in numpy.longdouble over the per-star terms of the test-side restatements
    (variant_helper.per_star for the value, grad_helper.per_star for the gradient), which share no expression with the
    kernel, and the accuracy rule of DESIGN 3.9 on the weighted scale:
        |got - exact| / S_k <= 2 err_np64 + floor,   S_k = sum_i w_i |dl_i/dtheta_k|,
    err_np64 the float64 run of the same weighted sum against its longdouble run, floor = grad_bounds.floors (1e-12 and
    the free-centre table); values: 1e-12 on the scale max(|sum w l|, sum w);
  * a NumPy quadratic with per-replicate weights whose weighted maximum is known in closed form (the stub of
    Runner.bootstrap's bookkeeping test and the reference of the end-to-end GPU test)."""
import ctypes
import os
import subprocess

import numpy as np

import double_helper as dh
import emul_helper as eh
import grad_bounds as gb
import grad_helper as gh
import variant_helper as vh

SRC = os.path.join(eh.ROOT, "tests", "emul", "weighted_emul.cpp")
OUT = os.path.join(eh.ROOT, "tests", "emul", "libmcd_weighted_emul.so")
EXPONENTIAL, POISSON, EXPLICIT = 0, 1, 2
SCHEMES = {"exponential": EXPONENTIAL, "poisson": POISSON, "explicit": EXPLICIT}
SEED = 20261020
BIG_REPLICATE = 1 << 40
L = vh.L
_lib = None


def lib():
    global _lib
    if _lib is None:
        deps = [SRC] + [os.path.join(eh.INC, h) for h in ("mcd_weighted.h", "mcd_weights.h", "mcd_rng.h", "mcd_grad.h", "mcd_math.h",
                                                          "mcd_exp_table.h", "mcd_dispatch.h")]
        if not os.path.exists(OUT) or any(os.path.getmtime(d) > os.path.getmtime(OUT) for d in deps):
            subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-I", eh.INC, SRC, "-o", OUT],
                           check=True)
        _lib = ctypes.CDLL(OUT)
        _lib.emul_weighted.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int64, ctypes.c_void_p, ctypes.c_void_p,
                                       ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p,
                                       ctypes.c_int64, ctypes.c_int64, ctypes.c_void_p]
        _lib.emul_bootstrap_weights.argtypes = [ctypes.c_int, ctypes.c_uint64, ctypes.c_int64, ctypes.c_int64, ctypes.c_int64,
                                                ctypes.c_int64, ctypes.c_void_p]
        _lib.emul_bootstrap_weights.restype = None
        _lib.emul_weight_words.argtypes = [ctypes.c_uint64, ctypes.c_int64, ctypes.c_int64, ctypes.c_void_p]
        _lib.emul_weight_words.restype = None
        _lib.emul_weight_key.restype = ctypes.c_uint64
        _lib.emul_poisson_thresholds.argtypes = [ctypes.c_void_p]
        _lib.emul_weight_uniform.argtypes = [ctypes.c_uint64]
        _lib.emul_weight_uniform.restype = ctypes.c_double
    return _lib


# ---- the generator -------------------------------------------------------------------------------------------------------
def weights(scheme, seed, rep0, n_reps, star0, n_stars):
    """The CPU build of mcd_weights.h: (n_reps, n_stars)."""
    w = np.empty((int(n_reps), int(n_stars)))
    lib().emul_bootstrap_weights(SCHEMES.get(scheme, scheme), int(seed) & 0xFFFFFFFFFFFFFFFF, int(rep0), int(n_reps), int(star0),
                                 int(n_stars), w.ctypes.data)
    return w


def words(seed, replicate, block):
    out = np.empty(4, dtype=np.uint64)
    lib().emul_weight_words(int(seed), int(replicate), int(block), out.ctypes.data)
    return out


def numpy_block(counter, key):
    """The four words NumPy's Philox produces for `counter` (four 64-bit words, little end first): NumPy increments the
    counter BEFORE it generates a block, so the generator is started one below."""
    value = (sum(int(x) << (64 * i) for i, x in enumerate(counter)) - 1) % (1 << 256)
    before = [(value >> (64 * i)) & 0xFFFFFFFFFFFFFFFF for i in range(4)]
    return np.random.Philox(counter=np.array(before, dtype=np.uint64), key=np.array(key, dtype=np.uint64)).random_raw(4)


def numpy_uniforms(seed, replicate, star0, n_stars):
    """u of stars star0 .. from NumPy's generator: counter (star >> 2, replicate, 0, 0), key (seed, kWeightKey1), word star & 3."""
    key = [int(seed), int(lib().emul_weight_key())]
    blocks = {}
    out = np.empty(n_stars, dtype=np.uint64)
    for j in range(n_stars):
        star = star0 + j
        if star >> 2 not in blocks:
            blocks[star >> 2] = numpy_block([star >> 2, int(replicate), 0, 0], key)
        out[j] = blocks[star >> 2][star & 3]
    return uniform_of_words(out)


def poisson_thresholds():
    out = np.empty(64)
    n = lib().emul_poisson_thresholds(out.ctypes.data)
    return out[:n].copy()


def poisson_count(u):
    """poisson_count of mcd_weights.h for every u."""
    u = np.ascontiguousarray(u, dtype=np.float64)
    out = np.empty_like(u)
    lib().emul_poisson_count.argtypes = [ctypes.c_int64, ctypes.c_void_p, ctypes.c_void_p]
    lib().emul_poisson_count.restype = None
    lib().emul_poisson_count(u.size, u.ctypes.data, out.ctypes.data)
    return out


def uniform_of_words(w):
    """u = ((word >> 11) + 0.5) 2^-53 in float64, as mcd_weights.h writes it."""
    return ((np.asarray(w, dtype=np.uint64) >> np.uint64(11)).astype(np.float64) + 0.5) * (1.0 / 9007199254740992.0)


def row_replicates(rows):
    """A non-monotone map with repeats, and one id of 2^40."""
    rep = (7 * np.arange(rows, dtype=np.int64) + 3) % 5
    rep[rows // 2] = BIG_REPLICATE
    return rep


def weights_of_rows(scheme, seed, rep, n_stars):
    """(rows, n_stars): the generated weights of every row's replicate."""
    table = {int(b): weights(scheme, seed, int(b), 1, 0, n_stars)[0] for b in np.unique(rep)}
    return np.stack([table[int(b)] for b in rep])


# ---- the CPU build of the loop -------------------------------------------------------------------------------------------
def emul_weighted(case, rows, rep, scheme, seed=SEED, explicit=None, chunk_len=96):
    """(values (R,), gradients (R, K)) of the rows `rows` of case["params"] under the replicates `rep`.
    explicit: (n_replicates, N) weights for scheme "explicit" (transposed here, as the library does on upload)."""
    model, free = case["model"], case["free"]
    params = np.ascontiguousarray(case["params"][rows])
    rec = eh.pack_records(case["cat"], model, case["centre"])
    wp = eh.pack_walkers(params, model, free)
    k = dh.n_columns(model, free) if model in dh.MODELS else gh.n_columns(model, free)
    rep = np.ascontiguousarray(rep, dtype=np.int64)
    assert rep.size == len(rows) and params.shape[1] == k
    wt = None if explicit is None else np.ascontiguousarray(np.asarray(explicit, dtype=np.float64).T)
    out = np.empty((len(rows), 1 + k))
    rc = lib().emul_weighted(model, int(free), SCHEMES.get(scheme, scheme), rec.shape[0], rec.ctypes.data, wp.ctypes.data,
                             params.ctypes.data, len(rows), rep.ctypes.data, int(seed), None if wt is None else wt.ctypes.data,
                             0 if wt is None else wt.shape[1], int(chunk_len), out.ctypes.data)
    assert rc == 0
    return out[:, 0], out[:, 1:]


# ---- the reference -------------------------------------------------------------------------------------------------------
_terms = {}


def star_terms(model, cat, row, centre):
    """{"v80", "v64": (N,) value terms; "g80", "g64": (K, N) gradient terms} of one parameter row, computed once."""
    key = (model, centre, np.asarray(row).tobytes(), tuple(sorted((k, np.asarray(v).tobytes()) for k, v in cat.items())))
    if key not in _terms and model in dh.MODELS:               # the double models: double_helper's restatements
        _terms[key] = {"v80": dh.per_star(model, cat, row, centre, L)[0], "v64": dh.per_star(model, cat, row, centre, np.float64)[0],
                       "g80": dh.grad_terms(model, cat, row, centre, L), "g64": dh.grad_terms(model, cat, row, centre, np.float64)}
    if key not in _terms:
        _terms[key] = {"v80": vh.per_star(model, cat, row, centre, L)[0],
                       "v64": vh.per_star(model, cat, row, centre, np.float64)[0],
                       "g80": gh.per_star(model, cat, row, centre, L), "g64": gh.per_star(model, cat, row, centre, np.float64)}
    return _terms[key]


def reference(model, cat, row, centre, w):
    """The weighted sums of one row in longdouble with their scales: value, sum w, g (K,), S (K,), err64 (K,)."""
    t = star_terms(model, cat, row, centre)
    keep = np.asarray(w) != 0                                 # (selected out: a weight 0 meets no term)
    w80, w64 = np.asarray(w, dtype=L)[keep], np.asarray(w, dtype=np.float64)[keep]
    g80 = (t["g80"][:, keep] * w80).sum(axis=1)
    s80 = (np.abs(t["g80"][:, keep]) * w80).sum(axis=1)
    g64 = (t["g64"][:, keep] * w64).sum(axis=1)
    return {"value": (t["v80"][keep] * w80).sum(), "sum_w": w80.sum(), "g": g80, "s": s80, "err64": gh.col_err(g64, g80, s80)}


def check_row(value, grad, ref, cell, column_floor):
    """The rule of the module docstring; returns (value error, largest column error)."""
    scale = max(abs(ref["value"]), ref["sum_w"], L(1e-300))
    v_err = float(abs(L(value) - ref["value"]) / scale)
    assert v_err <= 1e-12, (cell, "value", float(value), float(ref["value"]), v_err)
    err = gb.check_columns(grad, ref, cell, column_floor)
    return v_err, float(err.max())


# ---- a closed form -------------------------------------------------------------------------------------------------------
def closed_form_maximum(v, verr, sigma, w):
    """The maximum over v_sys of sum_i w_i log N(v_i; v_sys, verr_i^2 + sigma^2) for every row of w (B, N), in longdouble:
    mu_b = sum w_i v_i / n_i / sum w_i / n_i, and Lambda_b = sum w_i / n_i, the curvature there."""
    v, verr, w = np.asarray(v, dtype=L), np.asarray(verr, dtype=L), np.atleast_2d(np.asarray(w, dtype=L))
    n = verr * verr + L(sigma) * L(sigma)
    lam = (w / n).sum(axis=1)
    return (w * v / n).sum(axis=1) / lam, lam


class QuadraticStub(object):
    """value_and_grad of sum_i w(b, i) log N(v_i; x, n_i) in NumPy float64, with the signature of
    Runner.lnprob_weighted_grad_batch; records what it was called with."""

    def __init__(self, v, n, weights_of):
        self.v, self.n, self.weights_of, self.calls = np.asarray(v, float), np.asarray(n, float), weights_of, []

    def __call__(self, values, row_replicate, scheme="exponential", seed=0, weights=None):
        values = np.atleast_2d(np.asarray(values, dtype=np.float64))
        rep = np.asarray(row_replicate, dtype=np.int64)
        self.calls.append({"rows": values.shape[0], "replicate": rep.copy(), "scheme": scheme, "seed": seed, "first": values.copy()})
        w = self.weights_of(scheme, seed, rep)
        d = self.v[None, :] - values[:, :1]
        f = (w * (-0.5 * np.log(2.0 * np.pi * self.n) - 0.5 * d * d / self.n)).sum(axis=1)
        g = (w * d / self.n).sum(axis=1)[:, None]
        return f, g

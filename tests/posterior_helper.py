"""Test helper: CPU build of the per-star posterior summaries (tests/emul/posterior_emul.cpp + csrc/mcd_posterior.h +
csrc/mcd_math.h), and the NumPy restatement they are checked against, built from the per-star functions of
oracle/lnprob_numpy.py.  Test infrastructure only."""
import ctypes
import os
import subprocess

import numpy as np

import emul_helper as emul
from mcmc_dynamics_amd import synthetic
from oracle import lnprob_numpy as oracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "emul", "posterior_emul.cpp")
INC = os.path.join(ROOT, "mcmc_dynamics_amd", "csrc")
OUT = os.path.join(ROOT, "tests", "emul", "libposterior_emul.so")
_lib = None


def lib():
    global _lib
    if _lib is None:
        deps = [SRC] + [os.path.join(INC, f) for f in ("mcd_posterior.h", "mcd_math.h", "mcd_exp_table.h", "mcd_dispatch.h")]
        if not os.path.exists(OUT) or any(os.path.getmtime(d) > os.path.getmtime(OUT) for d in deps):
            subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-I", INC, SRC,
                            "-o", OUT], check=True)
        L = ctypes.CDLL(OUT)
        L.emul_posterior.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int64, ctypes.c_void_p,
                                     ctypes.c_void_p, ctypes.c_int64, ctypes.c_int64, ctypes.c_void_p]
        L.emul_posterior_terms.argtypes = [ctypes.c_int64, ctypes.c_int64, ctypes.c_void_p, ctypes.c_void_p,
                                           ctypes.c_int64, ctypes.c_void_p]
        L.emul_posterior_plan.argtypes = [ctypes.c_int64, ctypes.c_int64, ctypes.POINTER(ctypes.c_int64)]
        L.emul_posterior_plan.restype = ctypes.c_int64
        _lib = L
    return _lib


FIELDS = ("lppd", "lnl_var", "pmem_mean", "pmem_std")


def _unpack(out, mem):
    d = dict(zip(FIELDS, out))
    if not mem:
        del d["pmem_mean"], d["pmem_std"]
    return d


def posterior(cat, table, model, centre, mem, n_slices=0):
    """Emulated mcd_pointwise_posterior: table (S, K) in the C-ABI column order; n_slices 0 = the library's plan."""
    rec = emul.pack_records(cat, model, centre)
    wp = emul.pack_walkers(table, model, centre is None)
    n = rec.shape[0]
    out = np.empty((4, n))
    rc = lib().emul_posterior(model, int(centre is None), int(mem), n, rec.ctypes.data, wp.ctypes.data, wp.shape[0],
                              int(n_slices), out.ctypes.data)
    assert rc == 0
    return _unpack(out, mem)


def posterior_terms(x, p=None, n_slices=0):
    """The reduction alone over given terms x, p (n, S)."""
    x = np.ascontiguousarray(x, dtype=np.float64)
    p = np.zeros_like(x) if p is None else np.ascontiguousarray(p, dtype=np.float64)
    n, S = x.shape
    out = np.empty((4, n))
    assert lib().emul_posterior_terms(n, S, x.ctypes.data, p.ctypes.data, int(n_slices), out.ctypes.data) == 0
    return _unpack(out, True)


def plan(n, S):
    ln = ctypes.c_int64(0)
    k = lib().emul_posterior_plan(int(n), int(S), ctypes.byref(ln))
    return int(k), int(ln.value)


# ---- NumPy restatement ------------------------------------------------------------------------------------------
PROFILE = (3, 4, 5, 6)
DOUBLE = emul.DOUBLE_MODELS                     # the double Lynden-Bell models: profile models with a second rotation term
BG = emul.BG_OF


def abi_names(model, free):
    return emul.abi_names(model, free)


def double_rotation(ra, dec, P, rc, dc):
    """v_los of the double Lynden-Bell models the way the golden vectors were made: TWO calls of the oracle's
    model_rotation, the second with v_sys = 0, the ``_c`` amplitudes and the peak radius r_peak_ratio * r_peak.  Runs in
    the precision of its inputs."""
    zero = P["v_sys"] * 0
    return oracle.model_rotation(ra, dec, P["v_sys"], P["v_maxx"], P["v_maxy"], P["r_peak"], rc, dc) + \
        oracle.model_rotation(ra, dec, zero, P["v_maxx_c"], P["v_maxy_c"], P["r_peak_ratio"] * P["r_peak"], rc, dc)


def star_terms(cat, row, model, centre, dtype=np.float64):
    """(lnL_i, p_i) of one parameter row (C-ABI order) from the oracle's per-star functions: the star's term of lnlike
    (runner.py:280-284, constant.py:320-364, model.py:391-623) and its membership probability (constant.py:366-374,
    model.py:505-510, 680-687); p is None for the models without a background.  `dtype` other than float64 (the double
    models only): every input cast to it."""
    if model in DOUBLE:
        return double_star_terms(cat, row, model, centre, dtype)
    assert dtype is np.float64
    P = dict(zip(abi_names(model, centre is None), row))
    rc, dc = (P["ra_center"], P["dec_center"]) if centre is None else centre
    ra, dec, v, verr = cat["ra"], cat["dec"], cat["v"], cat["verr"]
    if model in PROFILE:
        v_los = oracle.model_rotation(ra, dec, P["v_sys"], P["v_maxx"], P["v_maxy"], P["r_peak"], rc, dc)
        sigma = oracle.model_dispersion(ra, dec, P["sigma_max"], P["a"], rc, dc)
    else:
        v_los = oracle.rotation_model(ra, dec, P["v_sys"], P["v_maxx"], P["v_maxy"], rc, dc)
        sigma = oracle.dispersion_model(len(v), P["sigma_max"])
    norm = verr * verr + sigma * sigma
    lc = -0.5 * np.log(2. * np.pi * norm) - 0.5 * np.power(v - v_los, 2) / norm
    bg = BG[model]
    if bg == 0:
        return lc, None
    if bg == 1:
        lb, m = cat["lnlike_bg"], cat["pmember"]
    elif bg == 3:
        lb, m = cat["lnlike_bg"], cat["density"] / (cat["density"] + P["f_back"])
    elif model == 2:
        lc_, lb, m = oracle.faithful_constant_gb_terms(cat, P["v_sys"], P["sigma_max"], P["v_maxx"], P["v_maxy"], rc, dc,
                                                       P["v_back"], P["sigma_back"], P["f_back"])
    else:
        lb = oracle.gaussian_background(v, verr, P["v_back"], P["sigma_back"])
        m = cat["density"] / (cat["density"] + P["f_back"])
    mx = np.max([lc, lb], axis=0)
    x = mx + np.log(m * np.exp(lc - mx) + (1. - m) * np.exp(lb - mx))
    if model in PROFILE:
        p = oracle.model_membership(cat, lc, lb, m)
    else:
        p = m * np.exp(lc) / (m * np.exp(lc) + (1. - m) * np.exp(lb))
    return x, p


def double_star_terms(cat, row, model, centre, dtype=np.float64):
    """star_terms of models 7 and 8 in `dtype` (float64 or numpy.longdouble)."""
    P = {k: dtype(x) for k, x in zip(abi_names(model, centre is None), row)}
    rc, dc = (P["ra_center"], P["dec_center"]) if centre is None else (dtype(centre[0]), dtype(centre[1]))
    ra, dec, v, verr = (np.asarray(cat[k]).astype(dtype) for k in ("ra", "dec", "v", "verr"))
    v_los = double_rotation(ra, dec, P, rc, dc)
    sigma = oracle.model_dispersion(ra, dec, P["sigma_max"], P["a"], rc, dc)
    norm = verr * verr + sigma * sigma
    lc = -0.5 * np.log(2. * np.pi * norm) - 0.5 * np.power(v - v_los, 2) / norm
    assert lc.dtype == dtype
    if BG[model] == 0:
        return lc, None
    lb = oracle.gaussian_background(v, verr, P["v_back"], P["sigma_back"])
    rho = np.asarray(cat["density"]).astype(dtype)
    m = rho / (rho + P["f_back"])
    mx = np.max([lc, lb], axis=0)
    ec, eb = m * np.exp(lc - mx), (1. - m) * np.exp(lb - mx)
    assert ec.dtype == dtype
    return mx + np.log(ec + eb), ec / (ec + eb)


def numpy_posterior(cat, table, model, centre):
    xs, ps = [], []
    for row in np.atleast_2d(table):
        x, p = star_terms(cat, row, model, centre)
        xs.append(x)
        ps.append(p)
    x = np.array(xs)                                   # (S, n)
    S = x.shape[0]
    mx = x.max(axis=0)
    out = {"lppd": mx + np.log(np.exp(x - mx).sum(axis=0)) - np.log(S),
           "lnl_var": x.var(axis=0, ddof=1) if S > 1 else np.zeros(x.shape[1])}
    if ps[0] is not None:
        p = np.array(ps)
        out["pmem_mean"] = p.mean(axis=0)
        out["pmem_std"] = p.std(axis=0, ddof=1) if S > 1 else np.zeros(p.shape[1])
    return out


def model_catalog(n, model, seed=7):
    """Synthetic catalogue with every column the models need (lnlike_bg: a fixed Gaussian background).  Stars within
    0.01 arcmin of the centre, where the reference's arctan2 of two O(0.4) differences is ill-conditioned, are moved onto
    the outermost star (as smoke() does)."""
    cat = synthetic.make_catalog(n, config=2, seed=seed, background=True)
    cat["lnlike_bg"] = oracle.gaussian_background(cat["v"], cat["verr"], 20.0, 40.0)
    dx, dy = oracle.calc_xy_offset(cat["ra"], cat["dec"], synthetic.CENTER_RA_DEG, synthetic.CENTER_DEC_DEG)
    r = np.hypot(dx, dy)
    near = r < 1e-2
    if near.any():
        donor = int(np.argmax(r))
        cat["ra"][near], cat["dec"][near] = cat["ra"][donor], cat["dec"][donor]
    return cat


CENTRE = (synthetic.CENTER_RA_DEG, synthetic.CENTER_DEC_DEG)


TRUTH_EXTRA = {"a": 60.0, "r_peak": 90.0, "v_maxx_c": 2.0, "v_maxy_c": -1.5, "r_peak_ratio": 0.4}


def samples(cat, model, free, S, seed=3):
    """S parameter rows (C-ABI order) scattered around the catalogue's truth."""
    rng = np.random.default_rng(seed)
    rows = []
    for name in abi_names(model, free):
        t = float(cat["truth"][name]) if name in cat["truth"] else TRUTH_EXTRA[name]
        g = rng.normal(size=S)
        if name in ("ra_center", "dec_center"):
            col = t + (0.05 / 60.0) * g
        elif name == "f_back":
            col = np.clip(t * (1.0 + 0.1 * g), 0.01, 0.99)
        else:
            col = t * (1.0 + 0.05 * g) if t != 0.0 else 0.5 * g
        rows.append(col)
    return np.ascontiguousarray(np.stack(rows, axis=1))

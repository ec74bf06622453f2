"""Test helper: CPU build of the per-star posterior predictive checks (tests/emul/predictive_emul.cpp +
csrc/mcd_predictive.h + csrc/mcd_math.h), and the independent NumPy restatement they and the device are checked against.
Test infrastructure only.

The restatement takes v_los and sigma_los from the oracle's functions (oracle/lnprob_numpy.py: rotation_model /
model_rotation, dispersion_model / model_dispersion), the way posterior_helper.star_terms does, and runs in float64 or in
numpy.longdouble.  The "exact" probabilities are scipy.special.erfc at the longdouble argument rounded to double: an
argument error of 2^-53 relative moves erfc by less than 1e-16 absolute (|x erfc'(x)| = 2 x exp(-x^2) / sqrt(pi) <= 0.49), and
scipy's erfc is pinned against mpmath in test_predictive_cpu.py.

The accuracy rule, per output and per star:
    |got - exact| <= 2 |np64 - exact| + 1e-12 scale
with scale = 1 for tail_p, pit and pit_mix, max(1, |z_mean|) for z_mean, max |v| for vlos_mean, max(1, sigma) for
sigma_mean; the three spreads are compared on the variance with var_ok of tests/test_posterior_cpu.py."""
import ctypes
import os
import subprocess

import numpy as np
from scipy import special

import emul_helper as emul
import posterior_helper as ph
from oracle import lnprob_numpy as oracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "emul", "predictive_emul.cpp")
INC = os.path.join(ROOT, "mcmc_dynamics_amd", "csrc")
OUT = os.path.join(ROOT, "tests", "emul", "libpredictive_emul.so")
L = np.longdouble
FIELDS = ("z_mean", "z_std", "tail_p", "pit", "vlos_mean", "vlos_std", "sigma_mean", "sigma_std")
MIX_MODELS = (2, 4, 8)
_lib = None


def lib():
    global _lib
    if _lib is None:
        deps = [SRC] + [os.path.join(INC, f) for f in ("mcd_predictive.h", "mcd_posterior.h", "mcd_math.h", "mcd_exp_table.h",
                                                       "mcd_dispatch.h")]
        if not os.path.exists(OUT) or any(os.path.getmtime(d) > os.path.getmtime(OUT) for d in deps):
            subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-I", INC, SRC,
                            "-o", OUT], check=True)
        lb = ctypes.CDLL(OUT)
        lb.emul_predictive.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int64, ctypes.c_void_p,
                                       ctypes.c_void_p, ctypes.c_int64, ctypes.c_int64, ctypes.c_void_p]
        lb.emul_normal_tail_cdf.argtypes = [ctypes.c_int64, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
        lb.emul_normal_tail_cdf.restype = None
        _lib = lb
    return _lib


def _unpack(out, mix):
    d = dict(zip(FIELDS, out[:8]))
    if mix:
        d["pit_mix"] = out[8]
    return d


def predictive(cat, table, model, centre, mix=False, n_slices=0, f32=False):
    """Emulated mcd_posterior_predictive: table (S, K) in the C-ABI column order; n_slices 0 = the library's plan."""
    rec = emul.pack_records(cat, model, centre)
    wp = emul.pack_walkers(table, model, centre is None)
    n = rec.shape[0]
    out = np.full((9, n), np.nan)
    rc = lib().emul_predictive(model, int(centre is None), int(mix), int(f32), n, rec.ctypes.data, wp.ctypes.data,
                               wp.shape[0], int(n_slices), out.ctypes.data)
    assert rc == 0
    return _unpack(out, mix)


def normal_tail_cdf(z):
    z = np.ascontiguousarray(z, dtype=np.float64)
    t, c = np.empty_like(z), np.empty_like(z)
    lib().emul_normal_tail_cdf(z.size, z.ctypes.data, t.ctypes.data, c.ctypes.data)
    return t, c


# ---- NumPy restatement ------------------------------------------------------------------------------------------
def _tail_cdf(z, dtype):
    """t = erfc(|z| / sqrt 2) through scipy at the double-rounded argument, and the CDF from it on the safe side."""
    t = special.erfc((np.abs(z) / np.sqrt(dtype(2))).astype(np.float64)).astype(dtype)
    return t, np.where(z < 0, t / 2, 1 - t / 2)


def star_terms(cat, row, model, centre, dtype=np.float64):
    """The (star, sample) quantities of one parameter row (C-ABI order), every input cast to `dtype`: dict of (n,) arrays
    z, t, pit, vlos, sig and, for the two models with a Gaussian background, pit_mix."""
    P = {k: dtype(x) for k, x in zip(ph.abi_names(model, centre is None), row)}
    rc, dc = (P["ra_center"], P["dec_center"]) if centre is None else (dtype(centre[0]), dtype(centre[1]))
    ra, dec, v, verr = (np.asarray(cat[k]).astype(dtype) for k in ("ra", "dec", "v", "verr"))
    if model in ph.DOUBLE:
        v_los = ph.double_rotation(ra, dec, P, rc, dc)                # both components
        sigma = oracle.model_dispersion(ra, dec, P["sigma_max"], P["a"], rc, dc)
    elif model in ph.PROFILE:
        v_los = oracle.model_rotation(ra, dec, P["v_sys"], P["v_maxx"], P["v_maxy"], P["r_peak"], rc, dc)
        sigma = oracle.model_dispersion(ra, dec, P["sigma_max"], P["a"], rc, dc)
    else:
        v_los = oracle.rotation_model(ra, dec, P["v_sys"], P["v_maxx"], P["v_maxy"], rc, dc)
        sigma = oracle.dispersion_model(len(v), P["sigma_max"])
    assert v_los.dtype == dtype and sigma.dtype == dtype
    z = (v - v_los) / np.sqrt(verr * verr + sigma * sigma)
    t, pit = _tail_cdf(z, dtype)
    out = {"z": z, "t": t, "pit": pit, "vlos": v_los, "sig": np.abs(sigma)}
    if model in MIX_MODELS:
        zb = (v - P["v_back"]) / np.sqrt(verr * verr + P["sigma_back"] * P["sigma_back"])
        rho = np.asarray(cat["density"]).astype(dtype)
        m = rho / (rho + P["f_back"])
        out["pit_mix"] = m * pit + (1 - m) * _tail_cdf(zb, dtype)[1]
    return out


def sample_terms(cat, table, model, centre, dtype):
    """The same for every row of `table`: dict of (S, n) arrays."""
    rows = [star_terms(cat, row, model, centre, dtype) for row in np.atleast_2d(table)]
    return {k: np.array([r[k] for r in rows]) for k in rows[0]}


def reduce_terms(terms, n=None, s=None):
    """Means and sample variances over the first `s` samples of the first `n` stars, in the terms' own precision."""
    out = {}
    for key, name in (("z", "z"), ("vlos", "vlos"), ("sig", "sigma")):
        x = terms[key][:s, :n]
        out[name + "_mean"] = x.mean(axis=0)
        out[name + "_var"] = x.var(axis=0, ddof=1) if x.shape[0] > 1 else np.zeros(x.shape[1], dtype=x.dtype)
    for key, name in (("t", "tail_p"), ("pit", "pit"), ("pit_mix", "pit_mix")):
        if key in terms:
            out[name] = terms[key][:s, :n].mean(axis=0)
    return out


class Reference(object):
    """The longdouble ("exact") and float64 runs of the restatement over (table, catalogue), computed once; `at(n, s)`
    reduces the first s samples of the first n stars."""

    def __init__(self, cat, table, model, centre):
        self.exact = sample_terms(cat, table, model, centre, L)
        self.np64 = sample_terms(cat, table, model, centre, np.float64)
        self.v = np.asarray(cat["v"], dtype=np.float64)

    def at(self, n=None, s=None):
        return reduce_terms(self.exact, n, s), reduce_terms(self.np64, n, s), float(np.max(np.abs(self.v[:n])))


SPREADS = (("z_std", "z_var", "z_mean"), ("vlos_std", "vlos_var", "vlos_mean"), ("sigma_std", "sigma_var", "sigma_mean"))


def scales(exact, vmax):
    one = np.ones_like(np.asarray(exact["z_mean"], dtype=np.float64))
    return {"tail_p": one, "pit": one, "pit_mix": one,
            "z_mean": np.maximum(1.0, np.abs(exact["z_mean"]).astype(np.float64)), "vlos_mean": vmax * one,
            "sigma_mean": np.maximum(1.0, exact["sigma_mean"].astype(np.float64))}


def rule_excess(got, exact, np64, vmax):
    """Per mean output: the largest (|got - exact| - 2 |np64 - exact|) / scale over the stars (the rule asks <= 1e-12)."""
    sc = scales(exact, vmax)
    out = {}
    for f in ("z_mean", "tail_p", "pit", "vlos_mean", "sigma_mean", "pit_mix"):
        if f in got:
            err = np.abs(got[f].astype(L) - exact[f]) - 2 * np.abs(np64[f].astype(L) - exact[f])
            out[f] = float(np.max(err / sc[f])) if err.size else 0.0
    return out


def check_rule(got, exact, np64, vmax, var_ok, rtol, floor=1e-12, cell=None):
    """The accuracy rule on every output of `got` (spreads on the variance through `var_ok` with `rtol`).  `floor`: one
    number, or a dict per mean output (predictive_bounds.floors)."""
    excess = rule_excess(got, exact, np64, vmax)
    for f, e in excess.items():
        fl = floor.get(f, 1e-12) if isinstance(floor, dict) else floor
        print("{0} {1}: excess {2:.3e} (floor {3:.1e})".format(cell, f, e, fl))
        assert e <= fl, (cell, f, e, fl)
    sc = scales(exact, vmax)
    for std, var, mean in SPREADS:
        want = exact[var].astype(np.float64)
        assert var_ok(got[std] ** 2, want, sc[mean], rtol=rtol), (cell, std, float(np.max(np.abs(got[std] ** 2 - want))))


# ---- catalogues and samples -------------------------------------------------------------------------------------
PLANTED = {"on_model": 1, "plus45": 2, "minus45": 3, "verr0": 4, "density0": 5}


def plant(cat, table, model, centre):
    """A copy of `cat` with the planted stars of PLANTED at their fixed indices: v_i on the model of the first sample
    (z ~ 0 there), z ~ +-45 under the first sample, verr = 0, density = 0."""
    cat = {k: (x.copy() if isinstance(x, np.ndarray) else x) for k, x in cat.items()}
    cat["verr"][PLANTED["verr0"]] = 0.0
    cat["density"][PLANTED["density0"]] = 0.0
    t0 = star_terms(cat, table[0], model, centre)
    norm = np.sqrt(cat["verr"] ** 2 + t0["sig"] ** 2)
    for key, k in (("on_model", 0.0), ("plus45", 45.0), ("minus45", -45.0)):
        i = PLANTED[key]
        cat["v"][i] = t0["vlos"][i] + k * norm[i]
    return cat


MATRIX_N = (1, 65, 4099)        # a lone lane, one tile plus one star, 17 workgroups with a partial last tile
MATRIX_S = (1, 65, 257)         # 257 samples at N = 65 give 5 slices with a short last one
_matrix = {}


def matrix_case(model, free):
    """The catalogue (4099 stars, the planted ones at indices 1 .. 5), the 257 samples and the Reference of one (model,
    centre mode) cell of the device matrix, computed once; the cells with fewer stars / samples take the first N / S."""
    key = (model, free)
    if key not in _matrix:
        cat = ph.model_catalog(max(MATRIX_N), 0, seed=7)
        table = ph.samples(cat, model, free, max(MATRIX_S))
        centre = None if free else ph.CENTRE
        cat = clear_of_centres(cat, *(sample_centres(table, model) if free else ph.CENTRE))
        cat = plant(cat, table, model, centre)
        _matrix[key] = (cat, table, centre, Reference(cat, table, model, centre))
    return _matrix[key]


def head(cat, n):
    """The first n stars of a catalogue."""
    return {k: (x[:n].copy() if isinstance(x, np.ndarray) else x) for k, x in cat.items()}


def device_catalog(ctx, cat, model, centre, precision="f64"):
    from mcmc_dynamics_amd import _native
    extra = {}
    bg = emul.BG_OF[model]
    if bg == 1:
        extra = {"lnlike_bg": cat["lnlike_bg"], "pmember": cat["pmember"]}
    elif bg == 2:
        extra = {"density": cat["density"]}
    elif bg == 3:
        extra = {"lnlike_bg": cat["lnlike_bg"], "density": cat["density"]}
    return _native.Catalog(ctx, cat["ra"], cat["dec"], cat["v"], cat["verr"], model=model, centre=centre,
                           precision=precision, **extra)


# ---- calibration ------------------------------------------------------------------------------------------------
CALIBRATION_SEED = 20240611
CALIBRATION_N = 20000
CHI2_19_Q999 = 43.82                                      # 0.999 quantile of chi^2 with 19 degrees of freedom


def calibration_case(seed=CALIBRATION_SEED, n=CALIBRATION_N):
    """20 000 stars whose velocities are drawn from the constant-rotation model itself at a truth vector,
    v = v_los + sqrt(verr^2 + sigma^2) N(0, 1) with v_los and sigma from the oracle's functions; returns (catalogue, truth
    row in C-ABI order for MODEL_CONST with a fixed centre)."""
    cat = ph.model_catalog(n, 0, seed=11)
    cat = {k: (x.copy() if isinstance(x, np.ndarray) else x) for k, x in cat.items()}
    truth = np.array([3.0, 8.0, 2.5, -1.5])              # v_sys, sigma_max, v_maxx, v_maxy
    v_los = oracle.rotation_model(cat["ra"], cat["dec"], truth[0], truth[2], truth[3], ph.CENTRE[0], ph.CENTRE[1])
    sigma = oracle.dispersion_model(n, truth[1])
    rng = np.random.default_rng(seed)
    cat["v"] = v_los + np.sqrt(cat["verr"] ** 2 + sigma ** 2) * rng.normal(size=n)
    return cat, truth


def clear_of_centres(cat, ra_c, dec_c, limit=0.8):
    """Stars within `limit` arcmin of ANY of the centres (ra_c, dec_c: arrays, degrees) are moved onto the outermost star,
    the exclusion model_catalog applies around the nominal centre, for its reason: next to a centre theta = arctan2(dy, dx)
    is ill-conditioned in the reference's own formula.  Fixed centre: dy of calc_xy_offset.py:31 is the difference of two
    O(0.4) products, so one ulp of the device's sin / cos against NumPy's leaves ~2e-16 rad in it.  Free centre: the records
    hold A = cos(dec) sin(ra), B = cos(dec) cos(ra) and the offsets are differences of O(0.4) products, x = B sin(ra_c) -
    A cos(ra_c): four rounded inputs (4.4e-17 each) and two rounded products (2.8e-17 each) leave up to 2.3e-16 rad in x and
    in y whatever follows.  Either way up to 3.3e-16 / r in theta and 3.3e-16 / r x v_max / sqrt(n) in z (a star 0.0015
    arcmin from a sample's centre carries 1e-10), which the oracle's float64 run shares only in part (it forms
    sin(ra - ra_c) from the angles' difference), so the rule's 2 |np64 - exact| allowance does not cover it.  With the
    samples of posterior_helper.samples on model_catalog (v_max <= 5.8, sqrt(n) >= 8.5 at three sigma of their scatter)
    that worst case stays within the rule's floor of 1e-12 for r >= 2.3e-4 rad = 0.8 arcmin; variant_helper.make_case keeps
    0.6 arcmin for the same reason."""
    ra_c, dec_c = np.atleast_1d(np.asarray(ra_c, dtype=np.float64)), np.atleast_1d(np.asarray(dec_c, dtype=np.float64))
    cat = {k: (x.copy() if isinstance(x, np.ndarray) else x) for k, x in cat.items()}
    dx, dy = oracle.calc_xy_offset(cat["ra"][:, None], cat["dec"][:, None], ra_c[None, :], dec_c[None, :])
    r = np.hypot(dx, dy)
    near = r.min(axis=1) < limit
    if near.any():
        donor = int(np.argmax(r.min(axis=1)))
        cat["ra"][near], cat["dec"][near] = cat["ra"][donor], cat["dec"][donor]
    return cat


def sample_centres(table, model):
    names = ph.abi_names(model, True)
    return table[:, names.index("ra_center")], table[:, names.index("dec_center")]

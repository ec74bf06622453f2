"""Test helper: CPU build of the replicated-data predictive checks (tests/emul/replicate_emul.cpp + csrc/mcd_replicate.h),
and the independent NumPy restatement they and the device are checked against.  Test infrastructure only.

The restatement reads the generator's numbers g, u from the emulated mcd_replicate_numbers (the generator itself is pinned
against numpy.random.Philox in test_replicate_cpu.py) and forms v_los and sigma_los from the oracle's functions
(oracle/lnprob_numpy.py: rotation_model / model_rotation, dispersion_model / model_dispersion) in float64 or in
numpy.longdouble, the way predictive_helper.star_terms does.

The accuracy rule, per field, sample and range:
    |got - exact| <= 2 |np64 - exact| + 1e-12 scale
with scale = the sum of the absolute terms for the six sums and the maximum itself for max |z|; the count of |z| > 3 is
compared exactly.  On the exact side the helper asserts that no |z| lies within 1e-9 of 3 and no u within 1e-9 of m, so
that neither the count nor the choice of the component can depend on a rounding error."""
import ctypes
import os
import subprocess

import numpy as np

import emul_helper as emul
import posterior_helper as ph
import predictive_helper as pr
from oracle import lnprob_numpy as oracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "emul", "replicate_emul.cpp")
INC = os.path.join(ROOT, "mcmc_dynamics_amd", "csrc")
OUT = os.path.join(ROOT, "tests", "emul", "libreplicate_emul.so")
L = np.longdouble
FIELDS = ("s1", "s2", "s3", "s4", "sin", "cos", "max", "tail3")
F_MAX, F_TAIL3 = 6, 7
BG_MEAN, BG_SIGMA = 20.0, 40.0          # the Gaussian behind posterior_helper.model_catalog's lnlike_bg column
SEED = 20240917                         # the committed generator seed of the matrix (checked by Reference's assertions)
_lib = None
_u64, _i64, _vp = ctypes.c_uint64, ctypes.c_int64, ctypes.c_void_p


def lib():
    global _lib
    if _lib is None:
        deps = [SRC] + [os.path.join(INC, f) for f in ("mcd_replicate.h", "mcd_predictive.h", "mcd_rng.h", "mcd_chunks.h",
                                                       "mcd_math.h", "mcd_exp_table.h", "mcd_dispatch.h")]
        if not os.path.exists(OUT) or any(os.path.getmtime(d) > os.path.getmtime(OUT) for d in deps):
            subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-I", INC, SRC,
                            "-o", OUT], check=True)
        lb = ctypes.CDLL(OUT)
        lb.emul_replicate.argtypes = [ctypes.c_int, ctypes.c_int, _vp, _vp, _i64, _u64, _i64, _i64, _vp, _vp,
                                      ctypes.c_double, ctypes.c_double, _i64, _vp]
        lb.emul_replicate_validate.argtypes = [ctypes.c_int, _i64, _vp, _vp, _i64, ctypes.c_double, ctypes.c_double,
                                               ctypes.c_char_p, ctypes.c_int]
        lb.emul_replicate_plan.argtypes = [_i64, _vp, _i64, _i64, _i64, _i64, _vp, _vp, _vp, _vp]
        lb.emul_replicate_plan.restype = _i64
        lb.emul_replicate_numbers.argtypes = [_u64, _i64, _i64, _i64, _i64, _vp, _vp]
        lb.emul_replicate_numbers.restype = None
        lb.emul_rep_normal.argtypes = [_u64, _i64, _i64, ctypes.c_int, ctypes.POINTER(ctypes.c_int)]
        lb.emul_rep_normal.restype = ctypes.c_double
        lb.emul_rep_key.restype = _u64
        lb.emul_rep_max_rows.restype = _i64
        lb.emul_rep_scratch_bytes.restype = _i64
        lb.emul_star_unit.argtypes = [ctypes.c_int, ctypes.c_int, _i64, _vp, _vp, _vp, _vp]
        _lib = lb
    return _lib


def numbers(seed, s0, S, i0, N):
    """g, u (S, N) of sample rows s0 .. and stars i0 .. (host build of csrc/mcd_replicate.h)."""
    g, u = np.empty((S, N)), np.empty((S, N))
    lib().emul_replicate_numbers(seed, s0, S, i0, N, g.ctypes.data, u.ctypes.data)
    return g, u


def rep_normal(seed, s, i, max_calls=None):
    """(the normal, pairs drawn) of one (seed, sample row, star)."""
    used = ctypes.c_int(0)
    z = lib().emul_rep_normal(seed, s, i, lib().emul_rep_normal_calls() if max_calls is None else max_calls,
                              ctypes.byref(used))
    return z, used.value


def rep_words(seed, s, i, slot, call):
    """The four words of the replicate stream's generator call with counter (s, i, slot, call)."""
    out = np.empty(4, dtype=np.uint64)
    lib().emul_rep_words.argtypes = [_u64, _i64, _i64, _i64, _i64, _vp]
    lib().emul_rep_words.restype = None
    lib().emul_rep_words(seed, s, i, slot, call, out.ctypes.data)
    return out


def background_of(model):
    """(bg_mean, bg_sigma) of a call: the catalogue's Gaussian for the fixed-background models, NaN otherwise."""
    return (BG_MEAN, BG_SIGMA) if emul.BG_OF[model] in (1, 3) else (float("nan"), float("nan"))


def replicate(cat, table, model, centre, seed, offs, order, bg=None, forced_len=0, row0=0):
    """Emulated mcd_replicate_check: (S, R, 8, 2)."""
    rec = emul.pack_records(cat, model, centre)
    wp = emul.pack_walkers(table, model, centre is None)
    offs = np.ascontiguousarray(offs, dtype=np.int64)
    order = np.ascontiguousarray(order, dtype=np.int64)
    bg = background_of(model) if bg is None else bg
    out = np.full((wp.shape[0], offs.size - 1, 8, 2), np.nan)
    rc = lib().emul_replicate(model, int(centre is None), rec.ctypes.data, wp.ctypes.data, wp.shape[0], seed, row0,
                              offs.size - 1, offs.ctypes.data, order.ctypes.data, bg[0], bg[1], int(forced_len), out.ctypes.data)
    assert rc == 0
    return out


def validate(model, offs, order, n_stars, bg=(float("nan"), float("nan"))):
    """The host checks of mcd_replicate_check on (ranges, order, background): None, or the message."""
    offs = np.ascontiguousarray(offs, dtype=np.int64)
    order = np.ascontiguousarray(order, dtype=np.int64)
    msg = ctypes.create_string_buffer(200)
    rc = lib().emul_replicate_validate(model, offs.size - 1, offs.ctypes.data, order.ctypes.data if order.size else None,
                                       n_stars, bg[0], bg[1], msg, 200)
    return msg.value.decode() if rc else None


def plan(offs, S, forced_len=0, scratch_bytes=0):
    """The pass length and chunk table of a call: dict."""
    offs = np.ascontiguousarray(offs, dtype=np.int64)
    cap = int(offs[-1]) // 8 + 2 * offs.size + 8
    begin, count, rng_, info = np.empty(cap, np.int64), np.empty(cap, np.int32), np.empty(cap, np.int32), np.zeros(4, np.int64)
    nc = lib().emul_replicate_plan(offs.size - 1, offs.ctypes.data, S, forced_len, scratch_bytes, cap, begin.ctypes.data,
                                   count.ctypes.data, rng_.ctypes.data, info.ctypes.data)
    assert nc <= cap
    return {"pass_rows": int(info[0]), "n_chunks": int(nc), "len": int(info[2]), "longest": int(info[3]),
            "begin": begin[:nc], "count": count[:nc], "range": rng_[:nc]}


def star_unit(cat, row, model, centre):
    rec = emul.pack_records(cat, model, centre)
    wp = emul.pack_walkers(np.asarray(row)[None, :], model, centre is None)
    c, s = np.empty(rec.shape[0]), np.empty(rec.shape[0])
    assert lib().emul_star_unit(model, int(centre is None), rec.shape[0], rec.ctypes.data, wp.ctypes.data, c.ctypes.data,
                                s.ctypes.data) == 0
    return c, s


# ---- range layouts ----------------------------------------------------------------------------------------------
LAYOUTS = ("one", "three", "sixteen")


def layout(kind, n, seed=5):
    """(range_offsets, order) over n stars.  one: every star in catalogue order.  three: a shuffled order with an empty and
    a singleton range and about a tenth of the stars in no range.  sixteen: 16 ranges of nearly equal size, shuffled."""
    rng = np.random.default_rng(seed + n)
    if kind == "one":
        return np.array([0, n], np.int64), np.arange(n, dtype=np.int64)
    perm = rng.permutation(n).astype(np.int64)
    if kind == "three":
        # the singleton is star 0, the star matrix_case prepares for standing alone (lone_star)
        perm = np.concatenate([[0], perm[perm != 0]]).astype(np.int64)
        used = max(1, n - n // 10)
        return np.array([0, 0, 1, used], np.int64), perm[:used]
    assert kind == "sixteen"
    return (np.arange(17, dtype=np.int64) * n) // 16, perm


# ---- NumPy restatement ------------------------------------------------------------------------------------------
def star_terms(cat, row, model, centre, g, u, bg, dtype=np.float64):
    """z_obs, z_rep, c, s, m (n,) of one parameter row (C-ABI order), every input cast to `dtype`; g, u: that row's numbers."""
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
        sigma = oracle.dispersion_model(len(v), P["sigma_max"]).astype(dtype)
    assert v_los.dtype == dtype and sigma.dtype == dtype
    dx, dy = oracle.calc_xy_offset(ra, dec, rc, dc)
    r = np.hypot(dx, dy)
    assert np.all(r > 0)
    sd = np.sqrt(verr * verr + sigma * sigma)
    d = v - v_los
    g, u = g.astype(dtype), u.astype(dtype)
    out = {"z_obs": d / sd, "c": dx / r, "s": dy / r}
    kind = emul.BG_OF[model]
    if kind == 0:
        out["z_rep"], out["m"] = g, np.ones_like(g)
        return out
    if kind == 1:
        m = np.asarray(cat["pmember"]).astype(dtype)
    else:
        rho = np.asarray(cat["density"]).astype(dtype)
        m = rho / (rho + P["f_back"])
    mu, sb = (P["v_back"], P["sigma_back"]) if kind == 2 else (dtype(bg[0]), dtype(bg[1]))
    zb = ((mu - v) + d + np.sqrt(verr * verr + sb * sb) * g) / sd
    out["z_rep"], out["m"] = np.where(u < m, g, zb), m
    return out


def sample_terms(cat, table, model, centre, g, u, bg, dtype):
    rows = [star_terms(cat, row, model, centre, g[s], u[s], bg, dtype) for s, row in enumerate(np.atleast_2d(table))]
    return {k: np.array([r[k] for r in rows]) for k in rows[0]}


def fields_of(t, offs, order, s=None):
    """(values, scales), each (S, R, 8, 2), of the terms `t` (dict of (S, n)) in the terms' own precision."""
    S = t["z_obs"][:s].shape[0]
    R = len(offs) - 1
    dtype = t["z_obs"].dtype
    val, scale = np.zeros((S, R, 8, 2), dtype=dtype), np.zeros((S, R, 8, 2), dtype=dtype)
    for r in range(R):
        idx = np.asarray(order[offs[r]:offs[r + 1]], dtype=np.int64)
        if idx.size == 0:
            continue
        c, sn = t["c"][:s][:, idx], t["s"][:s][:, idx]
        for w, key in enumerate(("z_obs", "z_rep")):
            z = t[key][:s][:, idx]
            cols = (z, z * z, z * z * z, (z * z) * (z * z), z * sn, z * c)
            for f, x in enumerate(cols):
                val[:, r, f, w] = x.sum(axis=1)
                scale[:, r, f, w] = np.abs(x).sum(axis=1)
            val[:, r, F_MAX, w] = scale[:, r, F_MAX, w] = np.abs(z).max(axis=1)
            val[:, r, F_TAIL3, w] = (np.abs(z) > 3).sum(axis=1)
    return val, scale


class Reference(object):
    """The longdouble ("exact") and float64 runs of the restatement over (catalogue, table) with the generator's numbers
    of `seed`, computed once; `at(offs, order, s)` reduces the first s samples over a layout."""

    def __init__(self, cat, table, model, centre, seed=SEED, bg=None, row0=0):
        table = np.atleast_2d(table)
        n = len(cat["v"])
        bg = background_of(model) if bg is None else bg
        g, u = numbers(seed, row0, table.shape[0], 0, n)
        self.exact = sample_terms(cat, table, model, centre, g, u, bg, L)
        self.np64 = sample_terms(cat, table, model, centre, g, u, bg, np.float64)
        # what the count and the choice of the component must not hinge on
        for key in ("z_obs", "z_rep"):
            assert np.min(np.abs(np.abs(self.exact[key]) - 3)) > 1e-9, (key, "a |z| within 1e-9 of 3: choose another seed")
        if emul.BG_OF[model]:
            assert np.min(np.abs(u.astype(L) - self.exact["m"])) > 1e-9, "a u within 1e-9 of m: choose another seed"

    def at(self, offs, order, s=None):
        e, sc = fields_of(self.exact, offs, order, s)
        d, _ = fields_of(self.np64, offs, order, s)
        return e, d, sc.astype(np.float64)


def rule_excess(got, exact, np64, scale):
    """Per field: the largest (|got - exact| - 2 |np64 - exact|) / scale over samples, ranges and the two residuals (the
    rule asks <= 1e-12); cells with scale 0 (an empty range) must be exactly +0.0.  The count is compared exactly."""
    assert got.shape == exact.shape, (got.shape, exact.shape)
    assert np.array_equal(got[:, :, F_TAIL3], exact[:, :, F_TAIL3].astype(np.float64)), "count of |z| > 3"
    out = {}
    for f in range(7):
        g_, e_, d_, s_ = got[:, :, f], exact[:, :, f], np64[:, :, f], scale[:, :, f]
        empty = s_ == 0
        assert np.all(g_[empty] == 0.0)
        err = np.abs(g_.astype(L) - e_) - 2 * np.abs(d_.astype(L) - e_)
        out[FIELDS[f]] = float(np.max(err[~empty] / s_[~empty])) if (~empty).any() else 0.0
    return out


def check_rule(got, exact, np64, scale, floor=1e-12, cell=None):
    for f, e in rule_excess(got, exact, np64, scale).items():
        print("{0} {1}: excess {2:.3e}".format(cell, f, e))
        assert e <= floor, (cell, f, e)


# ---- the matrix -------------------------------------------------------------------------------------------------
MATRIX_N = pr.MATRIX_N          # (1, 65, 4099)
MATRIX_S = pr.MATRIX_S          # (1, 65, 257)
_cases = {}
# The angular sums make the position angle itself an output: a term z sin(theta) moves by z cos(theta) d(theta), and
# predictive_helper.clear_of_centres derives d(theta) <= 3.3e-16 / r from the rounded products of the offsets, shared
# only in part by the oracle's float64 run.  The matrix has ranges of ONE and of FOUR stars (N = 1; N = 65 in sixteen
# ranges), whose scale, the sum of their absolute terms, can be a small part of a single term z: at posterior_helper's
# field (0.9 .. 5 arcmin; errors of 1e-13 in sin(theta) were seen at 1 arcmin) a relative bound of 1e-12 cannot hold
# there (seen: 1.2e-12 with a four-star range whose sum of |z sin| was 0.097).  The matrix therefore spreads the same
# stars over twenty times the field and keeps them CLEARANCE = 18 arcmin = 5.2e-3 rad from every centre:
# d(theta) <= 6.3e-14, a tenth of that typically (at ten times the field a four-star range that holds a background
# replicate of z = 19.6 at sin(theta) = 0.0024 still reached 8.3e-13).
FIELD_STRETCH, CLEARANCE = 20.0, 18.0


def wide_field(cat):
    """The catalogue with its offsets from the nominal centre multiplied by FIELD_STRETCH."""
    cat = {k: (x.copy() if isinstance(x, np.ndarray) else x) for k, x in cat.items()}
    cat["ra"] = ph.CENTRE[0] + FIELD_STRETCH * (cat["ra"] - ph.CENTRE[0])
    cat["dec"] = ph.CENTRE[1] + FIELD_STRETCH * (cat["dec"] - ph.CENTRE[1])
    return cat


def matrix_case(model, free):
    """(catalogue of 4099 stars clear of the centres with predictive_helper's planted stars, 257 samples, centre) of one
    (model, centre mode) cell, computed once; smaller cells take the first N stars / S samples."""
    key = (model, free)
    if key not in _cases:
        cat = wide_field(ph.model_catalog(max(MATRIX_N), 0, seed=7))
        table = ph.samples(cat, model, free, max(MATRIX_S))
        centre = None if free else ph.CENTRE
        cat = pr.clear_of_centres(cat, *(pr.sample_centres(table, model) if free else ph.CENTRE), limit=CLEARANCE)
        cat = lone_star(pr.plant(off_axis(cat), table, model, centre), table, model, centre)
        _cases[key] = (cat, table, centre)
    return _cases[key]


def off_axis(cat):
    """Stars 0 .. 5 -- the lone star (below) and predictive_helper's planted ones, two of them at |z| ~ 45 -- dominate the
    small ranges they sit in.  Next to an axis their term z cos(theta) (or z sin(theta)) is a small number that carries
    the absolute error z d(theta): relative to it, d(theta) / |cos(theta)|.  They take the positions of the first stars
    whose |cos theta| and |sin theta| about the nominal centre exceed 0.3."""
    cat = {k: (x.copy() if isinstance(x, np.ndarray) else x) for k, x in cat.items()}
    dx, dy = oracle.calc_xy_offset(cat["ra"], cat["dec"], *ph.CENTRE)
    first = max(pr.PLANTED.values()) + 1
    ok = np.flatnonzero((np.minimum(np.abs(dx), np.abs(dy)) > 0.3 * np.hypot(dx, dy)) & (np.arange(dx.size) >= first))
    for i in range(first):
        cat["ra"][i], cat["dec"][i] = cat["ra"][ok[i]], cat["dec"][ok[i]]
    return cat


def lone_star(cat, table, model, centre):
    """Star 0 is the only star of the N = 1 cells and of the singleton range, where the rule's scale (the sum of the
    absolute terms) is the one term itself.  A residual that cancels to |z| << 1 would carry the geometry's absolute
    error (d(theta) times v_max / sqrt(n) in z, which the oracle's float64 run shares only in part) relative
    to a term near zero, so no relative bound could hold.  Star 0 therefore gets a velocity 1.5 sigma above the model of
    the first sample (the samples scatter by ~0.1 sigma about it)."""
    cat = {k: (x.copy() if isinstance(x, np.ndarray) else x) for k, x in cat.items()}
    t0 = pr.star_terms(cat, table[0], model, centre)
    cat["v"][0] = t0["vlos"][0] + 1.5 * np.sqrt(cat["verr"][0] ** 2 + t0["sig"][0] ** 2)
    return cat


_refs = {}


def matrix_reference(model, free):
    """The Reference of a cell's 4099 stars and 257 samples, computed once.  A replicate is a function of (seed, sample,
    star) alone, so a layout over the first N stars and the first S samples reads its terms from the same arrays."""
    key = (model, free)
    if key not in _refs:
        cat, table, centre = matrix_case(model, free)
        _refs[key] = Reference(cat, table, model, centre)
    return _refs[key]


def check_matrix_cell(model, free, run, floor=1e-12):
    """The accuracy rule in every (N, S, layout) cell of one (model, centre mode); run(cat_n, table_s, centre, offs, order)
    gives the (S, R, 8, 2) fields under test.  Returns the largest excess seen."""
    cat, table, centre = matrix_case(model, free)
    ref = matrix_reference(model, free)
    worst = 0.0
    for n in MATRIX_N:
        for s in MATRIX_S:
            for kind in LAYOUTS:
                offs, order = layout(kind, n)
                got = run(pr.head(cat, n), table[:s], centre, offs, order)
                exact, np64, scale = ref.at(offs, order, s)
                ex = rule_excess(got, exact, np64, scale)
                worst = max(worst, max(ex.values()))
                for f, e in ex.items():
                    assert e <= floor, ((model, free, n, s, kind), f, e)
    print("model {0} free {1}: largest excess {2:.3e}".format(model, free, worst))
    return worst


# ---- calibration ------------------------------------------------------------------------------------------------
CAL_N, CAL_S, CAL_ANNULI = 4000, 256, 4
CAL_TRUTH = np.array([3.0, 8.0, 2.5, -1.5])              # v_sys, sigma_max, v_maxx, v_maxy (MODEL_CONST, fixed centre)


def annuli_of(cat, centre, n_annuli):
    """(range_offsets, order) of n_annuli annuli of equal star count in projected radius about `centre`."""
    dx, dy = oracle.calc_xy_offset(cat["ra"], cat["dec"], centre[0], centre[1])
    order = np.argsort(np.hypot(dx, dy), kind="stable").astype(np.int64)
    n = order.size
    return (np.arange(n_annuli + 1, dtype=np.int64) * n) // n_annuli, order


def calibration_case(kind, data_seed, row_seed=41):
    """4000 stars whose velocities are drawn from the constant-rotation model at CAL_TRUTH, altered by `kind`, and 256
    synthetic posterior rows: a narrow Gaussian ball about the generating parameters (no MCMC).
      model     as drawn                     outer     dispersion doubled in the outer half of the radii, the rows about
                                                       the pooled dispersion a constant fit of such data finds
      rotation  rotation amplitude 0.5 sigma in the data, rows with v_maxx = v_maxy = 0
      tails     5 % of the velocities redrawn with four times the dispersion"""
    cat = ph.model_catalog(CAL_N, 0, seed=11)
    cat = {k: (x.copy() if isinstance(x, np.ndarray) else x) for k, x in cat.items()}
    truth = CAL_TRUTH.copy()
    if kind == "rotation":
        truth[2], truth[3] = 0.5 * truth[1] / np.sqrt(2), -0.5 * truth[1] / np.sqrt(2)
    v_los = oracle.rotation_model(cat["ra"], cat["dec"], truth[0], truth[2], truth[3], ph.CENTRE[0], ph.CENTRE[1])
    rng = np.random.default_rng(data_seed)
    sigma = np.full(CAL_N, truth[1])
    offs, order = annuli_of(cat, ph.CENTRE, CAL_ANNULI)
    if kind == "outer":
        sigma[order[CAL_N // 2:]] *= 2.0
    if kind == "tails":
        sigma[rng.permutation(CAL_N)[:CAL_N // 20]] *= 4.0
    cat["v"] = v_los + np.sqrt(cat["verr"] ** 2 + sigma ** 2) * rng.normal(size=CAL_N)
    rows = np.random.default_rng(row_seed)
    centre_row = truth.copy()
    if kind == "outer":
        # what a constant-dispersion fit of these data finds: the pooled variance, (1 + 4) / 2 sigma^2
        centre_row[1] = np.sqrt(2.5) * truth[1]
    table = centre_row[None, :] + np.array([0.15, 0.1, 0.2, 0.2])[None, :] * rows.normal(size=(CAL_S, 4))
    if kind == "rotation":
        table[:, 2:] = 0.0
    return cat, np.ascontiguousarray(table), offs, order

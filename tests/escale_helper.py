"""Test helper: the error-scale models (device models 10 and 11; id 9 is unassigned, analysis/error_scale.py).  Test infrastructure only.

The reference.  The model at err_scale = s on the catalogue (v, verr) IS its base model (0 / 3) on the catalogue
(v, s verr): every reference here is the project's own oracle -- variant_helper.per_star / exact, grad_helper.per_star, on
oracle/lnprob_numpy.py -- evaluated on a copy of the catalogue whose error column is multiplied by that row's s, in the number
format asked for (in numpy.longdouble the product is formed in longdouble).  Rows with different s take one evaluation each.
The err_scale column of the gradient, d lnL_i / ds = (d l_i / d n_i) 2 s verr_i^2, is written out here from the oracle's
v_los and sigma_los; test_escale_cpu.py also checks it against a longdouble central difference of the value.

Live rows.  At s = 1 a launcher that never reads slot 19 of the walker row passes every comparison, so make_case draws s
log-uniform over [0.3, 3], different in every row, and ``guard`` demands that the reference on the live rows and on the same
rows with s = 1 differ by a median over the stars of >= 1e-6 (variant_helper.make_case has verr of 0.1 .. 0.6 and sigma_max of
0.5 .. 2 velocity scales: comparable sizes).

Column order (include/mcd.h): CONST_ESCALE v_sys, sigma_max, v_maxx, v_maxy, err_scale [, ra_center, dec_center];
PROFILE_ESCALE v_sys, sigma_max, a, v_maxx, v_maxy, r_peak, err_scale [, ra_center, dec_center]."""
import ctypes
import os
import subprocess

import numpy as np

import emul_helper as eh
import grad_bounds as gb
import grad_helper as gh
import variant_helper as vh
from oracle import lnprob_numpy as oracle

L = vh.L
CONST_ES, PROFILE_ES = 10, 11
SEED_OF = {CONST_ES: 9, PROFILE_ES: 10}             # arbitrary constants in make_case's seed, one per model (FREE_FLOOR_OTHER belongs to these rows)
MODELS = (CONST_ES, PROFILE_ES)
BASE = {CONST_ES: 0, PROFILE_ES: 3}
ES_COLUMN = {CONST_ES: 4, PROFILE_ES: 6}           # err_scale follows the cluster columns, in front of the centre
CELLS = [(m, f) for m in MODELS for f in (False, True)]
CELL_IDS = ["{0}-{1}".format(m, "free" if f else "fixed") for m, f in CELLS]
GUARD = 1e-6
S_RANGE = (0.3, 3.0)


def n_columns(model, free):
    return ES_COLUMN[model] + 1 + (2 if free else 0)


def column_names(model, free):
    names = gh.column_names(BASE[model], free)
    return names[:ES_COLUMN[model]] + ["err_scale"] + names[ES_COLUMN[model]:]


def split_rows(model, params):
    """(the rows without the err_scale column: the base model's rows, the err_scale column)."""
    p = np.atleast_2d(np.asarray(params))
    return np.ascontiguousarray(np.delete(p, ES_COLUMN[model], axis=1)), np.ascontiguousarray(p[:, ES_COLUMN[model]])


def with_scale(model, base_rows, s):
    base_rows = np.atleast_2d(base_rows)
    return np.ascontiguousarray(np.insert(base_rows, ES_COLUMN[model], s, axis=1))


def unit_rows(model, params):
    """The same rows with err_scale = 1."""
    p = np.array(np.atleast_2d(params), copy=True)
    p[:, ES_COLUMN[model]] = 1.0
    return np.ascontiguousarray(p)


def make_case(model, free, n, seed=None):
    """variant_helper.make_case of the base model with the err_scale column inserted: log-uniform over S_RANGE, every row
    its own."""
    case = vh.make_case(BASE[model], free, n, seed=seed)
    rng = np.random.default_rng(9000000 + 100000 * SEED_OF[model] + 50000 * int(free) + n if seed is None else seed + 1)
    w = case["params"].shape[0]
    s = np.exp(rng.uniform(np.log(S_RANGE[0]), np.log(S_RANGE[1]), w))
    assert len(np.unique(s)) == w
    case["params"] = with_scale(model, case["params"], s)
    case["base_model"] = BASE[model]
    case["model"] = model
    return case


def scaled_cat(cat, s, dtype=L):
    """The catalogue with its error column multiplied by s, formed in `dtype`."""
    out = {k: np.asarray(v).astype(dtype) for k, v in cat.items()}
    out["verr"] = out["verr"] * dtype(s)
    return out


def per_star(model, cat, row, centre, dtype=L):
    """The per-star log-likelihood of one row: variant_helper.per_star of the base model on the scaled catalogue."""
    base_row, s = split_rows(model, row)
    terms, none = vh.per_star(BASE[model], scaled_cat(cat, dtype(s[0]), dtype), base_row[0].astype(dtype), centre, dtype)
    assert none is None and terms.dtype == dtype
    return terms


def value(model, cat, row, centre, dtype=np.float64):
    """The reference's log-likelihood (oracle.faithful_*) of the base model on the scaled catalogue."""
    base_row, s = split_rows(model, row)
    return vh.value(BASE[model], scaled_cat(cat, dtype(s[0]), dtype), base_row[0], centre, dtype)


def exact(model, cat, row, centre):
    return value(model, cat, row, centre, L)


def star_moments(model, cat, row, centre, dtype=L):
    """(v_los, sigma_los^2, total variance) per star in `dtype`, from the oracle's model functions."""
    base_row, s = split_rows(model, row)
    c = {k: np.asarray(v).astype(dtype) for k, v in cat.items()}
    head, rc, dc, _ = vh._split(BASE[model], base_row[0], centre, dtype)
    if model == PROFILE_ES:
        v_los = oracle.model_rotation(c["ra"], c["dec"], head[0], head[3], head[4], head[5], rc, dc)
        sig = oracle.model_dispersion(c["ra"], c["dec"], head[1], head[2], rc, dc)
    else:
        v_los = oracle.rotation_model(c["ra"], c["dec"], head[0], head[2], head[3], rc, dc)
        sig = head[1] + 0 * c["v"]
    e2 = c["verr"] * c["verr"]
    return v_los, sig * sig, e2 * (dtype(s[0]) * dtype(s[0])) + sig * sig


def grad_terms(model, cat, row, centre, dtype=L):
    """(K, N) array of d lnL_i / d theta_k for one row (C-ABI column order): grad_helper.per_star of the base model on the
    scaled catalogue, and the err_scale row (d l / d n) 2 s verr^2 with d l / d n = ((v - v_los)^2 / n^2 - 1 / n) / 2."""
    base_row, s = split_rows(model, row)
    base = gh.per_star(BASE[model], scaled_cat(cat, dtype(s[0]), dtype), base_row[0], centre, dtype)
    v_los, _, norm = star_moments(model, cat, row, centre, dtype)
    c_v, c_e = np.asarray(cat["v"]).astype(dtype), np.asarray(cat["verr"]).astype(dtype)
    resid = c_v - v_los
    l_n = dtype(0.5) * (resid * resid / (norm * norm) - dtype(1) / norm)
    es = l_n * (dtype(2) * dtype(s[0]) * c_e * c_e)
    out = np.insert(base, ES_COLUMN[model], es, axis=0)
    assert out.dtype == dtype
    return out


def grad(model, cat, row, centre, dtype=L):
    terms = grad_terms(model, cat, row, centre, dtype)
    return terms.sum(axis=1), np.abs(terms).sum(axis=1)


_cache = {}


def reference(case, w):
    """{"g", "s", "err64", "value"} of walker row w of `case`, computed once (grad_bounds.reference's fields)."""
    key = (case["model"], case["free"], case["n"], w, case["params"][w].tobytes(), case["cat"]["v"].tobytes(),
           case["cat"]["verr"].tobytes(), case["cat"]["ra"].tobytes())
    if key not in _cache:
        args = (case["model"], case["cat"], case["params"][w], case["centre"])
        g80, s80 = grad(*args, L)
        g64, _ = grad(*args, np.float64)
        _cache[key] = {"g": g80, "s": s80, "err64": gh.col_err(g64, g80, s80), "value": exact(*args)}
    return _cache[key]


# (model, N) -> floor of the non-geometry columns (sigma_max, a, v_sys, err_scale), free centre, where it is above the base
# model's entry of grad_bounds.FREE_FLOOR.  grad_bounds' rule, max(1e-12, 2 x measured), with the figure measured by the host
# build of the BASE model's gradient (csrc/mcd_grad.h, models 0 and 3: no line of the error-scale code) on the catalogue whose
# error column is multiplied by the row's err_scale, over all 257 rows of make_case (`python tests/escale_floor_sweep.py`):
#     N = 1:    model 0 on CONST_ESCALE's rows: geometry 2.02e-11, other 2.43e-12;  model 3 on PROFILE_ESCALE's: 9.65e-12, 9.01e-13
#     N = 33:                              geometry 4.71e-13, other 7.91e-14;                         1.15e-12, 2.54e-13
#     N = 4099:                            geometry 1.50e-13, other 6.94e-14;                         3.48e-13, 6.23e-14
# (the error-scale models' own host build gives the same figures to three digits).  The cause is grad_bounds' own: the free-
# centre record's offsets carry ~1e-12 relative error, the residual d takes it, and with ONE star d l / d n = (d^2 / n^2 -
# 1 / n) / 2 has nothing but itself to be measured against; a scaled error column moves n, and with it how nearly the two
# terms cancel on a given row.  Every other cell stays inside the base model's floor.
FREE_FLOOR_OTHER = {(CONST_ES, 1): 4.9e-12, (PROFILE_ES, 1): 1.9e-12}


def floors(model, free, n):
    """grad_bounds.floors of the base model at the same cell (err_scale is no geometry column), raised by FREE_FLOOR_OTHER."""
    base = gb.floors(BASE[model], free, n)
    other = gb.FREE_FLOOR.get((BASE[model], n), (gb.FLOOR, gb.FLOOR))[1] if free and n <= gb.LARGE_N else gb.FLOOR
    out = np.insert(base, ES_COLUMN[model], other)
    if free and (model, n) in FREE_FLOOR_OTHER:
        geometry = np.insert(gb.is_geometry(BASE[model], free), ES_COLUMN[model], False)
        out = np.where(geometry, out, np.maximum(out, FREE_FLOOR_OTHER[(model, n)]))
    return out


def guard(case, rows, what):
    """The sensitivity guard of the module docstring on the first and the last of `rows` (cells with N >= 33)."""
    if case["n"] < 33:
        return
    model, cat, centre = case["model"], case["cat"], case["centre"]
    rows = np.atleast_2d(rows)
    dead = unit_rows(model, rows)
    for r in sorted({0, len(rows) - 1}):
        moved = np.abs(per_star(model, cat, rows[r], centre) - per_star(model, cat, dead[r], centre))
        med = float(np.median(moved))
        print("guard", what, (model, case["free"], case["n"]), "row", r, "err_scale %.3f" % rows[r][ES_COLUMN[model]],
              "median |l(s) - l(1)| %.2e" % med)
        assert med >= GUARD, (what, model, case["free"], case["n"], r, med)


def term_err(got, want):
    """|got - want| on max(|want|, 1) (the bound of the per-star tests: 1e-12)."""
    got = np.asarray(got).astype(L)
    return float(np.max(np.abs(got - want) / np.maximum(np.abs(want), L(1)))) if got.size else 0.0


def open_catalog(native, ctx, case, **more):
    c = case["cat"]
    return native.Catalog(ctx, c["ra"], c["dec"], c["v"], c["verr"], model=case["model"], centre=case["centre"], **more)


def chain_rows(case, s, seed=3):
    """`s` rows in a tight ball about row 0 of the case (a posterior-like sample table) with err_scale spread over S_RANGE
    row by row: the live column is the point of every table here."""
    rng = np.random.default_rng(seed)
    p0 = case["params"][0]
    scale = np.abs(p0) * 0.02 + 1e-4 * case["scale"]
    if case["free"]:
        k = ES_COLUMN[case["model"]] + 1
        scale[k:k + 2] = 2e-4
    rows = p0 + rng.normal(size=(s, p0.size)) * scale
    rows[:, ES_COLUMN[case["model"]]] = np.exp(rng.uniform(np.log(S_RANGE[0]), np.log(S_RANGE[1]), s))
    return np.ascontiguousarray(rows)


# ---- host build (tests/emul/escale_emul.cpp) ----------------------------------------------------------------------------
SRC = os.path.join(eh.ROOT, "tests", "emul", "escale_emul.cpp")
OUT = os.path.join(eh.ROOT, "tests", "emul", "libmcd_escale_emul.so")
_lib = None
P, I64, I, D = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int, ctypes.c_double


def lib():
    global _lib
    if _lib is None:
        deps = [SRC] + [os.path.join(eh.INC, h) for h in ("mcd_grad.h", "mcd_math.h", "mcd_exp_table.h", "mcd_dispatch.h",
                                                          "mcd_guard.h", "mcd_prep.h")]
        if not os.path.exists(OUT) or any(os.path.getmtime(d) > os.path.getmtime(OUT) for d in deps):
            subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-I", eh.INC, SRC,
                            "-o", OUT], check=True)
        _lib = ctypes.CDLL(OUT)
        _lib.escale_emul_dispatch.argtypes = [I, I, I, I, P]
        _lib.escale_emul_walkers.argtypes = [I, I, I, I64, P, P]
        _lib.escale_emul_walkers.restype = None
        _lib.escale_emul_loglike.argtypes = [I, I, I, I64, P, P, I64, I64, P]
        _lib.escale_emul_terms.argtypes = [I, I, I, I64, P, P, P, P, P]
        _lib.escale_emul_grad.argtypes = [I, I, I64, P, P, P, I64, I64, P]
        _lib.escale_emul_level.argtypes = [I, I, I64, P, P, P, P, P, P, P, D, D, I, P, I64, P]
    return _lib


def record_model(model):
    return BASE.get(model, eh.RECORD_MODEL.get(model, model))


def pack_records(cat, model, centre):
    """The base model's records: the error-scale models read the same fields."""
    return eh.pack_records(cat, record_model(model), centre)


def walkers(params, model, free):
    """walker_constants itself (csrc/mcd_prep.h, host pass) on every row: (W, KD)."""
    params = np.ascontiguousarray(np.atleast_2d(params), dtype=np.float64)
    out = np.full((params.shape[0], lib().escale_emul_kd()), np.nan)
    lib().escale_emul_walkers(model, int(free), params.shape[1], params.shape[0], params.ctypes.data, out.ctypes.data)
    return out


def emul_value(model, cat, params, centre, fast, chunk_len=96):
    params = np.ascontiguousarray(np.atleast_2d(params), dtype=np.float64)
    rec, wp = pack_records(cat, model, centre), walkers(params, model, centre is None)
    assert rec.shape[1] == lib().escale_emul_record_doubles(model, int(centre is None))
    out = np.empty(params.shape[0])
    assert lib().escale_emul_loglike(model, int(centre is None), int(fast), rec.shape[0], rec.ctypes.data, wp.ctypes.data,
                                     params.shape[0], chunk_len, out.ctypes.data) == 0
    return out


def emul_terms(model, cat, row, centre, fast):
    """(d, n, l) per star of one row: star_d_n plain (fast = 0) or FASTMATH (1), and gauss_lnl of them."""
    rec, wp = pack_records(cat, model, centre), walkers(row, model, centre is None)
    n = rec.shape[0]
    d, nn, l = np.empty(n), np.empty(n), np.empty(n)
    assert lib().escale_emul_terms(model, int(centre is None), int(fast), n, rec.ctypes.data, wp.ctypes.data, d.ctypes.data,
                                   nn.ctypes.data, l.ctypes.data) == 0
    return d, nn, l


def emul_grad(model, cat, params, centre, chunk_len=96):
    params = np.ascontiguousarray(np.atleast_2d(params), dtype=np.float64)
    free = centre is None
    assert params.shape[1] == lib().escale_emul_columns(model, int(free))
    rec, wp = pack_records(cat, model, centre), walkers(params, model, free)
    out = np.empty((params.shape[0], 1 + params.shape[1]))
    assert lib().escale_emul_grad(model, int(free), rec.shape[0], rec.ctypes.data, wp.ctypes.data, params.ctypes.data,
                                  params.shape[0], chunk_len, out.ctypes.data) == 0
    return out[:, 0], out[:, 1:]


def level(model, cat, params, centre, ranges=None):
    """csrc/mcd_guard.h: fast_level of a table with the statistics mcd_catalog_create gathers."""
    params = np.ascontiguousarray(np.atleast_2d(params), dtype=np.float64)
    cols = [np.ascontiguousarray(cat[k], dtype=np.float64) if k in cat else None
            for k in ("ra", "dec", "v", "verr", "lnlike_bg", "pmember", "density")]
    rc, dc = (0.0, 0.0) if centre is None else centre
    out = np.zeros(2)
    lv = lib().escale_emul_level(model, int(centre is None), len(cat["v"]), *[a.ctypes.data if a is not None else None for a in cols],
                                 rc, dc, params.shape[1], params.ctypes.data, params.shape[0], out.ctypes.data)
    if ranges is not None:
        ranges[:] = out
    return lv

"""Test helper: CPU build of the per-star arithmetic of mcd_psis_loo_expect (tests/emul/loo_expect_emul.cpp + csrc/mcd_psis.h
+ csrc/mcd_predictive.h) and the NumPy oracle it and the device are checked against: the PSIS weights restated from
psis_helper (tail_len, gpdfit, the steps of psis_star) and E_loo[x] = sum_s w~_s x_s.  Test infrastructure only.

The accuracy rule, per expectation and per star:
    |got - want| <= max(1e-11 scale, 10 noise)
1e-11 is the project's elpd tolerance (psis_helper.assert_matches); scale = max_s |x_s - mean_s x| (1 for pit / pit_mix);
noise = the oracle's own movement when every lnL_is moves by one ulp (psis_helper.k_noise's construction)."""
import ctypes
import os
import subprocess

import numpy as np

import emul_helper as emul
import posterior_helper as ph
import predictive_helper as pr
import psis_helper as ps

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "emul", "loo_expect_emul.cpp")
INC = os.path.join(ROOT, "mcmc_dynamics_amd", "csrc")
OUT = os.path.join(ROOT, "tests", "emul", "libloo_expect_emul.so")
PRED = ("pit", "z", "vlos", "sigma")                 # the rows after lnL, in the order of MCD_LOOX_*
TERM_KEY = {"pit": "pit", "z": "z", "vlos": "vlos", "sigma": "sig", "pit_mix": "pit_mix"}     # predictive_helper's names
REL_TOL = 1e-11
_lib = None


def lib():
    global _lib
    if _lib is None:
        deps = [SRC] + [os.path.join(INC, f) for f in ("mcd_psis.h", "mcd_predictive.h", "mcd_posterior.h", "mcd_math.h",
                                                       "mcd_exp_table.h", "mcd_dispatch.h")]
        if not os.path.exists(OUT) or any(os.path.getmtime(d) > os.path.getmtime(OUT) for d in deps):
            subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-I", INC, SRC,
                            "-o", OUT], check=True)
        lb = ctypes.CDLL(OUT)
        lb.emul_loo_expect.argtypes = [ctypes.c_int64, ctypes.c_int64, ctypes.c_void_p, ctypes.c_double, ctypes.c_int,
                                       ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p]
        lb.emul_loo_expect_model.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int64,
                                             ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_double, ctypes.c_void_p]
        lb.emul_psis_tile_stars_rows.argtypes = [ctypes.c_int64] * 5
        lb.emul_psis_tile_stars_rows.restype = ctypes.c_int64
        _lib = lb
    return _lib


def emul_expect(lnl, x=None, func=None, r_eff=1.0):
    """Emulated per-star routine: lnl (n, S), x (n, R, S) rows per star, func (S, Q) -> dict pareto_k, n_eff (n,),
    rows (n, R), func (n, Q)."""
    lnl = np.ascontiguousarray(lnl, dtype=np.float64)
    n, S = lnl.shape
    x = np.zeros((n, 0, S)) if x is None else np.ascontiguousarray(x, dtype=np.float64)
    func = np.zeros((S, 0)) if func is None else np.ascontiguousarray(func, dtype=np.float64)
    R, Q = x.shape[1], func.shape[1]
    assert x.shape == (n, R, S) and func.shape == (S, Q)
    out = np.full((2 + R + Q, n), np.nan)
    assert lib().emul_loo_expect(n, S, lnl.ctypes.data, float(r_eff), R, x.ctypes.data, Q, func.ctypes.data,
                                 out.ctypes.data) == 0
    return {"pareto_k": out[0], "n_eff": out[1], "rows": out[2:2 + R].T.copy(), "func": out[2 + R:].T.copy()}


def emul_model(cat, table, model, centre, mix=False, f32=False, r_eff=1.0):
    """Emulated mcd_psis_loo_expect from the catalogue: dict pareto_k, n_eff, pit, z, vlos, sigma (and pit_mix)."""
    rec = emul.pack_records(cat, model, centre)
    wp = emul.pack_walkers(table, model, centre is None)
    n = rec.shape[0]
    out = np.full((2 + 4 + int(mix), n), np.nan)
    assert lib().emul_loo_expect_model(model, int(centre is None), int(mix), int(f32), n, rec.ctypes.data, wp.ctypes.data,
                                       wp.shape[0], float(r_eff), out.ctypes.data) == 0
    d = {"pareto_k": out[0], "n_eff": out[1]}
    d.update({k: out[2 + i] for i, k in enumerate(PRED)})
    if mix:
        d["pit_mix"] = out[6]
    return d


def tile_stars_rows(n, S, rows, fixed, budget):
    return int(lib().emul_psis_tile_stars_rows(n, S, rows, fixed, budget))


# ---- NumPy oracle ------------------------------------------------------------------------------------------------
def star_weights(lnl, r_eff=1.0):
    """One star's normalised PSIS weights w~ (S,), its truncated log weights and k^: the steps of psis_helper.psis_star."""
    lnl = np.asarray(lnl, dtype=np.float64)
    S = lnl.size
    M = ps.tail_len(S, r_eff)
    r = -lnl
    lw = r - r.max()
    k_hat = np.inf
    if M >= 5:
        order = np.argsort(lw, kind="stable")                        # ascending, ties by sample index
        tail = order[S - M:]
        cutoff = lw[order[S - M - 1]]
        vals = lw[tail]
        if vals.max() - vals.min() < np.finfo(np.float64).eps / 100.0:
            k_hat = -np.inf
        else:
            k_hat, sigma = ps.gpdfit(np.exp(vals) - np.exp(cutoff))
            if np.isfinite(k_hat):
                p = (np.arange(1, M + 1) - 0.5) / M
                q = -sigma * np.log1p(-p) if k_hat == 0.0 else sigma * np.expm1(-k_hat * np.log1p(-p)) / k_hat
                lw = lw.copy()
                lw[tail] = np.log(q + np.exp(cutoff))
    lw = np.minimum(lw, 0.0)
    e = np.exp(lw - lw.max())
    return e / e.sum(), lw, k_hat


def oracle_expect(lnl, x=None, func=None, r_eff=1.0):
    """Oracle over an (n, S) matrix of lnL: dict pareto_k, n_eff, elpd_loo (n,), rows (n, R) for x (n, R, S), func (n, Q)
    for func (S, Q)."""
    lnl = np.atleast_2d(np.asarray(lnl, dtype=np.float64))
    n, S = lnl.shape
    x = np.zeros((n, 0, S)) if x is None else np.asarray(x, dtype=np.float64)
    func = np.zeros((S, 0)) if func is None else np.asarray(func, dtype=np.float64)
    out = {"pareto_k": np.empty(n), "n_eff": np.empty(n), "elpd_loo": np.empty(n), "rows": np.empty((n, x.shape[1])),
           "func": np.empty((n, func.shape[1]))}
    for i in range(n):
        w, lw, k = star_weights(lnl[i], r_eff)
        out["pareto_k"][i] = k
        out["n_eff"][i] = r_eff / np.sum(w * w)
        out["elpd_loo"][i] = ps._lse(lw + lnl[i]) - ps._lse(lw)
        out["rows"][i] = x[i] @ w
        out["func"][i] = w @ func
    return out


def moved(lnl, seed=0):
    """Every lnL_is moved by one ulp, up or down (psis_helper.k_noise)."""
    lnl = np.asarray(lnl, dtype=np.float64)
    sign = np.where(np.random.default_rng(seed).uniform(size=lnl.shape) < 0.5, -1.0, 1.0)
    return lnl + sign * np.spacing(lnl)


def noise(lnl, want, x=None, func=None, r_eff=1.0):
    """Per expectation, how far the oracle itself moves when every lnL_is moves by one ulp: dict rows (n, R), func (n, Q)."""
    other = oracle_expect(moved(lnl), x, func, r_eff)
    out = {}
    for key in ("rows", "func"):
        with np.errstate(invalid="ignore"):
            d = np.abs(other[key] - want[key])
        out[key] = np.where(np.isfinite(d), d, 0.0)
    return out


def spread(x, axis):
    """scale of the rule: max_s |x_s - mean_s x|."""
    x = np.asarray(x, dtype=np.float64)
    return np.max(np.abs(x - x.mean(axis=axis, keepdims=True)), axis=axis)


def rule_ok(got, want, scale, nz, what=""):
    """The accuracy rule; prints the worst ratio of error to allowance before it asserts."""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    tol = np.maximum(REL_TOL * np.broadcast_to(scale, want.shape), 10.0 * np.broadcast_to(nz, want.shape))
    err = np.abs(got - want)
    bad = ~(err <= tol)
    with np.errstate(divide="ignore", invalid="ignore"):
        worst = float(np.max(np.where(tol > 0, err / tol, np.where(err > 0, np.inf, 0.0)))) if err.size else 0.0
    print("{0}: worst |error| / allowance {1:.3e}, max |error| {2:.3e}".format(what, worst,
                                                                                float(err.max()) if err.size else 0.0))
    assert not bad.any(), (what, int(bad.sum()), float(err[bad].max()), float(tol[bad].min()))


def check_expect(got, lnl, x=None, func=None, r_eff=1.0, unit_rows=(), what=""):
    """`got` (emul_expect's layout) against the oracle by the rule; rows listed in ``unit_rows`` have scale 1 (pit)."""
    want = oracle_expect(lnl, x, func, r_eff)
    nz = noise(lnl, want, x, func, r_eff)
    if x is not None and np.asarray(x).shape[1]:
        scale = spread(x, axis=2)
        for r in unit_rows:
            scale[:, r] = 1.0
        rule_ok(got["rows"], want["rows"], scale, nz["rows"], what + " rows")
    if func is not None and np.asarray(func).shape[1]:
        rule_ok(got["func"], want["func"], spread(func, axis=0)[None, :], nz["func"], what + " func")
    k, wk = np.asarray(got["pareto_k"]), want["pareto_k"]
    fin = np.isfinite(wk)
    assert np.array_equal(np.isfinite(k), fin) and np.array_equal(k[~fin], wk[~fin])
    return want


# ---- model cases ------------------------------------------------------------------------------------------------
def term_rows(cat, table, model, centre, mix=False):
    """The oracle's (n, R, S) rows of predictive_helper.sample_terms in float64, in the order pit, z, vlos, sigma
    (, pit_mix)."""
    t = pr.sample_terms(cat, table, model, centre, np.float64)
    keys = list(PRED) + (["pit_mix"] if mix else [])
    return np.ascontiguousarray(np.stack([t[TERM_KEY[k]].T for k in keys], axis=1)), keys


def lnl_rows(cat, table, model, centre):
    """The oracle's lnL_is, (n, S) (posterior_helper.star_terms)."""
    return np.ascontiguousarray(np.array([ph.star_terms(cat, row, model, centre)[0] for row in np.atleast_2d(table)]).T)


def metropolis(cat, n_samples, seed, thin=4, n_burn=300):
    """Seeded random-walk Metropolis on the oracle's lnL of the constant-rotation model with a fixed centre (flat prior,
    sigma_max > 0): n_samples rows (v_sys, sigma_max, v_maxx, v_maxy), every ``thin``-th step after ``n_burn``.  The
    proposal is 2.4 / sqrt(4) of the parameters' approximate posterior spreads for n stars of total dispersion s:
    s / sqrt(n) for v_sys, s / sqrt(2 n) for sigma_max, s sqrt(2 / n) for the two amplitudes."""
    rng = np.random.default_rng(seed)
    n = cat["v"].size
    s = float(np.std(cat["v"]))
    step = 1.2 * np.array([s / np.sqrt(n), s / np.sqrt(2.0 * n), s * np.sqrt(2.0 / n), s * np.sqrt(2.0 / n)])

    def lnl(row):
        return float(np.sum(ph.star_terms(cat, row, 0, ph.CENTRE)[0])) if row[1] > 0.0 else -np.inf
    cur = np.array([float(np.mean(cat["v"])), s, 0.0, 0.0])
    l_cur = lnl(cur)
    out = np.empty((n_samples, 4))
    for it in range(n_burn + n_samples * thin):
        prop = cur + step * rng.normal(size=4)
        l_prop = lnl(prop)
        if np.log(rng.uniform()) < l_prop - l_cur:
            cur, l_cur = prop, l_prop
        if it >= n_burn and (it - n_burn) % thin == thin - 1:
            out[(it - n_burn) // thin] = cur
    return out


PLANTED_STAR = 7
SIGMA_MAX_COLUMN = 1
_planted = {}


def planted_case():
    """calibration_case(n=300) with star 7 moved to +4 sigma of the true model, 1 024 Metropolis samples: (catalogue,
    table (S, 4), lnL (n, S), standardised parameter columns (S, 4), their mean and std)."""
    if not _planted:
        cat, truth = pr.calibration_case(n=300)
        t0 = pr.star_terms(cat, truth, 0, ph.CENTRE)
        i = PLANTED_STAR
        cat["v"][i] = t0["vlos"][i] + 4.0 * np.sqrt(cat["verr"][i] ** 2 + t0["sig"][i] ** 2)
        table = metropolis(cat, 1024, seed=20240612)
        mean, std = table.mean(axis=0), table.std(axis=0)
        _planted["case"] = (cat, table, lnl_rows(cat, table, 0, ph.CENTRE), (table - mean) / std, mean, std)
    return _planted["case"]


def planted_property(shift):
    """Star 7 has the most negative sigma_max shift, at least twice as large as any other |shift| of any star and
    parameter; returns (its shift, the largest other |shift|)."""
    shift = np.asarray(shift)
    col = shift[:, SIGMA_MAX_COLUMN]
    other = np.abs(shift).copy()
    other[PLANTED_STAR, SIGMA_MAX_COLUMN] = 0.0
    print("planted star: sigma_max shift {0:.3f}, largest other |shift| {1:.3f}".format(col[PLANTED_STAR], other.max()))
    assert int(np.argmin(col)) == PLANTED_STAR and col[PLANTED_STAR] < 0.0
    assert -col[PLANTED_STAR] >= 2.0 * other.max()
    return float(col[PLANTED_STAR]), float(other.max())


CHI2_9_Q999 = 27.88                                     # 0.999 quantile of chi^2 with 9 degrees of freedom


def small_sample_sets(n_sets=40, n_stars=12, n_samples=512):
    """Data sets of n_stars stars drawn from the constant-rotation model itself, each with its Metropolis samples: list
    of (lnL (n, S), pit (n, S))."""
    sets = []
    for j in range(n_sets):
        cat, _ = pr.calibration_case(seed=pr.CALIBRATION_SEED + 1 + j, n=n_stars)
        table = metropolis(cat, n_samples, seed=977 + j)
        terms = pr.sample_terms(cat, table, 0, ph.CENTRE, np.float64)
        sets.append((lnl_rows(cat, table, 0, ph.CENTRE), np.ascontiguousarray(terms["pit"].T)))
    return sets

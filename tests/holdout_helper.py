"""Test helper of the exact leave-out refits: the CPU build of the hold-out rules (tests/emul/holdout_emul.cpp +
csrc/mcd_holdout.h, csrc/mcd_chunks.h) and the closed-form case the end-to-end tests share.

Closed form: ``ConstantFit`` on 200 synthetic stars without background, v_maxx = v_maxy = 0 and sigma_max = 10 km/s fixed,
only v_sys free in a wide box.  With n_j = verr_j^2 + sigma^2 the likelihood is exactly Gaussian in v_sys, so that the
posterior without a set of stars is N(mu, 1 / Lambda), Lambda = sum_{j not in set} 1 / n_j, mu = sum_{j not in set}
(v_j / n_j) / Lambda, and a held-out star's predictive density is N(v_i; mu, n_i + 1 / Lambda).

Test infrastructure only."""
import ctypes
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "emul", "holdout_emul.cpp")
INC = os.path.join(ROOT, "mcmc_dynamics_amd", "csrc")
OUT = os.path.join(ROOT, "tests", "emul", "libholdout_emul.so")
_lib = None
L = np.longdouble


def lib():
    global _lib
    if _lib is None:
        deps = [SRC] + [os.path.join(INC, h) for h in ("mcd_holdout.h", "mcd_chunks.h", "mcd_math.h")]
        if not os.path.exists(OUT) or any(os.path.getmtime(d) > os.path.getmtime(OUT) for d in deps):
            subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-Wno-unknown-pragmas", "-I", INC,
                            SRC, "-o", OUT], check=True)
        lb = ctypes.CDLL(OUT)
        lb.emul_holdout_offsets_error.argtypes = [ctypes.c_int64, ctypes.c_void_p, ctypes.c_int64, ctypes.c_char_p, ctypes.c_int]
        lb.emul_holdout_ranges.argtypes = [ctypes.c_int64, ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p]
        lb.emul_holdout_ranges.restype = ctypes.c_int64
        lb.emul_holdout_combine.argtypes = [ctypes.c_void_p, ctypes.c_int64, ctypes.c_int64, ctypes.c_int64, ctypes.c_void_p,
                                            ctypes.c_void_p]
        lb.emul_holdout_combine.restype = None
        lb.emul_holdout_plan.argtypes = [ctypes.c_int64, ctypes.c_void_p, ctypes.c_int64, ctypes.c_int64, ctypes.c_int64] + \
            [ctypes.c_void_p] * 5
        lb.emul_holdout_plan.restype = ctypes.c_int64
        lb.emul_holdout_max_rows.restype = ctypes.c_int64
        lb.emul_holdout_scratch_bytes.restype = ctypes.c_int64
        _lib = lb
    return _lib


def offsets_error(offsets, n_stars):
    """None for valid offsets, else the library's message."""
    offs = np.ascontiguousarray(offsets, dtype=np.int64)
    msg = ctypes.create_string_buffer(256)
    bad = lib().emul_holdout_offsets_error(offs.size - 1, offs.ctypes.data, int(n_stars), msg, 256)
    return msg.value.decode() if bad else None


def ranges(offsets, n_stars):
    offs = np.ascontiguousarray(offsets, dtype=np.int64)
    out = np.empty(offs.size + 1, dtype=np.int64)
    r = lib().emul_holdout_ranges(offs.size - 1, offs.ctypes.data, int(n_stars), out.ctypes.data)
    return out[:r + 1]


def combine(m, n_walkers):
    """m (R, rows) range sums -> (train, test) (rows,) by csrc/mcd_holdout.h: holdout_combine."""
    m = np.ascontiguousarray(m, dtype=np.float64)
    train, test = np.empty(m.shape[1]), np.empty(m.shape[1])
    lib().emul_holdout_combine(m.ctypes.data, m.shape[0], m.shape[1], int(n_walkers), train.ctypes.data, test.ctypes.data)
    return train, test


def plan(offsets, n_stars, n_rows):
    """The chunk table mcd_holdout_loglike plans: dict of begin, count, range per chunk, offsets per range, max, len."""
    offs = np.ascontiguousarray(offsets, dtype=np.int64)
    cap = int(n_stars) // 8 + 8 * offs.size + 64
    begin, count, rng = np.empty(cap, np.int64), np.empty(cap, np.int32), np.empty(cap, np.int32)
    offsets_out, info = np.zeros(offs.size + 1, np.int64), np.zeros(2, np.int64)
    nc = lib().emul_holdout_plan(offs.size - 1, offs.ctypes.data, int(n_stars), int(n_rows), cap, begin.ctypes.data,
                                 count.ctypes.data, rng.ctypes.data, offsets_out.ctypes.data, info.ctypes.data)
    assert nc >= 0, "chunk capacity"
    r = ranges(offs, n_stars).size - 1
    return {"begin": begin[:nc], "count": count[:nc], "range": rng[:nc], "offsets": offsets_out[:r + 1],
            "max_chunks_per_range": int(info[0]), "len": int(info[1])}


def sets_of_sizes(sizes, n):
    """Offsets (E + 1,) of consecutive sets of the given sizes, each capped to what is left of n stars."""
    offs = [0]
    for s in sizes:
        offs.append(min(n, offs[-1] + s))
    return np.array(offs, dtype=np.int64)


# ---- the closed-form case -------------------------------------------------------------------------------------------------
N_STARS, SIGMA, V_SYS = 200, 10.0, 3.0
PLANTED = {11: 6.0, 57: -5.0, 102: 4.5, 148: -4.0, 190: 3.5}       # star -> offset from v_sys in units of sqrt(n_i)
# The run the GPU test makes, sized by tests/test_holdout_cpu.py::test_closed_form_harness_sizes_the_run
N_WALKERS, N_STEPS, N_BURN = 64, 600, 200


def closed_form_columns():
    from mcmc_dynamics_amd import synthetic
    c = synthetic.make_catalog(N_STARS, config=2, background=False)
    rng = np.random.default_rng(20261019)
    verr = np.asarray(c["verr"], dtype=np.float64)
    n = verr ** 2 + SIGMA ** 2
    v = V_SYS + np.sqrt(n) * rng.normal(size=N_STARS)
    for i, z in PLANTED.items():
        v[i] = V_SYS + z * np.sqrt(n[i])
    return {"ra": np.asarray(c["ra"], dtype=np.float64), "dec": np.asarray(c["dec"], dtype=np.float64), "v": v, "verr": verr}


def closed_form_fit(cols, **kwargs):
    """ConstantFit with only v_sys free (in a wide box)."""
    from mcmc_dynamics_amd import DataReader, synthetic
    from mcmc_dynamics_amd.analysis import ConstantFit
    fit = ConstantFit(DataReader(dict(cols)), **kwargs)
    fit.parameters["v_sys"].set(min=-1000.0, max=1000.0)
    fit.parameters["sigma_max"].set(value=SIGMA, fixed=True)
    fit.parameters["v_maxx"].set(value=0.0, fixed=True)
    fit.parameters["v_maxy"].set(value=0.0, fixed=True)
    fit.parameters["ra_center"].set(value=synthetic.CENTER_RA_DEG, fixed=True)
    fit.parameters["dec_center"].set(value=synthetic.CENTER_DEC_DEG, fixed=True)
    return fit


def _norm_lnpdf(x, mean, var):
    return -0.5 * (np.log(2 * L(np.pi) * var) + (x - mean) ** 2 / var)


def posterior_without(cols, held):
    """(mu, 1 / Lambda) of v_sys without the stars ``held``, in long double."""
    v, n = cols["v"].astype(L), cols["verr"].astype(L) ** 2 + L(SIGMA) ** 2
    keep = np.ones(v.size, dtype=bool)
    keep[np.asarray(held, dtype=np.intp)] = False
    lam = np.sum(1 / n[keep])
    return np.sum(v[keep] / n[keep]) / lam, 1 / lam


def exact_elpd(cols, sets):
    """(n_data,) long double: log N(v_i; mu_-set, n_i + 1 / Lambda_-set) for the stars of the sets, NaN elsewhere."""
    v, n = cols["v"].astype(L), cols["verr"].astype(L) ** 2 + L(SIGMA) ** 2
    out = np.full(v.size, np.nan, dtype=L)
    for s in sets:
        s = np.asarray(s, dtype=np.intp)
        mu, var = posterior_without(cols, s)
        out[s] = _norm_lnpdf(v[s], mu, n[s] + var)
    return out


def exact_full_lppd(cols):
    """(n_data,) long double: every star's log predictive density under the posterior of ALL stars."""
    v, n = cols["v"].astype(L), cols["verr"].astype(L) ** 2 + L(SIGMA) ** 2
    mu, var = posterior_without(cols, [])
    return _norm_lnpdf(v, mu, n + var)


def numpy_log_prob(cols, sets):
    """values (E, W, 1) -> (E, W): the log-likelihood of all stars but set e (what holdout_loglike's ``train`` is), NumPy."""
    v, n = cols["v"], cols["verr"] ** 2 + SIGMA ** 2
    sets = [np.asarray(s, dtype=np.intp) for s in sets]

    def term(theta, idx):                                              # (W,), stars idx -> (W,)
        return np.sum(-0.5 * (np.log(2 * np.pi * n[idx]) + (v[idx][None, :] - theta[:, None]) ** 2 / n[idx]), axis=1)

    def fn(values):
        values = np.asarray(values, dtype=np.float64)
        out = np.empty(values.shape[:2])
        everything = np.arange(v.size)
        for e, s in enumerate(sets):
            theta = values[e, :, 0]
            out[e] = term(theta, everything) - term(theta, s)
        return out
    return fn


def walker_estimates(chain_e, cols, star):
    """chain_e (W, steps) of v_sys -> (pooled lppd, standard error) of one star: the spread of the per-walker estimates
    log mean_s exp(l_i) (batch means over walkers, as tests/test_gpu_hmc.py: walker_means)."""
    v, n = cols["v"][star], cols["verr"][star] ** 2 + SIGMA ** 2
    l = -0.5 * (np.log(2 * np.pi * n) + (v - chain_e) ** 2 / n)
    mx = l.max()
    per_walker = mx + np.log(np.mean(np.exp(l - mx), axis=1))
    pooled = mx + np.log(np.mean(np.exp(l - mx)))
    return pooled, per_walker.std(ddof=1) / np.sqrt(chain_e.shape[0])

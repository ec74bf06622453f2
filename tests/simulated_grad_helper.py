"""Test helper of the MAP fits of simulated catalogues (tests/test_simulated_grad_cpu.py, tests/test_gpu_simulated_grad.py).
Test infrastructure only.

  * the CPU build of the value-and-gradient loop (tests/emul/simulated_grad_emul.cpp: csrc/mcd_simulated_grad.h on top of
    csrc/mcd_grad.h and csrc/mcd_simulated.h) and of the plain gradient loop it must reproduce on the observed velocities
    (csrc/mcd_grad.h: chunk_grad);
  * the matrix: simulated_helper.make_case, models 0 .. 8 x {fixed, free} x N in {1, 33, 1027}, a set of E = 3 simulations
    drawn by the host build of the velocity rule at the first three rows of the case, rows mapped by
    simulated_helper.row_sims;
  * the reference: grad_helper.per_star (models 0 .. 6) or double_helper.grad_terms (7, 8) in numpy.longdouble on
    simulated_helper.substituted(case, v_e) -- restatements that share no expression with the kernel -- and the project's
    rule per column,
        |got - exact| / S_k <= 2 err_np64 + floor,      S_k = sum_i |dl_i/dtheta_k|,
    err_np64 the float64 run of the same restatement against its longdouble run; values: 1e-12 on max(|sum l|, N);
  * the floors (SIM_FLOOR below);
  * NumPy stand-ins for the Runner's device calls on linear-Gaussian catalogues whose maxima are known in closed form: the
    stub of the host-logic tests and the reference of the end-to-end GPU run.

SIM_FLOOR.  grad_bounds' tables were measured on variant_helper's field and on the observed velocities; this matrix has
simulated_helper's field (stretched twenty-fold: the free-centre cancellation of grad_bounds' docstring is twenty times
weaker) and velocities drawn from the model, so the floors are measured anew with THIS host build: per (model, centre, N)
cell the largest err - 2 err_np64 over all 257 rows that the GPU matrix can reach and every column
(`python tests/simulated_grad_floor_sweep.py` prints the table).  floor = max(1e-12, 2 x measured), rounded up to two digits.
Measured (largest err - 2 err_np64), N = 1, models 0 .. 8:
    fixed centre   1.03e-14  4.03e-15  4.95e-15  4.25e-14  2.10e-13  3.40e-14  7.84e-13  4.31e-13  2.63e-13
    free centre    1.44e-12  1.29e-13  4.19e-13  2.08e-12  3.21e-12  6.87e-13  1.01e-11  5.65e-13  3.62e-12
At N = 33 every cell is below 5.6e-14 and at N = 1027 below 2.1e-14 (fixed centre: below 1.4e-15 at both), so only N = 1
has entries.  With one star S_k is that star's own |dl/dtheta_k|: a derivative that nearly cancels inside the term has
nothing to be measured against.  The free-centre cells add the cause grad_bounds names, the record's offsets being
differences of O(0.4) products.  The one fixed-centre entry, model 6 (PROFILE_BGFIXED), is supposed to be the mixture's
responsibility of a star far in one component's tail, whose exponent lc - lb carries |lc - lb| ulps in any float64
formulation while err_np64 of that one star happens to be small; it was not taken apart further."""
import ctypes
import os
import subprocess

import numpy as np

import double_helper as dh
import emul_helper as eh
import grad_helper as gh
import holdout_helper as hh
import simulated_helper as sh
import variant_helper as vh
from oracle import lnprob_numpy as oracle

SRC = os.path.join(eh.ROOT, "tests", "emul", "simulated_grad_emul.cpp")
OUT = os.path.join(eh.ROOT, "tests", "emul", "libmcd_simulated_grad_emul.so")
L = vh.L
N_SIMS, STARS, ROWS = 3, (1, 33, 1027), (1, 65, 257)
CELLS = [(m, f) for m in sh.MODELS for f in (False, True)]
FLOOR = 1e-12
# (model, free centre, N) -> floor, where it is above FLOOR (measured: see the module docstring and sweep())
SIM_FLOOR = {(0, True, 1): 2.9e-12, (3, True, 1): 4.2e-12, (4, True, 1): 6.5e-12, (5, True, 1): 1.4e-12, (6, False, 1): 1.6e-12,
             (6, True, 1): 2.1e-11, (7, True, 1): 1.2e-12, (8, True, 1): 7.3e-12}
_lib = None
_i64, _vp, _dbl = ctypes.c_int64, ctypes.c_void_p, ctypes.c_double


def lib():
    global _lib
    if _lib is None:
        deps = [SRC] + [os.path.join(eh.INC, h) for h in ("mcd_simulated_grad.h", "mcd_grad.h", "mcd_simulated.h", "mcd_holdout.h",
                                                          "mcd_replicate.h", "mcd_predictive.h", "mcd_rng.h", "mcd_chunks.h",
                                                          "mcd_math.h", "mcd_exp_table.h", "mcd_dispatch.h")]
        if not os.path.exists(OUT) or any(os.path.getmtime(d) > os.path.getmtime(OUT) for d in deps):
            subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-Wno-unknown-pragmas", "-I", eh.INC,
                            SRC, "-o", OUT], check=True)
        _lib = ctypes.CDLL(OUT)
        _lib.emul_simulated_grad.argtypes = [ctypes.c_int, ctypes.c_int, _i64, _vp, _vp, _vp, _i64, _vp, _vp, _i64, _dbl, _dbl, _i64,
                                             _vp]
    return _lib


def n_columns(model, free):
    return dh.n_columns(model, free) if model in dh.MODELS else gh.n_columns(model, free)


def column_names(model, free):
    return dh.column_names(model, free) if model in dh.MODELS else gh.column_names(model, free)


def velocities(case):
    """The set of the matrix: N_SIMS simulations at the first rows of the case, by the host build of the velocity rule."""
    return sh.simulate(case, case["params"][:N_SIMS])


def emul(case, rows, row_sim, vel, chunk_len=96):
    """Emulated mcd_simulated_loglike_grad: (values (R,), gradients (R, K)) of the rows `rows` of case["params"], row j on
    the velocities vel[row_sim[j]] ((E, N), transposed here as the library keeps them).  vel = None: chunk_grad on the
    observed velocities."""
    model, free = case["model"], case["free"]
    params = np.ascontiguousarray(case["params"][rows])
    rec = eh.pack_records(case["cat"], model, case["centre"])
    wp = eh.pack_walkers(params, model, free)
    k = n_columns(model, free)
    assert params.shape[1] == k
    mean, s2 = sh._bg2(sh.background_of(case))
    out = np.empty((len(rows), 1 + k))
    if vel is None:
        sim, table, tp, sp, n_sims = None, None, None, None, 0
    else:
        sim = np.ascontiguousarray(row_sim, dtype=np.int64)
        table = np.ascontiguousarray(np.asarray(vel, dtype=np.float64).T)
        assert sim.size == len(rows) and table.shape[0] == rec.shape[0] and sim.min() >= 0 and sim.max() < table.shape[1]
        tp, sp, n_sims = table.ctypes.data, sim.ctypes.data, table.shape[1]
    assert lib().emul_simulated_grad(model, int(free), rec.shape[0], rec.ctypes.data, wp.ctypes.data, params.ctypes.data, len(rows),
                                     sp, tp, n_sims, mean, s2, int(chunk_len), out.ctypes.data) == 0
    return out[:, 0].copy(), out[:, 1:].copy()


def plain(case, rows, chunk_len=96):
    return emul(case, rows, None, None, chunk_len=chunk_len)


# ---- the reference -------------------------------------------------------------------------------------------------------
_cache = {}


def reference(case, w, e, vel):
    """{"g", "s", "err64", "value"} of row w of the case on simulation e of `vel`, computed once per (cell, w, e)."""
    model, n = case["model"], case["n"]
    key = (model, case["free"], n, w, e, case["params"][w].tobytes(), np.asarray(vel[e]).tobytes())
    if key not in _cache:
        cat64 = sh.substituted(case, vel[e])
        cat80 = dict(cat64)
        if "lnlike_bg" in cat80:
            mean, sigma = sh.background_of(case)
            cat80["lnlike_bg"] = oracle.gaussian_background(cat80["v"].astype(L), np.asarray(cat80["verr"]).astype(L), L(mean), L(sigma))
        terms = dh.grad_terms if model in dh.MODELS else gh.per_star
        per_star = dh.per_star if model in dh.MODELS else vh.per_star
        row, centre = case["params"][w], case["centre"]
        t80, t64 = terms(model, cat80, row, centre, L), terms(model, cat64, row, centre, np.float64)
        g80, s80 = t80.sum(axis=1), np.abs(t80).sum(axis=1)
        _cache[key] = {"g": g80, "s": s80, "err64": gh.col_err(t64.sum(axis=1), g80, s80),
                       "value": per_star(model, cat80, row, centre, L)[0].sum()}
    return _cache[key]


def floor(model, free, n):
    return SIM_FLOOR.get((model, bool(free), n), FLOOR)


def excess(grad, ref):
    """err - 2 err_np64 per column: what the floor has to cover."""
    return gh.col_err(grad, ref["g"], ref["s"]) - 2 * ref["err64"]


def check_row(value, grad, ref, n, cell, column_floor):
    """The rule of the module docstring on one row; returns (value error, largest column error)."""
    v_err = sh.value_error(value, ref["value"], n)
    assert v_err <= 1e-12, (cell, "value", float(value), float(ref["value"]), v_err)
    err = gh.col_err(grad, ref["g"], ref["s"])
    bound = 2 * ref["err64"] + column_floor
    bad = err > bound
    assert not bad.any(), (cell, "columns", np.nonzero(bad)[0].tolist(), "err", err[bad].tolist(), "bound", bound[bad].tolist())
    return v_err, float(err.max())


def _up(x):
    """x rounded up to two significant digits."""
    e = 10.0 ** (np.floor(np.log10(x)) - 1)
    return float(np.ceil(x / e - 1e-9) * e)


def sweep():
    """Prints, per cell, the largest err - 2 err_np64 of the host build over every row the GPU matrix can reach."""
    table = {}
    for model, free in CELLS:
        for n in STARS:
            case = sh.make_case(model, free, n)
            vel = velocities(case)
            rows = list(range(max(ROWS)))
            sim = sh.row_sims(len(rows), N_SIMS)
            _, grad = emul(case, rows, sim, vel)
            worst = max(float(excess(grad[j], reference(case, j, int(sim[j]), vel)).max()) for j in rows)
            # ... and the set of the observed velocities, on the 65 rows the GPU test evaluates there, by both loops
            obs = np.stack([case["cat"]["v"] + 1.0, case["cat"]["v"]])
            for g in (emul(case, rows[:65], np.ones(65, dtype=np.int64), obs)[1], plain(case, rows[:65])[1]):
                worst = max(worst, max(float(excess(g[j], reference(case, j, 1, obs)).max()) for j in rows[:65]))
            table[(model, free, n)] = worst
            print("model %d %-5s N = %4d: largest err - 2 err_np64 %9.2e%s" %
                  (model, "free" if free else "fixed", n, worst, "   -> floor %.1e" % _up(2 * worst) if 2 * worst > FLOOR else ""))
            _cache.clear()
    print("SIM_FLOOR = {%s}" % ", ".join("(%d, %s, %d): %.1e" % (k + (_up(2 * v),)) for k, v in sorted(table.items())
                                         if 2 * v > FLOOR))
    return table


# ---- linear-Gaussian catalogues: closed forms and NumPy stand-ins ----------------------------------------------------------
# holdout_helper's catalogue (200 stars, sigma_max fixed at 10 km/s, v_maxy = 0): v_i ~ N(v_sys + v_maxx sin(theta_i), n_i) is
# linear in (v_sys, v_maxx), so every maximum is a weighted least-squares solution.
GTOL, N_E, RUN_SEED = 1e-8, 64, 20261024


def sin_theta(cols, dtype=L):
    """sin(theta_i) of the constant-rotation model about the synthetic centre, from the oracle's rotation model."""
    from mcmc_dynamics_amd import synthetic
    ra, dec = (np.asarray(cols[k]).astype(dtype) for k in ("ra", "dec"))
    return oracle.rotation_model(ra, dec, dtype(0), dtype(1), dtype(0), dtype(synthetic.CENTER_RA_DEG), dtype(synthetic.CENTER_DEC_DEG))


def design(cols, names, dtype=L):
    """(N, P) design matrix of the free parameters `names` (v_sys, v_maxx)."""
    one = np.ones(len(cols["verr"]), dtype=dtype)
    return np.stack([{"v_sys": one, "v_maxx": sin_theta(cols, dtype)}[name] for name in names], axis=1)


def variances(cols, dtype=L):
    return np.asarray(cols["verr"]).astype(dtype) ** 2 + dtype(hh.SIGMA) ** 2


def least_squares(cols, names, vel, prior_sd=None):
    """In longdouble, for every row of vel (E, N): the maximiser (E, P) of  sum_i log N(v_i; (X b)_i, n_i) [+ log N(b_0; 0,
    prior_sd^2)], the maximum (E,) and the Hessian's negative A = X' X / n [+ 1 / prior_sd^2] (P, P)."""
    x, n = design(cols, names), variances(cols)
    vel = np.atleast_2d(np.asarray(vel)).astype(L)
    a = (x / n[:, None]).T @ x
    if prior_sd is not None:
        a[0, 0] += 1 / L(prior_sd) ** 2
    rhs = vel @ (x / n[:, None])                                   # (E, P)
    p = x.shape[1]
    if p == 1:
        beta = rhs / a[0, 0]
    else:
        det = a[0, 0] * a[1, 1] - a[0, 1] * a[1, 0]
        beta = np.stack([(a[1, 1] * rhs[:, 0] - a[0, 1] * rhs[:, 1]) / det, (a[0, 0] * rhs[:, 1] - a[1, 0] * rhs[:, 0]) / det], axis=1)
    resid = vel - beta @ x.T
    pi2 = 8 * np.arctan(L(1))
    value = -(resid * resid / n).sum(axis=1) / 2 - np.log(pi2 * n).sum() / 2
    if prior_sd is not None:
        value = value - (beta[:, 0] / L(prior_sd)) ** 2 / 2 - np.log(L(prior_sd) * np.sqrt(pi2))
    return beta, value, a


def lrt_fits(cols, **kwargs):
    """(full, null): ConstantFit on the closed-form catalogue with {v_sys, v_maxx} and {v_sys} free, in flat wide boxes."""
    full, null = hh.closed_form_fit(cols, **kwargs), hh.closed_form_fit(cols, **kwargs)
    full.parameters["v_maxx"].set(value=0.0, fixed=False, min=-1000.0, max=1000.0)
    return full, null


class NumpyLinear(object):
    """Stand-in for the device calls of a Runner on the closed-form catalogue, in NumPy float64: simulate (the velocity rule
    on the host: v' = X truth + sqrt(n) g), simulated_set, simulated_sims, lnprob_grad_batch (observed velocities) and
    lnprob_simulated_grad_batch.  `names`: the free parameters; prior_sd: a normal prior N(0, prior_sd^2) on the first.
    The boxes of the fits are wide.  Records what it was called with."""

    def __init__(self, cols, names, prior_sd=None):
        self.cols, self.names, self.prior_sd = cols, list(names), prior_sd
        self.x, self.n = design(cols, names, np.float64), variances(cols, np.float64)
        self.v = np.asarray(cols["v"], dtype=np.float64)
        self.velocities, self.calls, self.simulate_calls = None, [], []

    def simulate(self, truths, seed, sim0=0):
        truths = np.atleast_2d(np.asarray(truths, dtype=np.float64))
        self.simulate_calls.append({"truths": truths.copy(), "seed": seed, "sim0": sim0})
        g, _ = sh.numbers(seed, sim0, truths.shape[0], 0, self.n.size)
        self.velocities = truths @ self.x.T + np.sqrt(self.n)[None, :] * g
        return self.velocities.copy()

    def simulated_set(self, velocities):
        self.velocities = np.array(velocities, dtype=np.float64, copy=True)
        return self.velocities

    def simulated_sims(self):
        return 0 if self.velocities is None else self.velocities.shape[0]

    def _value_grad(self, values, vel):
        resid = vel - values @ self.x.T
        f = -0.5 * (resid * resid / self.n).sum(axis=1) - 0.5 * np.log(2.0 * np.pi * self.n).sum()
        g = (resid / self.n) @ self.x
        if self.prior_sd is not None:
            f = f - 0.5 * (values[:, 0] / self.prior_sd) ** 2 - np.log(self.prior_sd * np.sqrt(2.0 * np.pi))
            g[:, 0] -= values[:, 0] / self.prior_sd ** 2
        return f, g

    def lnprob_grad_batch(self, values):
        values = np.atleast_2d(np.asarray(values, dtype=np.float64))
        return self._value_grad(values, self.v[None, :])

    def lnprob_simulated_grad_batch(self, values, row_sim):
        values = np.atleast_2d(np.asarray(values, dtype=np.float64))
        sim = np.asarray(row_sim, dtype=np.int64).reshape(-1)
        self.calls.append({"rows": values.shape[0], "sim": sim.copy()})
        return self._value_grad(values, self.velocities[sim])

    def attach(self, monkeypatch, fit):
        for name in ("simulate", "simulated_set", "simulated_sims", "lnprob_grad_batch", "lnprob_simulated_grad_batch"):
            monkeypatch.setattr(fit, name, getattr(self, name))
        return self


def optimiser_room(a, scale, gtol=GTOL):
    """What the optimiser's stopping rule leaves of a quadratic's maximum: at a stop max_j |g_j| scale_j <= gtol, so
    2 (f_max - f) = g' A^-1 g <= |g|^2 / lambda_min(A) with |g_j| <= gtol / scale_j."""
    a = np.asarray(a, dtype=np.float64)
    g = gtol / np.asarray(scale, dtype=np.float64)
    return float((g * g).sum() / np.linalg.eigvalsh(a).min())

"""Test helper of the simulated catalogues (tests/test_simulated_cpu.py, tests/test_gpu_simulated.py).  Test infrastructure
only.

  * the CPU build of the velocity rule and the value loop (tests/emul/simulated_emul.cpp: csrc/mcd_simulated.h) and of the
    loop on the observed velocities it must reproduce (csrc/mcd_holdout.h: chunk_holdout);
  * the velocity rule restated in numpy.longdouble from the generator's g, u, with v_los*, n* and m* from the oracle's
    functions (as variant_helper.per_star / double_helper.per_star form them), and its bound
        |v' - exact| <= 1e-12 max(|v_i|, |v_los*|, sqrt(n*) |g|, 1);
    the helper asserts that no u lies within 1e-9 of m*, so that no star's component can hinge on a rounding error;
  * the value rule: |got - exact| <= 1e-12 max(|sum l|, N) against the longdouble sum of the per-star terms on the
    catalogue with the simulated velocities substituted (and, for the fixed-background families, lnlike_bg recomputed from
    the background's Gaussian);
  * the closed-form case of the end-to-end run: holdout_helper's catalogue with only v_sys free under the prior N(0, 2^2);
    catalogue e, simulated at truth e, has the exact posterior N(mu_e, 1 / Lambda_e), Lambda_e = sum 1 / n_i + 1 / 4; a NumPy
    stand-in for Runner.simulate / Runner.lnprob_simulated_batch; the run the GPU test makes (sized by
    tests/test_simulated_cpu.py) and the bounds it is held to."""
import ctypes
import os
import subprocess

import numpy as np

import double_helper as dh
import emul_helper as eh
import holdout_helper as hh
import variant_helper as vh
from oracle import lnprob_numpy as oracle

SRC = os.path.join(eh.ROOT, "tests", "emul", "simulated_emul.cpp")
OUT = os.path.join(eh.ROOT, "tests", "emul", "libmcd_simulated_emul.so")
L = vh.L
SEED = 20261022                         # the generator seed of the matrix (the margin assertion below holds for it)
MODELS = tuple(range(9))
MARGIN = 1e-9
_lib = None
_u64, _i64, _vp, _dbl = ctypes.c_uint64, ctypes.c_int64, ctypes.c_void_p, ctypes.c_double


def lib():
    global _lib
    if _lib is None:
        deps = [SRC] + [os.path.join(eh.INC, h) for h in ("mcd_simulated.h", "mcd_holdout.h", "mcd_replicate.h", "mcd_predictive.h",
                                                          "mcd_rng.h", "mcd_chunks.h", "mcd_math.h", "mcd_exp_table.h",
                                                          "mcd_dispatch.h")]
        if not os.path.exists(OUT) or any(os.path.getmtime(d) > os.path.getmtime(OUT) for d in deps):
            subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-Wno-unknown-pragmas", "-I", eh.INC,
                            SRC, "-o", OUT], check=True)
        _lib = ctypes.CDLL(OUT)
        _lib.emul_simulate.argtypes = [ctypes.c_int, ctypes.c_int, _i64, _vp, _vp, _i64, _u64, _i64, _dbl, _dbl, _i64, _vp]
        _lib.emul_simulated_value.argtypes = [ctypes.c_int, ctypes.c_int, _i64, _vp, _vp, _i64, _vp, _vp, _i64, _dbl, _dbl, _i64, _vp]
        _lib.emul_simulated_plain.argtypes = [ctypes.c_int, ctypes.c_int, _i64, _vp, _vp, _i64, _i64, _vp]
        _lib.emul_simulated_numbers.argtypes = [_u64, _i64, _i64, _i64, _i64, _vp, _vp]
        _lib.emul_simulated_numbers.restype = None
        _lib.emul_simulated_budget.argtypes = [_i64, _i64]
    return _lib


# The velocity rule makes the model velocity itself an output, on the scale of that velocity: v_los* moves by
# v_max d(theta) with the position angle, and the offsets' own rounding gives d(theta) <= 3.3e-16 / r (dy subtracts two
# O(0.45) products; predictive_helper.clear_of_centres has the derivation).  variant_helper.make_case keeps its stars 0.01
# deg = 1.7e-4 rad from the centre, d(theta) <= 1.9e-12: an input error of the catalogue's float64 geometry that no kernel
# can undo, and above the 1e-12 of the bound (seen: 1.04e-12 and 1.34e-12 on a star whose scale was |v_los*| itself).  The
# matrix therefore spreads the same stars over twenty times the field, as replicate_helper.wide_field does for the angular
# sums: 0.2 deg from every centre, d(theta) <= 9.5e-14.
FIELD_STRETCH = 20.0


def make_case(model, free, n):
    case = dh.make_case(model, free, n) if model in dh.MODELS else vh.make_case(model, free, n)
    cat = case["cat"]
    cat["ra"] = vh.CENTRE[0] + FIELD_STRETCH * (cat["ra"] - vh.CENTRE[0])
    cat["dec"] = vh.CENTRE[1] + FIELD_STRETCH * (cat["dec"] - vh.CENTRE[1])
    return case


def background_of(case):
    """(bg_mean, bg_sigma) of a call: the Gaussian behind variant_helper.make_case's lnlike_bg column for the
    fixed-background models, NaN otherwise."""
    if eh.BG_OF[case["model"]] in (1, 3):
        return 0.1 * case["scale"], 3.0 * case["scale"]
    return float("nan"), float("nan")


def _bg2(bg):
    return (0.0, 0.0) if not np.isfinite(bg[0]) else (float(bg[0]), float(bg[1]) * float(bg[1]))


def numbers(seed, s0, S, i0, N):
    """g, u (S, N) of simulations s0 .. and stars i0 .. (host build of csrc/mcd_replicate.h)."""
    g, u = np.empty((S, N)), np.empty((S, N))
    lib().emul_simulated_numbers(int(seed), int(s0), int(S), int(i0), int(N), g.ctypes.data, u.ctypes.data)
    return g, u


def simulate(case, truths, seed=SEED, sim0=0, chunk_len=96):
    """Emulated mcd_simulate: (E, N) velocities of the simulations sim0 .. at the truth rows `truths` (E, K)."""
    model, free = case["model"], case["free"]
    rec = eh.pack_records(case["cat"], model, case["centre"])
    wp = eh.pack_walkers(np.ascontiguousarray(truths), model, free)
    mean, s2 = _bg2(background_of(case))
    out = np.full((wp.shape[0], rec.shape[0]), np.nan)
    assert lib().emul_simulate(model, int(free), rec.shape[0], rec.ctypes.data, wp.ctypes.data, wp.shape[0], int(seed), int(sim0),
                               mean, s2, int(chunk_len), out.ctypes.data) == 0
    return out


def value(case, rows, row_sim, velocities, chunk_len=96):
    """Emulated mcd_simulated_loglike: (R,) values of the rows `rows` of case["params"], row j on the velocities
    velocities[row_sim[j]] ((E, N), transposed here as the library keeps them)."""
    model, free = case["model"], case["free"]
    rec = eh.pack_records(case["cat"], model, case["centre"])
    wp = eh.pack_walkers(np.ascontiguousarray(case["params"][rows]), model, free)
    sim = np.ascontiguousarray(row_sim, dtype=np.int64)
    table = np.ascontiguousarray(np.asarray(velocities, dtype=np.float64).T)
    assert sim.size == len(rows) and table.shape[0] == rec.shape[0] and sim.min() >= 0 and sim.max() < table.shape[1]
    mean, s2 = _bg2(background_of(case))
    out = np.empty(len(rows))
    assert lib().emul_simulated_value(model, int(free), rec.shape[0], rec.ctypes.data, wp.ctypes.data, len(rows), sim.ctypes.data,
                                      table.ctypes.data, table.shape[1], mean, s2, int(chunk_len), out.ctypes.data) == 0
    return out


def plain_value(case, rows, chunk_len=96):
    """(R,) sums of the terms on the observed velocities by chunk_holdout, chunked as `value` chunks."""
    model, free = case["model"], case["free"]
    rec = eh.pack_records(case["cat"], model, case["centre"])
    wp = eh.pack_walkers(np.ascontiguousarray(case["params"][rows]), model, free)
    out = np.empty(len(rows))
    assert lib().emul_simulated_plain(model, int(free), rec.shape[0], rec.ctypes.data, wp.ctypes.data, len(rows), int(chunk_len),
                                      out.ctypes.data) == 0
    return out


def row_sims(rows, n_sims):
    """A non-monotone map with repeats onto n_sims simulations."""
    return (7 * np.arange(rows, dtype=np.int64) + 3) % n_sims


# ---- the velocity rule, restated ----------------------------------------------------------------------------------------
def truth_parts(model, cat, row, centre, bg, dtype=L):
    """v_los*, n*, m* (None without a background), mu_b, s2_b of one truth row (C-ABI order), every input cast to `dtype`."""
    c = {k: np.asarray(v).astype(dtype) for k, v in cat.items()}
    if model in dh.MODELS:
        head, rc, dc, tail = dh._split(row, centre, dtype)
        v_sys, sigma, a, vx, vy, rp, vxc, vyc, ratio = head
        v_los = oracle.model_rotation(c["ra"], c["dec"], v_sys, vx, vy, rp, rc, dc) + \
            oracle.model_rotation(c["ra"], c["dec"], dtype(0), vxc, vyc, ratio * rp, rc, dc)
        sig = oracle.model_dispersion(c["ra"], c["dec"], sigma, a, rc, dc)
    else:
        head, rc, dc, tail = vh._split(model, row, centre, dtype)
        if model in vh.PROFILE_MODELS:
            v_los = oracle.model_rotation(c["ra"], c["dec"], head[0], head[3], head[4], head[5], rc, dc)
            sig = oracle.model_dispersion(c["ra"], c["dec"], head[1], head[2], rc, dc)
        else:
            v_los = oracle.rotation_model(c["ra"], c["dec"], head[0], head[2], head[3], rc, dc)
            sig = head[1]
    norm = c["verr"] * c["verr"] + sig * sig
    kind = eh.BG_OF[model]
    if kind == 0:
        return v_los, norm, None, None, None
    m = c["pmember"] if kind == 1 else c["density"] / (c["density"] + tail[-1])
    mu, sb = (tail[0], tail[1]) if kind == 2 else (dtype(bg[0]), dtype(bg[1]))
    return v_los, norm, m, mu, sb * sb


def exact_velocities(case, truths, g, u):
    """((E, N) velocities in longdouble, (E, N) float64 scales of the bound, the smallest |u - m*|) from the numbers g, u
    (E, N) of the simulations."""
    model, cat, centre = case["model"], case["cat"], case["centre"]
    bg = background_of(case)
    v, verr = np.asarray(cat["v"]).astype(L), np.asarray(cat["verr"]).astype(L)
    out, scale, margin = [], [], np.inf
    for e, row in enumerate(np.atleast_2d(truths)):
        v_los, norm, m, mu, s2 = truth_parts(model, cat, row, centre, bg)
        ge = g[e].astype(L)
        cluster = v_los + np.sqrt(norm) * ge
        if m is None:
            out.append(cluster)
        else:
            margin = min(margin, float(np.min(np.abs(u[e].astype(L) - m))))
            out.append(np.where(u[e].astype(L) < m, cluster, mu + np.sqrt(verr * verr + s2) * ge))
        scale.append(np.maximum.reduce([np.abs(v), np.abs(v_los), np.sqrt(norm) * np.abs(ge), np.ones_like(v)]).astype(np.float64))
    return np.array(out), np.array(scale), margin


def check_velocities(got, case, truths, seed=SEED, sim0=0, label=None, numbers=None):
    """The velocity bound on `got` (E, N) and the asserted margin; returns the largest error in units of the bound's scale.
    numbers: what replays the generator (default: the CPU build; the GPU tests pass _native.replicate_numbers)."""
    n = got.shape[1]
    g, u = (numbers or globals()["numbers"])(seed, sim0, got.shape[0], 0, n)
    exact, scale, margin = exact_velocities(case, truths, g, u)
    assert margin > MARGIN, (label, "a u within 1e-9 of m*: choose another seed", margin)
    err = np.abs(got.astype(L) - exact).astype(np.float64) / scale
    assert np.all(err <= 1e-12), (label, float(err.max()), np.unravel_index(int(np.argmax(err)), err.shape))
    return float(err.max())


# ---- the value rule -----------------------------------------------------------------------------------------------------
def substituted(case, v):
    """The case's catalogue with the velocities `v` (N,) in place of the observed ones; lnlike_bg recomputed from the
    background's Gaussian where the catalogue carries one."""
    cat = {k: (x.copy() if isinstance(x, np.ndarray) else x) for k, x in case["cat"].items()}
    cat["v"] = np.asarray(v, dtype=np.float64).copy()
    if "lnlike_bg" in cat:
        mean, sigma = background_of(case)
        cat["lnlike_bg"] = oracle.gaussian_background(cat["v"], cat["verr"], mean, sigma)
    return cat


def exact_value(case, row, v):
    """sum_i l_i(row; v) in longdouble."""
    model = case["model"]
    cat = substituted(case, v)
    if "lnlike_bg" in cat:
        mean, sigma = background_of(case)
        cat["lnlike_bg"] = oracle.gaussian_background(cat["v"].astype(L), np.asarray(cat["verr"]).astype(L), L(mean), L(sigma))
    per_star = dh.per_star if model in dh.MODELS else vh.per_star
    return per_star(model, cat, row, case["centre"], L)[0].sum()


def value_error(got, exact, n):
    return float(abs(L(got) - exact) / max(abs(exact), L(n)))


# ---- the closed-form case of the end-to-end run ---------------------------------------------------------------------------
# The runs tests/test_gpu_simulated.py makes, sized by tests/test_simulated_cpu.py::test_closed_form_harness_sizes_the_run:
# the stretch move's tau on this one-parameter posterior is 20 .. 28 steps, and every fit must keep 50 tau.
PRIOR_SD = 2.0
RUNS = {"ragged": dict(n_sims=64, n_walkers=32, n_steps=1900, n_burn=300),       # W / 2 = 16: four simulations per wave
        "tiled": dict(n_sims=64, n_walkers=128, n_steps=1900, n_burn=300)}       # W / 2 = 64: one simulation per wave
RUN_SEED = 20261023
CHI2_999, CHI2_99, N_BINS = 24.32, 18.48, 8                                       # quantiles of chi2(7)


def closed_form_fit(cols, **kwargs):
    """holdout_helper's fit (only v_sys free, in a wide box) with the proper prior N(0, PRIOR_SD^2) on v_sys."""
    fit = hh.closed_form_fit(cols, **kwargs)
    fit.parameters["v_sys"].set(prior=("normal", 0.0, PRIOR_SD))
    return fit


def host_velocities(cols, truths, seed, sim0=0):
    """Rule 1 on the closed-form catalogue in NumPy float64: v'(e, i) = truth_e + sqrt(n_i) g(seed, sim0 + e, i)."""
    truths = np.asarray(truths, dtype=np.float64).reshape(-1)
    n = np.asarray(cols["verr"], float) ** 2 + hh.SIGMA ** 2
    g, _ = numbers(seed, sim0, truths.size, 0, n.size)
    return truths[:, None] + np.sqrt(n)[None, :] * g


def closed_form_posteriors(cols, velocities):
    """(mu_e, Lambda_e) (E,) of the exact posteriors N(mu_e, 1 / Lambda_e) of v_sys given catalogue e, in longdouble."""
    n = np.asarray(cols["verr"]).astype(L) ** 2 + L(hh.SIGMA) ** 2
    lam = (1 / n).sum() + 1 / L(PRIOR_SD) ** 2
    return (np.asarray(velocities).astype(L) / n).sum(axis=1) / lam, np.full(len(velocities), lam)


class NumpySimulated(object):
    """Stand-in for Runner.simulate and Runner.lnprob_simulated_batch on the closed-form catalogue: velocities by
    host_velocities, values (..., 1) with one simulation per row -> sum_i log N(v'(e, i); v_sys, n_i) + log N(v_sys; 0,
    PRIOR_SD^2) in NumPy float64 (the box of the fit is wide).  Records what it was called with."""

    def __init__(self, cols):
        self.cols, self.n = cols, np.asarray(cols["verr"], float) ** 2 + hh.SIGMA ** 2
        self.velocities, self.calls, self.simulate_calls = None, [], []

    def simulate(self, truths, seed, sim0=0):
        self.simulate_calls.append({"truths": np.array(truths, copy=True), "seed": seed, "sim0": sim0})
        self.velocities = host_velocities(self.cols, truths, seed, sim0)
        self._a, self._b = (1.0 / self.n).sum(), (self.velocities / self.n).sum(axis=1)
        self._c = (self.velocities ** 2 / self.n).sum(axis=1) + np.log(2.0 * np.pi * self.n).sum()
        return self.velocities.copy()

    def simulated_set(self, velocities):
        self.velocities = np.array(velocities, dtype=np.float64, copy=True)
        self._a, self._b = (1.0 / self.n).sum(), (self.velocities / self.n).sum(axis=1)
        self._c = (self.velocities ** 2 / self.n).sum(axis=1) + np.log(2.0 * np.pi * self.n).sum()
        return self.velocities

    def __call__(self, values, row_sim):
        values = np.asarray(values, dtype=np.float64)
        sim = np.asarray(row_sim, dtype=np.int64).reshape(-1)
        self.calls.append({"shape": values.shape, "sim": sim.copy()})
        x = values.reshape(-1)
        # sum_i (v - x)^2 / n = c - 2 b x + a x^2 (+ the log terms in c): the same quadratic, in O(rows)
        lnl = -0.5 * (self._c[sim] - 2.0 * self._b[sim] * x + self._a * x * x)
        lp = -0.5 * (x / PRIOR_SD) ** 2 - np.log(PRIOR_SD * np.sqrt(2.0 * np.pi))
        return (lnl + lp).reshape(values.shape[:-1])


def check_fits(fits, mu, lam, label, n_walkers, t_kept):
    """Every fit's mean and variance against its exact posterior N(mu_e, 1 / Lambda_e), by the formulas of
    weighted_value_helper.check_bags: with W walkers, T kept steps and tau_e autocorrelation times the fit holds
    W T / tau_e effective draws, so its mean has standard error sqrt(tau_e / (W T) / Lambda_e) and its variance the
    relative standard error sqrt(2 tau_e / (W T)).  Six of them bound both.  Returns the largest standardised errors."""
    mu, lam = np.asarray(mu, dtype=np.float64), np.asarray(lam, dtype=np.float64)
    tau = np.max(np.atleast_2d(fits["tau"]), axis=1)
    assert fits["converged"].all() and np.all(t_kept >= 50.0 * tau), (label, tau.tolist())
    n_eff = float(n_walkers * t_kept) / tau
    z_mean = np.abs(fits["mean"][:, 0] - mu) / np.sqrt(1.0 / n_eff / lam)
    z_var = np.abs(fits["std"][:, 0] ** 2 * lam - 1.0) / np.sqrt(2.0 / n_eff)
    print("%s: tau %.1f .. %.1f, kept steps / tau >= %.1f, largest standardised mean error %.2f, variance error %.2f" %
          (label, tau.min(), tau.max(), float(t_kept / tau.max()), z_mean.max(), z_var.max()))
    assert np.all(z_mean <= 6.0), (label, "mean", z_mean.tolist())
    assert np.all(z_var <= 6.0), (label, "variance", z_var.tolist())
    return float(z_mean.max()), float(z_var.max())


def check_ranks(summary, label, bound=CHI2_999):
    print("%s: thin %d, %d draws per fit, rank chi2 %s (bound %.2f), largest ECDF distance %s" %
          (label, summary["thin"], summary["n_draws"], np.round(summary["chi2"], 2).tolist(), bound,
           np.round(summary["ecdf_max"], 3).tolist()))
    assert np.all(summary["chi2"] < bound), (label, summary["chi2"].tolist(), summary["hist"].tolist())
    return float(summary["chi2"].max())

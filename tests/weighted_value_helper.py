"""Test helper of the weighted value kernel and the bagged posterior (tests/test_weighted_value_cpu.py,
tests/test_bagged_cpu.py, tests/test_gpu_weighted_value.py, tests/test_gpu_bagged.py).  Test infrastructure only.

  * the CPU build of the weighted value loop (tests/emul/weighted_value_emul.cpp: csrc/mcd_weighted_value.h) and of the
    unweighted loop it must reproduce under unit weights (csrc/mcd_holdout.h: chunk_holdout);
  * the value rule: |got - exact| <= 1e-12 max(|sum w l|, sum w) against weighted_helper.reference (longdouble);
  * the closed-form case of the bagged posterior: on holdout_helper.closed_form_columns() with only v_sys free, bag b's
    posterior under the weights w(b, .) and a likelihood scale f is exactly N(mu_b, 1 / (f Lambda_b)), mu_b and Lambda_b
    from weighted_helper.closed_form_maximum; a NumPy stand-in for Runner.lnprob_weighted_batch on that catalogue; the run
    the GPU test makes (sized by tests/test_bagged_cpu.py); and the two bounds every bag is held to."""
import ctypes
import os
import subprocess

import numpy as np

import emul_helper as eh
import holdout_helper as hh
import variant_helper as vh
import weighted_helper as wh

SRC = os.path.join(eh.ROOT, "tests", "emul", "weighted_value_emul.cpp")
OUT = os.path.join(eh.ROOT, "tests", "emul", "libmcd_weighted_value_emul.so")
L = vh.L
_lib = None


def lib():
    global _lib
    if _lib is None:
        deps = [SRC] + [os.path.join(eh.INC, h) for h in ("mcd_weighted_value.h", "mcd_weighted.h", "mcd_holdout.h", "mcd_weights.h",
                                                          "mcd_rng.h", "mcd_grad.h", "mcd_math.h", "mcd_exp_table.h",
                                                          "mcd_dispatch.h")]
        if not os.path.exists(OUT) or any(os.path.getmtime(d) > os.path.getmtime(OUT) for d in deps):
            subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-Wno-unknown-pragmas", "-I", eh.INC,
                            SRC, "-o", OUT], check=True)
        _lib = ctypes.CDLL(OUT)
        _lib.emul_weighted_value.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int64, ctypes.c_void_p,
                                             ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p,
                                             ctypes.c_int64, ctypes.c_int64, ctypes.c_void_p]
        _lib.emul_plain_value.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_int64, ctypes.c_void_p, ctypes.c_void_p,
                                          ctypes.c_int64, ctypes.c_int64, ctypes.c_void_p]
    return _lib


def emul_weighted_value(case, rows, rep, scheme, seed=wh.SEED, explicit=None, chunk_len=96):
    """(R,) values of the rows `rows` of case["params"] under the replicates `rep`.  explicit: (n_replicates, N) weights
    for scheme "explicit" (transposed here, as the library does on upload)."""
    model, free = case["model"], case["free"]
    params = np.ascontiguousarray(case["params"][rows])
    rec = eh.pack_records(case["cat"], model, case["centre"])
    wp = eh.pack_walkers(params, model, free)
    rep = np.ascontiguousarray(rep, dtype=np.int64)
    assert rep.size == len(rows)
    wt = None if explicit is None else np.ascontiguousarray(np.asarray(explicit, dtype=np.float64).T)
    out = np.empty(len(rows))
    rc = lib().emul_weighted_value(model, int(free), wh.SCHEMES.get(scheme, scheme), rec.shape[0], rec.ctypes.data, wp.ctypes.data,
                                   len(rows), rep.ctypes.data, int(seed), None if wt is None else wt.ctypes.data,
                                   0 if wt is None else wt.shape[1], int(chunk_len), out.ctypes.data)
    assert rc == 0
    return out


def emul_plain_value(case, rows, chunk_len=96):
    """(R,) sums of the plain terms by chunk_holdout, chunked as emul_weighted_value chunks."""
    model, free = case["model"], case["free"]
    params = np.ascontiguousarray(case["params"][rows])
    rec = eh.pack_records(case["cat"], model, case["centre"])
    wp = eh.pack_walkers(params, model, free)
    out = np.empty(len(rows))
    assert lib().emul_plain_value(model, int(free), rec.shape[0], rec.ctypes.data, wp.ctypes.data, len(rows), int(chunk_len),
                                  out.ctypes.data) == 0
    return out


def value_error(value, ref):
    """|got - exact| / max(|sum w l|, sum w) against weighted_helper.reference."""
    scale = max(abs(ref["value"]), ref["sum_w"], L(1e-300))
    return float(abs(L(value) - ref["value"]) / scale)


# ---- the closed-form case of the bagged posterior ------------------------------------------------------------------------
# The run tests/test_gpu_bagged.py makes, sized by tests/test_bagged_cpu.py::test_closed_form_harness_sizes_the_run: the
# stretch move's tau on this one-parameter posterior is 20 .. 26 steps, and every bag must keep 50 tau.
N_BAGS, N_WALKERS, N_STEPS, N_BURN, RUN_SEED = 16, 64, 1900, 300, 20261021
SHORT_STEPS, SHORT_BURN = 700, 200                                    # the bag_fraction = 0.5 run: the same checks, fewer tau


def start_positions(cols, n_bags, n_walkers, seed=1):
    """(B, W, 1) around the full-data posterior, two of its widths wide: inside every bag's bulk."""
    mu, var = hh.posterior_without(cols, [])
    return float(mu) + 2.0 * np.sqrt(float(var)) * np.random.default_rng(seed).normal(size=(n_bags, n_walkers, 1))


def closed_form_bags(cols, weights, bag_fraction=1.0):
    """(mu_b, Lambda_b) (B,) of the bags' exact posteriors N(mu_b, 1 / Lambda_b): the likelihood scale multiplies the
    curvature and leaves the maximum where it is."""
    mu, lam = wh.closed_form_maximum(cols["v"], cols["verr"], hh.SIGMA, weights)
    return mu, lam * L(bag_fraction)


class NumpyWeightedValue(object):
    """Stand-in for Runner.lnprob_weighted_batch on the closed-form catalogue: values (..., 1), one replicate per row ->
    weight_scale sum_i w(b, i) log N(v_i; v_sys, n_i) in NumPy float64 (the box prior of the fit is flat and wide).
    ``weights_of(scheme, seed, replicates) -> (rows, N)``; records what it was called with."""

    def __init__(self, cols, weights_of):
        self.v, self.n = np.asarray(cols["v"], float), np.asarray(cols["verr"], float) ** 2 + hh.SIGMA ** 2
        self.weights_of, self.calls, self._table = weights_of, [], {}

    def __call__(self, values, row_replicate, scheme="exponential", seed=0, weights=None, weight_scale=1.0):
        values = np.asarray(values, dtype=np.float64)
        rep = np.asarray(row_replicate, dtype=np.int64).reshape(-1)
        self.calls.append({"shape": values.shape, "replicate": rep.copy(), "scheme": scheme, "seed": seed, "scale": weight_scale})
        for b in np.unique(rep):
            if (scheme, seed, int(b)) not in self._table:
                self._table[(scheme, seed, int(b))] = self.weights_of(scheme, seed, np.array([b]))[0]
        w = np.stack([self._table[(scheme, seed, int(b))] for b in rep])
        x = values.reshape(-1, 1)
        d = self.v[None, :] - x
        f = (w * (-0.5 * np.log(2.0 * np.pi * self.n) - 0.5 * d * d / self.n)).sum(axis=1)
        return (weight_scale * f).reshape(values.shape[:-1])


def check_bags(out, mu, lam, label, n_walkers, t_kept):
    """Every bag's mean and variance against its exact posterior N(mu_b, 1 / Lambda_b), and `between` against the variance
    of the exact means.  The bounds cap Monte-Carlo error in units of its own standard error: with W walkers, T kept steps
    and tau_b autocorrelation times the bag holds W T / tau_b effective draws, so its mean has standard error
    sqrt(tau_b / (W T) / Lambda_b) and its variance the relative standard error sqrt(2 tau_b / (W T)) (a Gaussian's).

    between = Var(mu_b + e_b), e_b the Monte-Carlo error of bag b's mean with standard error m_b = mean_mcse[b]: it exceeds
    Var(mu_b) by Var(e) -- expectation m^2 = mean(m_b^2), standard error m^2 sqrt(2 / (B - 1)) -- and by twice the sample
    covariance of mu and e, standard error sd(mu) m / sqrt(B - 1).  The budget is m^2 plus six of those standard errors.
    Returns the largest standardised errors."""
    mu, lam = np.asarray(mu, dtype=np.float64), np.asarray(lam, dtype=np.float64)
    tau, n_b = out["tau"], mu.size
    n_eff = float(n_walkers * t_kept) / tau
    z_mean = np.abs(out["bag_mean"][:, 0] - mu) / np.sqrt(1.0 / n_eff / lam)
    z_var = np.abs(out["bag_var"][:, 0] * lam - 1.0) / np.sqrt(2.0 / n_eff)
    var_mu = float(np.var(mu, ddof=1))
    m2 = float(np.mean(out["mean_mcse"][:, 0] ** 2))
    budget = m2 + 6.0 * (2.0 * np.sqrt(var_mu * m2 / (n_b - 1)) + m2 * np.sqrt(2.0 / (n_b - 1)))
    between, within = float(out["between"][0, 0]), float(out["within"][0, 0])
    print("%s: tau %.1f .. %.1f, kept steps / tau >= %.1f, largest standardised mean error %.2f, variance error %.2f; "
          "between %.6g against Var(mu_b) %.6g (budget %.3g), between / within %.4f against %.4f exact" %
          (label, tau.min(), tau.max(), float(t_kept / tau.max()), z_mean.max(), z_var.max(), between, var_mu, budget, between / within, var_mu * float(np.mean(lam))))
    assert np.all(z_mean <= 6.0), (label, "mean", z_mean.tolist())
    assert np.all(z_var <= 6.0), (label, "variance", z_var.tolist())
    assert abs(between - var_mu) <= budget, (label, between, var_mu, budget)
    return float(z_mean.max()), float(z_var.max())

"""CPU: the host layer of the weighted-likelihood bootstrap (analysis/runner.py: bootstrap_summary, Runner.bootstrap) and
the compiler's resource report of the weighted gradient kernels (profiles/weighted_resources.json).

  5. bootstrap_summary on known (B, P) arrays against NumPy's moments and percentiles; non-converged rows are excluded;
     the warning below 90 % converged; std_ratio against a Laplace covariance;
  6. Runner.bootstrap's bookkeeping on a stubbed lnprob_weighted_grad_batch, a NumPy quadratic with per-replicate weights
     (tests/weighted_helper.py: QuadraticStub): replicate ids 0 .. B - 1, one start per replicate at x_hat, the seed and
     the scheme passed through, and -- the condition the GPU end-to-end test relies on -- every replicate converges to the
     closed-form weighted maximum within the stopping rule's own bound gtol / Lambda_b; BinnedConstantFit raises;
  7. no instantiation of weighted_grad_kernel uses scratch memory or LDS."""
import json
import os
import warnings

import numpy as np
import pytest

import holdout_helper as hh
import weighted_helper as wh
from mcmc_dynamics_amd import DataReader, synthetic
from mcmc_dynamics_amd.analysis import BinnedConstantFit
from mcmc_dynamics_amd.analysis.runner import BOOTSTRAP_PERCENTILES, bootstrap_summary

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------ 5. bootstrap_summary
def _known(b=40, p=3, seed=2):
    rng = np.random.default_rng(seed)
    x_hat = np.array([1.0, -2.0, 30.0])[:p]
    x = x_hat + rng.normal(size=(b, p)) * np.array([0.5, 2.0, 0.01])[:p] + np.array([0.1, 0.0, 0.0])[:p]
    return x, x_hat


def test_summary_against_numpy_moments_and_percentiles():
    x, x_hat = _known()
    s = bootstrap_summary(x, x_hat, np.ones(40, dtype=bool), ["a", "b", "c"])
    assert s["n_converged"] == s["n_replicates"] == 40 and s["names"] == ["a", "b", "c"]
    assert np.allclose(s["mean"], x.mean(axis=0), rtol=1e-15, atol=0)
    assert np.allclose(s["covariance"], np.cov(x.T, ddof=1), rtol=1e-13, atol=0)
    assert np.allclose(s["std"], x.std(axis=0, ddof=1), rtol=1e-13, atol=0)
    assert np.array_equal(s["bias"], s["mean"] - x_hat)
    assert tuple(sorted(s["percentiles"])) == BOOTSTRAP_PERCENTILES == (2.5, 16.0, 50.0, 84.0, 97.5)
    for q in BOOTSTRAP_PERCENTILES:
        assert np.array_equal(s["percentiles"][q], np.percentile(x, q, axis=0))
    assert "std_ratio" not in s
    np.linalg.cholesky(s["covariance"])                          # a covariance get_initials_laplace and hmc can factor


def test_summary_excludes_the_replicates_that_did_not_converge():
    x, x_hat = _known()
    ok = np.ones(40, dtype=bool)
    ok[[3, 17, 30]] = False
    x[~ok] = 1e9                                                 # would wreck every moment
    with warnings.catch_warnings():
        warnings.simplefilter("error")                           # 37 of 40 is above 90 %: no warning
        s = bootstrap_summary(x, x_hat, ok, ["a", "b", "c"])
    assert s["n_converged"] == 37 and s["n_replicates"] == 40
    assert np.allclose(s["mean"], x[ok].mean(axis=0), rtol=1e-15, atol=0)
    assert np.allclose(s["covariance"], np.cov(x[ok].T, ddof=1), rtol=1e-13, atol=0)
    assert np.array_equal(s["percentiles"][50.0], np.percentile(x[ok], 50.0, axis=0))


def test_summary_warns_below_90_percent():
    x, x_hat = _known()
    ok = np.ones(40, dtype=bool)
    ok[:5] = False                                               # 35 of 40 = 87.5 %
    with pytest.warns(UserWarning, match="35 of 40"):
        bootstrap_summary(x, x_hat, ok, ["a", "b", "c"])
    ok[4] = True                                                 # 36 of 40 = 90 %: not fewer than 90 %
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        bootstrap_summary(x, x_hat, ok, ["a", "b", "c"])


def test_std_ratio():
    x, x_hat = _known()
    lap = np.diag([0.25, 1.0, 1e-4])                             # the widths the replicates were drawn with: 0.5, 2 (twice 1), 0.01
    s = bootstrap_summary(x, x_hat, np.ones(40, dtype=bool), ["a", "b", "c"], laplace_covariance=lap)
    assert np.allclose(s["std_ratio"], x.std(axis=0, ddof=1) / np.array([0.5, 1.0, 0.01]), rtol=1e-13, atol=0)
    assert 0.7 < s["std_ratio"][0] < 1.3 and 1.4 < s["std_ratio"][1] < 2.6
    with pytest.raises(ValueError):
        bootstrap_summary(x, x_hat, np.ones(40, dtype=bool), ["a", "b", "c"], laplace_covariance=np.eye(2))
    with pytest.raises(ValueError):
        bootstrap_summary(x, x_hat[:2], np.ones(40, dtype=bool), ["a", "b"])


def test_one_parameter_and_no_converged_replicate():
    x, x_hat = _known(p=1)
    s = bootstrap_summary(x, x_hat, np.ones(40, dtype=bool), ["a"])
    assert s["covariance"].shape == (1, 1) and s["std"].shape == (1,)
    with pytest.warns(UserWarning):
        s = bootstrap_summary(x, x_hat, np.zeros(40, dtype=bool), ["a"])
    assert s["n_converged"] == 0 and np.all(np.isnan(s["mean"])) and np.all(np.isnan(s["std"]))


# ------------------------------------------------------------------------------------------ 6. Runner.bootstrap
def _stubbed_fit(monkeypatch, laplace_var=None):
    cols = hh.closed_form_columns()
    fit = hh.closed_form_fit(cols)
    n = cols["verr"] ** 2 + hh.SIGMA ** 2

    def weights_of(scheme, seed, rep):
        return wh.weights_of_rows(scheme, seed, rep, hh.N_STARS)
    stub = wh.QuadraticStub(cols["v"], n, weights_of)
    monkeypatch.setattr(fit, "lnprob_weighted_grad_batch", stub)

    def laplace(x):
        if laplace_var is None:
            raise ValueError("no Laplace approximation in this test")
        return {"covariance": np.array([[laplace_var]])}
    monkeypatch.setattr(fit, "laplace", laplace)
    return fit, stub, cols


@pytest.mark.parametrize("scheme", ["exponential", "poisson"])
def test_bootstrap_bookkeeping_and_convergence_on_the_numpy_quadratic(monkeypatch, scheme):
    cols = hh.closed_form_columns()
    fit, stub, cols = _stubbed_fit(monkeypatch, laplace_var=1.0 / np.sum(1.0 / (cols["verr"] ** 2 + hh.SIGMA ** 2)))
    x_hat = np.array([float(wh.closed_form_maximum(cols["v"], cols["verr"], hh.SIGMA, np.ones(hh.N_STARS))[0][0])])
    out = fit.bootstrap(n_replicates=64, scheme=scheme, seed=1, x_hat=x_hat)
    # one start per replicate at x_hat, ids 0 .. B - 1 in every call, seed and scheme passed through
    assert np.array_equal(stub.calls[0]["first"], np.tile(x_hat, (64, 1)))
    for call in stub.calls:
        assert call["rows"] == 64 and np.array_equal(call["replicate"], np.arange(64))
        assert call["seed"] == 1 and call["scheme"] == scheme
    assert out["seed"] == 1 and out["scheme"] == scheme and out["x"].shape == (64, 1)
    assert out["converged"].shape == (64,) and out["n_iter"].shape == (64,) and np.array_equal(out["x_hat"], x_hat)
    assert out["names"] == ["v_sys"] and out["n_replicates"] == 64
    # the condition of the GPU end-to-end test: on a concave quadratic the optimiser converges, within gtol / Lambda_b
    assert out["converged"].all() and out["n_converged"] == 64
    w = wh.weights_of_rows(scheme, 1, np.arange(64), hh.N_STARS)
    mu, lam = wh.closed_form_maximum(cols["v"], cols["verr"], hh.SIGMA, w)
    err = np.abs(out["x"][:, 0] - mu)
    bound = 1e-8 / lam + 1e-12 * np.abs(mu)
    print(scheme, "largest |x_b - mu_b| / bound:", float(np.max(err / bound)), "iterations", int(out["n_iter"].max()))
    assert np.all(err <= bound)
    assert abs(out["std"][0] - float(np.std(mu.astype(np.float64), ddof=1))) <= float(np.max(bound))
    # Exp(1) and Poisson(1) weights have variance 1: on data drawn from the model the ratio is about 1
    # (its own sampling error at B = 64 is 1 / sqrt(2 B) = 9 %)
    assert 0.6 < out["std_ratio"][0] < 1.4
    again = fit.bootstrap(n_replicates=64, scheme=scheme, seed=1, x_hat=x_hat)
    assert again["x"].tobytes() == out["x"].tobytes()


def test_bootstrap_defaults_and_refusals(monkeypatch):
    fit, stub, cols = _stubbed_fit(monkeypatch)
    monkeypatch.setattr(fit, "maximize", lambda **kw: {"x": np.array([2.5])})
    out = fit.bootstrap(n_replicates=8)
    assert np.array_equal(stub.calls[0]["first"], np.full((8, 1), 2.5))       # x_hat defaults to maximize()["x"]
    assert out["scheme"] == "exponential" and 0 <= out["seed"] < 2 ** 63 and stub.calls[0]["seed"] == out["seed"]
    assert "std_ratio" not in out                                # no Laplace covariance: no ratio
    with pytest.raises(ValueError):
        fit.bootstrap(n_replicates=0)
    with pytest.raises(ValueError):
        fit.bootstrap(n_replicates=4, scheme="explicit", x_hat=[0.0])
    with pytest.raises(ValueError):
        fit.bootstrap(n_replicates=4, x_hat=[0.0, 1.0])


def test_binned_fit_raises():
    c = synthetic.make_catalog(120, config=2, background=False)
    data = DataReader({k: c[k] for k in ("ra", "dec", "v", "verr")})
    data.make_radial_bins(synthetic.CENTER_RA_DEG, synthetic.CENTER_DEC_DEG, nstars=40)
    fit = BinnedConstantFit(data)
    with pytest.raises(NotImplementedError, match="un-binned"):
        fit.bootstrap(n_replicates=4)
    with pytest.raises(NotImplementedError, match="un-binned"):
        fit.lnprob_weighted_grad_batch(np.zeros((1, 1)), [0])


# ------------------------------------------------------------------------------------------ 7. resources
def test_no_weighted_kernel_uses_scratch_or_lds():
    with open(os.path.join(ROOT, "profiles", "weighted_resources.json")) as fh:
        rows = json.load(fh)["rows"]
    cells = {(r["model_id"], r["free_centre"], r["scheme"]) for r in rows}
    assert cells == {(m, f, s) for m in range(9) for f in (False, True) for s in ("exponential", "poisson", "explicit")}
    for r in rows:
        # (scalar registers that the mixture families park in vector-register lanes are not memory: sgpr_spill is
        # reported in DESIGN 3.20 and not bounded here)
        assert r["scratch_bytes_per_lane"] == 0 and r["vgpr_spill"] == 0 and r["lds_bytes"] == 0, r


def test_resource_report_is_what_the_compiler_says_today():
    """The committed JSON against a fresh run of tools/weighted_resources.py (hipcc for gfx950; no device needed)."""
    import shutil
    import sys
    if shutil.which("hipcc") is None:
        pytest.skip("no hipcc on this machine")
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import weighted_resources
    with open(os.path.join(ROOT, "profiles", "weighted_resources.json")) as fh:
        committed = json.load(fh)["rows"]
    assert weighted_resources.analyse() == committed

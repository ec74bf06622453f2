"""CPU: the host layer of the bagged posterior (analysis/runner.py: bagged_summary, Runner.bagged,
Runner.lnprob_weighted_batch).

  6. bagged_summary on constructed (B, W, T, P) arrays against NumPy: the pooled moments and percentiles, bag_mean, bag_var,
     within, between, mismatch_ratio, mean_mcse, the burn-in / thin handling, and the warning below 90 % converged bags;
  7. the sizing harness: Runner.bagged's own loop around a NumPy stand-in for lnprob_weighted_batch on the closed-form
     catalogue (200 stars, only v_sys free), where bag b's posterior is exactly N(mu_b, 1 / Lambda_b) under the generator's
     weights.  Fixes the run of tests/test_gpu_bagged.py (weighted_value_helper.N_BAGS ...): every bag keeps 50 tau of
     post-burn-in steps and meets the two bounds of weighted_value_helper.check_bags;
  8. bookkeeping: replicate ids, seed, scheme and bag_fraction as passed to lnprob_weighted_batch, defaults and refusals;
     BinnedConstantFit raises."""
import warnings

import numpy as np
import pytest

import holdout_helper as hh
import weighted_helper as wh
import weighted_value_helper as wv
from mcmc_dynamics_amd import DataReader, synthetic
from mcmc_dynamics_amd.analysis import BinnedConstantFit
from mcmc_dynamics_amd.analysis.runner import BOOTSTRAP_PERCENTILES, bagged_summary


# ------------------------------------------------------------------------------------------ 6. bagged_summary
def _ar1(rng, shape, rho):
    """AR(1) series along axis 2 with unit marginal variance."""
    x = rng.normal(size=shape)
    for t in range(1, shape[2]):
        x[:, :, t] = rho * x[:, :, t - 1] + np.sqrt(1.0 - rho * rho) * x[:, :, t]
    return x


def _chains(b=12, w=8, t=700, p=2, rho=0.5, seed=4):
    """Bags with centres scattered by (0.7, 3.0) around (1, -20) and within-bag widths (1, 0.5); the first 100 steps sit
    far away (a burn-in that would wreck every moment)."""
    rng = np.random.default_rng(seed)
    centre = np.array([1.0, -20.0])[:p] + rng.normal(size=(b, p)) * np.array([0.7, 3.0])[:p]
    chain = centre[:, None, None, :] + _ar1(rng, (b, w, t, p), rho) * np.array([1.0, 0.5])[:p]
    chain[:, :, :100, :] += 1e6
    return chain


def test_summary_against_numpy():
    chain = _chains()
    s = bagged_summary(chain, 100, ["a", "b"])
    kept = chain[:, :, 100:, :]
    draws = kept.reshape(12, -1, 2)
    pooled = draws.reshape(-1, 2)
    assert s["names"] == ["a", "b"] and s["n_bags"] == 12 and s["n_samples"] == 8 * 600
    assert np.allclose(s["mean"], pooled.mean(axis=0), rtol=1e-13, atol=0)
    assert np.allclose(s["covariance"], np.cov(pooled.T, ddof=1), rtol=1e-12, atol=1e-14)
    assert np.allclose(s["std"], pooled.std(axis=0, ddof=1), rtol=1e-12, atol=0)
    assert tuple(sorted(s["percentiles"])) == BOOTSTRAP_PERCENTILES
    for q in BOOTSTRAP_PERCENTILES:
        assert np.array_equal(s["percentiles"][q], np.percentile(pooled, q, axis=0))
    assert s["bag_mean"].shape == s["bag_var"].shape == s["mean_mcse"].shape == (12, 2)
    assert np.allclose(s["bag_mean"], draws.mean(axis=1), rtol=1e-13, atol=0)
    assert np.allclose(s["bag_var"], draws.var(axis=1, ddof=1), rtol=1e-12, atol=0)
    within = np.mean([np.cov(d.T, ddof=1) for d in draws], axis=0)
    between = np.cov(draws.mean(axis=1).T, ddof=1)
    assert np.allclose(s["within"], within, rtol=1e-12, atol=1e-14) and np.allclose(s["between"], between, rtol=1e-12, atol=1e-14)
    assert np.allclose(s["mismatch_ratio"], np.diag(between) / np.diag(within), rtol=1e-12, atol=0)
    # the law of total covariance, in the sample formulas' own factors
    n = draws.shape[1]
    total = ((n - 1) * 12 * within + n * 11 * between) / (12 * n - 1)
    assert np.allclose(s["covariance"], total, rtol=1e-10, atol=1e-12)
    # what was planted: widths (1, 0.5) inside the bags, (0.7, 3.0) between them (B = 12: 1 / sqrt(2 B - 2) = 21 % on a width)
    assert np.allclose(np.sqrt(np.diag(s["within"])), [1.0, 0.5], rtol=0.05)
    assert np.allclose(np.sqrt(np.diag(s["between"])), [0.7, 3.0], rtol=0.6)
    assert s["mismatch_ratio"][1] > 10.0 * s["mismatch_ratio"][0]
    # tau of an AR(1) series is (1 + rho) / (1 - rho) = 3; 600 kept steps are 200 of them
    assert s["tau"].shape == (12,) and s["converged"].shape == (12,) and s["converged"].all() and s["n_converged"] == 12
    assert np.all(s["tau"] > 2.0) and np.all(s["tau"] < 4.5)
    assert np.allclose(s["mean_mcse"], np.sqrt(s["bag_var"] * s["tau"][:, None] / (8 * 600)), rtol=1e-14, atol=0)


@pytest.mark.filterwarnings("ignore:bagged_summary")
def test_burn_in_and_thin():
    chain = _chains()
    s = bagged_summary(chain, 100, ["a", "b"], thin=3)
    kept = chain[:, :, 100::3, :]
    assert s["n_samples"] == 8 * 200
    assert np.allclose(s["mean"], kept.reshape(-1, 2).mean(axis=0), rtol=1e-13, atol=0)
    assert np.allclose(s["bag_mean"], kept.reshape(12, -1, 2).mean(axis=1), rtol=1e-13, atol=0)
    assert np.allclose(s["mean_mcse"], np.sqrt(s["bag_var"] * s["tau"][:, None] / (8 * 200)), rtol=1e-14, atol=0)
    full = bagged_summary(chain, 100, ["a", "b"])
    assert np.all(s["tau"] < full["tau"])                        # tau is counted in KEPT steps
    assert np.all(np.abs(bagged_summary(chain, 0, ["a", "b"])["mean"]) > 1e4)      # the burn-in is in unless cut
    one = bagged_summary(chain[..., :1], 100, ["a"])
    assert one["covariance"].shape == one["within"].shape == one["between"].shape == (1, 1)
    assert np.allclose(one["between"], full["between"][:1, :1], rtol=1e-13)
    single = bagged_summary(chain[:1], 100, ["a", "b"])
    assert np.all(np.isnan(single["between"])) and np.all(np.isnan(single["mismatch_ratio"]))
    for bad in (dict(n_burn=700), dict(n_burn=-1), dict(n_burn=100, thin=0)):
        with pytest.raises(ValueError):
            bagged_summary(chain, names=["a", "b"], **bad)
    with pytest.raises(ValueError):
        bagged_summary(chain, 100, ["a"])
    with pytest.raises(ValueError):
        bagged_summary(chain[0], 100, ["a", "b"])


def test_summary_warns_below_90_percent_converged():
    """rho = 0.9: tau = 19, and 600 kept steps are fewer than 50 tau; rho = 0.5 bags keep 200 tau."""
    fast, slow = _chains(b=10, rho=0.5, seed=5), _chains(b=10, rho=0.9, seed=6)
    mixed = fast.copy()
    mixed[:2] = slow[:2]                                         # 8 of 10 = 80 %
    with pytest.warns(UserWarning, match="8 of 10"):
        s = bagged_summary(mixed, 100, ["a", "b"])
    assert np.array_equal(s["converged"], np.arange(10) >= 2) and s["n_converged"] == 8
    mixed[1] = fast[1]                                           # 9 of 10 = 90 %: not fewer than 90 %
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        s = bagged_summary(mixed, 100, ["a", "b"])
    assert s["n_converged"] == 9


# ------------------------------------------------------------------------------------------ 7. the sizing harness
def _stubbed_fit(monkeypatch):
    cols = hh.closed_form_columns()
    fit = hh.closed_form_fit(cols)
    stub = wv.NumpyWeightedValue(cols, lambda scheme, seed, rep: wh.weights_of_rows(scheme, seed, rep, hh.N_STARS))
    monkeypatch.setattr(fit, "lnprob_weighted_batch", stub)
    return fit, stub, cols


_start = wv.start_positions


@pytest.mark.parametrize("scheme", ["exponential", "poisson"])
def test_closed_form_harness_sizes_the_run(monkeypatch, scheme):
    """Runner.bagged's loop (BinnedSampler, rng="device": the numbers the GPU run takes) around the NumPy stand-in, with the
    run of tests/test_gpu_bagged.py: 16 bags x 64 walkers, 1900 steps of which 300 burn-in, seed 20261021 (1500 steps kept
    only 47 tau in one bag).  Recorded on this run -- exponential: tau 21.1 .. 25.4 (62.9 tau kept at least), largest
    standardised mean error 2.47, variance error 1.39, between / within 1.840 against 1.835 exact; Poisson: tau 21.8 ..
    25.4 (63.0 tau), 1.41, 1.66, 1.082 against 1.092.  (The ratio is not 1: the catalogue holds five planted outliers.)
    The test prints the run's figures."""
    fit, stub, cols = _stubbed_fit(monkeypatch)
    out = fit.bagged(n_bags=wv.N_BAGS, n_walkers=wv.N_WALKERS, n_steps=wv.N_STEPS, n_burn=wv.N_BURN, scheme=scheme,
                     seed=wv.RUN_SEED, pos=_start(cols, wv.N_BAGS, wv.N_WALKERS))
    t_kept = wv.N_STEPS - wv.N_BURN
    assert out["sampler"].chain.shape == (wv.N_BAGS, wv.N_WALKERS, wv.N_STEPS, 1)
    # the condition the bounds rest on: 50 autocorrelation times in every bag
    assert out["converged"].all() and np.all(t_kept >= 50.0 * out["tau"]), out["tau"].tolist()
    w = wh.weights(scheme, wv.RUN_SEED, 0, wv.N_BAGS, 0, hh.N_STARS)
    mu, lam = wv.closed_form_bags(cols, w)
    wv.check_bags(out, mu, lam, "numpy stand-in, " + scheme, wv.N_WALKERS, t_kept)
    # one call per half step with all B W / 2 proposals, bag b's rows under replicate b
    half = wv.N_WALKERS // 2
    steps = [c for c in stub.calls if c["shape"] == (wv.N_BAGS, half, 1)]
    assert len(steps) == 2 * wv.N_STEPS and len(stub.calls) <= len(steps) + 2
    for c in stub.calls:
        assert np.array_equal(c["replicate"], np.repeat(np.arange(wv.N_BAGS), c["shape"][1]))
        assert c["seed"] == wv.RUN_SEED and c["scheme"] == scheme and c["scale"] == 1.0


@pytest.mark.filterwarnings("ignore:bagged_summary")
def test_bag_fraction_scales_the_curvature(monkeypatch):
    fit, stub, cols = _stubbed_fit(monkeypatch)
    out = fit.bagged(n_bags=wv.N_BAGS, n_walkers=wv.N_WALKERS, n_steps=wv.SHORT_STEPS, n_burn=wv.SHORT_BURN, seed=wv.RUN_SEED,
                     pos=_start(cols, wv.N_BAGS, wv.N_WALKERS), bag_fraction=0.5)
    assert out["bag_fraction"] == 0.5 and all(c["scale"] == 0.5 for c in stub.calls)
    w = wh.weights("exponential", wv.RUN_SEED, 0, wv.N_BAGS, 0, hh.N_STARS)
    mu, lam = wv.closed_form_bags(cols, w, bag_fraction=0.5)
    wv.check_bags(out, mu, lam, "numpy stand-in, bag_fraction 0.5", wv.N_WALKERS, wv.SHORT_STEPS - wv.SHORT_BURN)
    # ... and not against the unscaled curvature: twice the variance is far outside the bound
    with pytest.raises(AssertionError):
        wv.check_bags(out, mu, 2.0 * lam, "(expected to miss)", wv.N_WALKERS, wv.SHORT_STEPS - wv.SHORT_BURN)


# ------------------------------------------------------------------------------------------ 8. bookkeeping
@pytest.mark.filterwarnings("ignore:bagged_summary")
def test_bagged_defaults_and_refusals(monkeypatch):
    fit, stub, cols = _stubbed_fit(monkeypatch)
    out = fit.bagged(n_bags=3, n_walkers=8, n_steps=20, n_burn=5, thin=2)
    assert out["scheme"] == "exponential" and out["bag_fraction"] == 1.0 and 0 <= out["seed"] < 2 ** 63
    assert stub.calls[0]["seed"] == out["seed"] and out["names"] == ["v_sys"]
    assert out["sampler"].chain.shape == (3, 8, 20, 1) and out["n_samples"] == 8 * 8 and out["bag_mean"].shape == (3, 1)
    again = fit.bagged(n_bags=3, n_walkers=8, n_steps=20, n_burn=5, seed=out["seed"], pos=out["sampler"].chain[:, :, 0, :])
    assert again["seed"] == out["seed"]
    a = fit.bagged(n_bags=3, n_walkers=8, n_steps=20, n_burn=5, seed=9, pos=_start(cols, 3, 8))
    b = fit.bagged(n_bags=3, n_walkers=8, n_steps=20, n_burn=5, seed=9, pos=_start(cols, 3, 8))
    assert a["sampler"].chain.tobytes() == b["sampler"].chain.tobytes()
    for bad in (dict(n_bags=0), dict(scheme="explicit"), dict(thin=0), dict(n_burn=20), dict(bag_fraction=0.0),
                dict(pos=np.zeros((3, 8, 2))), dict(pos=np.full((3, 8, 1), 1e6))):
        with pytest.raises(ValueError):
            fit.bagged(**dict(dict(n_bags=3, n_walkers=8, n_steps=20, n_burn=5), **bad))


def test_binned_fit_raises():
    c = synthetic.make_catalog(120, config=2, background=False)
    data = DataReader({k: c[k] for k in ("ra", "dec", "v", "verr")})
    data.make_radial_bins(synthetic.CENTER_RA_DEG, synthetic.CENTER_DEC_DEG, nstars=40)
    fit = BinnedConstantFit(data)
    with pytest.raises(NotImplementedError, match="un-binned"):
        fit.bagged(n_bags=4)
    with pytest.raises(NotImplementedError, match="un-binned"):
        fit.lnprob_weighted_batch(np.zeros((1, 1)), [0])

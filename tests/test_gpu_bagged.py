"""GPU: Runner.bagged and Runner.lnprob_weighted_batch end to end on the closed-form fit (ConstantFit on 200 synthetic
stars, only v_sys free: bag b's posterior is exactly N(mu_b, 1 / Lambda_b), tests/weighted_value_helper.py), with the run
fixed by tests/test_bagged_cpu.py::test_closed_form_harness_sizes_the_run.

  * every bag within the two Monte-Carlo bounds of weighted_value_helper.check_bags, against mu_b and Lambda_b from
    mcd_bootstrap_weights(scheme, seed, 0, B, 0, N) -- a wrong row -> replicate map would miss by about one posterior
    sigma, some 70 standard errors; `between` against the closed form's Var(mu_b) within the mean_mcse budget;
  * the same seed gives the same chain bits;
  * the stored lnprobability at a few (b, w, t) equals lnprob_weighted_batch(chain[b, w, t], [b]) within 1e-12 on
    max(|lnp|, N);
  * bag_fraction = 0.5 halves Lambda_b in the same checks on a short run;
  * lnprob_weighted_batch: shapes (..., P) -> (...), -inf outside the prior with a donor row, weight_scale."""
import numpy as np
import pytest

import holdout_helper as hh
import weighted_value_helper as wv

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def fit():
    f = hh.closed_form_fit(hh.closed_form_columns())
    yield f
    f.close()


@pytest.fixture(scope="module")
def cols():
    return hh.closed_form_columns()


_RUNS = {}


def _run(fit, cols, scheme):
    """The fixed run, made once per scheme for the whole module."""
    if scheme not in _RUNS:
        _RUNS[scheme] = fit.bagged(n_bags=wv.N_BAGS, n_walkers=wv.N_WALKERS, n_steps=wv.N_STEPS, n_burn=wv.N_BURN, scheme=scheme,
                                   seed=wv.RUN_SEED, pos=wv.start_positions(cols, wv.N_BAGS, wv.N_WALKERS))
    return _RUNS[scheme]


@pytest.mark.parametrize("scheme", ["exponential", "poisson"])
def test_every_bag_samples_its_own_weighted_posterior(fit, cols, scheme):
    from mcmc_dynamics_amd import _native
    out = _run(fit, cols, scheme)
    t_kept = wv.N_STEPS - wv.N_BURN
    assert out["sampler"].chain.shape == (wv.N_BAGS, wv.N_WALKERS, wv.N_STEPS, 1)
    assert out["seed"] == wv.RUN_SEED and out["scheme"] == scheme and out["bag_fraction"] == 1.0 and out["names"] == ["v_sys"]
    assert out["converged"].all() and np.all(t_kept >= 50.0 * out["tau"]), out["tau"].tolist()
    w = _native.bootstrap_weights(scheme, wv.RUN_SEED, 0, wv.N_BAGS, 0, hh.N_STARS)
    mu, lam = wv.closed_form_bags(cols, w)
    wv.check_bags(out, mu, lam, "device, " + scheme, wv.N_WALKERS, t_kept)
    # the bound tells the bags apart: against the NEXT bag's closed form the means miss
    with pytest.raises(AssertionError):
        wv.check_bags(out, np.roll(mu, 1), np.roll(lam, 1), "(expected to miss: bag b against replicate b - 1)", wv.N_WALKERS, t_kept)
    # the pooled moments are those of the draws
    draws = out["sampler"].chain[:, :, wv.N_BURN:, 0]
    assert np.allclose(out["mean"][0], draws.mean(), rtol=1e-13) and np.allclose(out["std"][0], draws.std(ddof=1), rtol=1e-12)


@pytest.mark.parametrize("scheme", ["exponential", "poisson"])
def test_stored_lnprobability_is_the_weighted_posterior_of_the_stored_position(fit, cols, scheme):
    out = _run(fit, cols, scheme)
    chain, lnp = out["sampler"].chain, out["sampler"].lnprobability
    assert lnp.shape == (wv.N_BAGS, wv.N_WALKERS, wv.N_STEPS)
    for b, w, t in ((0, 0, 0), (3, 17, 1), (7, 63, 299), (15, 31, wv.N_STEPS - 1), (9, 40, 1000)):
        got = fit.lnprob_weighted_batch(chain[b, w, t], [b], scheme=scheme, seed=wv.RUN_SEED)
        assert got.shape == ()
        assert abs(float(got) - lnp[b, w, t]) <= 1e-12 * max(abs(lnp[b, w, t]), hh.N_STARS), (b, w, t, float(got), lnp[b, w, t])
        other = fit.lnprob_weighted_batch(chain[b, w, t], [b + 1], scheme=scheme, seed=wv.RUN_SEED)
        assert abs(float(other) - lnp[b, w, t]) > 1e-6 * abs(lnp[b, w, t])


def test_the_same_seed_gives_the_same_chain_bits_and_bag_fraction_halves_the_curvature(fit, cols):
    from mcmc_dynamics_amd import _native
    kw = dict(n_bags=wv.N_BAGS, n_walkers=wv.N_WALKERS, n_steps=wv.SHORT_STEPS, n_burn=wv.SHORT_BURN, seed=wv.RUN_SEED,
              pos=wv.start_positions(cols, wv.N_BAGS, wv.N_WALKERS))
    # the first SHORT_STEPS steps of the fixed run again: the chain is a function of the seed and the start
    full = _run(fit, cols, "exponential")["sampler"]
    again = fit.bagged(**kw)["sampler"]
    assert again.chain.tobytes() == np.ascontiguousarray(full.chain[:, :, :wv.SHORT_STEPS]).tobytes()
    assert again.lnprobability.tobytes() == np.ascontiguousarray(full.lnprobability[:, :, :wv.SHORT_STEPS]).tobytes()
    other = fit.bagged(**dict(kw, seed=wv.RUN_SEED + 1, n_steps=20, n_burn=5))["sampler"]
    assert not np.array_equal(other.chain[:, :, 19], full.chain[:, :, 19])
    half = fit.bagged(bag_fraction=0.5, **kw)
    assert half["bag_fraction"] == 0.5
    w = _native.bootstrap_weights("exponential", wv.RUN_SEED, 0, wv.N_BAGS, 0, hh.N_STARS)
    mu, lam = wv.closed_form_bags(cols, w, bag_fraction=0.5)
    t_kept = wv.SHORT_STEPS - wv.SHORT_BURN
    wv.check_bags(half, mu, lam, "device, bag_fraction 0.5", wv.N_WALKERS, t_kept)
    with pytest.raises(AssertionError):
        wv.check_bags(half, mu, 2.0 * lam, "(expected to miss: the unscaled curvature)", wv.N_WALKERS, t_kept)


def test_lnprob_weighted_batch_shapes_prior_and_scale(fit, cols):
    from mcmc_dynamics_amd import _native
    rng = np.random.default_rng(8)
    values = hh.V_SYS + rng.normal(size=(3, 5, 1))
    rep = np.repeat(np.arange(3), 5)
    got = fit.lnprob_weighted_batch(values, rep, scheme="poisson", seed=4)
    assert got.shape == (3, 5) and np.all(np.isfinite(got))
    # against the device's own weighted value through the gradient kernel, and NumPy on the generator's weights
    v_grad, _ = fit.lnprob_weighted_grad_batch(values.reshape(-1, 1), rep, scheme="poisson", seed=4)
    assert np.all(np.abs(got.reshape(-1) - v_grad) <= 1e-12 * np.maximum(np.abs(v_grad), hh.N_STARS))
    stand_in = wv.NumpyWeightedValue(cols, lambda scheme, seed, r: np.stack(
        [_native.bootstrap_weights(scheme, seed, int(b), 1, 0, hh.N_STARS)[0] for b in r]))
    want = stand_in(values, rep, scheme="poisson", seed=4)
    prior = got - want                                           # the flat box's constant
    assert np.all(np.abs(prior - prior.flat[0]) <= 1e-10 * np.abs(want))
    # rows outside the box are -inf and leave the others as they were (the donor row stands in for them in the launch)
    outside = values.copy()
    outside[1, 2, 0] = 5000.0
    outside[0, 0, 0] = -5000.0
    masked = fit.lnprob_weighted_batch(outside, rep, scheme="poisson", seed=4)
    bad = np.zeros((3, 5), dtype=bool)
    bad[1, 2] = bad[0, 0] = True
    assert np.all(masked[bad] == -np.inf) and np.array_equal(masked[~bad], got[~bad])
    assert np.all(fit.lnprob_weighted_batch(np.full((2, 1), 5000.0), [0, 1]) == -np.inf)
    # weight_scale multiplies the likelihood and not the prior
    scaled = fit.lnprob_weighted_batch(values, rep, scheme="poisson", seed=4, weight_scale=0.5)
    assert np.all(np.abs(scaled - (0.5 * (got - prior.flat[0]) + prior.flat[0])) <= 1e-12 * np.abs(got))
    # explicit weights
    w = _native.bootstrap_weights("poisson", 4, 0, 3, 0, hh.N_STARS)
    explicit = fit.lnprob_weighted_batch(values, rep, scheme="explicit", weights=w)
    assert explicit.tobytes() == got.tobytes()
    with pytest.raises(ValueError):
        fit.lnprob_weighted_batch(values, rep[:-1])
    with pytest.raises(ValueError):
        fit.lnprob_weighted_batch(np.zeros((4, 2)), np.zeros(4))

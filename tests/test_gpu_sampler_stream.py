"""GPU: the layer users call -- ``Runner.__call__`` / ``BinnedConstantFit.__call__`` and the samplers they return -- held
to its random stream and, for the float32 precisions, to the float64 kernels.

* ``reset()`` between a burn-in and a production run continues the device generator's stream (resident blocks and
  host-driven ones), bit for bit the rows an uninterrupted run stores;
* a float32 chain is not lost to a proposal outside the float32 accuracy domain, reports it, and what it stores is as close
  to the float64 kernels as include/mcd.h states; library blocks equal the NumPy loop bit for bit.

The catalogue (tests/stream_helper.py): 257 stars, 16 walkers, at most 24 steps."""
import warnings

import numpy as np
import pytest

import stream_helper as sh

pytestmark = pytest.mark.gpu

TOL_INSIDE = {"f32acc64": 1e-6, "f32": 2e-5}                 # include/mcd.h, fixed centre, on the scale max(|lnL|, N, 32)
STEPS = 24


def _domain_warnings(caught):
    return [w for w in caught if issubclass(w.category, UserWarning) and "float32 accuracy domain" in str(w.message)]


def _run(fit, n_steps, pos, seed):
    """``fit(...)`` with the sampler's 64-bit name fixed: the un-binned Runner takes it from NumPy's global generator."""
    if hasattr(fit, "n_bins"):
        return fit(n_walkers=sh.W, n_steps=n_steps, pos=pos, seed=seed)
    np.random.seed(seed)
    return fit(n_walkers=sh.W, n_steps=n_steps, pos=pos, prefix=None)


def _rows(sampler):
    return sampler._chain[:sampler.iteration].copy(), sampler._lnprob[:sampler.iteration].copy()


@pytest.mark.parametrize("binned", [False, True], ids=["ConstantFit", "BinnedConstantFit"])
def test_reset_continues_the_resident_chain(binned):
    fit = sh.make_fit(binned=binned)
    pos = np.stack([sh.walkers(seed=30 + b) for b in range(3)]) if binned else sh.walkers()
    full = _run(fit, 12, pos, seed=99)
    assert full.rng == "device" and full.seeded_block_fn is not None
    chain12, lnp12 = _rows(full)
    assert chain12.shape == (12,) + pos.shape and np.all(np.isfinite(lnp12))
    assert np.unique(chain12.reshape(12, -1), axis=0).shape[0] == 12                  # the ensemble moves at every step
    cat = fit._catalog
    info0 = cat.stretch_info()
    assert info0["device_blocks"] >= 1 and info0["discarded_blocks"] == 0, info0

    sampler = _run(fit, 5, pos, seed=99)
    assert sampler.seed64 == full.seed64 and np.array_equal(_rows(sampler)[0], chain12[:5])
    last, accepted5 = sampler.get_chain()[-1].copy(), sampler._accepted.copy()
    sampler.reset()
    assert sampler.iteration == 0
    sampler.run_mcmc(last, 7)
    assert np.array_equal(sampler.get_chain(), chain12[5:12])          # (a rewound generator gives rows 0 .. 6 again)
    assert sampler.iteration == 7 and sampler.rng_step == 12 and full.rng_step == 12
    assert np.array_equal(_rows(sampler)[1], lnp12[5:12])
    assert np.array_equal(sampler._accepted, full._accepted - accepted5)
    info1 = fit._catalog.stretch_info()
    assert fit._catalog is cat and info1["device_blocks"] == info0["device_blocks"] + 2, (info0, info1)
    assert info1["discarded_blocks"] == 0 and info1["host_blocks"] == info0["host_blocks"], (info0, info1)

    # the same chain from host-driven blocks
    cat.set_option("device_chain", 0)
    host = _run(fit, 5, pos, seed=99)
    last = host.get_chain()[-1].copy()
    host.reset()
    host.run_mcmc(last, 7)
    info2 = cat.stretch_info()
    assert info2["device_blocks"] == info1["device_blocks"] and info2["host_blocks"] == info1["host_blocks"] + 2, info2
    assert np.array_equal(host.get_chain(), chain12[5:12]) and np.array_equal(_rows(host)[1], lnp12[5:12])
    for s in (full, sampler, host):
        if binned:
            s.close()
    fit.close()


@pytest.fixture(scope="module")
def f64_lnprob():
    """``lnprob_batch`` of a float64 Runner on the same data, one Runner per configuration: (n, 4) -> (n,)."""
    fits = {}

    def evaluate(config, background, positions):
        key = (config, background)
        if key not in fits:
            fits[key] = sh.make_fit(config, background=background)
        return fits[key].lnprob_batch(positions)
    yield evaluate
    for fit in fits.values():
        fit.close()


def _chain_error(sampler, want_fn):
    """Worst |stored float32 log-probability - float64 kernels at the stored position| over every (walker, step), on the
    scale of csrc/mcd_guard.h: max(|lnL|, N, 32)."""
    chain, got = _rows(sampler)
    want = want_fn(chain.reshape(-1, 4)).reshape(got.shape)
    assert np.all(np.isfinite(want)) and np.all(np.isfinite(got))
    return float(np.max(np.abs(got - want) / np.maximum(np.abs(want), max(sh.N, 32))))


@pytest.mark.parametrize("background", [False, True], ids=["model 0", "model 1 (Gaussian background)"])
@pytest.mark.parametrize("precision", ["f32", "f32acc64"])
def test_float32_chain_inside_the_domain(precision, background, f64_lnprob):
    """Every table of this run is inside the float32 accuracy domain (tests/test_sampler_stream_cpu.py): nothing is
    counted, nothing is warned about, and the stored log-probabilities keep the stated tolerance."""
    fit = sh.make_fit("inside", background=background, precision=precision)
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        sampler = _run(fit, STEPS, sh.walkers("inside"), seed=7)
    assert not _domain_warnings(caught)
    out = fit.f32_outside()
    assert out["calls"] == 0 and out["reason"] == "" and 0.0 < out["worst_kappa_v"] <= 85.0, out
    assert sampler.iteration == STEPS and 0.1 < sampler.acceptance_fraction.mean() < 0.95
    err = _chain_error(sampler, lambda x: f64_lnprob("inside", background, x))
    print("float32 chain inside: precision={0} background={1} worst error {2:.3e} (tolerance {3:.0e})".format(
        precision, background, err, TOL_INSIDE[precision]))
    assert err <= TOL_INSIDE[precision], err
    fit.close()


@pytest.mark.parametrize("background", [False, True], ids=["model 0", "model 1 (Gaussian background)"])
@pytest.mark.parametrize("precision", ["f32", "f32acc64"])
def test_float32_chain_that_leaves_the_domain_finishes_and_tells(precision, background, f64_lnprob):
    """Stars at +300 km/s: kappa_v crosses 96 whenever a walker of a table has sigma below about 6.6 km/s.  The chain
    completes, the Runner warns once, the counters tell, and the stored log-probabilities stay within the bound that the
    model of csrc/mcd_guard.h gives outside the domain: the residual's rounding enters through (d / sqrt n)^2, quadratically
    in kappa_v, so tol_inside * max(1, worst_kappa_v / 96)^2."""
    fit = sh.make_fit("outside", background=background, precision=precision)
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        sampler = _run(fit, STEPS, sh.walkers("outside"), seed=7)
        fit.lnprob_batch(sampler.get_chain()[-1])
    found = _domain_warnings(caught)
    assert len(found) == 1, [str(w.message) for w in caught]
    assert "exceeds 96" in str(found[0].message) and "kappa_v" in str(found[0].message)
    out = fit.f32_outside()
    assert out["calls"] > 0 and out["worst_kappa_v"] > 96.0 and "exceeds 96" in out["reason"], out
    assert out["calls"] < 2 * STEPS + 2                                        # ... and some tables were inside
    assert out == fit._catalog.f32_outside() and fit._catalog.f32_in_domain == (fit._catalog.f32_condition[0] <= 96.0)
    assert sampler.iteration == STEPS and 0.1 < sampler.acceptance_fraction.mean() < 0.95
    err = _chain_error(sampler, lambda x: f64_lnprob("outside", background, x))
    bound = TOL_INSIDE[precision] * max(1.0, out["worst_kappa_v"] / 96.0) ** 2
    print("float32 chain outside: precision={0} background={1} worst error {2:.3e} (bound {3:.3e}, worst kappa_v {4:.1f}, "
          "{5} tables outside)".format(precision, background, err, bound, out["worst_kappa_v"], out["calls"]))
    assert err <= bound, (err, bound)
    fit.close()


@pytest.mark.parametrize("config", ["inside", "outside"])
@pytest.mark.parametrize("precision", ["f32", "f32acc64"])
def test_float32_library_blocks_equal_the_numpy_loop(precision, config):
    """As tests/test_gpu_runner.py::test_library_stretch_move_equals_the_python_loop holds float64: the float32 chain driven
    through library blocks (host-driven: the resident chain is float64) is the chain of the NumPy loop around
    ``lnprob_batch``, bit for bit."""
    from mcmc_dynamics_amd.sampler import EnsembleSampler
    fit = sh.make_fit(config, background=True, precision=precision)
    pos = sh.walkers(config)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", UserWarning)
        native = fit._make_sampler(sh.W, seed=2 ** 40 + 5)
        assert native.seeded_block_fn is not None and native.rng == "device" and native.seed64 == 2 ** 40 + 5
        native.block_steps = 16
        native.run_mcmc(pos, STEPS)                              # a 16-step block and an 8-step block
        info = fit._catalog.stretch_info()
        assert info["host_blocks"] == 2 and info["device_blocks"] == 0, info
        python = EnsembleSampler(sh.W, 4, fit.lnprob_batch, vectorize=True, seed=2 ** 40 + 5, rng="device")
        python.block_steps = 7
        python.run_mcmc(pos, STEPS)
    assert np.array_equal(native.chain, python.chain) and np.array_equal(native.lnprobability, python.lnprobability)
    assert np.array_equal(native.acceptance_fraction, python.acceptance_fraction) and native.n_calls == python.n_calls
    assert 0.1 < native.acceptance_fraction.mean() < 0.95 and np.all(np.isfinite(native.lnprobability))
    fit.close()

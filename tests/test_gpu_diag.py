"""GPU: mcd_chain_diagnostics on the device (csrc/mcd_diag.hip) -- bit-identical to the library's host loop (``ctx = NULL``,
the same header: csrc/mcd_diag.h) whatever the shape and the tile plan, the AR(1) known answer, and the samplers'
``get_autocorr_time`` end to end.  What the host loop itself is held to: tests/test_diag_cpu.py."""
import functools

import numpy as np
import pytest

import diag_helper as dh
from mcmc_dynamics_amd import _native, diagnostics

pytestmark = pytest.mark.gpu
KEYS = ("tau", "window", "found", "rhat", "mean", "var", "rho")
SHAPES = [(1, 1, 1), (1, 5, 11), (3, 5, 11), (3, 66, 4)]


@pytest.fixture(scope="module")
def ctx():
    return _native.default_context()


@functools.lru_cache(maxsize=None)
def _chain(T, shape):
    G, W, P = shape
    x = dh.ar1(np.random.default_rng(T + 7 * G + 11 * W + 13 * P), 0.8, shape, T) + (1.0 + np.arange(P))
    if P >= 3:
        x[..., 2] = 56.345 + 1e-8 * x[..., 2]
    x = np.ascontiguousarray(x)
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def _host(T, shape, L):
    return _native.chain_diagnostics(_chain(T, shape), L, context=None, want_rho=True)


def _same(a, b, keys=KEYS):
    return all(np.array_equal(a[k], b[k], equal_nan=True) for k in keys)


@pytest.mark.parametrize("T", [17, 257, 1000])
@pytest.mark.parametrize("shape", SHAPES)
def test_device_equals_host_bit_for_bit(ctx, T, shape):
    x = _chain(T, shape)
    lags = sorted({L for L in (1, 16, 17, T - 1) if L <= T - 1})                  # (T = 17: max_lag = 17 is refused, below)
    for L in lags:
        got = _native.chain_diagnostics(x, L, context=ctx, want_rho=True)
        info = _native.chain_diagnostics_info()                                  # (of this thread's LAST call: before the host's)
        assert _same(got, _host(T, shape, L)), (T, shape, L)
        assert info["n_tiles"] == 1 and info["tile_groups"] == shape[0] and info["kernel_ms"] > 0.0
    again = _native.chain_diagnostics(x, 16, context=ctx, want_rho=True)          # repeated call, and without rho
    assert _same(again, _host(T, shape, 16))
    assert _same(_native.chain_diagnostics(x, 16, context=ctx), _host(T, shape, 16), KEYS[:-1])
    if T == 17:
        with pytest.raises(_native.NativeError, match="max_lag = 17 is outside"):
            _native.chain_diagnostics(x, 17, context=ctx)


def test_group_tiles_change_no_bit(ctx):
    """(3, 66, 4) x 1000 steps, L = 17: a group needs 2.05 MiB of scratch (its series 2.01), so 3 MiB hold one group per
    tile -- three tiles -- and 5 MiB two -- tiles of two groups and one."""
    T, shape, L = 1000, (3, 66, 4), 17
    x, want = _chain(T, shape), _host(T, shape, 17)
    for mb, groups, tiles in ((3, 1, 3), (5, 2, 2), (7, 3, 1)):
        assert dh.tile_groups(T, 3, 66, 4, L, mb << 20) == groups
        got = _native.chain_diagnostics(x, L, context=ctx, scratch_mb=mb, want_rho=True)
        info = _native.chain_diagnostics_info()
        assert (info["tile_groups"], info["n_tiles"]) == (groups, tiles)
        assert _same(got, want), mb
    # a budget below one group is refused, with a message, and nothing is written
    with pytest.raises(_native.NativeError, match="scratch_mb = 2 cannot hold one group"):
        _native.chain_diagnostics(x, L, context=ctx, scratch_mb=2)
    with pytest.raises(_native.NativeError, match="scratch_mb = 1 cannot hold one group"):
        _native.chain_diagnostics(x, L, context=ctx, scratch_mb=1)
    with pytest.raises(_native.NativeError, match="max_lag"):
        _native.chain_diagnostics(x, T, context=ctx)


def test_ar1_known_answer_on_the_device(ctx):
    x = dh.ar1(np.random.default_rng(2024), 0.9, (1, 64, 1), 20000)
    out = _native.chain_diagnostics(x, 2000, context=ctx)
    assert out["found"][0, 0] == 1 and abs(out["tau"][0, 0] - 19.0) < 1.9 and out["window"][0, 0] < 200
    assert _same(out, _native.chain_diagnostics(x, 2000, context=None), KEYS[:-1])
    short = dh.ar1(np.random.default_rng(7), 0.99, (16, 1), 4000)
    with pytest.raises(diagnostics.AutocorrError):
        diagnostics.integrated_time(short, context=ctx)


def _synthetic_reader(n, bins=0):
    from mcmc_dynamics_amd import DataReader, synthetic
    cat = synthetic.make_catalog(n, config=3)
    cols = {k: cat[k] for k in ("ra", "dec", "v", "verr")}
    if bins:
        cols["bin"] = (np.arange(n) * bins // n).astype(np.int16)
    return DataReader(cols)


def _fix_centre(fit):
    from mcmc_dynamics_amd import synthetic
    fit.parameters["ra_center"].set(value=synthetic.CENTER_RA_DEG, fixed=True)
    fit.parameters["dec_center"].set(value=synthetic.CENTER_DEC_DEG, fixed=True)


def test_constant_fit_end_to_end():
    from mcmc_dynamics_amd.analysis import ConstantFit
    fit = ConstantFit(_synthetic_reader(2000))
    _fix_centre(fit)
    sampler = fit(n_walkers=64, n_steps=600, n_out=None, prefix=None)
    with pytest.warns(UserWarning):                                              # 500 steps are not 50 tau
        tau = sampler.get_autocorr_time(discard=100, quiet=True)
    assert tau.shape == (fit.n_fitted_parameters,) and np.all(np.isfinite(tau)) and np.all(tau > 0)
    with pytest.warns(UserWarning):
        assert np.array_equal(tau, diagnostics.integrated_time(sampler.get_chain(discard=100), quiet=True))
    out = fit.chain_diagnostics(sampler.chain, n_burn=100)
    assert np.array_equal(out["tau"], tau) and out["names"] == fit.fitted_parameters and np.all(out["rhat"] < 1.5)
    fit.close()


def test_binned_fit_end_to_end():
    from mcmc_dynamics_amd.analysis import BinnedConstantFit
    fit = BinnedConstantFit(_synthetic_reader(2000, bins=3))
    _fix_centre(fit)
    sampler = fit(n_walkers=64, n_steps=600, seed=5)
    with pytest.warns(UserWarning):
        tau = sampler.get_autocorr_time(discard=100, quiet=True)
    assert tau.shape == (3, fit.n_fitted_parameters) and np.all(np.isfinite(tau)) and np.all(tau > 0)
    with pytest.warns(UserWarning):
        assert np.array_equal(tau, diagnostics.integrated_time(sampler.get_chain(discard=100), quiet=True))
    assert np.array_equal(fit.chain_diagnostics(sampler.chain, n_burn=100)["tau"], tau)
    fit.close()

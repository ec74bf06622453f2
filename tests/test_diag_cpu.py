"""CPU: the chain convergence diagnostics (``mcd_chain_diagnostics``, csrc/mcd_diag.h) -- integrated autocorrelation time,
split-R-hat, pooled moments -- through the library's host loop (``ctx = NULL``: no GPU) and through the CPU build of the
header (tests/emul/diag_emul.cpp), against the longdouble oracle of tests/diag_helper.py; then the Python layers on top:
``diagnostics.integrated_time`` / ``summary``, the samplers' ``get_autocorr_time``, ``Runner.chain_diagnostics`` and
``Runner.run_converged``.

Bounds.  |rho - rho_exact| <= 8 T 2^-53 per lag: a_k is a sequential fma chain of at most T terms whose absolute values
sum to at most a_0 (Cauchy-Schwarz), so its error is at most T 2^-53 a_0; the same for a_0; the quotient, the centring
(two subtractions per sample) and the walkers' mean add a few units more: 8 T 2^-53 has headroom.  tau sums window + 1
such terms twice.  rhat, mean and var: 1e-12 relative."""
import ctypes
import warnings

import numpy as np
import pytest

import diag_helper as dh
from mcmc_dynamics_amd import _native, diagnostics

C = 5.0
KEYS = ("tau", "window", "found", "rhat", "mean", "var", "rho")


def _chain(seed, T, G, W, P):
    """AR(1) series (phi = 0.7) around distinct means; from three parameters on, column 2 sits at 56.345 with a width of
    1e-8 (mean / sigma ~ 1e9: a free centre coordinate)."""
    rng = np.random.default_rng(seed)
    x = dh.ar1(rng, 0.7, (G, W, P), T) + (1.0 + np.arange(P))
    if P >= 3:
        x[..., 2] = 56.345 + 1e-8 * (x[..., 2] - 3.0)
    return np.ascontiguousarray(x)


def _same(a, b):
    return all(np.array_equal(a[k], b[k], equal_nan=True) for k in KEYS)


def _check(got, want, T, what):
    bound = 8 * T * dh.EPS
    assert want["margin"].min() > 1e-6, (what, want["margin"].min())
    err = np.abs(got["rho"] - want["rho"]).astype(np.float64)
    print(what, "max rho error / bound", err.max() / bound)
    assert err.max() <= bound, (what, err.max(), bound)
    assert np.array_equal(got["window"], want["window"]) and np.array_equal(got["found"], want["found"]), what
    assert np.all(np.abs(got["tau"] - want["tau"]).astype(np.float64) <= 2 * (want["window"] + 1) * bound), what
    for k in ("rhat", "mean", "var"):
        w = want[k].astype(np.float64)
        assert np.array_equal(np.isnan(got[k]), np.isnan(w)), (what, k)
        ok = ~np.isnan(w)
        assert np.all(np.abs(got[k][ok] - want[k][ok]).astype(np.float64) <= 1e-12 * np.abs(w[ok])), (what, k)


@pytest.mark.parametrize("T", [2, 3, 17, 257])
@pytest.mark.parametrize("G,W,P", [(g, w, p) for g in (1, 3) for w in (1, 2, 5) for p in (1, 3, 11)])
def test_against_the_longdouble_oracle(T, G, W, P):
    x = _chain(1000 * T + 100 * G + 10 * W + P, T, G, W, P)
    for L in sorted({L for L in (1, 15, 16, 17, T - 1) if 1 <= L <= T - 1}):
        want = dh.exact(x, L, C)
        got = _native.chain_diagnostics(x, L, c=C, context=None, want_rho=True)
        _check(got, want, T, (T, G, W, P, L))
        assert _same(got, dh.emul(x, L, C)), "library host loop and CPU build of the header differ"
        if T >= 4:
            assert np.all(np.isfinite(got["rhat"]))
        else:
            assert np.all(np.isnan(got["rhat"]))
        # without rho the host loop stops at the window: same numbers
        short = _native.chain_diagnostics(x, L, c=C, context=None)
        assert all(np.array_equal(short[k], got[k], equal_nan=True) for k in KEYS[:-1])


def test_group_tiles_change_no_bit():
    x = _chain(7, 257, 3, 5, 11)
    whole = dh.emul(x, 17, C)
    for tiles in ([(0, 1), (1, 1), (2, 1)], [(0, 2), (2, 1)], [(2, 1), (0, 2)]):
        assert _same(whole, dh.emul(x, 17, C, tiles=tiles))
    # the plan: whole groups within the budget; 0 when not even one fits
    per_group = 8 * (5 * 11 * (257 + 18 + 7) + 11 * 18)
    assert dh.tile_groups(257, 3, 5, 11, 17, 3 * per_group) == 3
    assert dh.tile_groups(257, 3, 5, 11, 17, 3 * per_group - 1) == 2
    assert dh.tile_groups(257, 3, 5, 11, 17, per_group - 1) == 0
    assert dh.tile_groups(257, 3, 5, 11, 17, 1 << 40) == 3


def test_the_lag_walk_in_blocks_equals_the_plain_sums():
    """a_k of the 16-lag ring walk against longdouble direct sums, at lengths around the block size."""
    rng = np.random.default_rng(3)
    for T in (2, 15, 16, 17, 31, 32, 33, 100):
        x = rng.standard_normal(T) + 3.0
        a = dh.emul_lag_sums(x, T - 1)
        d = np.asarray(x, dtype=dh.LD) - x[0]
        y = d - d.mean()
        want = np.array([(y[:T - k] * y[k:]).sum() for k in range(T)])
        assert np.all(np.abs(a - want).astype(np.float64) <= T * dh.EPS * float((y * y).sum()) * 2)


def test_ill_conditioned_column():
    """56.345 + 1e-8 AR(1): the header's shifted centring meets the bound; centring on the float64 mean does not."""
    T, L = 1000, 100
    rng = np.random.default_rng(11)
    x = (56.345 + 1e-8 * dh.ar1(rng, 0.9, (1, 4, 1), T))
    want = dh.exact(x, L, C)
    got = _native.chain_diagnostics(x, L, c=C, context=None, want_rho=True)
    _check(got, want, T, "conditioning")
    y = x - x.mean(axis=0)                                               # float64, naive
    a = np.array([(y[:T - k] * y[k:]).sum(axis=0) for k in range(L + 1)])
    naive = np.moveaxis((a / a[0]).mean(axis=2), 0, -1)
    naive_err = np.abs(naive - want["rho"]).astype(np.float64).max()
    print("naive centring error", naive_err, "bound", 8 * T * dh.EPS)
    assert naive_err > 100 * 8 * T * dh.EPS


def test_fft_form_agrees_with_the_direct_sums():
    x = _chain(5, 257, 1, 5, 2)
    got = _native.chain_diagnostics(x, 256, c=C, context=None, want_rho=True)
    assert np.max(np.abs(dh.fft_rho(x, 256) - got["rho"])) < 1e-13
    # emcee's all-lags estimate equals the windowed one wherever a window was found
    found = got["found"] == 1
    assert found.all() and np.allclose(dh.fft_tau(x, C)[found], got["tau"][found], rtol=0, atol=1e-12)


def test_degenerate_inputs():
    x = _chain(9, 64, 2, 3, 2)
    flat = x.copy()
    flat[:, 0, :, 1] = 2.5                                               # every walker of (0, 1) constant
    flat[:, 1, 1, 0] = flat[0, 1, 1, 0]                                  # one constant walker among moving ones in (1, 0)
    got = _native.chain_diagnostics(flat, 6, c=C, context=None, want_rho=True)
    want = dh.exact(flat, 6, C)
    for g, p in ((0, 1), (1, 0)):
        assert np.isnan(got["tau"][g, p]) and np.isnan(got["rhat"][g, p]) and got["found"][g, p] == 0
        assert got["window"][g, p] == 6 and np.all(np.isnan(got["rho"][g, p]))
    assert got["mean"][0, 1] == 2.5 and got["var"][0, 1] == 0.0
    for g, p in ((0, 0), (1, 1)):                                         # the neighbours are untouched
        assert got["found"][g, p] == want["found"][g, p] and np.isfinite(got["tau"][g, p]) and np.isfinite(got["rhat"][g, p])
    assert np.array_equal(np.isnan(got["rhat"]), np.isnan(want["rhat"].astype(np.float64)))
    for T in (2, 3):
        out = _native.chain_diagnostics(_chain(T, T, 1, 2, 2), 1, c=C, context=None)
        assert np.all(np.isnan(out["rhat"])) and np.all(np.isfinite(out["tau"]))


def test_refusals():
    x = _chain(2, 17, 1, 2, 2)
    for kwargs, word in (({"max_lag": 0}, "max_lag"), ({"max_lag": 17}, "max_lag"), ({"max_lag": 3, "c": 0.0}, "c must"),
                         ({"max_lag": 3, "c": -1.0}, "c must"), ({"max_lag": 3, "c": float("nan")}, "c must")):
        with pytest.raises(_native.NativeError, match=word):
            _native.chain_diagnostics(x, context=None, **kwargs)
    with pytest.raises(_native.NativeError, match="n_steps"):
        _native.chain_diagnostics(x[:1], 1, context=None)
    lib = _native.load_library()
    outs = [np.empty(2) for _ in range(6)]
    window, found = np.empty(2, dtype=np.int64), np.empty(2, dtype=np.int32)

    def call(desc, null=None, chain=x):
        ptr = [_native._ptr(outs[0]), window.ctypes.data_as(_native._c_int64_p),
               found.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))] + [_native._ptr(o) for o in outs[1:4]] + [None]
        if null is not None:
            ptr[null] = None
        return lib.mcd_chain_diagnostics(None, ctypes.byref(desc) if desc is not None else None,
                                         _native._ptr(chain) if chain is not None else None, *ptr)

    good = lambda: _native.DiagDesc(17, 1, 2, 2, 3, 5.0, 0)
    assert call(good()) == 0
    for field in ("n_groups", "n_walkers", "n_dim"):
        for bad in (0, -1):
            d = good()
            setattr(d, field, bad)
            assert call(d) == -1 and b"must be >= 1" in lib.mcd_last_error()
    d = good()
    d.n_steps = 1
    assert call(d) == -1 and b"n_steps" in lib.mcd_last_error()
    for null in range(6):                                                # every output but rho
        before = [o.copy() for o in outs]
        assert call(good(), null=null) == -1 and b"NULL" in lib.mcd_last_error()
        assert all(np.array_equal(a, b, equal_nan=True) for a, b in zip(before, outs))
    assert call(None) == -1 and call(good(), chain=None) == -1


def test_ar1_known_answer():
    """AR(1), phi = 0.9: tau = (1 + phi) / (1 - phi) = 19.  W = 64, T = 20 000, L = T / 10."""
    x = dh.ar1(np.random.default_rng(2024), 0.9, (1, 64, 1), 20000)
    out = _native.chain_diagnostics(x, 2000, c=C, context=None)
    print("tau", out["tau"], "window", out["window"])
    assert out["found"][0, 0] == 1 and abs(out["tau"][0, 0] - 19.0) < 1.9 and out["window"][0, 0] < 200
    assert abs(out["rhat"][0, 0] - 1.0) < 0.01 and abs(out["var"][0, 0] - 1.0) < 0.05
    s = diagnostics.summary(x[:, 0], context=None)
    assert s["converged"][0] and abs(s["ess"][0] - 64 * 20000 / out["tau"][0, 0]) < 1e-6 and s["n_steps"] == 20000
    assert s["tau"].shape == (1,) and s["found"][0] and abs(s["std"][0] - 1.0) < 0.03


def test_too_short_chain_raises_or_warns():
    """phi = 0.99 (tau = 199), W = 16, T = 4 000: no window up to L = T / 10."""
    x = dh.ar1(np.random.default_rng(7), 0.99, (16, 1), 4000)
    raw = _native.chain_diagnostics(x[:, None], 400, c=C, context=None)
    assert raw["found"][0, 0] == 0 and raw["window"][0, 0] == 400
    with pytest.raises(diagnostics.AutocorrError) as info:
        diagnostics.integrated_time(x, context=None)
    assert info.value.tau.shape == (1,) and info.value.tau[0] == raw["tau"][0, 0]
    with pytest.warns(UserWarning, match="too short"):
        tau = diagnostics.integrated_time(x, quiet=True, context=None)
    assert tau[0] == raw["tau"][0, 0]
    # tol = 0 switches the LENGTH test off, not the missing window
    with pytest.raises(diagnostics.AutocorrError):
        diagnostics.integrated_time(x, tol=0, context=None)
    # a found window on a chain shorter than tol tau: raised with tol, returned with tol = 0
    y = dh.ar1(np.random.default_rng(8), 0.9, (16, 1), 600)
    with pytest.raises(diagnostics.AutocorrError):
        diagnostics.integrated_time(y, max_lag=400, context=None)
    assert 10 < diagnostics.integrated_time(y, max_lag=400, tol=0, context=None)[0] < 30
    assert not diagnostics.summary(y, max_lag=400, context=None)["converged"][0]


# ---- the Python layers ----------------------------------------------------------------------------------------------
def _normal(rows):
    return -0.5 * np.sum(np.asarray(rows) ** 2, axis=-1)


def test_every_sampler_has_get_autocorr_time():
    from mcmc_dynamics_amd.analysis.binned import BinnedSampler
    from mcmc_dynamics_amd.sampler import EnsembleSampler, HMCSampler
    for cls in (EnsembleSampler, BinnedSampler, HMCSampler):
        assert callable(getattr(cls, "get_autocorr_time"))


def test_sampler_discard_and_thin():
    from mcmc_dynamics_amd.analysis.binned import BinnedSampler
    from mcmc_dynamics_amd.sampler import EnsembleSampler
    s = EnsembleSampler(16, 2, _normal, vectorize=True, seed=4)
    s.run_mcmc(np.random.default_rng(4).standard_normal((16, 2)), 700)
    chain = s.get_chain()
    assert chain.shape == (700, 16, 2)
    full = s.get_autocorr_time(tol=0, max_lag=300, context=None)
    assert full.shape == (2,) and np.array_equal(full, diagnostics.integrated_time(chain, tol=0, max_lag=300, context=None))
    cut = s.get_autocorr_time(discard=100, thin=3, tol=0, max_lag=100, context=None)
    assert np.array_equal(cut, 3 * diagnostics.integrated_time(chain[100::3], tol=0, max_lag=100, context=None))
    assert np.all(np.abs(cut / full - 1) < 0.5)                         # tau in steps of the un-thinned chain either way
    with pytest.raises(ValueError):
        s.get_autocorr_time(thin=0, context=None)
    b = BinnedSampler(3, 8, 2, _normal, seed=5)
    b.run_mcmc(np.random.default_rng(5).standard_normal((3, 8, 2)), 300)
    assert b.get_chain(discard=50).shape == (250, 3, 8, 2)
    with pytest.warns(UserWarning, match="too short"):                  # 250 steps, max_lag 25: no window
        tau = b.get_autocorr_time(discard=50, quiet=True, context=None)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        assert tau.shape == (3, 2) and np.array_equal(tau, diagnostics.integrated_time(b.get_chain(50), quiet=True, context=None))
        # the bins are independent: bin 1 alone gives bin 1's row
        assert np.array_equal(tau[1], diagnostics.integrated_time(b.get_chain(50)[:, 1], quiet=True, context=None))


def _reader(g):
    from mcmc_dynamics_amd import DataReader
    return DataReader({k: g[k] for k in ("ra", "dec", "v", "verr")})


def test_runner_chain_diagnostics_layouts():
    from conftest import load_golden
    from mcmc_dynamics_amd.analysis import BinnedConstantFit, ConstantFit

    class HostFit(ConstantFit):
        def _diagnostics_context(self):
            return None

    class HostBinned(BinnedConstantFit):
        def _diagnostics_context(self):
            return None

    g = load_golden("radial_bins")
    cf = HostFit(_reader(g))
    P = cf.n_fitted_parameters
    steps = dh.ar1(np.random.default_rng(1), 0.5, (8, P), 400) + 2.0    # (T, W, P)
    out = cf.chain_diagnostics(np.swapaxes(steps, 0, 1), n_burn=50)     # the reference's (W, steps, P)
    want = diagnostics.summary(steps[50:], context=None)
    assert out["names"] == cf.fitted_parameters and out["n_steps"] == 350 and out["tau"].shape == (P,)
    assert set(out) == {"tau", "window", "found", "converged", "ess", "rhat", "mean", "std", "n_steps", "names"}
    assert all(np.array_equal(out[k], want[k]) for k in want)
    with pytest.raises(ValueError):
        cf.chain_diagnostics(steps[0], n_burn=0)
    reader = _reader(g)
    reader.make_radial_bins(float(g["ra_center"]), float(g["dec_center"]), nstars=200, dlogr=0.05)
    bf = HostBinned(reader)
    B, P = bf.n_bins, bf.n_fitted_parameters
    steps = dh.ar1(np.random.default_rng(2), 0.5, (B, 8, P), 300) - 1.0  # (T, B, W, P)
    out = bf.chain_diagnostics(np.transpose(steps, (1, 2, 0, 3)), n_burn=20)   # (B, W, steps, P)
    want = diagnostics.summary(steps[20:], context=None)
    assert out["tau"].shape == (B, P) and out["names"] == bf.fitted_parameters
    assert all(np.array_equal(out[k], want[k]) for k in want)


def test_run_converged_on_a_stub_posterior():
    from conftest import load_golden
    from mcmc_dynamics_amd.analysis import ConstantFit
    from mcmc_dynamics_amd.sampler import EnsembleSampler

    class Stub(ConstantFit):
        """A standard normal in the fitted parameters, sampled by the built-in NumPy loop: no device anywhere."""
        def _diagnostics_context(self):
            return None

        def _rank_group(self):
            return None

        def lnprior_batch(self, values):
            return np.zeros(len(values))

        def get_initials(self, n_walkers):
            return np.random.default_rng(3).standard_normal((n_walkers, self.n_fitted_parameters))

        def _make_sampler(self, n_walkers, seed=None):
            return EnsembleSampler(n_walkers, self.n_fitted_parameters, _normal, vectorize=True, seed=17)

    g = load_golden("radial_bins")
    fit = Stub(_reader(g))
    for name in ("v_maxx", "v_maxy", "ra_center", "dec_center"):       # two free parameters: tau ~ 10 steps
        fit.parameters[name].set(value=float(g[name]) if name in g else 0.0, fixed=True)
    assert fit.n_fitted_parameters == 2
    rtol = 0.05
    sampler, history = fit.run_converged(n_walkers=64, max_steps=20000, check_every=500, tol=50.0, rtol=rtol)
    steps, tau = history[-1]
    print("run_converged:", [(s, np.round(t, 2)) for s, t in history])
    assert sampler.iteration == steps < 20000 and len(history) >= 2 and steps == 500 * len(history)
    assert steps > 50.0 * tau.max()
    assert np.max(np.abs(tau - history[-2][1]) / tau) < rtol
    assert np.array_equal(tau, sampler.get_autocorr_time(quiet=True, context=None))
    with pytest.raises(TypeError):
        fit.run_converged(n_walkers=8, n_burn=3)

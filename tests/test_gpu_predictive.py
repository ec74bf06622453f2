"""GPU: mcd_posterior_predictive -- per-star posterior predictive checks over posterior samples (standardised residual,
tail probability, PIT, the model's v_los and sigma_los with their spreads) -- against the exact oracle of
predictive_helper under the accuracy rule stated there, and through Catalog.posterior_predictive, Runner.posterior_predictive
and Runner.ppc."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import posterior_helper as ph
import predictive_helper as pr
from conftest import ROOT
from test_posterior_cpu import var_ok
from test_predictive_cpu import _merge_scale, _rotation_free, calibration_chi2, planted_case

pytestmark = pytest.mark.gpu
MODELS = [0, 1, 2, 3, 4, 5, 6]
WORKER = os.path.join(ROOT, "tests", "predictive_sharded_worker.py")


@pytest.fixture(scope="module")
def ctx():
    from mcmc_dynamics_amd import _native
    return _native.default_context()


@pytest.mark.parametrize("model", MODELS)
@pytest.mark.parametrize("free", [False, True])
def test_device_summaries_follow_the_rule(ctx, model, free):
    """N in {1, 65, 4099} x S in {1, 65, 257} with the planted stars (z ~ 0, z ~ +-45, verr = 0, density = 0) among the
    first six; spreads on the variance with the device's rtol of 1e-10."""
    cat, table, centre, ref = pr.matrix_case(model, free)
    mix = model in pr.MIX_MODELS
    for n in pr.MATRIX_N:
        gpu = pr.device_catalog(ctx, pr.head(cat, n), model, centre)
        for s in pr.MATRIX_S:
            got = gpu.posterior_predictive(table[:s], mixture=mix)
            assert ("pit_mix" in got) == mix and all(v.shape == (n,) for v in got.values())
            exact, np64, vmax = ref.at(n, s)
            pr.check_rule(got, exact, np64, vmax, var_ok, rtol=1e-10, cell=(model, free, n, s))
            if s == 1:
                assert all(np.all(got[f] == 0.0) for f in ("z_std", "vlos_std", "sigma_std"))
            if n > 5:
                # 45 sigma under the first sample, 35 .. 55 under the others: erfc underflows to an exact 0 at S = 1 and
                # stays below 1e-200 otherwise; the CDF is an exact 1 on the high side and t / 2 on the low side, never 1 - (a value near 1)
                hi, lo = pr.PLANTED["plus45"], pr.PLANTED["minus45"]
                tiny = 0.0 if s == 1 else 1e-200
                assert got["pit"][hi] == 1.0 and 0.0 <= got["pit"][lo] <= tiny
                assert max(got["tail_p"][hi], got["tail_p"][lo]) <= tiny
                assert abs(got["z_mean"][hi] - 45.0) < 10.0 and abs(got["z_mean"][lo] + 45.0) < 10.0
        gpu.close()


def test_planted_stars_on_the_device(ctx):
    """The exact statements of the host test on the device: z = 0 in every sample, erfc's underflow at z ~ +-45, m = 1 and
    m = 0 of the mixture CDF, and a non-finite term that stays with its star."""
    cat, table = planted_case()
    gpu = pr.device_catalog(ctx, cat, 2, ph.CENTRE)
    got = gpu.posterior_predictive(table, mixture=True)
    assert got["z_mean"][0] == 0.0 and got["z_std"][0] == 0.0 and got["tail_p"][0] == 1.0 and got["pit"][0] == 0.5
    assert got["tail_p"][1] == 0.0 and got["pit"][1] == 1.0 and got["tail_p"][2] == 0.0 and got["pit"][2] == 0.0
    assert np.isfinite(got["z_mean"][1]) and np.isfinite(got["z_std"][1])
    assert all(np.isfinite(got[f][3]) for f in got)
    exact, np64, vmax = pr.Reference(cat, table, 2, ph.CENTRE).at()
    pr.check_rule(got, exact, np64, vmax, var_ok, rtol=1e-10, cell="planted")
    g0 = gpu.posterior_predictive(_rotation_free(130, f_back=0.0), mixture=True)
    keep = np.arange(8) != 4
    assert g0["pit_mix"][keep].tobytes() == g0["pit"][keep].tobytes()
    host = pr.predictive(cat, table, 2, ph.CENTRE, True)
    assert abs(got["pit_mix"][4] - host["pit_mix"][4]) < 1e-15            # density = 0: the background CDF alone
    # sigma = 0 with verr = 0
    dead = table.copy()
    dead[:, 1] = 0.0
    bad = gpu.posterior_predictive(dead, mixture=True)
    assert not np.isfinite(bad["z_mean"][3])
    for f in bad:
        assert np.all(np.isfinite(bad[f][[0, 1, 2, 4, 5, 6, 7]])), f
    gpu.close()


def test_bits_repeat_and_passes_agree(ctx):
    """Two calls bit for bit; option posterior_pass = 100 at S = 257 (three passes) within the merge tolerance."""
    cat, table, centre, _ = pr.matrix_case(4, True)
    vmax = float(np.max(np.abs(cat["v"])))
    gpu = pr.device_catalog(ctx, cat, 4, centre)
    a = gpu.posterior_predictive(table, mixture=True)
    b = gpu.posterior_predictive(table, mixture=True)
    for k in a:
        assert a[k].tobytes() == b[k].tobytes(), k
    gpu.set_option("posterior_pass", 100)
    c = gpu.posterior_predictive(table, mixture=True)
    gpu.set_option("posterior_pass", 65536)
    for k in a:
        assert np.max(np.abs(c[k] - a[k]) / _merge_scale(a, k, vmax)) < 1e-13, k
    gpu.close()


@pytest.mark.parametrize("model,precision", [(0, "f32acc64"), (2, "f32acc64"), (4, "f32"), (5, "f32")])
def test_float32_catalogues(ctx, model, precision):
    """float32 terms, float64 after them: within the per-term float32 tolerance of DESIGN.md section 5 (2e-5 of the scale)
    of the float64 device result (confirmed on the host build by test_predictive_cpu.py)."""
    cat, table, centre, _ = pr.matrix_case(model, False)
    vmax = float(np.max(np.abs(cat["v"])))
    mix = model in pr.MIX_MODELS
    g32 = pr.device_catalog(ctx, cat, model, centre, precision)
    g64 = pr.device_catalog(ctx, cat, model, centre)
    a, b = g32.posterior_predictive(table[:100], mixture=mix), g64.posterior_predictive(table[:100], mixture=mix)
    for f in b:
        dev = float(np.max(np.abs(a[f] - b[f]) / _merge_scale(b, f, vmax)))
        print(model, precision, f, "%.2e" % dev)
        assert dev < 2e-5, (f, dev)
    g32.close()
    g64.close()


def test_pit_mix_and_the_refusals(ctx):
    from mcmc_dynamics_amd import _native
    small = pr.head(ph.model_catalog(256, 0), 200)
    n = 200
    F = 8
    dbl = ctypes.POINTER(ctypes.c_double)
    for model in MODELS:
        gpu = pr.device_catalog(ctx, small, model, ph.CENTRE)
        row = ph.samples(small, model, False, 3)
        if model in pr.MIX_MODELS:
            assert "pit_mix" in gpu.posterior_predictive(row, mixture=True)
            assert "pit_mix" not in gpu.posterior_predictive(row)
        else:
            with pytest.raises(_native.NativeError, match="pit_mix"):
                gpu.posterior_predictive(row, mixture=True)
        gpu.close()
    const = pr.device_catalog(ctx, small, 0, ph.CENTRE)
    lib = const.lib
    out, mix = np.full((F, n), 7.0), np.full(n, 7.0)
    optr, mptr = out.ctypes.data_as(dbl), mix.ctypes.data_as(dbl)
    row = np.ascontiguousarray(ph.samples(small, 0, False, 3))
    rowp = row.ctypes.data_as(dbl)
    call = lib.mcd_posterior_predictive
    assert call(const.handle, 0, 4, rowp, optr, None) == -1 and b"n_samples" in lib.mcd_last_error()       # S < 1
    assert call(const.handle, 3, 5, rowp, optr, None) == -1 and b"columns" in lib.mcd_last_error()         # k mismatch
    assert call(const.handle, 3, 4, rowp, None, None) == -1 and b"out" in lib.mcd_last_error()             # NULL out
    assert call(const.handle, 3, 4, rowp, optr, mptr) == -1 and b"pit_mix" in lib.mcd_last_error()         # pit_mix, CONST
    assert call(const.handle, 3, 4, None, optr, None) == -1                                                # NULL params
    assert call(None, 3, 4, rowp, optr, None) == -1                                                        # NULL catalogue
    binned = _native.Catalog(ctx, small["ra"], small["dec"], small["v"], small["verr"], centre=ph.CENTRE,
                             bin_offsets=[0, 80, 200])
    assert call(binned.handle, 3, 4, rowp, optr, None) == -1 and b"un-binned" in lib.mcd_last_error()
    with pytest.raises(ValueError, match="un-binned"):
        binned.posterior_predictive(row)
    assert np.all(out == 7.0) and np.all(mix == 7.0)                      # every refusal left the outputs untouched
    assert call(const.handle, 3, 4, rowp, optr, None) == 0
    assert np.all(out != 7.0) and np.all(mix == 7.0)
    want = const.posterior_predictive(row)
    for f, k in enumerate(const.PREDICTIVE_FIELDS):
        assert out[f].tobytes() == want[k].tobytes()
    empty = _native.Catalog(ctx, np.empty(0), np.empty(0), np.empty(0), np.empty(0), centre=ph.CENTRE)
    assert empty.posterior_predictive(row)["pit"].size == 0
    # option "timing": the kernel time is reported as for mcd_pointwise_posterior
    const.set_option("timing", 1)
    const.posterior_predictive(row)
    assert const.last_kernel_ms > 0.0
    for c in (const, binned, empty):
        c.close()


def _fit(cls, cat, columns):
    from mcmc_dynamics_amd import DataReader
    fit = cls(DataReader({k: cat[k] for k in columns}))
    fit.parameters["ra_center"].set(value=ph.CENTRE[0], fixed=True)
    fit.parameters["dec_center"].set(value=ph.CENTRE[1], fixed=True)
    return fit


def test_runner_posterior_predictive_resolves_the_chain():
    """ConstantFit with a fixed parameter, a parameter in another unit (v_sys in m/s: a unit factor of 1e-3) and thinning:
    the rows the Runner hands the kernel are those of the resolved table, and the result is the native call's, bit for
    bit."""
    from mcmc_dynamics_amd import DataReader, units
    from mcmc_dynamics_amd.analysis import ConstantFit
    from mcmc_dynamics_amd.analysis.constant import _CONSTANT_DEFAULTS, _build_defaults
    cat = ph.model_catalog(500, 0)
    rows = tuple((("v_sys", "m/s") + r[2:]) if r[0] == "v_sys" else r for r in _CONSTANT_DEFAULTS)
    fit = ConstantFit(DataReader({k: cat[k] for k in ("ra", "dec", "v", "verr")}), parameters=_build_defaults(rows))
    fit.parameters["ra_center"].set(value=ph.CENTRE[0], fixed=True)
    fit.parameters["dec_center"].set(value=ph.CENTRE[1], fixed=True)
    fit.parameters["sigma_max"].set(value=9.0, fixed=True)
    free = ph.samples(cat, 0, False, 8 * 20)
    names = ph.abi_names(0, False)
    free[:, names.index("v_sys")] *= 1000.0                              # the chain holds v_sys in m/s
    keep = [names.index(n) for n in fit.fitted_parameters]
    chain = free[:, keep].reshape(8, 20, len(keep))
    got = fit.posterior_predictive(chain, n_burn=5, thin=3)
    table = free.reshape(8, 20, -1)[:, 5::3, :].reshape(-1, len(names)).copy()
    table[:, names.index("sigma_max")] = 9.0
    table[:, names.index("v_sys")] *= units.conversion_factor("m/s", "km/s")
    want = fit._catalog.posterior_predictive(table)
    assert got["n_samples"] == 40 and "pit_mix" not in got
    for k in want:
        assert np.array_equal(got[k], want[k]), k
    assert np.all(got["sigma_mean"] == 9.0) and np.all(got["sigma_std"] == 0.0)
    assert abs(float(np.mean(got["vlos_mean"]))) < 20.0                  # km/s, not m/s
    fit.close()


def test_runner_ppc_on_the_calibration_catalogue():
    """Runner.ppc of ConstantFit on the calibration catalogue under its truth vector repeated: the chi2 of the host test
    (the histogram counts are integers: equal unless a PIT sits within rounding of a bin edge), no background -> unit
    weights, and the Bonferroni default of outlier_p."""
    from mcmc_dynamics_amd.analysis import ConstantFit
    cat, truth = pr.calibration_case()
    fit = _fit(ConstantFit, cat, ("ra", "dec", "v", "verr"))
    names = ph.abi_names(0, False)
    vec = np.array([truth[names.index(n)] for n in fit.fitted_parameters])
    chain = np.tile(vec, (4, 3, 1))
    out = fit.ppc(chain, n_burn=1)
    want = calibration_chi2()
    assert abs(out["chi2"] - want["chi2"]) <= 1e-9 * want["chi2"]
    assert out["n"] == pr.CALIBRATION_N and out["n_stars"] == pr.CALIBRATION_N and out["n_samples"] == 8
    assert out["chi2"] < pr.CHI2_19_Q999 and np.all(out["weight"] == 1.0)
    assert out["outlier_p"] == pytest.approx(0.05 / pr.CALIBRATION_N, rel=1e-15)
    assert np.array_equal(out["outliers"], np.flatnonzero(out["tail_p"] < out["outlier_p"]))
    assert out["outliers"].size <= 3                     # 0.05 expected among 20 000 calibrated stars
    loose = fit.ppc(chain, n_burn=1, outlier_p=0.01)
    assert 100 < loose["outliers"].size < 300            # 200 expected
    fit.close()


def test_runner_ppc_of_the_background_models():
    """pit_mix is present for ConstantFitGB and its summary is unweighted; the outliers are weighted by the membership
    probability."""
    from mcmc_dynamics_amd.analysis import ConstantFitGB
    cat = ph.model_catalog(2000, 0)
    fit = _fit(ConstantFitGB, cat, ("ra", "dec", "v", "verr", "density"))
    table = ph.samples(cat, 2, False, 6 * 10)
    names = ph.abi_names(2, False)
    chain = table[:, [names.index(n) for n in fit.fitted_parameters]].reshape(6, 10, -1)
    out = fit.ppc(chain, n_burn=2, n_bins=10)
    from mcmc_dynamics_amd.analysis.runner import ppc_summary
    want = ppc_summary(out["pit_mix"], None, 10)
    assert out["chi2"] == want["chi2"] and out["n"] == 2000.0 and out["hist"].size == 10
    pm = fit.posterior_membership_probabilities(chain, 2)[0]
    assert np.array_equal(out["weight"], pm)
    assert np.array_equal(out["outliers"], np.flatnonzero((pm > 0.5) & (out["tail_p"] < 0.05 / 2000)))
    fit.close()


def test_binned_fits_refuse():
    from mcmc_dynamics_amd import DataReader
    from mcmc_dynamics_amd.analysis.binned import BinnedConstantFit
    cat = ph.model_catalog(200, 0)
    reader = DataReader({k: cat[k] for k in ("ra", "dec", "v", "verr")})
    reader.make_radial_bins(ph.CENTRE[0], ph.CENTRE[1], nstars=50)
    bf = BinnedConstantFit(reader)
    chain = np.tile(ph.samples(cat, 0, True, 1)[0], (4, 3, 1))
    with pytest.raises(NotImplementedError, match="un-binned"):
        bf.posterior_predictive(chain, 1)
    with pytest.raises(NotImplementedError, match="un-binned"):
        bf.ppc(chain, 1)
    bf.close()


def test_three_shards_equal_one_device():
    """Three shards on device 0 over tests/fake_rccl, in a fresh child process under its own time limit: every output
    equals the one-device result to 1e-13 of its scale, and the stars of the second and third shard land at their
    star_begin."""
    subprocess.run(["make", "-C", os.path.join(ROOT, "tests", "fake_rccl")], check=True, capture_output=True)
    res = subprocess.run(["timeout", "-k", "10", "120", sys.executable, WORKER], capture_output=True, text=True)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-3000:]
    assert "PREDICTIVE_SHARDED_OK" in res.stdout

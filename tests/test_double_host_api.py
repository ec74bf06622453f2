"""Host logic of the double Lynden-Bell classes (no GPU): parameters, bounds, kernel column order, what is refused, the
derived peak radius, the profile table, the planted-core generator."""
import numpy as np
import pytest

import double_helper as dh

from mcmc_dynamics_amd import DataReader, Gaussian, _native, synthetic
from mcmc_dynamics_amd import analysis
from mcmc_dynamics_amd.analysis import DoubleModelFit, DoubleModelFitGB, ModelFit, ModelFitGB

KMS = ("v_sys", "sigma_max", "v_maxx", "v_maxy", "v_maxx_c", "v_maxy_c")


def reader(n=200, background=False):
    c = synthetic.make_catalog(n, config=3, background=background)
    return DataReader({k: c[k] for k in c if k != "truth"}), c


def fixed_centre(fit):
    fit.parameters["ra_center"].set(value=synthetic.CENTER_RA_DEG, fixed=True)
    fit.parameters["dec_center"].set(value=synthetic.CENTER_DEC_DEG, fixed=True)
    return fit


def test_model_ids_and_exports():
    assert (_native.MODEL_DOUBLE, _native.MODEL_DOUBLE_BGGAUSS) == (7, 8)
    assert "DoubleModelFit" in analysis.__all__ and "DoubleModelFitGB" in analysis.__all__
    assert issubclass(DoubleModelFit, ModelFit) and issubclass(DoubleModelFitGB, DoubleModelFit)
    assert DoubleModelFit._model_id == 7 and DoubleModelFitGB._model_id == 8


def test_default_parameters_are_modelfits_plus_the_second_component():
    single, double = ModelFit.default_parameters(), DoubleModelFit.default_parameters()
    assert list(double) == list(single) + ["v_maxx_c", "v_maxy_c", "r_peak_ratio"]
    for name in single:
        assert (double[name].min, double[name].max, double[name].unit) == (single[name].min, single[name].max, single[name].unit)
    for name in ("v_maxx_c", "v_maxy_c"):
        assert (double[name].min, double[name].max, double[name].unit) == (-50.0, 50.0, "km/s")
    assert (double["r_peak_ratio"].min, double["r_peak_ratio"].max) == (1e-3, 1.0) and not double["r_peak_ratio"].unit
    gb = DoubleModelFitGB.default_parameters()
    assert list(gb) == list(ModelFitGB.default_parameters()) + ["v_maxx_c", "v_maxy_c", "r_peak_ratio"]


@pytest.mark.parametrize("cls, background, free", [(DoubleModelFit, False, False), (DoubleModelFit, False, True),
                                                    (DoubleModelFitGB, True, False), (DoubleModelFitGB, True, True)])
def test_kernel_table_has_the_c_abi_column_order(cls, background, free):
    rd, _ = reader(background=background)
    fit = cls(rd)
    if not free:
        fixed_centre(fit)
    names = list(fit.fitted_parameters)
    row = np.arange(1.0, len(names) + 1.0)
    resolved = fit.parameters.resolve_batch(row.reshape(1, -1))
    (model, centre), _ = fit._catalog_spec()
    assert model == cls._model_id and (centre is None) == free
    fit._catalog_key = (model, centre)
    table = fit._kernel_table(resolved)
    want = dh.column_names(model, free)
    assert table.shape == (1, dh.n_columns(model, free)) and table.shape[1] in (9, 11, 12, 14)
    assert [float(row[names.index(n)]) for n in want] == table[0].tolist()
    fit._catalog_key = None


def test_inclusive_default_bounds_of_the_new_parameters():
    rd, _ = reader()
    fit = fixed_centre(DoubleModelFit(rd))
    names = list(fit.fitted_parameters)
    base = np.array([0.0, 8.0, 30.0, 1.0, 1.0, 60.0, 1.0, -1.0, 0.5])
    assert names == ["v_sys", "sigma_max", "a", "v_maxx", "v_maxy", "r_peak", "v_maxx_c", "v_maxy_c", "r_peak_ratio"]
    for name, value, inside in (("r_peak_ratio", 1.0, True), ("r_peak_ratio", 1e-3, True), ("r_peak_ratio", 1.0000001, False),
                                ("r_peak_ratio", 9e-4, False), ("v_maxx_c", 50.0, True), ("v_maxx_c", 50.1, False),
                                ("v_maxy_c", -50.0, True), ("v_maxy_c", -50.1, False)):
        row = base.copy()
        row[names.index(name)] = value
        assert np.isfinite(fit.lnprior(row)) == inside, (name, value)


def test_out_of_scope_requests_are_refused_with_a_message():
    rd, _ = reader(background=True)
    with pytest.raises(NotImplementedError, match="background"):
        DoubleModelFit(rd, background=Gaussian(mean=20.0, sigma=40.0))
    with pytest.raises(NotImplementedError, match="background"):
        DoubleModelFitGB(rd, background=Gaussian(mean=20.0, sigma=40.0))
    for precision in ("f32", "f32acc64"):
        with pytest.raises(NotImplementedError, match="float64 only"):
            DoubleModelFit(rd, precision=precision)


def test_hmc_and_tempered_refuse_more_than_twelve_free_parameters_before_the_library_is_called(monkeypatch):
    rd, _ = reader(background=True)
    fit = DoubleModelFitGB(rd)                                 # free centre: P = 14
    assert len(fit.fitted_parameters) == 14
    monkeypatch.setattr(_native, "load_library", lambda *a, **k: pytest.fail("the library was loaded"))
    monkeypatch.setattr(fit, "_ensure_catalog", lambda *a, **k: pytest.fail("a catalogue was asked for"))
    with pytest.raises(NotImplementedError, match="at most 12"):
        fit.hmc(n_walkers=8, n_steps=2)
    with pytest.raises(NotImplementedError, match="at most 12"):
        fit.tempered(n_temps=2, n_walkers=28, n_steps=2)
    fixed = fixed_centre(DoubleModelFitGB(rd))                 # fixed centre: P = 12 fits
    assert len(fixed.fitted_parameters) == 12
    fixed._check_resident_dim("hmc", 12)


def test_rotation_model_on_the_host_is_the_helpers():
    rd, c = reader()
    fit = fixed_centre(DoubleModelFit(rd))
    centre = (synthetic.CENTER_RA_DEG, synthetic.CENTER_DEC_DEG)
    got = fit.rotation_model(v_sys=1.5, v_maxx=3.0, v_maxy=-2.0, ra_center=centre[0], dec_center=centre[1], r_peak=70.0,
                             v_maxx_c=-5.0, v_maxy_c=4.0, r_peak_ratio=0.2)
    from oracle import lnprob_numpy as oracle
    want = oracle.model_rotation(c["ra"], c["dec"], 1.5, 3.0, -2.0, 70.0, *centre) + \
        oracle.model_rotation(c["ra"], c["dec"], 0.0, -5.0, 4.0, 14.0, *centre)
    assert np.max(np.abs(got - want)) < 1e-12
    single = ModelFit.rotation_model(fit, v_sys=1.5, v_maxx=3.0, v_maxy=-2.0, ra_center=centre[0], dec_center=centre[1], r_peak=70.0)
    nested = fit.rotation_model(v_sys=1.5, v_maxx=3.0, v_maxy=-2.0, ra_center=centre[0], dec_center=centre[1], r_peak=70.0,
                                r_peak_ratio=0.2)
    assert np.max(np.abs(nested - single)) < 1e-12


def test_r_peak_c_profiles_and_component_angles():
    rd, _ = reader()
    fit = fixed_centre(DoubleModelFit(rd))
    names = list(fit.fitted_parameters)
    rng = np.random.default_rng(5)
    mid = np.array([0.0, 9.0, 40.0, 3.0, 1.0, 80.0, -4.0, -3.0, 0.25])
    chain = mid + rng.normal(size=(6, 10, len(names))) * 0.02 * np.maximum(np.abs(mid), 0.1)
    n_burn = 2
    rc = fit.r_peak_c(chain, n_burn)
    flat = chain[:, n_burn:].reshape(-1, len(names))
    assert rc.shape == (48,) and np.allclose(np.sort(rc), np.sort(flat[:, 8] * flat[:, 5]), rtol=1e-14)
    prof = fit.create_profiles(chain, n_burn)
    suffixes = ("", "_lower_1s", "_upper_1s", "_lower_3s", "_upper_3s")
    assert list(prof.columns) == ["r"] + [k + s for k in ("v_rot", "v_rot_c", "sigma", "r_peak_c") for s in suffixes]
    assert np.all(prof["r_peak_c"] == np.median(rc)) and np.all(prof["r_peak_c_lower_1s"] <= prof["r_peak_c_upper_1s"])
    rr = np.asarray(prof["r"])
    want_c = np.median(2.0 * rc[None, :] * np.hypot(flat[:, 6], flat[:, 7])[None, :] * rr[:, None] / (rc[None, :] ** 2 + rr[:, None] ** 2),
                       axis=1)
    assert np.allclose(np.sort(prof["v_rot_c"]), np.sort(want_c), rtol=1e-12)
    assert np.all(prof["v_rot"] >= prof["v_rot_c"])
    outer = fit.compute_theta_vmax(chain, n_burn)
    inner = fit.compute_theta_vmax(chain, n_burn, component=2)
    assert abs(outer.loc["median"]["v_max"] - np.hypot(3.0, 1.0)) < 0.2
    assert abs(inner.loc["median"]["v_max"] - 5.0) < 0.2
    assert abs(inner.loc["median"]["theta_0"] - np.arctan2(-3.0, -4.0)) < 0.1
    with pytest.raises(ValueError):
        fit.compute_theta_vmax(chain, n_burn, component=3)


def test_planted_core_generator_counter_rotates_inside():
    before = synthetic.make_catalog(50, config=2)
    cat = synthetic.make_double_catalog(4000)
    after = synthetic.make_catalog(50, config=2)
    assert all(np.array_equal(before[k], after[k]) for k in ("ra", "dec", "v", "verr"))
    t = cat["truth"]
    assert set(dh.HEAD) <= set(t) and 0 < t["r_peak_ratio"] < 1
    assert t["v_maxx"] * t["v_maxx_c"] + t["v_maxy"] * t["v_maxy_c"] < 0           # the inner axis is turned by pi
    row = np.array([t[n] for n in dh.HEAD])
    centre = (t["ra_center"], t["dec_center"])
    data = {k: cat[k] for k in ("ra", "dec", "v", "verr")}
    flipped = row.copy()
    flipped[6:8] *= -1.0
    assert dh.value(dh.DOUBLE, data, row, centre) > dh.value(dh.DOUBLE, data, flipped, centre) + 50.0

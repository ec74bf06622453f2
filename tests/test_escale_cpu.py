"""Host checks of the error-scale models (device models 10 and 11; id 9 stays unassigned; ConstantFitES / ModelFitES), no GPU.

The kernels' own text (csrc/mcd_math.h: star_d_n through chunk_loglike, csrc/mcd_grad.h: grad_term, csrc/mcd_prep.h:
walker_constants, csrc/mcd_guard.h, csrc/mcd_dispatch.h) is compiled for the host by tests/emul/escale_emul.cpp and held
against escale_helper's reference: the project's own oracle on a copy of the catalogue whose error column is multiplied by
the row's err_scale, in numpy.longdouble.

Bounds, none of them new: values 1e-12 on max(|lnL|, N) and per-star terms 1e-12 on max(|l_i|, 1), plain and fast, as
test_double_emul_cpu.py and test_gpu_double_live.py hold the other models; gradient columns err <= 2 err_np64 + floor with
grad_bounds' floors of models 0 and 3 at the same cell (err_scale takes the floor of the non-geometry columns).  The verdicts
of models 0 .. 8 on random tables are pinned in tests/test_escale_guard_cpu.py against the guard as it was before."""
import ctypes
import os
import sys

import numpy as np
import pytest

import emul_helper as eh
import escale_helper as es
import grad_bounds as gb
import grad_helper as gh
import variant_helper as vh

pytestmark = pytest.mark.skipif(not vh.HAVE_LONGDOUBLE, reason="numpy.longdouble is not wider than float64 here")

L = vh.L
ROWS = vh.sample_rows(8)
N_CELLS = (1, 33, 4099)


# ---------------------------------------------------------------------------------------------- ids, helpers, dispatch
def test_model_ids_helpers_and_counts():
    lib = es.lib()
    assert [lib.escale_emul_counts(i) for i in range(3)] == [7, 9, 12]
    assert lib.escale_emul_kd() == 20 and lib.escale_emul_slot() == 19 and lib.escale_emul_grad_max_columns() == 14
    assert [lib.escale_emul_is_escale(m) for m in range(13)] == [0] * 10 + [1, 1, 0]
    assert [lib.escale_emul_is_profile(m) for m in range(13)] == [0, 0, 0, 1, 1, 1, 1, 1, 1, 0, 0, 1, 0]
    assert [lib.escale_emul_cluster_columns(m) for m in range(9)] + [lib.escale_emul_cluster_columns(m) for m in (10, 11)] == \
        [4, 4, 4, 6, 6, 6, 6, 9, 9, 5, 7]
    assert lib.escale_emul_bg_kind(10) == lib.escale_emul_bg_kind(11) == 0
    for model, base in es.BASE.items():
        for free in (0, 1):
            assert lib.escale_emul_record_doubles(model, free) == lib.escale_emul_record_doubles(base, free)
            assert lib.escale_emul_columns(model, free) == lib.escale_emul_columns(base, free) + 1 == es.n_columns(model, bool(free))
    assert lib.escale_emul_columns(11, 1) == 9


@pytest.mark.parametrize("free", [0, 1])
@pytest.mark.parametrize("model", list(range(9)) + [10, 11])
def test_the_launchers_dispatcher_reaches_all_eleven_models_with_their_own_constants(model, free):
    calls = ctypes.c_int(0)
    assert es.lib().escale_emul_dispatch(0, model, free, -7, ctypes.byref(calls)) == model * 2 + free and calls.value == 1


@pytest.mark.parametrize("model", [-1, 9, 12])
def test_the_launchers_dispatcher_calls_nothing_for_an_unknown_model(model):
    calls = ctypes.c_int(0)
    assert es.lib().escale_emul_dispatch(0, model, 0, -7, ctypes.byref(calls)) == -7 and calls.value == 0


@pytest.mark.parametrize("model", [9, 10, 11])
def test_dispatch_any_model_still_calls_nothing_for_the_error_scale_models(model):
    calls = ctypes.c_int(0)
    assert es.lib().escale_emul_dispatch(1, model, 0, -7, ctypes.byref(calls)) == -7 and calls.value == 0
    assert es.lib().escale_emul_dispatch(1, 8, 1, -7, ctypes.byref(calls)) == 17 and calls.value == 1


# ---------------------------------------------------------------------------------------------- walker constants
@pytest.mark.parametrize("model, free", es.CELLS, ids=es.CELL_IDS)
def test_slot_19_is_the_squared_scale_and_every_other_slot_the_base_models(model, free):
    case = es.make_case(model, free, 33)
    rows = case["params"][:64]
    base_rows, s = es.split_rows(model, rows)
    got, base = es.walkers(rows, model, free), es.walkers(base_rows, es.BASE[model], free)
    assert np.array_equal(got[:, 19], s * s) and np.all(got[:, 19] != 1.0)
    assert np.array_equal(got[:, :19], base[:, :19]) and np.all(base[:, 19] == 0.0)
    # ... which is what the Python packing of the older harnesses gives for the base model
    assert np.array_equal(base, eh.pack_walkers(base_rows, es.BASE[model], free))


@pytest.mark.parametrize("model", range(9))
def test_slot_19_stays_zero_for_every_other_model(model):
    free = False
    if model in eh.DOUBLE_MODELS:
        import double_helper as dh
        rows = dh.make_case(model, free, 33)["params"][:16]
    else:
        rows = vh.make_case(model, free, 33)["params"][:16]
    got = es.walkers(rows, model, free)
    assert np.all(got[:, 19] == 0.0) and not np.any(np.signbit(got[:, 19])) and np.all(np.isfinite(got))
    assert np.array_equal(got, eh.pack_walkers(rows, model, free))


# ---------------------------------------------------------------------------------------------- nested, bit for bit
@pytest.mark.parametrize("n", N_CELLS)
@pytest.mark.parametrize("model, free", es.CELLS, ids=es.CELL_IDS)
def test_unit_scale_is_the_base_model_bit_for_bit(model, free, n):
    """Value (plain and fast), per-star d, n and term (plain and FASTMATH) and the shared gradient columns at s = 1 against
    models 0 and 3 with array_equal."""
    case = es.make_case(model, free, n)
    base, cat, centre = es.BASE[model], case["cat"], case["centre"]
    rows = es.unit_rows(model, case["params"][ROWS])
    base_rows, s = es.split_rows(model, rows)
    assert np.all(s == 1.0)
    assert es.level(model, cat, rows, centre) == 1 and es.level(base, cat, base_rows, centre) >= 1      # the guard admits the fast form
    for fast in (0, 1):
        assert np.array_equal(es.emul_value(model, cat, rows, centre, fast), es.emul_value(base, cat, base_rows, centre, fast)), fast
        for j in range(len(rows)):
            for got, want in zip(es.emul_terms(model, cat, rows[j], centre, fast), es.emul_terms(base, cat, base_rows[j], centre, fast)):
                assert np.array_equal(got, want), (fast, j)
    v, g = es.emul_grad(model, cat, rows, centre)
    v0, g0 = es.emul_grad(base, cat, base_rows, centre)
    assert np.array_equal(v, v0) and np.array_equal(np.delete(g, es.ES_COLUMN[model], axis=1), g0)
    assert np.all(g[:, es.ES_COLUMN[model]] != 0.0)


# ---------------------------------------------------------------------------------------------- live rows
@pytest.mark.parametrize("n", N_CELLS)
@pytest.mark.parametrize("model, free", es.CELLS, ids=es.CELL_IDS)
def test_live_values_terms_and_gradient_against_the_scaled_catalogue_reference(model, free, n):
    case = es.make_case(model, free, n)
    cat, centre = case["cat"], case["centre"]
    rows = case["params"][ROWS]
    es.guard(case, rows, "host build")
    assert es.level(model, cat, rows, centre) == 1
    plain, fast = es.emul_value(model, cat, rows, centre, 0), es.emul_value(model, cat, rows, centre, 1)
    value, grad = es.emul_grad(model, cat, rows, centre)
    floors = es.floors(model, free, n)
    worst = {"plain": 0.0, "fast": 0.0, "terms": 0.0, "grad - 2 err64": -np.inf}
    for j, w in enumerate(ROWS):
        ref = es.reference(case, w)
        for name, got in (("plain", plain[j]), ("fast", fast[j]), ("gradient's value", value[j])):
            err = float(vh.scaled_err(got, ref["value"], n))
            worst[name if name in worst else "plain"] = max(worst[name if name in worst else "plain"], err)
            assert err < 1e-12, ((model, free, n), w, name, err)
        want = es.per_star(model, cat, rows[j], centre)
        for f in (0, 1):
            e = es.term_err(es.emul_terms(model, cat, rows[j], centre, f)[2], want)
            worst["terms"] = max(worst["terms"], e)
            assert e < 1e-12, ((model, free, n), w, "terms", f, e)
        err = gb.check_columns(grad[j], ref, ((model, free, n), w), floors)
        worst["grad - 2 err64"] = max(worst["grad - 2 err64"], float((err - 2 * ref["err64"]).max()))
    print("host build", (model, int(free), n), {k: "%.2e" % v for k, v in worst.items()})


@pytest.mark.parametrize("model, free", es.CELLS, ids=es.CELL_IDS)
def test_the_err_scale_column_is_the_central_difference_of_the_longdouble_value(model, free):
    """h = 2^-20 s in longdouble: the truncation error s^3 h^2 f''' / 6 is ~1e-12 relative, the rounding 1e-19 / 1e-6."""
    case = es.make_case(model, free, 33)
    cat, centre, k = case["cat"], case["centre"], es.ES_COLUMN[model]
    _, grad = es.emul_grad(model, cat, case["params"][ROWS], centre)
    for j, w in enumerate(ROWS):
        row = case["params"][w].astype(L)
        h = row[k] * L(2.0) ** -20
        up, down = row.copy(), row.copy()
        up[k], down[k] = row[k] + h, row[k] - h
        diff = (es.per_star(model, cat, up, centre).sum() - es.per_star(model, cat, down, centre).sum()) / (up[k] - down[k])
        ref = es.reference(case, w)
        assert abs(ref["g"][k] - diff) <= 1e-9 * ref["s"][k], (w, float(ref["g"][k]), float(diff))
        assert abs(L(grad[j, k]) - diff) <= 1e-9 * ref["s"][k], (w, grad[j, k], float(diff))


# ---------------------------------------------------------------------------------------------- guard
@pytest.mark.parametrize("model, free", es.CELLS, ids=es.CELL_IDS)
def test_the_guard_sees_the_scale(model, free):
    case = es.make_case(model, free, 4099)
    cat, centre, k = case["cat"], case["centre"], es.ES_COLUMN[model]
    rows = np.array(case["params"][:64], copy=True)
    ranges = np.zeros(2)
    assert es.level(model, cat, rows, centre, ranges) == 1                       # inside the domain: the fast form, never 2
    s = rows[:, k]
    assert ranges[0] == min(1.0, (s * s).min()) and ranges[1] == max(1.0, (s * s).max())
    if model == es.PROFILE_ES and not free:
        single = vh.make_case(3, False, 4099)
        assert eh.fast_level_at(single["cat"], single["params"][:64], 3, single["centre"]) == 2
        assert es.level(model, single["cat"], es.with_scale(model, single["params"][:64], 1.0), single["centre"]) == 1
    for bad in (0.0, -1.0, np.nan, np.inf):
        table = rows.copy()
        table[5, k] = bad
        assert es.level(model, cat, table, centre) == 0, bad
    # es2_max e2_max above the domain (2^55 for the trees of the models without a background): one row is enough
    e2_max = float(np.max(cat["verr"] ** 2))
    table = rows.copy()
    table[7, k] = np.sqrt(2.0 ** 56 / e2_max)
    assert es.level(model, cat, table, centre) == 0
    table[7, k] = np.sqrt(2.0 ** 50 / e2_max)
    assert es.level(model, cat, table, centre) == 1
    # the same table is inside the base model's domain whatever the scale column held
    assert es.level(es.BASE[model], cat, es.split_rows(model, table)[0], centre) >= 1


# ---------------------------------------------------------------------------------------------- ISA
@pytest.fixture(scope="module")
def isa_rows(tmp_path_factory):
    sys.path.insert(0, os.path.join(eh.ROOT, "tools"))
    import isa_mix
    import shutil
    if shutil.which("hipcc") is None:
        pytest.skip("hipcc is not on the path")
    out = str(tmp_path_factory.mktemp("isa_mix_escale"))
    rows = isa_mix.analyse(out)
    return {(r["model"], r["prefetch"]): r for r in rows}, os.path.join(out, "mcd_kernels-hip-amdgcn-amd-amdhsa-gfx950.s")


@pytest.mark.parametrize("key, base", [("const_escale", "const"), ("profile_escale", "profile_general")])
def test_the_new_loops_cost_at_most_one_vector_instruction_per_term_more(isa_rows, key, base):
    """One fused multiply-add in place of an add (CONST) / one multiply in front of the variance's fma (PROFILE): at most
    +1.0 VALU per term, and no more reciprocal sequences than the base loop."""
    rows, _ = isa_rows
    for prefetch in (False, True):
        new, old = rows[(key, prefetch)], rows[(base, prefetch)]
        print(key, "prefetch" if prefetch else "", "VALU/term %.3f against %.3f" % (new["valu_per_term"], old["valu_per_term"]))
        assert new["valu_per_term"] <= old["valu_per_term"] + 1.0
        assert new["trans_f64_per_term"] == old["trans_f64_per_term"]
        assert new["stars_per_iteration"] == old["stars_per_iteration"]
        assert new["lds_per_term"] == 0.0


def test_the_new_kernels_use_no_scratch_and_at_most_128_vgprs(isa_rows):
    _, path = isa_rows
    import re
    text = open(path).read()
    seen = 0
    for m in re.finditer(r"\.amdhsa_kernel (_ZN3mcd12_GLOBAL__N_114loglike_kernelILi(?:10|11)E\w+)(.*?)\.end_amdhsa_kernel", text, re.S):
        body = m.group(2)
        vgpr = int(re.search(r"\.amdhsa_next_free_vgpr (\d+)", body).group(1))
        scratch = int(re.search(r"\.amdhsa_private_segment_fixed_size (\d+)", body).group(1))
        assert scratch == 0 and vgpr <= 128, (m.group(1), vgpr, scratch)
        seen += 1
    assert seen >= 8                                        # 2 models x 2 centres x (plain, fast) at the least


# ---------------------------------------------------------------------------------------------- host classes
def _reader(n=64, config=2):
    from mcmc_dynamics_amd import DataReader, synthetic
    c = synthetic.make_catalog(n, config=config)
    return DataReader({k: c[k] for k in ("ra", "dec", "v", "verr")}), c


def _fix_centre(fit):
    from mcmc_dynamics_amd import synthetic
    fit.parameters["ra_center"].set(value=synthetic.CENTER_RA_DEG, fixed=True)
    fit.parameters["dec_center"].set(value=synthetic.CENTER_DEC_DEG, fixed=True)
    return fit


def test_classes_ids_parameters_and_exports():
    from mcmc_dynamics_amd import _native, analysis
    from mcmc_dynamics_amd.analysis import ConstantFit, ConstantFitES, ModelFit, ModelFitES
    assert (_native.MODEL_CONST_ESCALE, _native.MODEL_PROFILE_ESCALE) == (10, 11)
    assert "ConstantFitES" in analysis.__all__ and "ModelFitES" in analysis.__all__
    assert issubclass(ConstantFitES, ConstantFit) and issubclass(ModelFitES, ModelFit)
    assert ConstantFitES._model_id == 10 and ModelFitES._model_id == 11
    for cls, base in ((ConstantFitES, ConstantFit), (ModelFitES, ModelFit)):
        pars, plain = cls.default_parameters(), base.default_parameters()
        assert list(pars) == list(plain) + ["err_scale"] and cls.MODEL_PARAMETERS == base.MODEL_PARAMETERS + ["err_scale"]
        p = pars["err_scale"]
        assert (p.min, p.max, p.value, p.fixed) == (0.1, 10.0, 1.0, False) and not p.unit and p.prior is None
        assert cls._KERNEL_HEAD == base._KERNEL_HEAD + (("err_scale", None),)
        for name in plain:
            assert (pars[name].min, pars[name].max, pars[name].unit) == (plain[name].min, plain[name].max, plain[name].unit)


def test_initials_and_the_inclusive_box():
    from mcmc_dynamics_amd.analysis import ConstantFitES
    rd, _ = _reader()
    fit = _fix_centre(ConstantFitES(rd))
    names = list(fit.fitted_parameters)
    assert names == ["v_sys", "sigma_max", "v_maxx", "v_maxy", "err_scale"]
    row = np.array([0.0, 5.0, 1.0, 1.0, 1.0])
    for value, inside in ((0.1, True), (10.0, True), (0.0999, False), (10.001, False)):
        row[4] = value
        assert np.isfinite(fit.lnprior(row)) == inside, value
    from mcmc_dynamics_amd.parameter import Parameters
    assert fit.parameters["err_scale"].initials == "rng.uniform(0.8, 1.2, size=n)"
    start = fit.get_initials(64)[:, names.index("err_scale")]                   # drawn the way Runner draws them
    assert start.shape == (64,) and np.all((start >= 0.8) & (start <= 1.2)) and len(np.unique(start)) > 32
    assert isinstance(fit.parameters, Parameters)


@pytest.mark.parametrize("name, free", [("ConstantFitES", False), ("ConstantFitES", True), ("ModelFitES", False), ("ModelFitES", True)])
def test_kernel_table_has_the_c_abi_column_order(name, free):
    from mcmc_dynamics_amd import analysis
    cls = getattr(analysis, name)
    rd, _ = _reader(config=2 if name == "ConstantFitES" else 3)
    fit = cls(rd)
    if not free:
        _fix_centre(fit)
    names = list(fit.fitted_parameters)
    row = np.arange(1.0, len(names) + 1.0)
    resolved = fit.parameters.resolve_batch(row.reshape(1, -1))
    (model, centre), spec = fit._catalog_spec()
    assert model == cls._model_id and (centre is None) == free and sorted(spec) == ["centre", "model"]
    fit._catalog_key = (model, centre)
    table = fit._kernel_table(resolved)
    want = es.column_names(model, free)
    assert table.shape == (1, es.n_columns(model, free)) and table.shape[1] in (5, 7, 9)
    assert [float(row[names.index(n)]) for n in want] == table[0].tolist()
    assert not fit._has_background() and not fit._has_mixture_cdf()


def test_out_of_scope_requests_are_refused_with_a_message():
    from mcmc_dynamics_amd import Gaussian
    from mcmc_dynamics_amd.analysis import BinnedConstantFit, ConstantFitES, ModelFitES
    rd, _ = _reader()
    for cls in (ConstantFitES, ModelFitES):
        with pytest.raises(NotImplementedError, match="background"):
            cls(rd, background=Gaussian(mean=20.0, sigma=40.0))
        for precision in ("f32", "f32acc64"):
            with pytest.raises(NotImplementedError, match="float64 only"):
                cls(rd, precision=precision)

    class BinnedES(ConstantFitES, BinnedConstantFit):
        pass
    with pytest.raises(NotImplementedError, match="radial bins"):
        BinnedES(rd)


class _HostCatalog(object):
    """Stands in for ``_native.Catalog``: the host build of the kernels' arithmetic for the catalogue's model."""

    def __init__(self, cols, model, centre):
        self.cols, self.model, self.centre, self.tables = cols, model, centre, []

    def loglike(self, table):
        self.tables.append(np.array(table, copy=True))
        return es.emul_value(self.model, self.cols, table, self.centre, 1)

    def close(self):
        pass


def _host_fit(cls, cols, centre):
    from mcmc_dynamics_amd import DataReader
    fit = _fix_centre(cls(DataReader({k: cols[k] for k in ("ra", "dec", "v", "verr")})))
    (model, c), _ = fit._catalog_spec()
    assert c == centre
    fit._catalog = _HostCatalog(cols, model, centre)
    fit._catalog_key = fit._plan().catalog_key
    fit._ensure_catalog = lambda: fit._catalog
    return fit


def test_err_scale_fixed_at_one_reproduces_constantfits_lnprob_batch_bits():
    from mcmc_dynamics_amd import synthetic
    from mcmc_dynamics_amd.analysis import ConstantFit, ConstantFitES
    centre = (synthetic.CENTER_RA_DEG, synthetic.CENTER_DEC_DEG)
    cols = synthetic.make_catalog(300, config=2)
    pos = synthetic.make_walkers(16, ["v_sys", "sigma_max", "v_maxx", "v_maxy"], cols["truth"], config=2)
    plain, scaled = _host_fit(ConstantFit, cols, centre), _host_fit(ConstantFitES, cols, centre)
    scaled.parameters["err_scale"].set(value=1.0, fixed=True)
    scaled._catalog_key = scaled._plan().catalog_key
    assert list(scaled.fitted_parameters) == list(plain.fitted_parameters)
    want, got = plain.lnprob_batch(pos), scaled.lnprob_batch(pos)
    assert np.all(np.isfinite(want)) and np.array_equal(got, want)
    assert scaled._catalog.model == 10 and plain._catalog.model == 0
    assert np.array_equal(scaled._catalog.tables[-1], np.insert(plain._catalog.tables[-1], 4, 1.0, axis=1))
    # a free err_scale moves the value, and the host restatement of the reference API follows the device's
    scaled.parameters["err_scale"].set(fixed=False)
    scaled._catalog_key = scaled._plan().catalog_key
    live = np.concatenate([pos, np.linspace(0.4, 2.5, 16)[:, None]], axis=1)
    got = scaled.lnprob_batch(live)
    assert np.all(got != want)
    host = np.array([scaled.lnlike_host(row) for row in live])
    assert np.all(np.abs(host - got) <= 1e-11 * np.maximum(np.abs(got), 300.0))


def test_the_err_scale_accessor():
    from mcmc_dynamics_amd.analysis import ConstantFitES
    rd, _ = _reader()
    fit = _fix_centre(ConstantFitES(rd))
    rng = np.random.default_rng(3)
    chain = np.array([0.0, 5.0, 1.0, 1.0, 2.0]) + 0.01 * rng.normal(size=(6, 10, 5))
    got = fit.err_scale(chain, 2)
    assert got.shape == (48,) and np.allclose(np.sort(got), np.sort(chain[:, 2:, 4].reshape(-1)), rtol=1e-14)


@pytest.mark.parametrize("name", ["ConstantFitES", "ModelFitES"])
def test_lnlike_host_is_the_oracle_on_the_scaled_catalogue(name):
    """The host restatement of both classes (ModelFitES: a and r_peak in arcsec through the base class's model functions)
    against escale_helper's reference, 1e-11 on max(|lnL|, N)."""
    from mcmc_dynamics_amd import DataReader, analysis
    model = es.CONST_ES if name == "ConstantFitES" else es.PROFILE_ES
    case = es.make_case(model, False, 33)
    c = case["cat"]
    fit = getattr(analysis, name)(DataReader({k: c[k] for k in ("ra", "dec", "v", "verr")}))
    fit.parameters["ra_center"].set(value=vh.CENTRE[0], fixed=True)
    fit.parameters["dec_center"].set(value=vh.CENTRE[1], fixed=True)
    names, abi = list(fit.fitted_parameters), es.column_names(model, False)
    assert sorted(names) == sorted(abi)
    for w in ROWS:
        row = case["params"][w]
        got = fit.lnlike_host(row[[abi.index(k) for k in names]])
        want = es.exact(model, c, row, case["centre"])
        assert float(vh.scaled_err(got, want, 33)) < 1e-11, (name, w, got, float(want))
    dead = es.unit_rows(model, case["params"][:1])[0]
    assert abs(fit.lnlike_host(dead[[abi.index(k) for k in names]]) - fit.lnlike_host(case["params"][0][[abi.index(k) for k in names]])) > 1e-6

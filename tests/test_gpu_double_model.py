"""GPU: the double Lynden-Bell models (device models 7 and 8; analysis/double_model.py) through every launcher.

* the reference's golden vectors (tools/make_golden_double.py) through Runner.lnprob_batch, plain and fast kernels, and the
  per-star membership of the GB goldens;
* value and gradient against the longdouble helper (tests/double_helper.py) over models x centre x N in {1, 33, 4099} x W
  in {1, 65, 257} in chunks of 96 stars, bitwise repeatability, a binned catalogue against its un-binned bins;
* nesting: zero second amplitudes against the single-component models 3 and 4 on the same stars -- value, gradient and the
  summary launchers (pointwise posterior, PSIS-LOO, posterior predictive, replicate check);
* edges: a star on the centre, r_peak_ratio at both bounds, f_back = 0, rows outside the box, the float32 refusal;
* the resident stretch move (P = 9, and P = 14 with a normal prior), HMC and tempering blocks against their host-driven
  loops, bit for bit; hold-out refits and moment matching run and repeat bit for bit.

The summary, hold-out, moment-matching and weighted launchers with the second component LIVE (nothing here but value and
gradient feels slots 15 .. 18 of the walker row): tests/test_gpu_double_live.py."""
import os

import numpy as np
import pytest

import double_helper as dh
import grad_bounds as gb
import grad_helper as gh
import variant_helper as vh

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
STARS = (1, 33, 4099)
WALKERS = (1, 65, 257)
N = 4099


@pytest.fixture(scope="module")
def native():
    from mcmc_dynamics_amd import _native
    return _native


@pytest.fixture(scope="module")
def ctx(native):
    return native.default_context()


def open_catalog(native, ctx, case, sl=slice(None), model=None, **more):
    c = case["cat"]
    model = case["model"] if model is None else model
    kw = {"density": c["density"][sl]} if "density" in c else {}
    kw.update(more)
    cat = native.Catalog(ctx, c["ra"][sl], c["dec"][sl], c["v"][sl], c["verr"][sl], model=model, centre=case["centre"], **kw)
    cat.set_option("balance", 0)
    cat.set_option("chunk_len", vh.CHUNK_LEN)
    return cat


def close_to(got, want, tol=1e-12):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    err = np.abs(got - want) / np.maximum(np.abs(want), 1.0)
    return bool(np.all(err <= tol)), float(np.max(err)) if err.size else 0.0


# ------------------------------------------------------------------------------------------ goldens
def golden_runner(name):
    from mcmc_dynamics_amd import DataReader
    from mcmc_dynamics_amd.analysis import DoubleModelFit, DoubleModelFitGB
    g = dict(np.load(os.path.join(GOLDEN, name + ".npz"), allow_pickle=False))
    gb_ = "gb" in name
    cols = {k: g[k] for k in ("ra", "dec", "v", "verr") + (("density",) if gb_ else ())}
    fit = (DoubleModelFitGB if gb_ else DoubleModelFit)(DataReader(cols))
    if not name.endswith("free"):
        fit.parameters["ra_center"].set(value=float(g["ra_center"]), fixed=True)
        fit.parameters["dec_center"].set(value=float(g["dec_center"]), fixed=True)
    names = [str(n) for n in g["names"]]
    assert sorted(fit.fitted_parameters) == sorted(names)
    values = np.ascontiguousarray(g["values"][:, [names.index(n) for n in fit.fitted_parameters]])
    return g, fit, values


@pytest.mark.parametrize("name", ["double_model", "double_model_free", "double_model_gb", "double_model_gb_free"])
def test_goldens_through_the_runner(name):
    g, fit, values = golden_runner(name)
    ok = np.isfinite(g["lnprob"])
    n = len(g["v"])
    for fast_path in (1, 0):
        fit._ensure_catalog().set_option("fast_path", fast_path)
        got = fit.lnprob_batch(values)
        assert np.array_equal(np.isfinite(got), ok) and np.all(got[~ok] == -np.inf)      # rows outside the box: -inf, not NaN
        err = vh.scaled_err(got[ok], g["lnprob"][ok], n)
        print(name, "fast_path", fast_path, "level", fit._catalog.fast_level, "max scaled err {0:.3e}".format(err.max()))
        assert np.all(err < 1e-12)
        assert fit._catalog.fast_level == (1 if fast_path else 0)
    if "membership" in g:
        for i, want in zip(g["membership_rows"].astype(int), g["membership"]):
            got = fit.membership_probabilities(values[i])
            assert np.max(np.abs(got - want)) < 1e-11
    fit.close()


# ------------------------------------------------------------------------------------------ value and gradient matrix
def check_cell(cat, case, w, log):
    model, free, n = case["model"], case["free"], case["n"]
    params = np.ascontiguousarray(case["params"][:w])
    value, grad = cat.loglike_grad(params)
    assert value.shape == (w,) and grad.shape == (w, dh.n_columns(model, free))
    assert np.all(np.isfinite(grad)) and np.all(np.isfinite(value))
    value2, grad2 = cat.loglike_grad(params)
    assert value.tobytes() == value2.tobytes() and grad.tobytes() == grad2.tobytes(), ("not repeatable", model, free, n, w)
    out = {}
    for fast_path in (0, 1):
        cat.set_option("fast_path", fast_path)
        out[fast_path] = cat.loglike(params)
        assert cat.fast_level == fast_path, (model, free, n, w, cat.fast_level)
        assert out[fast_path].tobytes() == cat.loglike(params).tobytes()
    if n > 1:
        assert cat.launch_info()["chunks"] == -(-n // vh.CHUNK_LEN)
    failures = []
    for r in vh.sample_rows(w):
        ref = dh.reference(case, r)
        for name, got in (("gradient's value", value[r]), ("plain", out[0][r]), ("fast", out[1][r])):
            e = float(vh.scaled_err(got, ref["value"], n))
            log.append((n, w, r, name, e))
            if not e < 1e-12:
                failures.append((n, w, r, name, e))
        err = gh.col_err(grad[r], ref["g"], ref["s"])
        log.append((n, w, r, "gradient excess", float(np.max(err - 2 * ref["err64"]))))
        bound = 2 * ref["err64"] + dh.floors(model, free, n)
        if np.any(err > bound):
            failures.append((n, w, r, err.tolist(), bound.tolist()))
    return failures


@pytest.mark.parametrize("free", [False, True])
@pytest.mark.parametrize("model", dh.MODELS)
def test_value_and_gradient_against_the_longdouble_helper(native, ctx, model, free):
    log, failures = [], []
    for n in STARS:
        case = dh.make_case(model, free, n)
        cat = open_catalog(native, ctx, case)
        assert cat.k == dh.n_columns(model, free)
        for w in WALKERS:
            failures += check_cell(cat, case, w, log)
        cat.close()
        for name in ("plain", "fast", "gradient excess"):
            print("model {0} free {1} N = {2}: worst {3} = {4:.3e}".format(
                model, int(free), n, name, max(t[4] for t in log if t[0] == n and t[3] == name)))
    assert not failures, failures


def test_binned_catalogue_matches_unbinned_bins(native, ctx):
    case = dh.make_case(dh.DOUBLE, False, N)
    offs = [0, 5, 705, N]
    w = 65
    params = np.ascontiguousarray(np.stack([case["params"][b * w:(b + 1) * w] for b in range(3)]))
    binned = open_catalog(native, ctx, case, bin_offsets=offs)
    value, grad = binned.loglike_grad(params)
    fast = binned.loglike(params)
    assert value.shape == (3, w) and grad.shape == (3, w, 9)
    for b in range(3):
        sl = slice(offs[b], offs[b + 1])
        sub = dict(case, cat={k: v[sl] for k, v in case["cat"].items()}, n=offs[b + 1] - offs[b], params=params[b])
        one = open_catalog(native, ctx, sub)
        v1, g1 = one.loglike_grad(params[b])
        f1 = one.loglike(params[b])
        one.close()
        assert np.all(vh.scaled_err(value[b], v1, sub["n"]) < 1e-12) and np.all(vh.scaled_err(fast[b], f1, sub["n"]) < 1e-12)
        for r in vh.sample_rows(w):
            ref = dh.reference(sub, r)
            gb.check_columns(grad[b, r], ref, ("bin", b, r), dh.floors(dh.DOUBLE, False, sub["n"]))
            gb.check_columns(g1[r], ref, ("un-binned", b, r), dh.floors(dh.DOUBLE, False, sub["n"]))
            assert vh.scaled_err(fast[b, r], ref["value"], sub["n"]) < 1e-12
    binned.close()


# ------------------------------------------------------------------------------------------ nesting
def chain_rows(case, s, seed=3):
    """`s` rows in a tight ball around row 0 of `case` (a posterior-like table), r_peak_ratio and f_back kept in their boxes."""
    rng = np.random.default_rng(seed)
    model, free = case["model"], case["free"]
    base = case["params"][0]
    scale = dh.column_scales(model, free, base, case["scale"])
    names = dh.column_names(model, free)
    width = np.array([1e-5 if n in ("ra_center", "dec_center") else 0.01 for n in names]) * np.where(scale > 0, scale, 1.0)
    rows = base + width * rng.normal(size=(s, base.size))
    rows[:, 8] = np.clip(rows[:, 8], 1e-3, 1.0)
    if model == dh.DOUBLE_GB:
        rows[:, -1] = np.clip(rows[:, -1], 0.0, 1.0)
    return np.ascontiguousarray(rows)


@pytest.mark.parametrize("free", [False, True])
@pytest.mark.parametrize("model", dh.MODELS)
def test_zero_second_amplitudes_are_the_single_component_model(native, ctx, model, free):
    case = dh.make_case(model, free, N)
    rows, base_rows = dh.nested_rows(case["params"][:65])
    double = open_catalog(native, ctx, case)
    single = open_catalog(native, ctx, case, model=dh.BASE[model])
    v2, g2 = double.loglike_grad(rows)
    v1, g1 = single.loglike_grad(base_rows)
    assert np.all(vh.scaled_err(v2, v1, N) < 1e-13)
    for fast_path in (0, 1):                               # (the single-component catalogue may take its level-2 variant)
        double.set_option("fast_path", fast_path)
        single.set_option("fast_path", 2 if fast_path else 0)
        assert np.all(vh.scaled_err(double.loglike(rows), single.loglike(base_rows), N) < 1e-13), fast_path
    shared = [k for k in range(rows.shape[1]) if k not in (6, 7, 8)]
    nested_case = dict(case, params=rows)
    for r in vh.sample_rows(65):
        ref = dh.reference(nested_case, r)
        err = gh.col_err(g2[r][shared], g1[r], ref["s"][shared])
        assert np.all(err < 1e-13), (r, err.tolist())
        assert np.all(g2[r][[6, 7]] != 0.0)
        gb.check_columns(g2[r], ref, (model, free, "nested", r), dh.floors(model, free, N))
    double.close()
    single.close()


@pytest.mark.parametrize("model", dh.MODELS)
def test_summary_launchers_agree_with_the_single_component_model(native, ctx, model):
    """S = 64 samples with zero second amplitudes on N = 4099 stars: every summary launcher of the double catalogue against
    the same launcher of the single-component catalogue."""
    case = dh.make_case(model, False, N)
    rows, base_rows = dh.nested_rows(chain_rows(case, 64))
    double = open_catalog(native, ctx, case)
    single = open_catalog(native, ctx, case, model=dh.BASE[model])
    mem = model == dh.DOUBLE_GB
    order, offs = np.arange(N), [0, 1500, N]
    calls = {
        "pointwise_posterior": lambda c, t: c.pointwise_posterior(t, membership=mem),
        "psis_loo": lambda c, t: c.psis_loo(t),
        "posterior_predictive": lambda c, t: c.posterior_predictive(t, mixture=mem),
        "replicate_check": lambda c, t: {"fields": c.replicate_check(t, 7, offs, order)},
    }
    worst = {}
    for name, call in calls.items():
        got, want = call(double, rows), call(single, base_rows)
        assert sorted(got) == sorted(want)
        for key in got:
            assert np.all(np.isfinite(got[key])), (name, key)
            ok, err = close_to(got[key], want[key])
            worst[name + "." + key] = err
    print("model", model, {k: "{0:.2e}".format(v) for k, v in worst.items()})
    assert all(v <= 1e-12 for v in worst.values()), {k: v for k, v in worst.items() if v > 1e-12}
    double.close()
    single.close()


# ------------------------------------------------------------------------------------------ edges
@pytest.mark.parametrize("free", [False, True])
@pytest.mark.parametrize("model", dh.MODELS)
def test_star_on_the_centre_ratio_bounds_and_f_back_zero(native, ctx, model, free):
    case = dh.make_case(model, free, 33)
    c = case["cat"]
    case["params"] = np.ascontiguousarray(case["params"][:3])
    case["params"][0, 8], case["params"][1, 8] = 1.0, 1e-3
    if model == dh.DOUBLE_GB:
        case["params"][2, -1] = 0.0                               # f_back = 0: every star a certain member
    if free:
        c["ra"], c["dec"] = c["ra"] - vh.CENTRE[0], c["dec"] - vh.CENTRE[1]
        case["params"][:, 9:11] -= np.array(vh.CENTRE)
        case["params"][0, 9:11] = 0.0
        c["ra"][-1], c["dec"][-1] = 0.0, 0.0
    else:
        c["ra"][-1], c["dec"][-1] = vh.CENTRE
    cat = open_catalog(native, ctx, case)
    value, grad = cat.loglike_grad(case["params"])
    assert np.all(np.isfinite(value)) and np.all(np.isfinite(grad))
    for fast_path in (0, 1):
        cat.set_option("fast_path", fast_path)
        got = cat.loglike(case["params"])
        for r in range(3):
            assert vh.scaled_err(got[r], dh.reference(case, r)["value"], 33) < 1e-12, (fast_path, r)
    for r in range(3):
        gb.check_columns(grad[r], dh.reference(case, r), (model, free, "edges", r), dh.floors(model, free, 33))
    cat.close()


def test_float32_catalogues_are_refused(native, ctx):
    case = dh.make_case(dh.DOUBLE, False, 33)
    c = case["cat"]
    for precision in ("f32", "f32acc64"):
        with pytest.raises(native.NativeError, match="float64 only"):
            native.Catalog(ctx, c["ra"], c["dec"], c["v"], c["verr"], model=dh.DOUBLE, centre=case["centre"], precision=precision)
    with pytest.raises(native.NativeError, match="unknown model"):
        native.Catalog(ctx, c["ra"], c["dec"], c["v"], c["verr"], model=9, centre=case["centre"])


# ------------------------------------------------------------------------------------------ resident == host-driven
def ensemble(case, w, seed=11):
    """W start positions in a ball around row 0 (a few posterior widths of a 4099-star catalogue) and the box."""
    pos = chain_rows(case, w, seed=seed)
    names = dh.column_names(case["model"], case["free"])
    lo, hi = np.full(len(names), -np.inf), np.full(len(names), np.inf)
    for name, (a, b) in {"sigma_max": (0.0, np.inf), "a": (1.0, np.inf), "r_peak": (1.0, np.inf), "r_peak_ratio": (1e-3, 1.0),
                         "sigma_back": (0.0, np.inf), "f_back": (0.0, 1.0)}.items():
        if name in names:
            lo[names.index(name)], hi[names.index(name)] = a, b
    k = len(names)
    plan = {"col_source": np.arange(k, dtype=np.int32), "col_const": np.zeros(k), "col_factor": np.ones(k), "lo": lo, "hi": hi,
            "fixed_ok": True}
    return pos, plan


@pytest.mark.parametrize("model, free, prior", [(dh.DOUBLE, False, False), (dh.DOUBLE_GB, True, True)])
def test_resident_stretch_move_is_the_host_driven_loop(native, ctx, model, free, prior):
    """64 walkers x 20 seeded steps at P = 9 (the in-LDS step kernel) and at P = 14 with a normal prior on v_sys (more than
    the 12 columns that kernel holds: the general step kernel)."""
    case = dh.make_case(model, free, N)
    cat = open_catalog(native, ctx, case)
    pos0, plan = ensemble(case, 64)
    assert pos0.shape[1] == (14 if free else 9) == cat.k
    if prior:
        kind, p0, p1 = np.zeros(cat.k, dtype=np.int32), np.zeros(cat.k), np.ones(cat.k)
        kind[0], p0[0], p1[0] = 1, pos0[0, 0], 0.05 * case["scale"]
        plan = dict(plan, prior=(kind, p0, p1))
    lnp0 = cat.loglike(pos0)
    if prior:
        lnp0 = lnp0 + native.prior_eval(plan["prior"], pos0)           # the _prior form carries lnL + ln prior
    assert np.all(np.isfinite(lnp0))
    runs = {}
    for device in (1, 0):
        cat.set_option("device_chain", device)
        pos, lnp = pos0.copy(), lnp0.copy()
        chain, lnpc, acc = np.full((20, 64, cat.k), np.nan), np.full((20, 64), np.nan), np.zeros(64, dtype=np.int64)
        before = cat.stretch_info()
        cat.stretch_move_seeded(plan, pos, lnp, 23, 4, 20, chain, lnpc, acc)
        after = cat.stretch_info()
        key = "device_blocks" if device else "host_blocks"
        assert after[key] == before[key] + 1 and after["discarded_blocks"] == before["discarded_blocks"], (device, before, after)
        runs[device] = (pos, lnp, chain, lnpc, acc)
    cat.set_option("device_chain", 1)
    for a, b in zip(runs[1], runs[0]):
        assert a.tobytes() == b.tobytes()
    assert np.all(np.isfinite(runs[1][3])) and 0 < runs[1][4].sum() < 20 * 64
    cat.close()


def test_resident_hmc_block_is_the_host_driven_loop(native, ctx):
    import test_gpu_hmc as hmc_cases
    case = dh.make_case(dh.DOUBLE, False, N)
    cat = open_catalog(native, ctx, case)
    pos, plan = ensemble(case, 16)
    chol = np.diag(0.003 * np.where(dh.column_scales(dh.DOUBLE, False, pos[0], case["scale"]) > 0,
                                    dh.column_scales(dh.DOUBLE, False, pos[0], case["scale"]), 1.0))
    dev = hmc_cases.run(cat, plan, chol, 0.5, 2, pos, 31, 2, 5, resident=True)
    host = hmc_cases.run(cat, plan, chol, 0.5, 2, pos, 31, 2, 5, resident=False)
    assert (dev["device_blocks"], dev["host_blocks"]) == (1, 0) and (host["device_blocks"], host["host_blocks"]) == (0, 1)
    for key in hmc_cases.KEYS:
        assert dev[key].tobytes() == host[key].tobytes(), key
    assert np.all(np.isfinite(dev["chain"])) and np.all(np.isfinite(dev["lnprob_chain"]))
    assert dev["accepted"].sum() > 0 and not np.array_equal(dev["pos"], pos)
    cat.close()


def test_resident_temper_block_is_the_host_driven_loop(native, ctx):
    import test_gpu_temper as temper_cases
    case = dh.make_case(dh.DOUBLE, False, N)
    cat = open_catalog(native, ctx, case)
    pos, plan = ensemble(case, 4 * 16)
    pos = np.ascontiguousarray(pos.reshape(4, 16, 9))
    ll = temper_cases.plain_loglike(cat, plan, pos.reshape(64, 9), 4 * 8).reshape(4, 16)
    betas = np.array([1.0, 0.5, 0.25, 0.0])
    dev = temper_cases.run(cat, plan, betas, pos, ll, 31, 3, 10, resident=True)
    host = temper_cases.run(cat, plan, betas, pos, ll, 31, 3, 10, resident=False)
    assert (dev["device_blocks"], dev["host_blocks"]) == (1, 0) and (host["device_blocks"], host["host_blocks"]) == (0, 1)
    for key in temper_cases.KEYS:
        assert dev[key].tobytes() == host[key].tobytes(), key
    assert np.all(np.isfinite(dev["chain"])) and np.all(np.isfinite(dev["lnlike_chain"]))
    assert dev["accepted"].sum() > 0 and not np.array_equal(dev["pos"], pos)
    cat.close()


# ------------------------------------------------------------------------------------------ hold-out and moment matching
def test_holdout_fit_and_moment_matching_run_and_repeat(ctx):
    from mcmc_dynamics_amd import DataReader
    from mcmc_dynamics_amd.analysis import DoubleModelFit
    case = dh.make_case(dh.DOUBLE, False, 33)
    c = case["cat"]
    fit = DoubleModelFit(DataReader({k: c[k] for k in ("ra", "dec", "v", "verr")}))
    fit.parameters["ra_center"].set(value=vh.CENTRE[0], fixed=True)
    fit.parameters["dec_center"].set(value=vh.CENTRE[1], fixed=True)
    fit.parameters["v_maxx_c"].set(min=-np.inf, max=np.inf)          # (make_case's velocity scale may exceed 50 km/s)
    fit.parameters["v_maxy_c"].set(min=-np.inf, max=np.inf)
    names = dh.column_names(dh.DOUBLE, False)
    assert sorted(fit.fitted_parameters) == sorted(names)
    cols = [names.index(n) for n in fit.fitted_parameters]
    rows = np.ascontiguousarray(chain_rows(case, 2 * 20, seed=5)[:, cols])
    sets = [np.array([0, 3, 7]), np.array([12, 30])]
    runs = [fit.holdout_fit(sets, n_walkers=20, n_steps=12, n_burn=4, pos=rows.reshape(2, 20, 9), seed=19) for _ in range(2)]
    held = np.concatenate(sets)
    for key in ("elpd", "lnl_var"):
        assert runs[0][key].tobytes() == runs[1][key].tobytes()
        assert np.all(np.isfinite(runs[0][key][held])) and np.isnan(np.delete(runs[0][key], held)).all()
    assert np.asarray(runs[0]["sampler"].chain).tobytes() == np.asarray(runs[1]["sampler"].chain).tobytes()
    sampler = fit(n_walkers=20, n_steps=30, n_out=None, prefix=None, pos=np.ascontiguousarray(rows[:20]))
    chain = np.asarray(sampler.chain)
    loo = fit.loo(chain, n_burn=10)
    matched = [fit.loo_moment_match(loo, chain, n_burn=10, stars=[1, 4, 32], max_iters=3) for _ in range(2)]
    for key in ("pointwise", "pareto_k", "k_before", "iterations"):
        assert np.asarray(matched[0][key]).tobytes() == np.asarray(matched[1][key]).tobytes(), key
    assert np.array_equal(matched[0]["matched"], [1, 4, 32]) and np.all(np.isfinite(matched[0]["pointwise"]))
    fit.close()

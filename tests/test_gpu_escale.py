"""GPU: the error-scale models (device models 10 and 11; ConstantFitES / ModelFitES) through every launcher of the library,
on LIVE rows: err_scale spread over [0.3, 3], different in every row (escale_helper.make_case / chain_rows).

The reference of every launcher is the project's own oracle on a copy of the catalogue whose error column is multiplied by
the row's err_scale (escale_helper; variant_helper / grad_helper / predictive_helper / replicate_helper restatements on
oracle/lnprob_numpy.py, one evaluation per row), and the comparison rule and the bound are the ones each launcher's own test
applies to models 0 and 3 (tests/test_gpu_double_live.py has them side by side).  Every accuracy cell with N >= 33 carries
escale_helper.guard: the reference on the live rows and on the same rows with err_scale = 1 differ by a median over the
stars of >= 1e-6 -- a launcher that never read slot 19 of the walker row cannot pass.

Chains: a seeded resident stretch block and a DE block of 40 steps at N = 4099 against the host-driven block (and the DE
block against de_helper's NumPy loop) with array_equal, one stretch block from a start so wide in err_scale that the guard
hands it back; HMC and tempering blocks against their host-driven forms.  End to end: ConstantFitES on 2 000 stars whose
stated errors are half the true ones recovers err_scale = 2 and sigma_max = 5 within 4 Laplace standard deviations, where
ConstantFit's sigma_max lies more than 4 of its own above 5."""
import numpy as np
import pytest

import de_helper
import escale_helper as es
import grad_bounds as gb
import grad_helper as gh
import holdout_helper as hh
import mmatch_helper as mh
import predictive_helper as pr
import psis_helper as psh
import replicate_helper as rh
import variant_helper as vh
import weighted_helper as wh
from test_posterior_cpu import rel, var_ok

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not vh.HAVE_LONGDOUBLE, reason="numpy.longdouble is not wider than float64 here")]

L = vh.L
CELLS, CELL_IDS = es.CELLS, es.CELL_IDS
SEED = wh.SEED


@pytest.fixture(scope="module")
def native():
    from mcmc_dynamics_amd import _native
    return _native


@pytest.fixture(scope="module")
def ctx(native):
    return native.default_context()


# ------------------------------------------------------------------------------------------ references, computed once
_cases, _tables, _terms = {}, {}, {}


def case_of(model, free, n):
    if (model, free, n) not in _cases:
        _cases[(model, free, n)] = es.make_case(model, free, n)
    return _cases[(model, free, n)]


def table_of(case, s, seed=3):
    key = (case["model"], case["free"], case["n"], s, seed)
    if key not in _tables:
        _tables[key] = es.chain_rows(case, s, seed=seed)
    return _tables[key]


def terms_of(case, row, dtype=L):
    key = (case["model"], case["free"], case["n"], np.asarray(row).tobytes(), np.dtype(dtype).name)
    if key not in _terms:
        _terms[key] = es.per_star(case["model"], case["cat"], row, case["centre"], dtype)
    return _terms[key]


def term_matrix(case, rows, dtype=L):
    return np.array([terms_of(case, row, dtype) for row in rows])


def open_catalog(native, ctx, case, **more):
    cat = es.open_catalog(native, ctx, case, **more)
    cat.set_option("balance", 0)
    cat.set_option("chunk_len", vh.CHUNK_LEN)
    return cat


def star_sample(n):
    if n <= 140:
        return np.arange(n)
    return np.unique(np.concatenate([np.arange(70), np.arange(n - 70, n), np.arange(0, n, 17)]))


def device_lnl(gpu, rows):
    """(S, N) per-star terms: the models without a background have no loglike_per_star; pointwise_posterior's lppd over ONE
    sample is the term itself."""
    return np.array([gpu.pointwise_posterior(row[None, :])["lppd"] for row in rows])


# ------------------------------------------------------------------------------------------ creation
def test_catalogue_creation_columns_and_refusals(native, ctx):
    case = case_of(es.CONST_ES, False, 33)
    c = case["cat"]
    for model, free in CELLS:
        cs = case_of(model, free, 33)
        cat = es.open_catalog(native, ctx, cs)
        assert cat.k == es.n_columns(model, free)
        cat.close()
    for model in es.MODELS:
        for precision in ("f32", "f32acc64"):
            with pytest.raises(native.NativeError, match="float64 only"):
                native.Catalog(ctx, c["ra"], c["dec"], c["v"], c["verr"], model=model, centre=case["centre"], precision=precision)
    for unknown in (9, 12):                                 # (9 stays unassigned)
        with pytest.raises(native.NativeError, match="unknown model"):
            native.Catalog(ctx, c["ra"], c["dec"], c["v"], c["verr"], model=unknown, centre=case["centre"])


# ------------------------------------------------------------------------------------------ value and gradient
@pytest.mark.parametrize("model, free", CELLS, ids=CELL_IDS)
def test_value_plain_and_fast_and_gradient_against_the_scaled_catalogue_reference(native, ctx, model, free):
    """loglike_batch at the plain and the fast level and loglike_grad_batch, N in {1, 33, 4099} x W in {1, 65, 257}:
    1e-12 on max(|lnL|, N); gradient columns err <= 2 err_np64 + floor (escale_helper.floors)."""
    failures, worst = [], {}
    for n in (1, 33, 4099):
        case = case_of(model, free, n)
        cat = open_catalog(native, ctx, case)
        floors = es.floors(model, free, n)
        for w in (1, 65, 257):
            params = np.ascontiguousarray(case["params"][:w])
            es.guard(case, params, "value / gradient")
            value, grad = cat.loglike_grad(params)
            assert value.shape == (w,) and grad.shape == (w, es.n_columns(model, free)) and np.all(np.isfinite(grad))
            again = cat.loglike_grad(params)
            assert value.tobytes() == again[0].tobytes() and grad.tobytes() == again[1].tobytes()
            out = {}
            for fast_path in (0, 1):
                cat.set_option("fast_path", fast_path)
                out[fast_path] = cat.loglike(params)
                assert cat.fast_level == fast_path, (model, free, n, w, cat.fast_level)
                assert out[fast_path].tobytes() == cat.loglike(params).tobytes()
            for r in vh.sample_rows(w):
                ref = es.reference(case, r)
                for name, got in (("gradient's value", value[r]), ("plain", out[0][r]), ("fast", out[1][r])):
                    e = float(vh.scaled_err(got, ref["value"], n))
                    worst[name] = max(worst.get(name, 0.0), e)
                    if not e < 1e-12:
                        failures.append((n, w, r, name, e))
                err = gh.col_err(grad[r], ref["g"], ref["s"])
                worst["gradient excess"] = max(worst.get("gradient excess", -np.inf), float(np.max(err - 2 * ref["err64"])))
                bound = 2 * ref["err64"] + floors
                if np.any(err > bound):
                    failures.append((n, w, r, err.tolist(), bound.tolist()))
        cat.close()
    print("value / gradient model", model, int(free), {k: "%.2e" % v for k, v in worst.items()})
    assert not failures, failures


# ------------------------------------------------------------------------------------------ per-star terms, pointwise posterior
@pytest.mark.parametrize("model, free", CELLS, ids=CELL_IDS)
def test_per_star_terms_and_pointwise_posterior(native, ctx, model, free):
    """loglike_per_star / membership refuse the models without a background; the terms (pointwise_posterior over one
    sample) to 1e-12 on max(|l_i|, 1); S in {1, 65, 257} x N in {1, 65, 4099}: lppd to 1e-11 (fixed) / 1e-12 (free)
    relative, variances by var_ok with rtol 1e-10 (the bounds of tests/test_gpu_posterior.py)."""
    worst = {"terms": 0.0, "lppd": 0.0}
    for n in (1, 65, 4099):
        case = case_of(model, free, n)
        gpu = open_catalog(native, ctx, case)
        table = table_of(case, 257)
        es.guard(case, table, "pointwise_posterior")
        for call in (gpu.loglike_per_star, gpu.membership):
            with pytest.raises(native.NativeError, match="background model"):
                call(table[0])
        x80 = term_matrix(case, table)
        for r in vh.sample_rows(257):
            e = es.term_err(gpu.pointwise_posterior(table[r][None, :])["lppd"], x80[r])
            worst["terms"] = max(worst["terms"], e)
            assert e < 1e-12, (n, r, e)
        for s in (1, 65, 257):
            got = gpu.pointwise_posterior(table[:s])
            assert sorted(got) == ["lnl_var", "lppd"]
            x = x80[:s]
            mx = x.max(axis=0)
            lppd = (mx + np.log(np.exp(x - mx).sum(axis=0)) - np.log(L(s))).astype(np.float64)
            var = (x.var(axis=0, ddof=1) if s > 1 else np.zeros(n)).astype(np.float64)
            e = rel(got["lppd"], lppd)
            worst["lppd"] = max(worst["lppd"], e)
            assert e < (1e-12 if free else 1e-11), (n, s, e)
            assert var_ok(got["lnl_var"], var, lppd, rtol=1e-10), (n, s)
        gpu.close()
    print("per-star / pointwise_posterior model", model, int(free), {k: "%.2e" % v for k, v in worst.items()})


# ------------------------------------------------------------------------------------------ PSIS-LOO and its expectations
_lnl = {}


def lnl_rows(case, gpu, s=1000):
    """The device's (N, s) lnL rows of the cell's table, computed once, pinned to the longdouble terms on a sample of rows."""
    key = (case["model"], case["free"], case["n"], s)
    if key not in _lnl:
        table = table_of(case, s)
        x = device_lnl(gpu, table)
        worst = max(es.term_err(x[r], terms_of(case, table[r])) for r in vh.sample_rows(s))
        print("lnL rows", key, "against the longdouble terms: %.2e" % worst)
        assert worst < 1e-12, (key, worst)
        _lnl[key] = np.ascontiguousarray(x.T)
    return _lnl[key]


@pytest.mark.parametrize("n", [33, 4099])
@pytest.mark.parametrize("model, free", CELLS, ids=CELL_IDS)
def test_psis_loo_matches_the_oracle(native, ctx, model, free, n):
    case = case_of(model, free, n)
    gpu = open_catalog(native, ctx, case)
    s_all = 1000 if n == 33 else 300
    table = table_of(case, s_all)
    es.guard(case, table, "psis_loo")
    lnl = lnl_rows(case, gpu, s_all)
    some = star_sample(n)
    for s in (130, s_all):
        got = gpu.psis_loo(table[:s])
        assert all(v.shape == (n,) for v in got.values())
        sub = np.ascontiguousarray(lnl[some, :s])
        psh.assert_matches({k: v[some] for k, v in got.items()}, psh.numpy_psis(sub), k_tol=np.maximum(1e-10, 10.0 * psh.k_noise(sub)))
        pp = gpu.pointwise_posterior(table[:s])
        assert np.all(np.abs(got["lppd"] - pp["lppd"]) <= 1e-13 * np.maximum(np.abs(pp["lppd"]), 1.0))
    gpu.close()


def predictive_terms(case, rows, dtype, sl=slice(None)):
    """predictive_helper.star_terms of the base model, row by row on the catalogue scaled by the row's err_scale: dict of
    (S, n) arrays.  z, tail_p and pit standardise with the TOTAL variance, sig stays the model's sigma_los."""
    model, base = case["model"], es.BASE[case["model"]]
    cat = {k: np.asarray(v)[sl] for k, v in case["cat"].items()}
    base_rows, s = es.split_rows(model, rows)
    per = [pr.star_terms(es.scaled_cat(cat, dtype(s[j]), dtype), base_rows[j], base, case["centre"], dtype) for j in range(len(base_rows))]
    return {k: np.array([r[k] for r in per]) for k in per[0]}


def centres_of(case, table):
    if case["centre"] is not None:
        return case["centre"]
    k = es.ES_COLUMN[case["model"]] + 1
    return table[:, k], table[:, k + 1]


@pytest.mark.parametrize("model, free", CELLS, ids=CELL_IDS)
def test_psis_loo_expect_follows_the_rule(native, ctx, model, free):
    """loo_expect_helper's rule as tests/test_gpu_loo_expect.py applies it, N = 33, S in {130, 400}: against the oracle fed
    the device's lnL rows and (a) the NumPy terms of the scaled catalogues for the stars clear of the centres, (b) the
    device's own per-sample terms."""
    import loo_expect_helper as lh
    from oracle import lnprob_numpy as oracle
    from test_gpu_loo_expect import _device_terms
    n, s_all = 33, 400
    case = case_of(model, free, n)
    gpu = open_catalog(native, ctx, case)
    table = table_of(case, s_all)
    es.guard(case, table, "psis_loo_expect")
    lnl = lnl_rows(case, gpu, s_all)
    keys = list(lh.PRED)
    t = predictive_terms(case, table, np.float64)
    x_all = np.ascontiguousarray(np.stack([t[lh.TERM_KEY[k]].T for k in keys], axis=1))
    own_all = _device_terms(gpu, table, keys)
    unit = tuple(i for i, k in enumerate(keys) if k == "pit")
    ra_c, dec_c = (np.atleast_1d(np.asarray(a, dtype=np.float64)) for a in centres_of(case, table))
    dx, dy = oracle.calc_xy_offset(case["cat"]["ra"][:, None], case["cat"]["dec"][:, None], ra_c[None, :], dec_c[None, :])
    clear = np.hypot(dx, dy).min(axis=1) >= 0.8
    print("stars clear of the centres:", int(clear.sum()), "of", clear.size)
    for s in (130, s_all):
        got = gpu.psis_loo_expect(table[:s])
        assert "pit_mix" not in got
        rows = np.stack([got[k] for k in keys], axis=1)
        k_hat, sub = got["pareto_k"], np.ascontiguousarray(lnl[:, :s])
        what = "model {0} free {1} ({2}, {3})".format(model, int(free), n, s)
        if clear.any():
            lh.check_expect({"rows": rows[clear], "pareto_k": k_hat[clear]}, sub[clear], x_all[clear][:, :, :s], unit_rows=unit,
                            what=what + " (NumPy terms)")
        lh.check_expect({"rows": rows, "pareto_k": k_hat}, sub, own_all[:, :, :s], unit_rows=unit, what=what + " (device terms)")
        ref = gpu.psis_loo(table[:s])
        assert np.array_equal(got["pareto_k"], ref["pareto_k"]) and np.array_equal(got["n_eff"], ref["n_eff"])
    gpu.close()


# ------------------------------------------------------------------------------------------ posterior predictive
@pytest.mark.parametrize("model, free", CELLS, ids=CELL_IDS)
def test_posterior_predictive_follows_the_rule(native, ctx, model, free):
    """N in {1, 65, 4099} x S in {1, 65, 257}, the rule and the floor (1e-12; spreads with rtol 1e-10) of
    tests/test_gpu_predictive.py.  The sigma_* outputs are the model's sigma_los, whatever err_scale."""
    for n in (1, 65, 4099):
        case = case_of(model, free, n)
        gpu = open_catalog(native, ctx, case)
        table = table_of(case, 257)
        es.guard(case, table, "posterior_predictive")
        exact, np64 = predictive_terms(case, table, L), predictive_terms(case, table, np.float64)
        assert float(np.median(np.abs(exact["z"][0] - predictive_terms(case, es.unit_rows(model, table[:1]), L)["z"][0]))) >= es.GUARD or n < 33
        vmax = float(np.max(np.abs(case["cat"]["v"])))
        for s in (1, 65, 257):
            got = gpu.posterior_predictive(table[:s])
            assert "pit_mix" not in got and all(v.shape == (n,) for v in got.values())
            pr.check_rule(got, pr.reduce_terms(exact, n, s), pr.reduce_terms(np64, n, s), vmax, var_ok, rtol=1e-10, cell=(model, free, n, s))
            if s == 1:
                assert all(np.all(got[f] == 0.0) for f in ("z_std", "vlos_std", "sigma_std"))
        gpu.close()


# ------------------------------------------------------------------------------------------ replicate check
@pytest.mark.parametrize("model, free", CELLS, ids=CELL_IDS)
def test_replicate_check_follows_the_rule(native, ctx, model, free):
    """N in {65, 4099}, 65 sample rows, two ranges over a permuted order that leaves a tenth of the stars out: the observed
    residual standardises with the total variance; replicate_helper's rule and floor."""
    base = es.BASE[model]
    for n in (65, 4099):
        case = case_of(model, free, n)
        gpu = open_catalog(native, ctx, case)
        table = table_of(case, 65)
        es.guard(case, table, "replicate_check")
        order = np.random.default_rng(n).permutation(n).astype(np.int64)[:n - n // 10]
        offs = np.array([0, order.size // 3, order.size], dtype=np.int64)
        got = gpu.replicate_check(table, rh.SEED, offs, order)
        assert got.shape == (65, 2, 8, 2)
        g, u = rh.numbers(rh.SEED, 0, 65, 0, n)
        base_rows, s = es.split_rows(model, table)
        runs = {}
        for dtype in (L, np.float64):
            per = [rh.star_terms(es.scaled_cat(case["cat"], dtype(s[j]), dtype), base_rows[j], base, case["centre"], g[j], u[j],
                                 (np.nan, np.nan), dtype) for j in range(65)]
            runs[dtype] = {k: np.array([r[k] for r in per]) for k in per[0]}
        for key in ("z_obs", "z_rep"):
            assert np.min(np.abs(np.abs(runs[L][key]) - 3)) > 1e-9, (key, "a |z| within 1e-9 of 3: choose another seed")
        e, sc = rh.fields_of(runs[L], offs, order)
        d, _ = rh.fields_of(runs[np.float64], offs, order)
        rh.check_rule(got, e, d, sc.astype(np.float64), cell=(model, free, n))
        assert got.tobytes() == gpu.replicate_check(table, rh.SEED, offs, order).tobytes()
        gpu.close()


# ------------------------------------------------------------------------------------------ hold-out
@pytest.mark.parametrize("n", [33, 4099])
@pytest.mark.parametrize("model, free", CELLS, ids=CELL_IDS)
def test_holdout_against_longdouble_sums(native, ctx, model, free, n):
    """(E, W) in {(1, 2), (3, 66)} with the prefix sets of sizes (1, 0, 7): 1e-12 on max(|lnL|, N)."""
    case = case_of(model, free, n)
    gpu = open_catalog(native, ctx, case)
    worst = 0.0
    for E, W in ((1, 2), (3, 66)):
        offs = hh.sets_of_sizes((1, 0, 7), n)[:E + 1]
        table = table_of(case, E * W, seed=5)
        es.guard(case, table, "holdout")
        train, test = gpu.holdout_loglike(offs, table.reshape(E, W, -1))
        assert train.shape == test.shape == (E, W)
        for e in range(E):
            b0, b1 = int(offs[e]), int(offs[e + 1])
            for w in vh.sample_rows(W):
                l = terms_of(case, table[e * W + w])
                held = l[b0:b1].sum()
                for got, want in ((train[e, w], l.sum() - held), (test[e, w], held)):
                    err = float(vh.scaled_err(got, want, n))
                    worst = max(worst, err)
                    assert err <= 1e-12, (E, W, e, w, got, float(want), err)
            if b1 == b0:
                assert np.all(test[e] == 0.0) and not np.any(np.signbit(test[e]))
        again = gpu.holdout_loglike(offs, table.reshape(E, W, -1))
        assert again[0].tobytes() == train.tobytes() and again[1].tobytes() == test.tobytes()
    print("holdout model", model, int(free), "N", n, "largest error on max(|lnL|, N): %.2e" % worst)
    gpu.close()


# ------------------------------------------------------------------------------------------ moment matching
def box_plan(case, margin=None):
    names = es.column_names(case["model"], case["free"])
    lo, hi = np.full(len(names), -np.inf), np.full(len(names), np.inf)
    for name, (a, b) in {"sigma_max": (0.0, np.inf), "a": (1.0, np.inf), "r_peak": (1.0, np.inf), "err_scale": (0.1, 10.0)}.items():
        if name in names:
            lo[names.index(name)], hi[names.index(name)] = a, b
    return de_helper.identity_plan(len(names), lo, hi)


@pytest.mark.parametrize("n, n_match, s", [(33, 3, 400), (4099, 1, 130)])
@pytest.mark.parametrize("model, free", CELLS, ids=CELL_IDS)
def test_moment_match_final_weights_against_the_oracle(native, ctx, model, free, n, n_match, s):
    """tests/test_gpu_mmatch.py: check_against_oracle's rule with the oracle's evaluate() made of escale_helper's terms
    (train = the sum over the other stars, test = the star's own term); every cell is within the 12 free parameters."""
    from test_gpu_mmatch import check_bookkeeping, stars_of
    case = case_of(model, free, n)
    gpu = open_catalog(native, ctx, case)
    gpu.set_option("fast_path", 0)
    draws, plan = table_of(case, s, seed=11), box_plan(case)
    es.guard(case, draws, "moment_match")
    stars = stars_of(n, n_match)
    got = gpu.moment_match(plan, draws, stars, -np.inf, max_iters=3)
    check_bookkeeping(got, draws.shape[1], 3)
    dtype = L if n * s <= 600000 else np.float64
    seen = {}

    def matrix(rows):
        key = rows.tobytes()
        if key not in seen:
            seen[key] = np.array([es.per_star(model, case["cat"], row, case["centre"], dtype) for row in rows])
        return seen[key]

    inside = lambda rows: np.all((rows >= plan["lo"]) & (rows <= plan["hi"]), axis=1)
    lnprior = lambda rows: np.zeros(len(rows))
    delta = 2e-12 * max(abs(float(matrix(draws[:1]).sum())), n)
    for e, star in enumerate(stars):
        def ev(rows, star=int(star)):
            x = matrix(np.ascontiguousarray(rows))
            te = x[:, star]
            return (x.sum(axis=1) - te).astype(np.float64), te.astype(np.float64)
        want = mh.moment_match(draws, ev, inside, lnprior, 0.0, fixed_map=(got["A"][e], got["b"][e]))
        moved = {"pareto_k": 0.0, "n_eff": 0.0, "elpd": 0.0}
        for seed in (0, 1):
            sign = np.where(np.random.default_rng(seed).uniform(size=draws.shape[0]) < 0.5, -1.0, 1.0)
            lw_s, k = mh.psis_lw(want["lw_raw"] + sign * delta)
            elpd, n_eff, _ = mh.weights_summary(lw_s, want["li"])
            for key, v in (("pareto_k", k), ("n_eff", n_eff), ("elpd", elpd)):
                d = abs(v - want[key])
                moved[key] = max(moved[key], d if np.isfinite(d) else 0.0)
        for key in moved:
            g, w = float(got[key][e]), float(want[key])
            if not np.isfinite(w):
                assert g == w or (np.isnan(g) and np.isnan(w)), (key, e, g, w)
                continue
            tol = max(1e-10 * max(1.0, abs(w)), 10.0 * moved[key])
            print("star %d %s: device %.17g oracle %.17g diff %.3e bound %.3e" % (star, key, g, w, abs(g - w), tol))
            assert abs(g - w) <= tol, (key, e, g, w, tol)
        seen = {draws.tobytes(): seen[draws.tobytes()]} if draws.tobytes() in seen else {}
    gpu.close()


# ------------------------------------------------------------------------------------------ weighted gradient and value
def weighted_reference(case, row, w):
    """weighted_helper.reference with escale_helper's terms."""
    model, cat, centre = case["model"], case["cat"], case["centre"]
    key = ("w", model, case["free"], case["n"], np.asarray(row).tobytes())
    if key not in _terms:
        _terms[key] = {"v80": es.per_star(model, cat, row, centre, L), "g80": es.grad_terms(model, cat, row, centre, L),
                       "g64": es.grad_terms(model, cat, row, centre, np.float64)}
    t = _terms[key]
    keep = np.asarray(w) != 0
    w80, w64 = np.asarray(w, dtype=L)[keep], np.asarray(w, dtype=np.float64)[keep]
    g80 = (t["g80"][:, keep] * w80).sum(axis=1)
    s80 = (np.abs(t["g80"][:, keep]) * w80).sum(axis=1)
    g64 = (t["g64"][:, keep] * w64).sum(axis=1)
    return {"value": (t["v80"][keep] * w80).sum(), "sum_w": w80.sum(), "g": g80, "s": s80, "err64": gh.col_err(g64, g80, s80)}


@pytest.mark.parametrize("n", [33, 4099])
@pytest.mark.parametrize("model, free", CELLS, ids=CELL_IDS)
def test_weighted_calls_against_the_longdouble_weighted_sums(native, ctx, model, free, n):
    """Three schemes x rows in {2, 66, 258}: weighted_helper.check_row against the weighted longdouble sums with
    escale_helper.floors, and the value kernel against the gradient call's value, 1e-12 on max(|sum w l|, sum w)."""
    case = case_of(model, free, n)
    gpu = open_catalog(native, ctx, case)
    floors = es.floors(model, free, n)
    worst = [0.0, 0.0, -np.inf]
    for rows in (2, 66, 258):
        table = np.ascontiguousarray(case["params"][:rows])
        es.guard(case, table, "weighted")
        for scheme in ("exponential", "poisson", "explicit"):
            rep, explicit = wh.row_replicates(rows), None
            if scheme == "explicit":
                rep, explicit = rep % 5, native.bootstrap_weights("poisson", SEED, 0, 5, 0, n)
                w_rows = explicit[rep]
            else:
                w_rows = np.stack([native.bootstrap_weights(scheme, SEED, int(b), 1, 0, n)[0] for b in rep])
            value, grad = gpu.weighted_loglike_grad(table, rep, scheme=scheme, seed=SEED, weights=explicit)
            only = gpu.weighted_loglike(table, rep, scheme=scheme, seed=SEED, weights=explicit)
            assert value.shape == only.shape == (rows,) and grad.shape == (rows, es.n_columns(model, free))
            for j in vh.sample_rows(rows):
                ref = weighted_reference(case, table[j], w_rows[j])
                excess = float((gh.col_err(grad[j], ref["g"], ref["s"]) - 2 * ref["err64"]).max())
                scale = max(abs(ref["value"]), ref["sum_w"], L(1e-300))
                e_v, e_o = float(abs(L(value[j]) - ref["value"]) / scale), float(abs(L(only[j]) - L(value[j])) / scale)
                worst = [max(a, b) for a, b in zip(worst, (e_v, e_o, excess))]
                wh.check_row(value[j], grad[j], ref, (model, free, n, rows, scheme, j), floors)
                assert float(abs(L(only[j]) - ref["value"]) / scale) <= 1e-12 and e_o <= 1e-12, (rows, scheme, j, e_o)
    print("weighted model", model, int(free), "N", n, "value %.2e, value kernel against it %.2e, column err - 2 err_np64 %.2e" % tuple(worst))
    gpu.close()


# ------------------------------------------------------------------------------------------ simulate
@pytest.mark.parametrize("model, free", CELLS, ids=CELL_IDS)
def test_simulate_and_the_simulated_value_and_gradient(native, ctx, model, free):
    """Velocities are v_los + sqrt(sigma_los^2 + s^2 verr^2) z with z replayed by _native.replicate_numbers, to 1e-12 on
    max(|v_obs|, |v_los|, sqrt(n) |z|, 1) (the bound of tests/test_gpu_simulated.py: simulated_helper.check_velocities); simulated_loglike and simulated_loglike_grad of live rows on
    that set against the scaled-catalogue reference with the simulated velocities in place of the observed ones."""
    worst = {"velocity": 0.0, "value": 0.0, "gradient excess": -np.inf}
    import simulated_helper as sh
    for n in (33, 4099):
        # (the field of tests/test_gpu_simulated.py, simulated_helper.make_case: the stars FIELD_STRETCH times further from
        # the centre, where the position angle is well conditioned in the reference's own float64 formula)
        case = dict(case_of(model, free, n))
        cat = dict(case["cat"])
        cat["ra"] = vh.CENTRE[0] + sh.FIELD_STRETCH * (cat["ra"] - vh.CENTRE[0])
        cat["dec"] = vh.CENTRE[1] + sh.FIELD_STRETCH * (cat["dec"] - vh.CENTRE[1])
        case["cat"] = cat
        gpu = es.open_catalog(native, ctx, case)
        n_sims = 7
        truths = np.ascontiguousarray(case["params"][:n_sims])
        es.guard(case, truths, "simulate")
        vel = gpu.simulate(truths, 77)
        assert vel.shape == (n_sims, n) and gpu.simulated_sims == n_sims
        g, _ = native.replicate_numbers(77, 0, n_sims, 0, n)
        for e in range(n_sims):
            v_los, _, norm = es.star_moments(model, case["cat"], truths[e], case["centre"], L)
            want = v_los + np.sqrt(norm) * g[e].astype(L)
            # (the device forms v' = (v - d) + sqrt(n) g: the observed velocity is part of the scale, simulated_helper.exact_velocities)
            scale = np.maximum.reduce([np.abs(case["cat"]["v"]).astype(L), np.abs(v_los), np.sqrt(norm) * np.abs(g[e].astype(L)), np.ones(n, dtype=L)])
            err = float(np.max(np.abs(vel[e].astype(L) - want) / scale))
            worst["velocity"] = max(worst["velocity"], err)
            assert err <= 1e-12, (n, e, err)
            dead = es.star_moments(model, case["cat"], es.unit_rows(model, truths[e])[0], case["centre"], L)
            assert float(np.median(np.abs(np.sqrt(dead[2]) * g[e] - np.sqrt(norm) * g[e]))) >= es.GUARD
        rows = np.ascontiguousarray(case["params"][100:100 + 2 * n_sims])
        sim = np.arange(2 * n_sims, dtype=np.int64)[::-1] % n_sims
        value = gpu.simulated_loglike(rows, sim)
        v2, grad = gpu.simulated_loglike_grad(rows, sim)
        assert v2.tobytes() == value.tobytes()
        floors = es.floors(model, free, n)
        for j in range(2 * n_sims):
            swapped = dict(case, cat=dict(case["cat"], v=vel[sim[j]]), params=rows)
            ref = es.reference(swapped, j)
            e_v = float(vh.scaled_err(value[j], ref["value"], n))
            worst["value"] = max(worst["value"], e_v)
            assert e_v <= 1e-12, (n, j, e_v)
            err = gb.check_columns(grad[j], ref, (model, free, n, "simulated", j), floors)
            worst["gradient excess"] = max(worst["gradient excess"], float((err - 2 * ref["err64"]).max()))
        gpu.close()
    print("simulate model", model, int(free), {k: "%.2e" % v for k, v in worst.items()})


# ------------------------------------------------------------------------------------------ chains
def ensemble(case, w, seed=11, wide=False):
    pos = es.chain_rows(case, w, seed=seed)
    k = es.ES_COLUMN[case["model"]]
    # a posterior-like ball in err_scale too (the table's spread over [0.3, 3] would reject nearly every proposal) ...
    pos[:, k] = 1.7 * np.exp(0.02 * np.random.default_rng(seed + 1).normal(size=w))
    plan = box_plan(case)
    if wide:
        # ... or a start just inside the fast forms' domain, err_scale^2 max(verr^2) within [0.94, 1] x 2^55: every walker is
        # admitted, and the first stretch proposals beyond the largest of them are not
        e2_max = float(np.max(case["cat"]["verr"] ** 2))
        pos[:, k] = np.sqrt(2.0 ** 55 / e2_max * (1.0 - 0.06 * np.random.default_rng(seed + 2).uniform(size=w)))
        plan["hi"][k] = np.inf
    return np.ascontiguousarray(pos), plan


def run_stretch(cat, plan, pos0, lnp0, device, n_steps=40, seed=23, step0=4):
    cat.set_option("device_chain", device)
    pos, lnp = pos0.copy(), lnp0.copy()
    w = pos.shape[0]
    chain, lnpc, acc = np.full((n_steps, w, cat.k), np.nan), np.full((n_steps, w), np.nan), np.zeros(w, dtype=np.int64)
    before = cat.stretch_info()
    cat.stretch_move_seeded(plan, pos, lnp, seed, step0, n_steps, chain, lnpc, acc)
    after = cat.stretch_info()
    cat.set_option("device_chain", 1)
    return (pos, lnp, chain, lnpc, acc), {k: after[k] - before[k] for k in ("device_blocks", "host_blocks", "discarded_blocks")}


@pytest.mark.parametrize("model, free", CELLS, ids=CELL_IDS)
def test_resident_stretch_block_is_the_host_driven_loop(native, ctx, model, free):
    """64 walkers x 40 seeded steps at N = 4099; then a block whose start is so wide in err_scale that the guard's verdict
    changes under way: the device hands it back and the host-driven loop gives the same bits."""
    case = case_of(model, free, 4099)
    cat = open_catalog(native, ctx, case)
    pos0, plan = ensemble(case, 64)
    lnp0 = cat.loglike(pos0)
    assert np.all(np.isfinite(lnp0)) and cat.fast_level == 1
    dev, where_dev = run_stretch(cat, plan, pos0, lnp0, 1)
    host, where_host = run_stretch(cat, plan, pos0, lnp0, 0)
    assert where_dev == {"device_blocks": 1, "host_blocks": 0, "discarded_blocks": 0}, where_dev
    assert where_host["host_blocks"] == 1 and where_host["device_blocks"] == 0
    for a, b in zip(dev, host):
        assert np.array_equal(a, b)
    assert np.all(np.isfinite(dev[3])) and 0 < dev[4].sum() < 40 * 64
    k = es.ES_COLUMN[model]
    assert np.ptp(dev[2][:, :, k]) > 0 and not np.array_equal(dev[0][:, k], pos0[:, k])     # err_scale moved
    # the last stored lnprob row against the reference at the chain's own rows
    for r in vh.sample_rows(64):
        swapped = dict(case, params=dev[2][-1])
        assert float(vh.scaled_err(dev[3][-1, r], es.reference(swapped, r)["value"], 4099)) <= 1e-12
    wide0, wide_plan = ensemble(case, 64, wide=True)
    lnp_w = cat.loglike(wide0)
    assert np.all(np.isfinite(lnp_w)) and cat.fast_level == 1
    dev_w, where_w = run_stretch(cat, wide_plan, wide0, lnp_w, 1, n_steps=10)
    host_w, _ = run_stretch(cat, wide_plan, wide0, lnp_w, 0, n_steps=10)
    print("wide start:", where_w, "level after", cat.fast_level)
    assert where_w["discarded_blocks"] + where_w["host_blocks"] >= 1, where_w          # handed back for a rerun
    for a, b in zip(dev_w, host_w):
        assert np.array_equal(a, b)
    cat.close()


@pytest.mark.parametrize("model, free", CELLS, ids=CELL_IDS)
def test_resident_de_block_is_the_host_driven_loop_and_the_numpy_loop(native, ctx, model, free):
    from mcmc_dynamics_amd.sampler import default_gamma0
    case = case_of(model, free, 4099)
    cat = open_catalog(native, ctx, case)
    w, n_steps = 48, 40
    pos, plan = ensemble(case, w)
    lnp = cat.loglike(pos)
    g0, sigma, seed = default_gamma0(cat.k), 1e-5, 20261021 + model
    runs = {}
    for device in (1, 0):
        cat.set_option("device_chain", device)
        p, l = pos.copy(), lnp.copy()
        chain, lnpc, acc = np.empty((n_steps, w, cat.k)), np.empty((n_steps, w)), np.zeros(w, dtype=np.int64)
        before = cat.de_info()
        cat.de_move_seeded(plan, p, l, g0, sigma, seed, 100, n_steps, chain, lnpc, acc)
        after = cat.de_info()
        key = "device_blocks" if device else "host_blocks"
        assert after[key] == before[key] + 1 and after["discarded_blocks"] == before["discarded_blocks"], (device, before, after)
        runs[device] = (p, l, chain, lnpc, acc)
    cat.set_option("device_chain", 1)
    assert de_helper.same(runs[1], runs[0])
    nums = tuple(np.ascontiguousarray(a) for a in native.de_numbers(seed, 100, n_steps, 1, w, cat.k, g0, sigma, squeeze=True))
    loop = de_helper.numpy_de_block(cat, plan, pos, lnp, nums)
    assert de_helper.same(runs[1], loop[:5])
    assert 0 < runs[1][4].sum() < n_steps * w and np.all(np.isfinite(runs[1][3]))
    assert np.ptp(runs[1][2][:, :, es.ES_COLUMN[model]]) > 0
    cat.close()


def test_resident_hmc_and_temper_blocks_are_the_host_driven_loops(native, ctx):
    import test_gpu_hmc as hmc_cases
    import test_gpu_temper as temper_cases
    for model, free in CELLS:
        case = case_of(model, free, 4099)
        cat = open_catalog(native, ctx, case)
        pos, plan = ensemble(case, 16)
        names = es.column_names(model, free)
        scale = np.array([{"a": abs(pos[0, i]), "r_peak": abs(pos[0, i]), "ra_center": 0.01, "dec_center": 0.01,
                           "err_scale": 1.0}.get(nm, case["scale"]) for i, nm in enumerate(names)])
        chol = np.diag(0.003 * scale)
        dev = hmc_cases.run(cat, plan, chol, 0.5, 2, pos, 31, 2, 5, resident=True)
        host = hmc_cases.run(cat, plan, chol, 0.5, 2, pos, 31, 2, 5, resident=False)
        assert (dev["device_blocks"], dev["host_blocks"]) == (1, 0) and (host["device_blocks"], host["host_blocks"]) == (0, 1)
        for key in hmc_cases.KEYS:
            assert dev[key].tobytes() == host[key].tobytes(), (model, key)
        assert np.all(np.isfinite(dev["chain"])) and dev["accepted"].sum() > 0 and not np.array_equal(dev["pos"], pos)
        assert not np.array_equal(dev["pos"][:, es.ES_COLUMN[model]], pos[:, es.ES_COLUMN[model]])
        pos4, _ = ensemble(case, 4 * 16)
        pos4 = np.ascontiguousarray(pos4.reshape(4, 16, cat.k))
        ll = temper_cases.plain_loglike(cat, plan, pos4.reshape(64, cat.k), 4 * 8).reshape(4, 16)
        betas = np.array([1.0, 0.5, 0.25, 0.0])
        dev = temper_cases.run(cat, plan, betas, pos4, ll, 31, 3, 10, resident=True)
        host = temper_cases.run(cat, plan, betas, pos4, ll, 31, 3, 10, resident=False)
        assert (dev["device_blocks"], dev["host_blocks"]) == (1, 0) and (host["device_blocks"], host["host_blocks"]) == (0, 1)
        for key in temper_cases.KEYS:
            assert dev[key].tobytes() == host[key].tobytes(), (model, key)
        assert np.all(np.isfinite(dev["chain"])) and dev["accepted"].sum() > 0 and not np.array_equal(dev["pos"], pos4)
        cat.close()


# ------------------------------------------------------------------------------------------ Runner level, end to end
E2E_SEED = 20261021


def understated_cluster(seed=E2E_SEED, n=2000):
    """A constant cluster of `n` stars: sigma_max 5 km/s, verr uniform in [1, 8] km/s, velocities drawn with the true
    errors; the catalogue states HALF of them."""
    from mcmc_dynamics_amd import synthetic
    rng = np.random.default_rng(seed)
    sep = np.maximum(np.abs(rng.normal(0, 2.0 / 60.0, n)), 0.002)
    th = rng.uniform(-np.pi, np.pi, n)
    ra = synthetic.CENTER_RA_DEG + sep * np.cos(th) / np.cos(np.radians(synthetic.CENTER_DEC_DEG))
    dec = synthetic.CENTER_DEC_DEG + sep * np.sin(th)
    verr = rng.uniform(1.0, 8.0, n)
    v_los = 3.0 + 2.0 * np.sin(th) - (-1.0) * np.cos(th)
    v = v_los + np.sqrt(verr ** 2 + 5.0 ** 2) * rng.normal(size=n)
    return {"ra": ra, "dec": dec, "v": v, "verr": 0.5 * verr}


def test_constantfites_recovers_the_error_scale_where_constantfit_is_biased(native, ctx):
    from mcmc_dynamics_amd import DataReader, synthetic
    from mcmc_dynamics_amd.analysis import ConstantFit, ConstantFitES
    cols = understated_cluster()
    out = {}
    for cls in (ConstantFitES, ConstantFit):
        fit = cls(DataReader(cols))
        fit.parameters["ra_center"].set(value=synthetic.CENTER_RA_DEG, fixed=True)
        fit.parameters["dec_center"].set(value=synthetic.CENTER_DEC_DEG, fixed=True)
        names = list(fit.fitted_parameters)
        best = fit.maximize()
        assert best["converged"], (cls.__name__, best)
        lap = fit.laplace(best["x"])
        sd = np.sqrt(np.diag(np.asarray(lap["covariance"])))
        out[cls.__name__] = {nm: (float(best["x"][i]), float(sd[i])) for i, nm in enumerate(names)}
        print(cls.__name__, {k: "%.3f +- %.3f" % v for k, v in out[cls.__name__].items()})
        fit.close()
    s, s_sd = out["ConstantFitES"]["err_scale"]
    sig, sig_sd = out["ConstantFitES"]["sigma_max"]
    assert abs(s - 2.0) <= 4.0 * s_sd and 0.0 < s_sd < 0.5, (s, s_sd)
    assert abs(sig - 5.0) <= 4.0 * sig_sd, (sig, sig_sd)
    sig0, sig0_sd = out["ConstantFit"]["sigma_max"]
    assert sig0 - 5.0 > 4.0 * sig0_sd, (sig0, sig0_sd)


def test_runner_methods_reach_the_new_models(native, ctx):
    """ConstantFitES on 300 stars: a short seeded chain with each move, loo / waic / ppc / replicate_check from it, and the
    nested pair -- err_scale fixed at 1 gives ConstantFit's lnprob_batch bits on the device, and lrt against that null runs."""
    from mcmc_dynamics_amd import DataReader, synthetic
    from mcmc_dynamics_amd.analysis import ConstantFit, ConstantFitES
    cols = understated_cluster(n=300)
    centre = (synthetic.CENTER_RA_DEG, synthetic.CENTER_DEC_DEG)

    def make(cls):
        fit = cls(DataReader(cols))
        fit.parameters["ra_center"].set(value=centre[0], fixed=True)
        fit.parameters["dec_center"].set(value=centre[1], fixed=True)
        return fit
    full, null, plain = make(ConstantFitES), make(ConstantFitES), make(ConstantFit)
    null.parameters["err_scale"].set(value=1.0, fixed=True)
    rng = np.random.default_rng(5)
    pos4 = np.array([3.0, 6.0, 2.0, -1.0]) + 0.1 * rng.normal(size=(24, 4))
    assert np.array_equal(null.lnprob_batch(pos4), plain.lnprob_batch(pos4))
    pos5 = np.concatenate([pos4, rng.uniform(0.8, 1.2, size=(24, 1))], axis=1)
    assert np.all(np.isfinite(full.lnprob_batch(pos5))) and not np.array_equal(full.lnprob_batch(pos5), plain.lnprob_batch(pos4))
    sampler = full(n_walkers=24, n_steps=40, n_out=None, prefix=None, pos=pos5.copy())
    chain = np.asarray(sampler.chain)
    assert chain.shape == (24, 40, 5) and np.all(np.isfinite(chain))
    assert full.err_scale(chain, 10).shape == (24 * 30,)
    loo = full.loo(chain, n_burn=10)
    assert np.all(np.isfinite(loo["pointwise"])) and loo["pointwise"].shape == (300,)
    ppc = full.posterior_predictive(chain, 10)
    assert np.all(np.isfinite(ppc["z_mean"])) and np.allclose(ppc["sigma_std"] >= 0, True)
    rep = full.replicate_check(chain, 10, annuli=2, seed=7)
    assert rep is not None
    res = full.lrt(null, n_sims=8, seed=3)
    print("lrt:", {k: v for k, v in res.items() if np.ndim(v) == 0 and not isinstance(v, dict)})
    assert np.isfinite(res["stat_obs"]) and res["stat_obs"] > 0.0 and res["df"] == 1 and res["n_negative"] == 0
    for fit in (full, null, plain):
        fit.close()

"""GPU: the double Lynden-Bell models (device models 7 and 8) with a LIVE second component through every launcher that
reaches them by dispatch_any_model, each against a longdouble (or independent NumPy) restatement with both rotation terms.

tests/test_gpu_double_model.py pins the value and the gradient with a live second component; the summary launchers it
compares on double_helper.nested_rows only, where v_maxx_c = v_maxy_c = 0 and slots 15 .. 18 of the walker row are never
felt.  Here every catalogue is double_helper.make_case, every single row case["params"], every sample table
test_gpu_double_model.chain_rows (a tight ball, second amplitudes of ~0.3 velocity scales left as they are):

  * loglike_per_star / membership (model 8; model 7 is refused and gives its terms through a one-sample
    pointwise_posterior) against double_helper.per_star in longdouble;
  * pointwise_posterior against longdouble reductions of those terms;
  * psis_loo / psis_loo_expect against their NumPy oracles, fed the way tests/test_gpu_psis.py and
    tests/test_gpu_loo_expect.py feed them, the device's lnL rows themselves pinned to the longdouble terms;
  * posterior_predictive and replicate_check under the rules of predictive_helper / replicate_helper;
  * holdout_loglike / holdout_pointwise against longdouble sums over the complement / the held set;
  * moment_match's final weights against the mmatch_helper oracle fed the returned maps and double_helper's terms;
  * weighted_loglike_grad / weighted_loglike against weighted_helper.reference (double_helper's terms), the hold-out train
    value and loglike_grad;
  * DoubleModelFitGB's methods against the Catalog-level calls on the rows mapped by double_helper.abi_columns.

Sensitivity guard (``guard``): for every launcher's cells with N >= 33 the longdouble reference on the live rows and on
nested_rows of the same rows differ by a median over the stars of >= 1e-6, a million times the tolerance -- a launcher that
dropped or mis-addressed the second component cannot pass.

The oracles of psis_loo, psis_loo_expect and moment_match cost a Python loop per star: at N = 4099 they run on
``star_sample`` (the first and the last 70 stars and every 17th), the device on all stars.  moment_match's oracle
re-evaluates every star's terms on transformed draws: longdouble up to 6e5 (star, draw) pairs, float64 NumPy beyond (its
own error, ~1e-16 sqrt(N) per sum, is far inside the check's allowance of 2e-12 max(|lnL|, N))."""
import numpy as np
import pytest

import double_helper as dh
import grad_helper as gh
import holdout_helper as hh
import loo_expect_helper as lh
import mmatch_helper as mh
import predictive_helper as pr
import psis_helper as psh
import replicate_helper as rh
import variant_helper as vh
import weighted_helper as wh
from test_gpu_double_model import chain_rows, ensemble, open_catalog
from test_posterior_cpu import rel, var_ok

pytestmark = pytest.mark.gpu

L = vh.L
CELLS = [(m, f) for m in dh.MODELS for f in (False, True)]
CELL_IDS = ["{0}-{1}".format(m, "free" if f else "fixed") for m, f in CELLS]
SEED = wh.SEED
GUARD = 1e-6


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
        _cases[(model, free, n)] = dh.make_case(model, free, n)
    return _cases[(model, free, n)]


def table_of(case, s, seed=3):
    key = (case["model"], case["free"], case["n"], s, seed)
    if key not in _tables:
        _tables[key] = chain_rows(case, s, seed=seed)
    return _tables[key]


def terms_of(case, row, dtype=L):
    """(lnL_i, p_i) of one row by double_helper.per_star, computed once per (catalogue, row, precision)."""
    key = (case["model"], case["free"], case["n"], np.asarray(row).tobytes(), np.dtype(dtype).name)
    if key not in _terms:
        _terms[key] = dh.per_star(case["model"], case["cat"], row, case["centre"], dtype)
    return _terms[key]


def term_matrix(case, rows, dtype=L):
    """(S, N) lnL and (S, N) membership (None for model 7) of the rows."""
    out = [terms_of(case, row, dtype) for row in rows]
    return np.array([o[0] for o in out]), (None if out[0][1] is None else np.array([o[1] for o in out]))


def guard(case, rows, what, outputs=("lnl",)):
    """The sensitivity guard of the module docstring on rows 0 and S - 1: the longdouble reference of one of `outputs`
    (lnl: the per-star term every lnL-based output is made of; vlos, z: predictive_helper's terms) on the live rows
    against nested_rows of the same rows."""
    if case["n"] < 33:
        return
    model, cat, centre = case["model"], case["cat"], case["centre"]
    nested, _ = dh.nested_rows(rows)
    for r in sorted({0, len(rows) - 1}):
        moved = {}
        if "lnl" in outputs:
            moved["lnl"] = np.abs(terms_of(case, rows[r])[0] - dh.per_star(model, cat, nested[r], centre, L)[0])
        if "vlos" in outputs or "z" in outputs:
            live, dead = pr.star_terms(cat, rows[r], model, centre, L), pr.star_terms(cat, nested[r], model, centre, L)
            moved.update({k: np.abs(live[k] - dead[k]) for k in ("vlos", "z") if k in outputs})
        med = {k: float(np.median(v)) for k, v in moved.items()}
        print("guard", what, (model, case["free"], case["n"]), "row", r, {k: "%.2e" % v for k, v in med.items()})
        assert max(med.values()) >= GUARD, (what, model, case["free"], case["n"], r, med)


def star_sample(n):
    """Every star up to 140; beyond, the first and the last 70 and every 17th (wave and tile boundaries among them)."""
    if n <= 140:
        return np.arange(n)
    return np.unique(np.concatenate([np.arange(70), np.arange(n - 70, n), np.arange(0, n, 17)]))


def device_lnl(gpu, case, rows):
    """(S, N) lnL rows from the per-row entries of the library: loglike_per_star for model 8; for model 7, which it
    refuses, pointwise_posterior's lppd over that ONE sample, which is the term itself."""
    if case["model"] == dh.DOUBLE_GB:
        return np.array([gpu.loglike_per_star(row) for row in rows])
    return np.array([gpu.pointwise_posterior(row[None, :])["lppd"] for row in rows])


def term_err(got, want):
    """|got - want| on max(|want|, 1), the bound of test_per_star_kernels_against_the_80_bit_terms."""
    got = np.asarray(got).astype(L)
    return float(np.max(np.abs(got - want) / np.maximum(np.abs(want), L(1)))) if got.size else 0.0


# ------------------------------------------------------------------------------------------ per-star terms
@pytest.mark.parametrize("model, free", CELLS, ids=CELL_IDS)
def test_per_star_terms_against_the_80_bit_terms(native, ctx, model, free):
    for n in (1, 33, 4099):
        case = case_of(model, free, n)
        gpu = open_catalog(native, ctx, case)
        rows = case["params"][vh.sample_rows(257)]
        guard(case, rows, "per-star")
        for row in rows:
            want_l, want_p = terms_of(case, row)
            if model == dh.DOUBLE_GB:
                got_l, got_p = gpu.loglike_per_star(row), gpu.membership(row)
                assert got_l.shape == got_p.shape == (n,)
                e_p = float(np.max(np.abs(got_p.astype(L) - want_p)))
                assert e_p < 1e-11, (n, e_p)
                assert got_l.tobytes() == gpu.loglike_per_star(row).tobytes()
            else:
                for call in (gpu.loglike_per_star, gpu.membership):
                    with pytest.raises(native.NativeError, match="background model"):
                        call(row)
                got_l, e_p = gpu.pointwise_posterior(row[None, :])["lppd"], 0.0
            e_l = term_err(got_l, want_l)
            print("per-star model", model, int(free), "N", n, "terms %.2e membership %.2e" % (e_l, e_p))
            assert e_l < 1e-12, (n, e_l)
        gpu.close()


# ------------------------------------------------------------------------------------------ pointwise posterior
@pytest.mark.parametrize("model, free", CELLS, ids=CELL_IDS)
def test_pointwise_posterior_against_longdouble_reductions(native, ctx, model, free):
    """S in {1, 65, 257} x N in {1, 65, 4099} under the bounds tests/test_gpu_posterior.py holds models 0 .. 6 to against
    an oracle: lppd to 1e-11 (fixed centre) / 1e-12 (free) relative, variances by var_ok with rtol 1e-10, the membership
    mean to 1e-12 and its spread to 1e-10."""
    mem = model == dh.DOUBLE_GB
    worst = {}
    for n in (1, 65, 4099):
        case = case_of(model, free, n)
        gpu = open_catalog(native, ctx, case)
        table = table_of(case, 257)
        guard(case, table, "pointwise_posterior")
        x80, p80 = term_matrix(case, table)
        for s in (1, 65, 257):
            got = gpu.pointwise_posterior(table[:s], membership=mem)
            assert sorted(got) == sorted(("lppd", "lnl_var") + (("pmem_mean", "pmem_std") if mem else ()))
            x = x80[:s]
            mx = x.max(axis=0)
            lppd = (mx + np.log(np.exp(x - mx).sum(axis=0)) - np.log(L(s))).astype(np.float64)
            var = (x.var(axis=0, ddof=1) if s > 1 else np.zeros(n)).astype(np.float64)
            e = {"lppd": rel(got["lppd"], lppd)}
            assert e["lppd"] < (1e-12 if free else 1e-11), (n, s, e)
            assert var_ok(got["lnl_var"], var, lppd, rtol=1e-10), (n, s)
            if mem:
                p = p80[:s]
                e["pmem_mean"] = float(np.max(np.abs(got["pmem_mean"] - p.mean(axis=0).astype(np.float64))))
                std = (p.std(axis=0, ddof=1) if s > 1 else np.zeros(n)).astype(np.float64)
                e["pmem_std"] = float(np.max(np.abs(got["pmem_std"] - std)))
                assert e["pmem_mean"] < 1e-12 and e["pmem_std"] < 1e-10, (n, s, e)
            for k, v in e.items():
                worst[k] = max(worst.get(k, 0.0), v)
        gpu.close()
    print("pointwise_posterior model", model, int(free), {k: "%.2e" % v for k, v in worst.items()})


# ------------------------------------------------------------------------------------------ PSIS-LOO and its expectations
_lnl = {}


def lnl_rows(native, ctx, case, gpu):
    """The device's (N, 1000) lnL rows of the cell's table, computed once, and pinned to the longdouble terms on a sample
    of the rows (1e-12 on max(|l_i|, 1))."""
    key = (case["model"], case["free"], case["n"])
    if key not in _lnl:
        table = table_of(case, 1000)
        x = device_lnl(gpu, case, table)
        worst = max(term_err(x[r], terms_of(case, table[r])[0]) for r in vh.sample_rows(1000))
        print("lnL rows", key, "against the longdouble terms: %.2e" % worst)
        assert worst < 1e-12, (key, worst)
        _lnl[key] = np.ascontiguousarray(x.T)
    return _lnl[key]


@pytest.mark.parametrize("n", [33, 4099])
@pytest.mark.parametrize("model, free", CELLS, ids=CELL_IDS)
def test_psis_loo_matches_the_oracle(native, ctx, model, free, n):
    case = case_of(model, free, n)
    gpu = open_catalog(native, ctx, case)
    table = table_of(case, 1000)
    guard(case, table, "psis_loo")
    lnl = lnl_rows(native, ctx, case, gpu)
    some = star_sample(n)
    for s in (130, 1000):
        got = gpu.psis_loo(table[:s])
        assert all(v.shape == (n,) for v in got.values())
        sub = np.ascontiguousarray(lnl[some, :s])
        psh.assert_matches({k: v[some] for k, v in got.items()}, psh.numpy_psis(sub),
                           k_tol=np.maximum(1e-10, 10.0 * psh.k_noise(sub)))
        pp = gpu.pointwise_posterior(table[:s])
        assert np.all(np.abs(got["lppd"] - pp["lppd"]) <= 1e-13 * np.maximum(np.abs(pp["lppd"]), 1.0))
    gpu.close()


@pytest.mark.parametrize("n", [33, 4099])
@pytest.mark.parametrize("model, free", CELLS, ids=CELL_IDS)
def test_psis_loo_expect_follows_the_rule(native, ctx, model, free, n):
    """loo_expect_helper's rule as tests/test_gpu_loo_expect.py applies it: against the oracle fed the device's lnL rows
    and (a) predictive_helper's NumPy terms -- both rotation components -- for the stars clear of the centres, (b) the
    device's own per-sample terms."""
    from test_gpu_loo_expect import _clear_of_centres, _device_terms
    case = case_of(model, free, n)
    cat, centre = case["cat"], case["centre"]
    gpu = open_catalog(native, ctx, case)
    table = table_of(case, 1000)
    guard(case, table, "psis_loo_expect", outputs=("lnl", "vlos", "z"))
    lnl = lnl_rows(native, ctx, case, gpu)
    mix = model in pr.MIX_MODELS
    some = star_sample(n)
    small = {k: np.asarray(v)[some] for k, v in cat.items()}
    x_all, keys = lh.term_rows(small, table, model, centre, mix=mix)
    own_all = _device_terms(gpu, table, keys)[some]
    unit = tuple(i for i, k in enumerate(keys) if k in ("pit", "pit_mix"))
    clear = _clear_of_centres(small, table, model, centre)
    print("stars clear of the centres:", int(clear.sum()), "of", clear.size)
    for s in (130, 1000):
        got = gpu.psis_loo_expect(table[:s], mixture=mix)
        assert ("pit_mix" in got) == mix
        rows = np.stack([got[k] for k in keys], axis=1)[some]
        k_hat, sub = got["pareto_k"][some], np.ascontiguousarray(lnl[some, :s])
        what = "model {0} free {1} ({2}, {3})".format(model, int(free), n, s)
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
    tests/test_gpu_predictive.py; vlos_mean holds both components."""
    mix = model in pr.MIX_MODELS
    for n in (1, 65, 4099):
        case = case_of(model, free, n)
        gpu = open_catalog(native, ctx, case)
        table = table_of(case, 257)
        guard(case, table, "posterior_predictive", outputs=("vlos", "z"))
        ref = pr.Reference(case["cat"], table, model, case["centre"])
        for s in (1, 65, 257):
            got = gpu.posterior_predictive(table[:s], mixture=mix)
            assert ("pit_mix" in got) == mix and all(v.shape == (n,) for v in got.values())
            exact, np64, vmax = ref.at(n, s)
            pr.check_rule(got, exact, np64, vmax, var_ok, rtol=1e-10, cell=(model, free, n, s))
            if s == 1:
                assert all(np.all(got[f] == 0.0) for f in ("z_std", "vlos_std", "sigma_std"))
        gpu.close()


# ------------------------------------------------------------------------------------------ replicate check
@pytest.mark.parametrize("model, free", CELLS, ids=CELL_IDS)
def test_replicate_check_follows_the_rule(native, ctx, model, free):
    """N in {65, 4099}, 65 sample rows, two ranges over a permuted order that leaves a tenth of the stars out."""
    for n in (65, 4099):
        case = case_of(model, free, n)
        gpu = open_catalog(native, ctx, case)
        table = table_of(case, 65)
        guard(case, table, "replicate_check", outputs=("z",))
        order = np.random.default_rng(n).permutation(n).astype(np.int64)[:n - n // 10]
        offs = np.array([0, order.size // 3, order.size], dtype=np.int64)
        got = gpu.replicate_check(table, rh.SEED, offs, order)
        assert got.shape == (65, 2, 8, 2)
        ref = rh.Reference(case["cat"], table, model, case["centre"])
        rh.check_rule(got, *ref.at(offs, order), cell=(model, free, n))
        assert got.tobytes() == gpu.replicate_check(table, rh.SEED, offs, order).tobytes()
        gpu.close()


# ------------------------------------------------------------------------------------------ hold-out
@pytest.mark.parametrize("n", [33, 4099])
@pytest.mark.parametrize("model, free", CELLS, ids=CELL_IDS)
def test_holdout_against_longdouble_sums(native, ctx, model, free, n):
    """(E, W) in {(1, 2), (3, 66)} with the prefix sets of sizes (1, 0, 7): train and held values against longdouble sums of
    double_helper.per_star over the complement / the held set, 1e-12 on max(|lnL|, N); holdout_pointwise against
    pointwise_posterior on the same rows, as tests/test_gpu_holdout.py compares them."""
    case = case_of(model, free, n)
    gpu = open_catalog(native, ctx, case)
    worst = 0.0
    for E, W in ((1, 2), (3, 66)):
        offs = hh.sets_of_sizes((1, 0, 7), n)[:E + 1]
        table = table_of(case, E * W, seed=5)
        guard(case, table, "holdout")
        train, test = gpu.holdout_loglike(offs, table.reshape(E, W, -1))
        assert train.shape == test.shape == (E, W)
        for e in range(E):
            b0, b1 = int(offs[e]), int(offs[e + 1])
            for w in vh.sample_rows(W):
                l = terms_of(case, table[e * W + w])[0]
                held = l[b0:b1].sum()
                for got, want in ((train[e, w], l.sum() - held), (test[e, w], held)):
                    err = float(vh.scaled_err(got, want, n))
                    worst = max(worst, err)
                    assert err <= 1e-12, (E, W, e, w, got, float(want), err)
            if b1 == b0:
                assert np.all(test[e] == 0.0) and not np.any(np.signbit(test[e]))
        again = gpu.holdout_loglike(offs, table.reshape(E, W, -1))
        assert again[0].tobytes() == train.tobytes() and again[1].tobytes() == test.tobytes()
        tables = table.reshape(E, W, -1)
        got = gpu.holdout_pointwise(offs, tables)
        assert got["lppd"].shape == (int(offs[-1]),)
        for e in range(E):
            b0, b1 = int(offs[e]), int(offs[e + 1])
            ref = gpu.pointwise_posterior(tables[e])
            for key in ("lppd", "lnl_var"):
                a, b = got[key][b0:b1], ref[key][b0:b1]
                assert np.all(np.isfinite(a)) and np.all(np.abs(a - b) <= 1e-12 * np.abs(b)), (key, e)
    print("holdout model", model, int(free), "N", n, "largest error on max(|lnL|, N): %.2e" % worst)
    gpu.close()


# ------------------------------------------------------------------------------------------ moment matching
def mmatch_check(case, plan, draws, stars, got, dtype):
    """tests/test_gpu_mmatch.py: check_against_oracle with the oracle's evaluate() made of double_helper's terms in
    `dtype`: train = the sum over the other stars, test = the star's own term.  The bound is that function's."""
    n = case["n"]
    seen = {}

    def matrix(rows):
        key = rows.tobytes()
        if key not in seen:
            seen[key] = np.array([dh.per_star(case["model"], case["cat"], row, case["centre"], dtype)[0] for row in rows])
        return seen[key]

    inside = lambda rows: np.all((rows >= plan["lo"]) & (rows <= plan["hi"]), axis=1)
    lnprior = lambda rows: np.zeros(len(rows))
    delta = 2e-12 * max(abs(float(matrix(draws[:1]).sum())), n)
    worst = {"pareto_k": 0.0, "n_eff": 0.0, "elpd": 0.0}
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
            worst[key] = max(worst[key], abs(g - w))
            assert abs(g - w) <= tol, (key, e, g, w, tol)
        seen = {draws.tobytes(): seen[draws.tobytes()]} if draws.tobytes() in seen else {}
    return worst


@pytest.mark.parametrize("n_match, s", [(1, 130), (3, 1000)])
@pytest.mark.parametrize("n", [33, 4099])
@pytest.mark.parametrize("model, free", [(dh.DOUBLE, False), (dh.DOUBLE, True), (dh.DOUBLE_GB, False)],
                         ids=["7-fixed", "7-free", "8-fixed"])
def test_moment_match_final_weights_against_the_oracle(native, ctx, model, free, n, n_match, s):
    """N in {33, 4099} x (n_match, S) in {(1, 130), (3, 1000)} for every cell within the 12 free parameters
    mcd_moment_match takes: model 7 with a fixed (P = 9) and a free centre (11), model 8 with a fixed one (12).  Model 8
    with a free centre has 14 columns and is refused as a whole table ("1 <= n_dim <= 12"); it would run with two columns
    held constant by the plan, which is left out here: the launcher's double-model code does not depend on which columns
    are free, and both its background and its free-centre instantiations are among the three cells."""
    from test_gpu_mmatch import check_bookkeeping, stars_of
    case = case_of(model, free, n)
    gpu = open_catalog(native, ctx, case)
    gpu.set_option("fast_path", 0)
    draws, plan = ensemble(case, s)
    guard(case, draws, "moment_match")
    stars = stars_of(n, n_match)
    got = gpu.moment_match(plan, draws, stars, -np.inf, max_iters=3)
    check_bookkeeping(got, draws.shape[1], 3)
    print("accepted trials per level:", got["accepted"].sum(axis=0))
    worst = mmatch_check(case, plan, draws, stars, got, L if n * s <= 600000 else np.float64)
    print("moment_match model", model, int(free), (n, n_match, s), "largest differences:", worst)
    again = gpu.moment_match(plan, draws, stars, -np.inf, max_iters=3)
    for key in ("elpd", "pareto_k", "n_eff", "A", "b"):
        assert np.asarray(again[key]).tobytes() == np.asarray(got[key]).tobytes(), key
    gpu.close()


# ------------------------------------------------------------------------------------------ weighted gradient and value
@pytest.mark.parametrize("n", [33, 4099])
@pytest.mark.parametrize("model, free", CELLS, ids=CELL_IDS)
def test_weighted_calls_against_the_longdouble_weighted_sums(native, ctx, model, free, n):
    """Three schemes x rows in {2, 66, 258} with weighted_helper.row_replicates (the explicit scheme is handed the
    generator's Poisson weights of replicates 0 .. 4, as tests/test_gpu_weighted.py hands them): weighted_helper.check_row
    against weighted_helper.reference with double_helper.floors, and the value kernel against the gradient call's value,
    1e-12 on max(|sum w l|, sum w)."""
    case = case_of(model, free, n)
    gpu = open_catalog(native, ctx, case)
    floors = dh.floors(model, free, n)
    worst = [0.0, 0.0, -np.inf]                          # value, value kernel against it, column err - 2 err_np64
    for rows in (2, 66, 258):
        table = np.ascontiguousarray(case["params"][:rows])
        guard(case, table, "weighted")
        for scheme in ("exponential", "poisson", "explicit"):
            rep, explicit = wh.row_replicates(rows), None
            if scheme == "explicit":
                rep, explicit = rep % 5, native.bootstrap_weights("poisson", SEED, 0, 5, 0, n)
                w_rows = explicit[rep]
            else:
                w_rows = np.stack([native.bootstrap_weights(scheme, SEED, int(b), 1, 0, n)[0] for b in rep])
            value, grad = gpu.weighted_loglike_grad(table, rep, scheme=scheme, seed=SEED, weights=explicit)
            only = gpu.weighted_loglike(table, rep, scheme=scheme, seed=SEED, weights=explicit)
            assert value.shape == only.shape == (rows,) and grad.shape == (rows, dh.n_columns(model, free))
            for j in vh.sample_rows(rows):
                ref = wh.reference(model, case["cat"], table[j], case["centre"], w_rows[j])
                excess = float((gh.col_err(grad[j], ref["g"], ref["s"]) - 2 * ref["err64"]).max())
                scale = max(abs(ref["value"]), ref["sum_w"], L(1e-300))
                e_v, e_o = float(abs(L(value[j]) - ref["value"]) / scale), float(abs(L(only[j]) - L(value[j])) / scale)
                if excess > worst[2]:
                    k = int(np.argmax(gh.col_err(grad[j], ref["g"], ref["s"]) - 2 * ref["err64"]))
                    where = (rows, scheme, j, dh.column_names(model, free)[k], float(floors[k]))
                worst = [max(a, b) for a, b in zip(worst, (e_v, e_o, excess))]
                print((model, int(free), n, rows, scheme, j), "value %.2e value kernel %.2e column err - 2 err_np64 %.2e" % (e_v, e_o, excess))
                wh.check_row(value[j], grad[j], ref, (model, free, n, rows, scheme, j), floors)
                assert float(abs(L(only[j]) - ref["value"]) / scale) <= 1e-12 and e_o <= 1e-12, (rows, scheme, j, e_o)
    print("weighted model", model, int(free), "N", n, "value %.2e, value kernel against it %.2e, column err - 2 err_np64 %.2e" % tuple(worst),
          "at (rows, scheme, row, column, floor)", where)
    gpu.close()


@pytest.mark.parametrize("n", [33, 4099])
@pytest.mark.parametrize("model, free", CELLS, ids=CELL_IDS)
def test_zero_one_weights_are_the_holdout_train_value_and_unit_weights_the_gradient(native, ctx, model, free, n):
    case = case_of(model, free, n)
    gpu = open_catalog(native, ctx, case)
    offs = hh.sets_of_sizes((1, 0, 7), n)
    E, W = 3, 22
    table = np.ascontiguousarray(case["params"][:E * W])
    train, _ = gpu.holdout_loglike(offs, table.reshape(E, W, -1))
    weights = np.ones((E, n))
    for e in range(E):
        weights[e, int(offs[e]):int(offs[e + 1])] = 0.0
    rep = np.repeat(np.arange(E), W)
    value, _ = gpu.weighted_loglike_grad(table, rep, scheme="explicit", weights=weights)
    only = gpu.weighted_loglike(table, rep, scheme="explicit", weights=weights)
    for got in (value, only):
        assert np.all(vh.scaled_err(got, train.reshape(-1), n) <= 1e-12)
    v_ref, g_ref = gpu.loglike_grad(table)
    value, grad = gpu.weighted_loglike_grad(table, np.zeros(E * W, dtype=np.int64), scheme="explicit", weights=np.ones((1, n)))
    assert np.all(vh.scaled_err(value, v_ref, n) <= 1e-12)
    for j in vh.sample_rows(E * W):
        ref = wh.reference(model, case["cat"], table[j], case["centre"], np.ones(n))
        assert np.all(gh.col_err(grad[j], g_ref[j], ref["s"]) <= 1e-12), (j,)
        assert float(vh.scaled_err(v_ref[j], ref["value"], n)) <= 1e-12
    gpu.close()


# ------------------------------------------------------------------------------------------ Runner level
def test_runner_methods_are_the_catalogue_calls_on_the_mapped_rows(native, ctx):
    """DoubleModelFitGB on 33 stars with a fixed centre: every method once, against the Catalog-level call on the same rows
    in the C-ABI order (double_helper.abi_columns) -- the column plan of v_maxx_c, v_maxy_c and r_peak_ratio."""
    from mcmc_dynamics_amd import DataReader
    from mcmc_dynamics_amd.analysis import DoubleModelFitGB
    from mcmc_dynamics_amd.analysis.runner import replicate_summary
    from mcmc_dynamics_amd.optimize import maximize_batch
    model, n, W, steps = dh.DOUBLE_GB, 33, 8, 16
    case = case_of(model, False, n)
    c = case["cat"]
    fit = DoubleModelFitGB(DataReader({k: c[k] for k in ("ra", "dec", "v", "verr", "density")}))
    fit.parameters["ra_center"].set(value=vh.CENTRE[0], fixed=True)
    fit.parameters["dec_center"].set(value=vh.CENTRE[1], fixed=True)
    for name in ("v_sys", "v_maxx", "v_maxy", "v_maxx_c", "v_maxy_c", "v_back"):      # (make_case's velocity scale may exceed the boxes)
        fit.parameters[name].set(min=-np.inf, max=np.inf)
    for name in ("sigma_max", "sigma_back", "a", "r_peak"):
        fit.parameters[name].set(max=np.inf)
    names = dh.column_names(model, False)
    fitted = list(fit.fitted_parameters)
    assert sorted(fitted) == sorted(names)
    rows = table_of(case, W * steps)
    guard(case, rows, "runner")
    values = np.ascontiguousarray(rows[:, [names.index(k) for k in fitted]])
    table = dh.abi_columns(fitted, values, model, False)
    assert np.array_equal(table, rows)
    chain = values.reshape(W, steps, -1)
    gpu = native.Catalog(ctx, c["ra"], c["dec"], c["v"], c["verr"], model=model, centre=case["centre"], density=c["density"])
    assert np.all(np.isfinite(fit.lnprob_batch(values)))

    got, want = fit.posterior_predictive(chain, 0), gpu.posterior_predictive(table, mixture=True)
    assert got.pop("n_samples") == W * steps and sorted(got) == sorted(want)
    for key in want:
        assert np.array_equal(got[key], want[key]), key

    offs, order, _ = fit._replicate_groups(2, None)
    got = fit.replicate_check(chain, 0, annuli=2, seed=7)
    want = replicate_summary(gpu.replicate_check(table, 7, offs, order), np.diff(offs))
    for key, ref in want.items():
        same = list(got[key]) == list(ref) if key == "names" else np.array_equal(np.asarray(got[key]), np.asarray(ref), equal_nan=True)
        assert same, key

    got, want = fit.loo(chain, 0), gpu.psis_loo(table)
    for key, ref in (("pointwise", "elpd_loo"), ("pareto_k", "pareto_k"), ("n_eff", "n_eff")):
        assert np.array_equal(got[key], want[ref]), key

    got, want = fit.loo_pit(chain, 0), gpu.psis_loo_expect(table, predictive=True, mixture=True)
    for key, ref in (("loo_pit", "pit_mix"), ("pit", "pit"), ("z", "z"), ("vlos", "vlos"), ("sigma", "sigma"), ("pareto_k", "pareto_k")):
        assert np.array_equal(got[key], want[ref]), key
    assert np.array_equal(got["weight"], gpu.pointwise_posterior(table, membership=True)["pmem_mean"])

    rep = wh.row_replicates(W * steps) % 7
    lp = fit.parameters.lnprior_batch(fit.parameters.resolve_batch(values))
    got = fit.lnprob_weighted_batch(values, rep, scheme="poisson", seed=SEED)
    assert np.array_equal(got, gpu.weighted_loglike(table, rep, scheme="poisson", seed=SEED) + lp)

    cols = [names.index(k) for k in fitted]
    lo = np.array([fit.parameters[k].min for k in fitted], dtype=np.float64)
    hi = np.array([fit.parameters[k].max for k in fitted], dtype=np.float64)

    def value_and_grad(x):
        v, g = gpu.weighted_loglike_grad(dh.abi_columns(fitted, x, model, False), np.zeros(1, dtype=np.int64), scheme="exponential", seed=5)
        return v, g[:, cols]
    got = fit.bootstrap(n_replicates=1, scheme="exponential", seed=5, x_hat=values[0], max_iter=2)
    want = maximize_batch(value_and_grad, values[:1].copy(), lo, hi, max_iter=2, gtol=1e-8)
    assert got["x"].shape == (1, len(fitted)) and not np.array_equal(got["x"][0], values[0])
    assert np.array_equal(got["x"], want["x"]) and np.array_equal(got["n_iter"], want["n_iter"])
    gpu.close()
    fit.close()

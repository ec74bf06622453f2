"""GPU: mcd_holdout_loglike and mcd_holdout_pointwise (csrc/mcd_holdout.hip, csrc/mcd_api_holdout.hip) against the value
path, the per-star outputs and mcd_pointwise_posterior; determinism; refusals; and Runner.reloo / Runner.kfold end to end
against a closed form (tests/holdout_helper.py).

Catalogues and models: the three setups of tests/test_gpu_hmc.py.  Shapes: N in {33, 4099} x (E, W) in {(1, 2), (3, 66),
(5, 258)} -- one row tile, a ragged second tile, and 1 290 rows (more than four tiles: the XCD-grouped branch of wave_task)
-- with sets of sizes {1}, {1, 0, 7}, {1, 1, 40, 0, 300}, each capped to N: at N = 33 the last case covers all stars (no
remainder range) and ends on two empty sets; at N = 4099 its last boundary (342) lies inside what the un-binned plan makes
one chunk."""
import ctypes

import numpy as np
import pytest

import holdout_helper as hh
from test_gpu_hmc import MODELS, setup as model_setup

pytestmark = pytest.mark.gpu

SHAPES = {(1, 2): (1,), (3, 66): (1, 0, 7), (5, 258): (1, 1, 40, 0, 300)}
_I64P = ctypes.POINTER(ctypes.c_int64)
_F64P = ctypes.POINTER(ctypes.c_double)


@pytest.fixture(scope="module")
def native():
    from mcmc_dynamics_amd import _native
    return _native


@pytest.fixture(scope="module")
def ctx(native):
    return native.default_context()


_CASES = {}


def case(native, ctx, kind, n):
    """One catalogue per (model, N) for the whole module: (catalogue, constructor arguments, table maker)."""
    if (kind, n) not in _CASES:
        kw, plan, x, scale, _ = model_setup(kind, n)
        cols = [kw.pop(k) for k in ("ra", "dec", "v", "verr")]
        cat = native.Catalog(ctx, *cols, **kw)

        def table(rows, seed):
            pos = x + 0.5 * scale * np.random.default_rng(seed).normal(size=(rows, x.size))
            pos = np.clip(pos, plan["lo"], plan["hi"])
            return np.ascontiguousarray(np.stack(
                [pos[:, s] * plan["col_factor"][j] if s >= 0 else np.full(rows, plan["col_const"][j])
                 for j, s in enumerate(plan["col_source"])], axis=1))
        _CASES[(kind, n)] = (cat, cols, kw, table)
    return _CASES[(kind, n)]


def plain_loglike(cat, table):
    cat.set_option("fast_path", 0)
    try:
        return cat.loglike(table)
    finally:
        cat.set_option("fast_path", 1)


def per_star(cat, kind, row):
    """The plain per-star terms of one row.  mcd_loglike_per_star refuses the models without a background ("const"); for
    them the term is mcd_pointwise_posterior's lppd over that ONE sample, which is the term itself (shift = l, sumexp = 1,
    so lppd = l + (log 1 - log 1))."""
    if kind == "const":
        return cat.pointwise_posterior(row[None, :])["lppd"]
    return cat.loglike_per_star(row)


def within(got, want, scale_n):
    """The project's bound for kernel families: 1e-12 on the scale max(|lnL|, N)."""
    return np.abs(got - want) <= 1e-12 * np.maximum(np.abs(want), float(scale_n))


@pytest.mark.parametrize("shape", sorted(SHAPES))
@pytest.mark.parametrize("n", [33, 4099])
@pytest.mark.parametrize("kind", MODELS)
def test_train_and_test_against_the_value_path_and_the_per_star_terms(native, ctx, kind, n, shape):
    cat, _, _, make = case(native, ctx, kind, n)
    (E, W), offs = shape, hh.sets_of_sizes(SHAPES[shape], n)
    table = make(E * W, seed=E * 1000 + W)
    train, test = cat.holdout_loglike(offs, table.reshape(E, W, -1))
    assert train.shape == test.shape == (E, W)
    full = plain_loglike(cat, table).reshape(E, W)
    err = np.abs(train + test - full) / np.maximum(np.abs(full), n)
    print(kind, n, shape, "largest |train + test - lnL| / max(|lnL|, N):", err.max())
    assert np.all(within(train + test, full, n))                                           # 1
    worst = 0.0
    for e in range(E):
        b0, b1 = int(offs[e]), int(offs[e + 1])
        if b1 == b0:                                                                       # 3: an empty set
            assert np.all(test[e] == 0.0) and not np.any(np.signbit(test[e]))
            assert np.all(within(train[e], full[e], n))
            continue
        for w in range(W):                                                                 # 2
            want = per_star(cat, kind, table[e * W + w])[b0:b1].sum()
            worst = max(worst, abs(test[e, w] - want) / max(abs(want), b1 - b0))
            assert within(test[e, w], want, b1 - b0), (e, w, test[e, w], want)
    print("largest |test - sum of per-star terms| / max(|sum|, n_set):", worst)
    if int(offs[-1]) == n:                                                                 # no remainder range
        assert E == 1 or np.all(np.isfinite(train))
    # 4: bitwise repeatable, also across an interleaved call with another (set_offsets, W)
    other = make(2 * 4, seed=3)
    cat.holdout_loglike(hh.sets_of_sizes((2, 3), n), other.reshape(2, 4, -1))
    again = cat.holdout_loglike(offs, table.reshape(E, W, -1))
    assert again[0].tobytes() == train.tobytes() and again[1].tobytes() == test.tobytes()
    # 5: test = NULL
    only, none = cat.holdout_loglike(offs, table.reshape(E, W, -1), want_test=False)
    assert none is None and only.tobytes() == train.tobytes()


def test_one_set_that_covers_everything_trains_on_nothing(native, ctx):
    cat, _, _, make = case(native, ctx, "bgfixed", 33)
    table = make(6, seed=1)
    train, test = cat.holdout_loglike([0, 33], table.reshape(1, 6, -1))
    assert np.all(train == 0.0) and not np.any(np.signbit(train))
    assert np.all(within(test[0], plain_loglike(cat, table), 33))


@pytest.mark.parametrize("n,S", [(33, 1), (33, 3), (33, 70000), (4099, 1), (4099, 3)])      # 70 000: two upload passes
@pytest.mark.parametrize("kind", MODELS)
def test_pointwise_against_pointwise_posterior(native, ctx, kind, n, S):
    cat, _, _, make = case(native, ctx, kind, n)
    # E = 1, the set covers all stars: mcd_pointwise_posterior's bits
    table = make(S, seed=S)
    want = cat.pointwise_posterior(table)
    got = cat.holdout_pointwise([0, n], table[None])
    assert got["lppd"].tobytes() == want["lppd"].tobytes() and got["lnl_var"].tobytes() == want["lnl_var"].tobytes()
    # in general: set e's stars under table e
    offs = hh.sets_of_sizes((1, 0, 7) if S == 70000 else (1, 1, 40, 0, 300), n)
    E = offs.size - 1
    tables = np.stack([make(S, seed=10 * S + e) for e in range(E)])
    got = cat.holdout_pointwise(offs, tables)
    assert got["lppd"].shape == (int(offs[-1]),)
    for e in range(E):
        b0, b1 = int(offs[e]), int(offs[e + 1])
        if b1 == b0:
            continue
        ref = cat.pointwise_posterior(tables[e])
        for key in ("lppd", "lnl_var"):
            a, b = got[key][b0:b1], ref[key][b0:b1]
            assert np.all(np.isfinite(a))
            assert np.all(np.abs(a - b) <= 1e-12 * np.abs(b)), (key, e, np.max(np.abs(a - b) / np.abs(b)))
    if S == 1:
        assert np.all(got["lnl_var"] == 0.0)
    again = cat.holdout_pointwise(offs, tables)
    assert again["lppd"].tobytes() == got["lppd"].tobytes() and again["lnl_var"].tobytes() == got["lnl_var"].tobytes()


def _raw(cat, which, offs, table, k=None):
    """The C entry point itself, on sentinel-filled outputs: (status, out0, out1)."""
    offs = np.ascontiguousarray(offs, dtype=np.int64)
    E, rows, K = table.shape
    n_out = E * rows if which == "loglike" else max(1, int(np.max(offs)))
    a, b = np.full(n_out, -7.25), np.full(n_out, -7.25)
    fn = cat.lib.mcd_holdout_loglike if which == "loglike" else cat.lib.mcd_holdout_pointwise
    rc = fn(cat.handle, offs.size - 1, offs.ctypes.data_as(_I64P), rows, K if k is None else k, table.ctypes.data_as(_F64P),
            a.ctypes.data_as(_F64P), b.ctypes.data_as(_F64P))
    return rc, a, b


def test_refusals_leave_the_outputs_untouched(native, ctx):
    cat, cols, kw, make = case(native, ctx, "const", 33)
    table = make(8, seed=2).reshape(2, 4, -1)

    def refused(c, offs, t, k=None, what=None):
        for which in ("loglike", "pointwise"):
            rc, a, b = _raw(c, which, offs, t, k)
            assert rc == -1, (which, rc)
            assert np.all(a == -7.25) and np.all(b == -7.25)
            if what:
                assert what in c.lib.mcd_last_error().decode()
    refused(cat, [0, 5, 4], table, what="non-decreasing")
    refused(cat, [1, 2, 3], table, what="must be 0")
    refused(cat, [0, 2, 34], table, what="exceeds")
    refused(cat, [0, 1, 2], table, k=5, what="columns")
    for more, what in (({"bin_offsets": np.array([0, 10, 33], dtype=np.int64)}, "un-binned"), ({"precision": "f32"}, "MCD_F64")):
        other = native.Catalog(ctx, *cols, **dict(kw, **more))
        refused(other, [0, 1, 2], table, what=what)
        other.close()
    # E W over the cap (the pointwise call has no such cap: its rows are samples)
    big = np.ascontiguousarray(np.broadcast_to(table[0, 0], (2, 32769, table.shape[2])))
    rc, a, b = _raw(cat, "loglike", [0, 1, 2], big)
    assert rc == -1 and "65536" in cat.lib.mcd_last_error().decode() and np.all(a == -7.25) and np.all(b == -7.25)
    # n_sets < 1
    offs = np.zeros(1, dtype=np.int64)
    out = np.full(4, -7.25)
    rc = cat.lib.mcd_holdout_loglike(cat.handle, 0, offs.ctypes.data_as(_I64P), 4, table.shape[2], table.ctypes.data_as(_F64P),
                                     out.ctypes.data_as(_F64P), None)
    assert rc == -1 and np.all(out == -7.25)
    # the catalogue still works after the refusals
    train, test = cat.holdout_loglike([0, 1, 2], table)
    assert np.all(np.isfinite(train)) and np.all(np.isfinite(test))


# ------------------------------------------------------------------------------------------ end to end
def test_reloo_and_kfold_against_the_closed_form():
    """ConstantFit on 200 synthetic stars, only v_sys free: the likelihood is exactly Gaussian in v_sys, so every held-out
    star's predictive density is log N(v_i; mu_-set, verr_i^2 + sigma^2 + 1 / Lambda_-set) (tests/holdout_helper.py, long
    double).  reloo of the five planted stars and kfold(4) must agree with it within 5 standard errors, the standard error
    being the spread of the per-walker estimates.  Run length: holdout_fit's defaults, 64 walkers x 600 steps, 200 of them
    burn-in, sized by tests/test_holdout_cpu.py::test_closed_form_harness_sizes_the_run: standard error 0.0136 against a
    difference of 0.1765 between the exact leave-one-out value and the full-posterior lppd of the most extreme star."""
    cols = hh.closed_form_columns()
    fit = hh.closed_form_fit(cols)
    try:
        np.random.seed(5)
        sampler = fit(n_walkers=32, n_steps=300, n_out=None, prefix=None)
        chain = np.asarray(sampler.chain)
        loo = fit.loo(chain, 100)
        stars = sorted(hh.PLANTED, key=lambda i: -abs(hh.PLANTED[i]))
        run = dict(n_walkers=hh.N_WALKERS, n_steps=hh.N_STEPS, n_burn=hh.N_BURN)
        refit = dict(n_walkers=hh.N_WALKERS, n_steps=hh.N_STEPS, refit_burn=hh.N_BURN)
        re = fit.reloo(loo, chain, 100, stars=stars, seed=11, **refit)
        exact, full = hh.exact_elpd(cols, [[i] for i in stars]), hh.exact_full_lppd(cols)
        refit_chain = re["fit"]["sampler"].chain[:, :, hh.N_BURN:, 0]
        assert refit_chain.shape == (5, hh.N_WALKERS, hh.N_STEPS - hh.N_BURN)
        for e, i in enumerate(stars):
            _, se = hh.walker_estimates(refit_chain[e], cols, i)
            z = float((re["pointwise"][i] - exact[i]) / se)
            print("reloo star %3d: exact %.5f device %.5f psis %.5f full lppd %.5f se %.5f z %.2f" %
                  (i, float(exact[i]), re["pointwise"][i], loo["pointwise"][i], float(full[i]), se, z))
            assert abs(z) < 5.0
            if e == 0:
                assert se <= 0.5 * float(abs(exact[i] - full[i]))
        assert np.array_equal(re["refit"], stars)
        untouched = np.setdiff1d(np.arange(hh.N_STARS), stars)
        assert np.array_equal(re["pointwise"][untouched], loo["pointwise"][untouched])
        assert re["elpd_loo"] == pytest.approx(re["pointwise"].sum(), rel=1e-13)
        # the same seed gives the same chain, bit for bit (9)
        twice = fit.reloo(loo, chain, 100, stars=stars, seed=11, **refit)
        assert twice["fit"]["sampler"].chain.tobytes() == re["fit"]["sampler"].chain.tobytes()
        assert twice["pointwise"].tobytes() == re["pointwise"].tobytes()

        kf = fit.kfold(n_folds=4, seed=3, **run)
        assert kf["n_folds"] == 4 and kf["n_stars"] == hh.N_STARS and np.all(np.isfinite(kf["pointwise"]))
        sets = [np.flatnonzero(kf["folds"] == f) for f in range(4)]
        assert sorted(s.size for s in sets) == [50, 50, 50, 50]
        exact = hh.exact_elpd(cols, sets)
        fold_chain = kf["fit"]["sampler"].chain[:, :, hh.N_BURN:, 0]
        zs = np.empty(hh.N_STARS)
        for f, s in enumerate(sets):
            for i in s:
                _, se = hh.walker_estimates(fold_chain[f], cols, i)
                zs[i] = float((kf["pointwise"][i] - exact[i]) / se)
        print("kfold: largest |z| %.2f at star %d; elpd_kfold %.4f (exact %.4f)" %
              (np.abs(zs).max(), int(np.argmax(np.abs(zs))), kf["elpd_kfold"], float(exact.sum())))
        assert np.all(np.abs(zs) < 5.0)
        from mcmc_dynamics_amd.analysis.runner import elpd_compare
        assert elpd_compare(kf, re)["n_stars"] == hh.N_STARS
    finally:
        fit.close()

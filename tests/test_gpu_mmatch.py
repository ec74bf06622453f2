"""GPU: mcd_moment_match (csrc/mcd_mmatch.hip, csrc/mcd_api_mmatch.hip) -- the baseline against mcd_psis_loo, the final
weights against the NumPy oracle of tests/mmatch_helper.py fed the returned maps, the bookkeeping, repeatability, the
refusals, and Runner.loo_moment_match end to end on the closed-form case.

Building blocks: the three model setups of tests/test_gpu_hmc.py x N in {33, 4099} x (n_match, S) in {(1, 130), (3, 1000),
(20, 4096)} (the last makes two groups of 16 and 4 stars); draws from a Gaussian ball round the setup's parameters.  The
loop is made to work on every star by k_threshold = -inf (a narrow ball gives negative k^) and bounded by max_iters = 3."""
import numpy as np
import pytest

import mmatch_helper as mh
import psis_helper as psh
from test_gpu_hmc import setup

pytestmark = pytest.mark.gpu

MODELS = ("const", "bgfixed", "profile_gb_free")
SHAPES = ((1, 130), (3, 1000), (20, 4096))
K_THR = -np.inf
ARRAYS = ("ra", "dec", "v", "verr", "lnlike_bg", "pmember", "density")


@pytest.fixture(scope="module")
def native():
    from mcmc_dynamics_amd import _native
    return _native


@pytest.fixture(scope="module")
def ctx(native):
    return native.default_context()


_CASES = {}


def case(native, ctx, kind, n):
    """(catalogue, its keyword arguments, plan, parameters, scales) per (model, N) for the whole module."""
    if (kind, n) not in _CASES:
        kw, plan, x, scale, _dense = setup(kind, n)
        args = dict(kw)
        cat = native.Catalog(ctx, args.pop("ra"), args.pop("dec"), args.pop("v"), args.pop("verr"), **args)
        cat.set_option("fast_path", 0)
        _CASES[(kind, n)] = (cat, kw, plan, x, scale)
    return _CASES[(kind, n)]


def one_star(native, ctx, kw, i):
    """The catalogue of star i alone: its log-likelihood is the star's plain term."""
    args = {k: (np.ascontiguousarray(v[i:i + 1]) if k in ARRAYS else v) for k, v in kw.items()}
    cat = native.Catalog(ctx, args.pop("ra"), args.pop("dec"), args.pop("v"), args.pop("verr"), **args)
    cat.set_option("fast_path", 0)
    return cat


def ball(x, scale, plan, S, seed=3, keep=None):
    rng = np.random.default_rng(seed)
    pos = x + 0.5 * scale * rng.normal(size=(2 * S, x.size))
    ok = np.all((pos >= plan["lo"]) & (pos <= plan["hi"]), axis=1)
    if keep is not None:
        ok &= keep(pos)
    assert ok.sum() >= S
    return np.ascontiguousarray(pos[ok][:S])


def table_of(plan, rows):
    src, fac = plan["col_source"], plan["col_factor"]
    return np.ascontiguousarray(np.where(src < 0, plan["col_const"], rows[:, np.maximum(src, 0)] * fac))


def stars_of(n, n_match):
    """Spread over the catalogue, with the first star, two neighbours and the last one among them."""
    picks = {0, n - 1, n // 2, n // 2 + 1} if n_match >= 4 else ({n // 3} if n_match == 1 else {0, n // 2, n - 1})
    rng = np.random.default_rng(n + n_match)
    while len(picks) < n_match:
        picks.add(int(rng.integers(0, n)))
    return np.array(sorted(picks)[:n_match], dtype=np.int64)


def evaluator(native, ctx, cat, kw, plan, star):
    """evaluate() of the oracle by the library's own plain terms: test = the one-star catalogue's value, train = all - test."""
    single = one_star(native, ctx, kw, int(star))

    def fn(rows):
        t = table_of(plan, rows)
        te = single.loglike(t)
        return cat.loglike(t) - te, te
    return fn, single


def prior_fns(native, plan):
    def inside(rows):
        ok = np.all((rows >= plan["lo"]) & (rows <= plan["hi"]), axis=1)
        if plan.get("prior") is not None:
            ok &= native.prior_eval(plan["prior"], rows) > -np.inf
        return ok

    def lnprior(rows):
        return native.prior_eval(plan["prior"], rows) if plan.get("prior") is not None else np.zeros(len(rows))
    return inside, lnprior


def check_against_oracle(native, ctx, cat, kw, plan, draws, stars, got, n_stars, split=True):
    """The oracle, fed the draws and the returned maps, against pareto_k, n_eff and elpd of the final weights.  The
    inputs differ by at most delta = 2e-12 max(|lnL|, N) (section 3.16's bound on train, applied twice): the oracle's raw
    log weights are moved by +-delta, and ten times the largest movement of each output, floored at 1e-10, is the bound."""
    inside, lnprior = prior_fns(native, plan)
    worst = {"pareto_k": 0.0, "n_eff": 0.0, "elpd": 0.0}
    lnl = abs(float(cat.loglike(table_of(plan, draws[:1]))[0]))
    delta = 2e-12 * max(lnl, n_stars)
    for e, star in enumerate(stars):
        ev, single = evaluator(native, ctx, cat, kw, plan, star)
        want = mh.moment_match(draws, ev, inside, lnprior, 0.0, split=split, fixed_map=(got["A"][e], got["b"][e]))
        single.close()
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
    print("largest differences:", worst)


def check_bookkeeping(got, P, max_iters):
    acc = got["accepted"].sum(axis=1)
    it = got["iterations"]
    assert np.all((acc == it) | (acc == it - 1)) and np.all(it <= max_iters) and np.all(got["accepted"] >= 0)
    assert np.all(got["k_loop"] <= got["k_before"])
    none = acc == 0
    assert np.array_equal(got["k_loop"] == got["k_before"], none)
    eye = np.all(got["A"] == np.eye(P), axis=(1, 2)) & np.all(got["b"] == 0.0, axis=1)
    assert np.array_equal(eye, none)
    assert np.array_equal(got["pareto_k"][none], got["k_before"][none])


# ---------------------------------------------------------------------------------------------------- building blocks
@pytest.mark.parametrize("n_match,S", SHAPES)
@pytest.mark.parametrize("n", [33, 4099])
@pytest.mark.parametrize("kind", MODELS)
def test_baseline_is_plain_psis(native, ctx, kind, n, n_match, S):
    cat, kw, plan, x, scale = case(native, ctx, kind, n)
    draws = ball(x, scale, plan, S)
    stars = stars_of(n, n_match)
    got = cat.moment_match(plan, draws, stars, 0.0, max_iters=0)
    ref = cat.psis_loo(table_of(plan, draws))
    lnl = []
    for star in stars:
        single = one_star(native, ctx, kw, int(star))
        lnl.append(single.loglike(table_of(plan, draws)))
        single.close()
    lnl = np.array(lnl)
    k_tol = np.maximum(1e-10, 10.0 * psh.k_noise(lnl))
    e, we = got["elpd"], ref["elpd_loo"][stars]
    assert np.all(np.abs(e - we) <= 1e-11 * np.maximum(1.0, np.abs(we))), float(np.max(np.abs(e - we)))
    k, wk = got["pareto_k"], ref["pareto_k"][stars]
    fin = np.isfinite(wk)
    assert np.array_equal(np.isfinite(k), fin) and np.array_equal(k[~fin], wk[~fin])
    assert np.all(np.abs(k[fin] - wk[fin]) <= k_tol[fin]), float(np.max(np.abs(k[fin] - wk[fin]) - k_tol[fin]))
    assert np.all(np.abs(got["n_eff"] - ref["n_eff"][stars]) <= 1e-9 * np.abs(ref["n_eff"][stars]))
    assert np.array_equal(got["k_before"], k) and np.array_equal(got["k_loop"], k)
    assert not got["iterations"].any() and not got["accepted"].any()
    assert np.all(got["A"] == np.eye(x.size)) and not got["b"].any()


@pytest.mark.parametrize("n_match,S", SHAPES)
@pytest.mark.parametrize("n", [33, 4099])
@pytest.mark.parametrize("kind", MODELS)
def test_full_run_against_the_oracle(native, ctx, kind, n, n_match, S):
    cat, kw, plan, x, scale = case(native, ctx, kind, n)
    draws = ball(x, scale, plan, S)
    stars = stars_of(n, n_match)
    got = cat.moment_match(plan, draws, stars, K_THR, max_iters=3)
    check_bookkeeping(got, x.size, 3)
    print("accepted trials per level:", got["accepted"].sum(axis=0), "stars moved:", np.count_nonzero(got["accepted"].sum(axis=1)))
    if n_match == 20:
        assert got["accepted"].sum() > 0                                 # the loop had work to do (a few stars may have none)
    if S <= 10 * x.size:
        assert not got["accepted"][:, 2].any()                           # no covariance trial with S <= 10 P
    # the oracle on a few of the stars (every star of the small shapes)
    some = np.arange(n_match) if n_match <= 3 else np.array([0, 7, 15, 16, 19])
    sub = {k: v[some] for k, v in got.items()}
    check_against_oracle(native, ctx, cat, kw, plan, draws, stars[some], sub, n)


def test_normal_prior(native, ctx):
    cat, kw, plan, x, scale = case(native, ctx, "const", 4099)
    kind = np.array([1, 0, 1, 0], dtype=np.int32)
    plan = dict(plan, prior=(kind, x + 0.3 * scale, 2.0 * scale))
    draws = ball(x, scale, plan, 1000, seed=4)
    stars = stars_of(4099, 3)
    got = cat.moment_match(plan, draws, stars, K_THR, max_iters=3)
    check_bookkeeping(got, 4, 3)
    assert got["accepted"].sum() > 0
    check_against_oracle(native, ctx, cat, kw, plan, draws, stars, got, 4099)
    flat = cat.moment_match(dict(plan, prior=None), draws, stars, K_THR, max_iters=3)
    assert not np.array_equal(flat["elpd"], got["elpd"])


def test_box_that_cuts_transformed_rows(native, ctx):
    """The closed-form case of tests/mmatch_helper.py (star 0 is 8 sigma off, so its maps move the rows a long way) with a
    box of +-2.25 posterior standard deviations on v_sys; the draws are the exact posterior's rows inside it.  The NumPy
    oracle alone left 6.3 % of star 0's transformed rows outside a box of 2.0 and 3.7 % outside one of 2.5: about 5 % here.
    Such rows get weight 0 and a donor takes their place in the launch."""
    from mcmc_dynamics_amd import synthetic
    cols = mh.closed_form_columns(0)
    X = mh.design(cols)
    mu, cov = mh.posterior(cols, X)
    mu, sd = mu.astype(np.float64), np.sqrt(np.diag(cov.astype(np.float64)))
    lo0, hi0 = mu[0] - 2.25 * sd[0], mu[0] + 2.25 * sd[0]
    kw = dict(cols, model=0, centre=(synthetic.CENTER_RA_DEG, synthetic.CENTER_DEC_DEG))
    plan = {"col_source": np.array([0, -1, 1, 2], dtype=np.int32), "col_const": np.array([0.0, mh.SIGMA, 0.0, 0.0]),
            "col_factor": np.ones(4), "lo": np.array([lo0, -1000.0, -1000.0]), "hi": np.array([hi0, 1000.0, 1000.0]),
            "fixed_ok": True}
    full = mh.exact_draws(cols, X, 7, n=6000)
    draws = np.ascontiguousarray(full[(full[:, 0] >= lo0) & (full[:, 0] <= hi0)][:4096])
    args = dict(kw)
    cat = native.Catalog(ctx, args.pop("ra"), args.pop("dec"), args.pop("v"), args.pop("verr"), **args)
    cat.set_option("fast_path", 0)
    stars = np.array([0, 5], dtype=np.int64)
    got = cat.moment_match(plan, draws, stars, K_THR, max_iters=3)
    check_bookkeeping(got, 3, 3)
    rows = draws @ got["A"][0].T + got["b"][0]
    cut = np.mean((rows[:, 0] < lo0) | (rows[:, 0] > hi0))
    print("fraction of star 0's transformed rows outside the box: %.4f" % cut)
    assert 0.02 <= cut <= 0.10
    check_against_oracle(native, ctx, cat, kw, plan, draws, stars, got, mh.N_STARS)
    cat.close()


def test_split_off_returns_the_loop_estimate(native, ctx):
    cat, kw, plan, x, scale = case(native, ctx, "const", 33)
    draws = ball(x, scale, plan, 1000)
    stars = stars_of(33, 3)
    a = cat.moment_match(plan, draws, stars, K_THR, max_iters=3)
    b = cat.moment_match(plan, draws, stars, K_THR, max_iters=3, split=False)
    for key in ("k_before", "k_loop", "iterations", "accepted", "A", "b"):
        assert np.array_equal(a[key], b[key]), key
    moved = a["accepted"].sum(axis=1) > 0
    assert moved.any() and np.array_equal(b["pareto_k"], b["k_loop"])
    assert np.all(a["elpd"][moved] != b["elpd"][moved])
    check_against_oracle(native, ctx, cat, kw, plan, draws, stars, b, 33, split=False)


def test_bits_repeat(native, ctx):
    cat, kw, plan, x, scale = case(native, ctx, "profile_gb_free", 4099)
    draws = ball(x, scale, plan, 4096)
    stars = stars_of(4099, 20)
    a = cat.moment_match(plan, draws, stars, K_THR, max_iters=2)
    cat.holdout_loglike(np.array([0, 3, 9]), np.ascontiguousarray(np.broadcast_to(table_of(plan, draws[:5]), (2, 5, 11))))
    b = cat.moment_match(plan, draws, stars, K_THR, max_iters=2)
    for key in a:
        assert np.array_equal(a[key], b[key], equal_nan=True), key
    # another group has another range plan, i.e. another order of the sum `train`: the same values to rounding
    c = cat.moment_match(plan, draws, stars[[3, 17]], K_THR, max_iters=0)
    b0 = cat.moment_match(plan, draws, stars, K_THR, max_iters=0)
    assert np.all(np.abs(b0["elpd"][[3, 17]] - c["elpd"]) <= 1e-11 * np.abs(c["elpd"]))
    cat.set_option("timing", 1)
    cat.moment_match(plan, draws[:130], stars[:2], K_THR, max_iters=1)
    assert cat.last_kernel_ms > 0.0
    cat.set_option("timing", 0)


def _sentinels(n, P):
    out = {k: np.full(n, -7.5) for k in ("elpd", "pareto_k", "n_eff", "k_before", "k_loop")}
    out.update({"iterations": np.full(n, -7, np.int32), "accepted": np.full((n, 3), -7, np.int32), "A": np.full((n, P, P), -7.5),
                "b": np.full((n, P), -7.5)})
    return out


def test_refusals_leave_the_outputs_untouched(native, ctx):
    cat, kw, plan, x, scale = case(native, ctx, "const", 33)
    draws = ball(x, scale, plan, 130)

    def refused(cat_, plan_, draws_, stars_, **opts):
        out = _sentinels(len(stars_), draws_.shape[1])
        with pytest.raises(native.NativeError):
            cat_.moment_match(plan_, draws_, np.array(stars_, dtype=np.int64), 0.7, out=out, **opts)
        want = _sentinels(len(stars_), draws_.shape[1])
        assert all(np.array_equal(out[k], want[k]) for k in out)

    refused(cat, plan, draws, [5, 3])                                     # unsorted
    refused(cat, plan, draws, [3, 3])                                     # repeated
    refused(cat, plan, draws, [3, 33])                                    # outside the catalogue
    refused(cat, plan, draws, [-1, 3])
    refused(cat, plan, draws, [3], r_eff=0.0)
    refused(cat, plan, draws, [3], r_eff=-1.0)
    refused(cat, plan, draws, [3], max_iters=-1)
    refused(cat, plan, draws[:20], [3])                                   # a PSIS tail of 4 values
    refused(cat, plan, np.ascontiguousarray(np.broadcast_to(draws[:1], (65537, 4))), [3])
    refused(cat, dict(plan, prior=(np.array([1, 0, 0, 0], np.int32), np.zeros(4), np.array([-1.0, 1, 1, 1]))), draws, [3])
    refused(cat, dict(plan, prior=(np.array([7, 0, 0, 0], np.int32), np.zeros(4), np.ones(4))), draws, [3])
    args = dict(kw)
    f32 = native.Catalog(ctx, args.pop("ra"), args.pop("dec"), args.pop("v"), args.pop("verr"), precision="f32", **args)
    refused(f32, plan, draws, [3])
    f32.close()
    args = dict(kw)
    binned = native.Catalog(ctx, args.pop("ra"), args.pop("dec"), args.pop("v"), args.pop("verr"),
                            bin_offsets=np.array([0, 10, 33], dtype=np.int64), **args)
    refused(binned, plan, draws, [3])
    binned.close()
    # a draw outside the prior is an error too, and writes nothing
    outside = draws.copy()
    outside[7, 1] = -1.0
    refused(cat, plan, outside, [3])
    # ... and the catalogue still works
    ok = cat.moment_match(plan, draws, np.array([3]), 0.7, max_iters=0)
    assert np.isfinite(ok["elpd"][0])


# ------------------------------------------------------------------------------------- end to end with a closed form
def test_closed_form_end_to_end(ctx):
    """ConstantFit, sigma_max fixed, v_sys / v_maxx / v_maxy free: 20 stars, star 0 moved 8 sigma off, S = 4096 exact
    posterior draws passed as a chain, seeds 0 .. 5 (tests/mmatch_helper.py; sized on the oracle by
    tests/test_mmatch_cpu.py::test_closed_form_harness_on_the_oracle: 0.423 against 0.0233, k^ <= 0.46).  Against loo() on
    the same draws the mean |error| of star 0's moment-matched pointwise value is at most a quarter of plain PSIS's, and
    every seed's k^ after matching is at or below the threshold.  With split = 0 the loop's estimate is returned and differs
    from the split one (the bias of choosing the map with the draws that carry the estimate: recorded, not asserted)."""
    cols = mh.closed_form_columns(0)
    X = mh.design(cols)
    exact = mh.exact_loo(cols, X, 0)
    fit = mh.closed_form_fit(cols, context=ctx)
    plain, matched, loop = [], [], []
    for seed in range(6):
        chain = mh.exact_draws(cols, X, seed)[None]
        loo = fit.loo(chain, 0)
        out = fit.loo_moment_match(loo, chain, 0)
        assert 0 in out["matched"] and loo["pareto_k"][0] > loo["k_threshold"]
        e = int(np.flatnonzero(out["matched"] == 0)[0])
        assert out["pareto_k"][0] <= loo["k_threshold"], (seed, out["pareto_k"][0])
        assert out["accepted"][e].sum() >= 1 and out["k_loop"][e] < out["k_before"][e]
        assert abs(out["k_before"][e] - loo["pareto_k"][0]) <= 1e-8
        assert out["n_bad_k"] <= loo["n_bad_k"] - 1
        rest = np.setdiff1d(np.arange(mh.N_STARS), out["matched"])
        assert np.array_equal(out["pointwise"][rest], loo["pointwise"][rest])
        assert out["elpd_loo"] == pytest.approx(np.sum(out["pointwise"]), abs=1e-9)
        off = fit.loo_moment_match(loo, chain, 0, split=False)
        assert off["pareto_k"][0] == off["k_loop"][e] == out["k_loop"][e] and off["pointwise"][0] != out["pointwise"][0]
        plain.append(abs(loo["pointwise"][0] - exact))
        matched.append(abs(out["pointwise"][0] - exact))
        loop.append(abs(off["pointwise"][0] - exact))
        print("seed %d: plain %.4f matched %.4f loop only %.4f, k^ %.3f -> %.3f" % (seed, plain[-1], matched[-1], loop[-1],
                                                                                   loo["pareto_k"][0], out["pareto_k"][0]))
    print("mean |error|: plain %.4f, matched %.4f, loop only %.4f" % (np.mean(plain), np.mean(matched), np.mean(loop)))
    assert np.mean(matched) <= 0.25 * np.mean(plain)
    # reloo on the result has nothing left to refit for star 0
    assert 0 not in np.flatnonzero(out["pareto_k"] > out["k_threshold"])
    fit.close()

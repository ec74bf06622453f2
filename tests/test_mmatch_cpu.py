"""CPU: moment matching for PSIS-LOO -- the algebra of csrc/mcd_mmatch.h (compiled by tests/emul/mmatch_emul.cpp) against
the NumPy restatement of tests/mmatch_helper.py, the decision loop's bookkeeping, the star ranges, the refusals, the
bookkeeping of Runner.loo_moment_match on a stubbed native call, and the closed-form harness on the oracle alone."""
import numpy as np
import pytest

import mmatch_helper as mh
import psis_helper as psh


def _rows_and_weights(P, S=400, seed=0, heavy=True):
    rng = np.random.default_rng(seed)
    mix = rng.normal(size=(P, P)) / np.sqrt(P) + np.eye(P)
    rows = rng.normal(size=(S, P)) @ mix.T + rng.normal(size=P) * 3.0
    lw = rows @ rng.normal(size=P) * (0.8 if heavy else 0.1)
    w = np.exp(lw - lw.max())
    return rows, w


def _close(a, b, tol):
    a, b = np.asarray(a), np.asarray(b)
    return np.all(np.abs(a - b) <= tol * np.maximum(1.0, np.abs(b)))


# ------------------------------------------------------------------------------------------------- moments, transforms
@pytest.mark.parametrize("P", [1, 3, 12])
def test_moments_and_transforms_match_numpy(P):
    rows, w = _rows_and_weights(P, seed=P)
    got = mh.emul_moments(rows, w)
    want = mh.moments(rows, w / w.sum())
    for key in ("mu", "mu_w", "v_w", "C", "C_w"):
        assert _close(got[key], want[key], 1e-12), key
    for level in (mh.SHIFT, mh.SCALE, mh.COV):
        ok, At, bt = mh.emul_trial(level, got["raw"], P)
        t = mh.trial(level, want)
        assert ok and t is not None
        assert _close(At, t[0], 1e-12) and _close(bt, t[1], 1e-12), level
    # the Cholesky map itself
    ok, l = mh.emul_cholesky(want["C"])
    assert ok and _close(l, np.linalg.cholesky(want["C"]), 1e-12)


@pytest.mark.parametrize("P", [1, 4, 12])
def test_covariance_trial_reproduces_the_weighted_moments(P):
    rows, w = _rows_and_weights(P, S=500, seed=10 + P)
    m = mh.emul_moments(rows, w)
    ok, At, bt = mh.emul_trial(mh.COV, m["raw"], P)
    assert ok
    moved = mh.emul_apply(At, bt, rows)
    assert _close(moved, rows @ At.T + bt, 1e-12)
    assert _close(moved.mean(axis=0), m["mu_w"], 1e-10)
    assert _close(np.atleast_2d(np.cov(moved.T)), m["C_w"], 1e-10)
    # T2 matches the mean and the variances, T1 the mean
    ok, As, bs = mh.emul_trial(mh.SCALE, m["raw"], P)
    moved = mh.emul_apply(As, bs, rows)
    assert _close(moved.mean(axis=0), m["mu_w"], 1e-10) and _close(moved.var(axis=0, ddof=1), m["v_w"], 1e-10)
    ok, A1, b1 = mh.emul_trial(mh.SHIFT, m["raw"], P)
    assert np.array_equal(A1, np.eye(P)) and _close(mh.emul_apply(A1, b1, rows).mean(axis=0), m["mu_w"], 1e-10)


def test_zero_variance_column_keeps_scale_one():
    rows, w = _rows_and_weights(3, seed=5)
    rows[:, 1] = 2.5
    m = mh.emul_moments(rows, w)
    ok, At, bt = mh.emul_trial(mh.SCALE, m["raw"], 3)
    assert ok and At[1, 1] == 1.0 and abs(bt[1]) < 1e-13 and At[0, 0] != 1.0       # (bt: the weighted mean's rounding)
    t = mh.trial(mh.SCALE, mh.moments(rows, w / w.sum()))
    assert _close(At, t[0], 1e-12) and _close(bt, t[1], 1e-12)
    # the sample covariance is singular: T3 is skipped
    assert not mh.emul_trial(mh.COV, m["raw"], 3)[0]
    assert mh.trial(mh.COV, mh.moments(rows, w / w.sum())) is None


def test_cholesky_refuses_what_is_not_positive_definite():
    assert not mh.emul_cholesky(np.array([[1.0, 2.0], [2.0, 1.0]]))[0]
    assert not mh.emul_cholesky(np.array([[1.0, 0.0], [0.0, np.nan]]))[0]
    assert not mh.emul_cholesky(np.zeros((3, 3)))[0]
    assert mh.emul_cholesky(np.array([[4.0, 2.0], [2.0, 3.0]]))[0]


@pytest.mark.parametrize("P", [1, 5, 12])
def test_affine_bookkeeping(P):
    rng = np.random.default_rng(P)
    A, b = rng.normal(size=(P, P)) + 2 * np.eye(P), rng.normal(size=P)
    At, bt = rng.normal(size=(P, P)) + 2 * np.eye(P), rng.normal(size=P)
    A2, b2 = mh.emul_compose(At, bt, A, b)
    assert _close(A2, At @ A, 1e-12) and _close(b2, At @ b + bt, 1e-12)
    x = rng.normal(size=(7, P))
    assert _close(mh.emul_apply(A2, b2, x), mh.emul_apply(At, bt, mh.emul_apply(A, b, x)), 1e-12)
    ok, Ai, bi, lad = mh.emul_inverse(A2, b2)
    assert ok and _close(mh.emul_apply(Ai, bi, mh.emul_apply(A2, b2, x)), x, 1e-10)
    assert abs(lad - np.linalg.slogdet(A2)[1]) <= 1e-12 * max(1.0, abs(lad))
    assert not mh.emul_inverse(np.zeros((P, P)), b)[0]


# --------------------------------------------------------------------------------------------------- box, donors, -inf
def test_rows_outside_the_prior_get_minus_infinity():
    x = np.array([[0.0, 1.0], [1.0, 1.0], [1.0 + 1e-12, 1.0], [0.5, np.nan], [0.5, -2.0], [0.5, 0.0]])
    lo, hi = np.array([0.0, -2.0]), np.array([1.0, np.inf])
    inside = mh.emul_rows_inside(x, lo, hi)
    assert inside.tolist() == [True, True, False, False, True, True]                 # the box is inclusive
    assert mh.emul_rows_inside(x, lo, hi, kind=[0, 2]).tolist() == [True, True, False, False, False, False]  # lognormal: x > 0
    assert not mh.emul_rows_inside(x, lo, hi, fixed_ok=0).any()
    lw = mh.emul_lw_trial(inside, np.arange(6.0), np.full(6, 0.5), np.full(6, 2.0))
    assert np.array_equal(lw[inside], (np.arange(6.0) + 0.5 - 2.0)[inside]) and np.all(lw[~inside] == -np.inf)
    # the split step: -inf numerators stay, an inverse row outside the prior drops out of the mixture
    num, lpf = np.array([-np.inf, 1.0, 1.0]), np.array([0.0, 2.0, 2.0])
    got = mh.emul_lw_split(num, lpf, [1, 1, 0], np.array([0.0, 3.0, 3.0]), 0.25)
    assert got[0] == -np.inf and abs(got[1] - (1.0 - np.logaddexp(2.0, 2.75))) < 1e-15 and got[2] == -1.0
    # the oracle gives such rows weight 0 and evaluates a donor in their place
    seen = []

    def evaluate(rows):
        seen.append(rows.copy())
        return -0.5 * np.sum(rows ** 2, axis=1), -0.5 * (rows[:, 0] - 3.0) ** 2

    draws = np.random.default_rng(1).normal(size=(400, 2))
    box = lambda t: np.all((t >= -3.5) & (t <= 1.2), axis=1)                        # noqa: E731
    draws = draws[box(draws)][:300]
    out = mh.moment_match(draws, evaluate, box, lambda t: np.zeros(len(t)), 0.0, max_iters=3, split=False)
    assert all(box(rows).all() for rows in seen)                                     # nothing outside was ever evaluated
    moved = draws @ out["A"].T + out["b"]
    assert out["accepted"].sum() > 0 and (~box(moved)).any() and np.all(out["weights"][~box(moved)] == 0.0)


# ------------------------------------------------------------------------------------------------- the decision loop
def test_loop_bookkeeping():
    thr = 0.7
    # T1 fails, T2 accepted (back to T1), T1 accepted and below the threshold: done
    r = mh.emul_loop(1.2, thr, 30, 3, [1.3, 0.9, 0.5, 0.1], [1, 1, 1, 1])
    assert r["levels"].tolist() == [1, 2, 1] and r["accepts"].tolist() == [0, 1, 1]
    assert r["k"] == 0.5 and r["iterations"] == 2 and r["accepted"].tolist() == [1, 1, 0] and not r["running"]
    # a pass without an accepted trial ends the loop: iterations = accepted + 1
    r = mh.emul_loop(1.2, thr, 30, 3, [1.0, 1.1, 1.0, 1.0, 0.2], [1, 1, 1, 1, 1])
    assert r["levels"].tolist() == [1, 1, 2, 3] and r["k"] == 1.0 and r["iterations"] == 2
    assert r["accepted"].tolist() == [1, 0, 0] and not r["running"]
    # an unusable trial (T3 skipped, no row inside the prior) is never accepted, an equal k^ neither
    r = mh.emul_loop(1.2, thr, 30, 3, [0.1, 1.2, 0.1], [0, 1, 0])
    assert r["accepts"].tolist() == [0, 0, 0] and r["k"] == 1.2 and r["accepted"].sum() == 0 and r["iterations"] == 1
    # max_iters bounds the passes; 0 and a k^ at the threshold never start; without cov the third level is not tried
    r = mh.emul_loop(5.0, thr, 2, 3, [4.0, 3.0, 2.0], [1, 1, 1])
    assert r["iterations"] == 2 and r["accepted"].tolist() == [2, 0, 0] and r["k"] == 3.0 and not r["running"]
    assert mh.emul_loop(5.0, thr, 0, 3, [1.0], [1])["iterations"] == 0
    assert mh.emul_loop(thr, thr, 30, 3, [0.1], [1])["levels"].size == 0
    assert mh.emul_loop(np.inf, thr, 30, 2, [np.inf, np.inf], [1, 1])["levels"].tolist() == [1, 2]
    assert mh.lib().emul_mm_max_level(1, 121, 12) == 3 and mh.lib().emul_mm_max_level(1, 120, 12) == 2
    assert mh.lib().emul_mm_max_level(0, 4096, 3) == 2


# ------------------------------------------------------------------------------------------------- ranges and refusals
def test_star_ranges():
    r, sr = mh.emul_ranges(100, [0, 1, 7, 99])
    assert r.tolist() == [0, 1, 2, 7, 8, 99, 100] and sr.tolist() == [0, 1, 3, 5]
    r, sr = mh.emul_ranges(10, [4])
    assert r.tolist() == [0, 4, 5, 10] and sr.tolist() == [1]
    r, sr = mh.emul_ranges(3, [0, 1, 2])
    assert r.tolist() == [0, 1, 2, 3] and sr.tolist() == [0, 1, 2]
    assert np.all(np.diff(mh.emul_ranges(4099, [5, 6, 4000])[0]) > 0)


def test_refusals_of_the_star_list():
    assert mh.emul_stars_error([3, 5, 9], 10) is None
    assert "ascending" in mh.emul_stars_error([3, 3], 10)
    assert "ascending" in mh.emul_stars_error([5, 3], 10)
    assert "outside" in mh.emul_stars_error([3, 10], 10)
    assert "outside" in mh.emul_stars_error([-1], 10)
    assert "n_match" in mh.emul_stars_error([], 10)


# ------------------------------------------------------------------------------------ Runner.loo_moment_match, stubbed
class _StubCatalog(object):
    def __init__(self):
        self.calls = []

    def moment_match(self, plan, draws, stars, k_threshold, max_iters=30, cov=True, split=True, r_eff=1.0):
        self.calls.append(dict(draws=draws, stars=np.array(stars), thr=k_threshold, max_iters=max_iters, cov=cov, split=split))
        n, p = len(stars), draws.shape[1]
        return {"elpd": -10.0 - np.arange(n), "pareto_k": np.full(n, 0.2), "n_eff": np.full(n, 99.0),
                "k_before": np.full(n, 1.5), "k_loop": np.full(n, 0.3), "iterations": np.full(n, 2, np.int32),
                "accepted": np.tile(np.array([1, 1, 0], np.int32), (n, 1)), "A": np.tile(np.eye(p), (n, 1, 1)),
                "b": np.zeros((n, p))}


def test_runner_bookkeeping_on_a_stubbed_native_call():
    from mcmc_dynamics_amd.analysis import runner as rn
    cols = mh.closed_form_columns(0)
    fit = mh.closed_form_fit(cols)
    stub = _StubCatalog()
    fit._stretch_catalog = lambda pos: stub
    chain = np.random.default_rng(0).normal(size=(4, 30, 3))
    n = mh.N_STARS
    k = np.full(n, 0.1)
    k[[3, 7, 12]] = [0.9, 1.4, 0.75]
    pointwise = -np.arange(1.0, n + 1)
    loo = {"pareto_k": k, "pointwise": pointwise, "n_eff": np.full(n, 50.0), "k_threshold": 0.7, "lppd": -100.0,
           "n_samples": 4 * 20, "elpd_loo": pointwise.sum(), "n_bad_k": 3, "n_stars": n}
    out = fit.loo_moment_match(loo, chain, 10, max_stars=2, max_iters=5, cov=False)
    call = stub.calls[0]
    assert call["stars"].tolist() == [3, 7] and call["thr"] == 0.7 and call["max_iters"] == 5 and call["cov"] is False
    assert np.array_equal(call["draws"], chain[:, 10:, :].reshape(-1, 3))
    assert out["matched"].tolist() == [3, 7] and out["n_bad_k"] == 1
    want = pointwise.copy()
    want[[3, 7]] = [-10.0, -11.0]
    assert np.array_equal(out["pointwise"], want) and out["pareto_k"][7] == 0.2 and out["n_eff"][3] == 99.0
    assert out["pareto_k"][12] == 0.75 and out["n_eff"][12] == 50.0
    s_elpd, se, _ = rn._elpd_totals(want)
    assert out["elpd_loo"] == s_elpd and out["se"] == se and out["looic"] == -2.0 * s_elpd and out["p_loo"] == -100.0 - s_elpd
    assert out["k_before"].tolist() == [1.5, 1.5] and out["transform"]["A"].shape == (2, 3, 3)
    assert out["accepted"].shape == (2, 3) and out["iterations"].tolist() == [2, 2]
    assert loo["pareto_k"][7] == 1.4 and loo["pointwise"][3] == -4.0               # the input is left alone
    # explicit stars are sorted; none at all makes no native call
    out = fit.loo_moment_match(loo, chain, 10, stars=[12, 3], k_threshold=0.5)
    assert stub.calls[1]["stars"].tolist() == [3, 12] and stub.calls[1]["thr"] == 0.5
    quiet = dict(loo, pareto_k=np.full(n, 0.1))
    out = fit.loo_moment_match(quiet, chain, 10)
    assert len(stub.calls) == 2 and out["matched"].size == 0 and out["n_bad_k"] == 0 and out["elpd_loo"] == rn._elpd_totals(pointwise)[0]
    with pytest.raises(ValueError):
        fit.loo_moment_match(loo, chain, 5)                                      # another number of draws than loo saw
    with pytest.raises(ValueError):
        fit.loo_moment_match(loo, chain, 10, stars=[n])
    fit.close()


def test_runner_refusals():
    cols = mh.closed_form_columns(0)
    loo = {"pareto_k": np.full(mh.N_STARS, 2.0), "pointwise": np.zeros(mh.N_STARS), "n_eff": np.ones(mh.N_STARS),
           "k_threshold": 0.7, "lppd": 0.0, "n_samples": 8}
    chain = np.zeros((1, 8, 3))
    fit = mh.closed_form_fit(cols, precision="f32")
    with pytest.raises(NotImplementedError):
        fit.loo_moment_match(loo, chain, 0)
    fit.close()
    fit = mh.closed_form_fit(cols)
    fit.parameters["v_maxx"].set(expr="2 * v_sys")
    with pytest.raises(NotImplementedError):
        fit.loo_moment_match(loo, np.zeros((1, 8, 2)), 0)
    fit.close()


# ------------------------------------------------------------------------------------------- the closed-form harness
def test_closed_form_harness_on_the_oracle():
    """Sizes the end-to-end GPU test (tests/test_gpu_mmatch.py) on the NumPy oracle alone: one data set (20 stars, verr in
    U(0.5, 2), star 0 moved 8 sigma off), S = 4096 exact posterior draws per seed 0 .. 5.  The oracle gave
        plain PSIS            mean |error| of star 0's elpd 0.423, k^ 0.89 .. 1.14
        moment matching       mean |error| 0.0233 (a factor 18 where the GPU test asks for 4: a margin of 4.5), k^ <= 0.46
        loop only (split=0)   differs from the split estimate on every seed
    With the data redrawn per seed the factor was 10.8 (one unlucky geometry carries most of the error), below the margin
    of 3 the harness is asked to keep, hence the fixed data set; at 7 sigma the factor is 13.9, at 6 sigma 3.3."""
    cols = mh.closed_form_columns(0)
    X = mh.design(cols)
    exact = mh.exact_loo(cols, X, 0)
    ev = mh.numpy_evaluate(cols, X, 0)
    inside = lambda t: np.all(np.abs(t) <= 1000.0, axis=1)                          # noqa: E731
    flat = lambda t: np.zeros(len(t))                                                # noqa: E731
    thr = psh.k_threshold(mh.N_DRAWS)
    plain, matched = [], []
    for seed in range(6):
        draws = mh.exact_draws(cols, X, seed)
        a = mh.moment_match(draws, ev, inside, flat, thr, max_iters=0)
        b = mh.moment_match(draws, ev, inside, flat, thr)
        c = mh.moment_match(draws, ev, inside, flat, thr, split=False)
        assert a["iterations"] == 0 and a["pareto_k"] == a["k_before"] == b["k_before"] > thr
        assert b["pareto_k"] <= thr and b["k_loop"] < b["k_before"] and b["accepted"].sum() >= 1
        assert c["pareto_k"] == c["k_loop"] == b["k_loop"] and c["elpd"] != b["elpd"]
        assert np.array_equal(b["A"], c["A"])
        plain.append(abs(a["elpd"] - exact))
        matched.append(abs(b["elpd"] - exact))
        # the baseline is plain PSIS
        want = psh.psis_star(ev(draws)[1])
        assert abs(a["elpd"] - want[0]) < 1e-12 and abs(a["pareto_k"] - want[1]) < 1e-12
    assert np.mean(matched) * 12.0 <= np.mean(plain)                                 # margin 3 over the GPU test's factor 4

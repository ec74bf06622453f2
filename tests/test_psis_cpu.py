"""CPU check of the per-star PSIS-LOO of mcd_psis_loo (csrc/mcd_psis.h compiled for the host by tests/emul/psis_emul.cpp)
against the NumPy oracle of tests/psis_helper.py on synthetic lnL matrices; the GPD fit on samples of known shape; the
totals of Runner.loo (loo_summary) and elpd_compare."""
import numpy as np
import pytest

import psis_helper as ph
from mcmc_dynamics_amd.analysis.runner import elpd_compare, loo_summary, waic_summary


@pytest.mark.parametrize("name,lnl", [
    ("near_gaussian", ph.near_gaussian(40, 4096)),
    ("heavy_tailed", ph.heavy_tailed(40, 2000)),
    ("repeated_rows", ph.repeated_rows(40, 3000)),
    ("short_s", ph.near_gaussian(12, 20)),
    ("tiny_s", ph.near_gaussian(6, 3)),
])
def test_emulated_star_matches_numpy(name, lnl):
    got = ph.emul_psis(lnl)
    ph.assert_matches(got, ph.numpy_psis(lnl))
    if name == "heavy_tailed":
        assert np.count_nonzero(got["pareto_k"] > 0.7) >= 30
    if name in ("short_s", "tiny_s"):                        # M < 5: no smoothing, k^ = +inf
        assert ph.tail_len(lnl.shape[1]) < 5 and np.all(got["pareto_k"] == np.inf)
    if name == "near_gaussian":
        assert np.all(got["pareto_k"] < 0.5)


def test_repeated_rows_tie_at_the_cutoff():
    """Ties are the normal case in a chain: the cutoff sits inside a run of equal values for many stars."""
    lnl = ph.repeated_rows(60, 500, seed=8)
    M = ph.tail_len(500)
    ties = 0
    for row in lnl:
        lw = -row - (-row).max()
        o = np.argsort(lw, kind="stable")
        ties += lw[o[500 - M - 1]] == lw[o[500 - M]]
    assert ties >= 5
    ph.assert_matches(ph.emul_psis(lnl), ph.numpy_psis(lnl))


def test_r_eff_changes_the_tail():
    lnl = ph.heavy_tailed(10, 1000, seed=4)
    for r_eff in (0.3, 2.0):
        assert lib_tail(1000, r_eff) == ph.tail_len(1000, r_eff)
        ph.assert_matches(ph.emul_psis(lnl, r_eff), ph.numpy_psis(lnl, r_eff))


def lib_tail(S, r_eff):
    return int(ph.lib().emul_psis_tail_len(S, r_eff))


def test_tail_length():
    assert lib_tail(4096, 1.0) == 192 and lib_tail(65536, 1.0) == 768
    for S in (1, 2, 19, 20, 21, 25, 100, 1000, 70000):
        assert lib_tail(S, 1.0) == ph.tail_len(S)


def test_constant_star():
    lnl = np.full((3, 600), -3.25)
    lnl[1] = -1234.5
    lnl[2] = 0.0
    got = ph.emul_psis(lnl)
    assert np.all(got["pareto_k"] == -np.inf)
    assert np.all(np.abs(got["elpd_loo"] - got["lppd"]) <= 2 * np.spacing(np.abs(got["lppd"]) + 1.0))
    assert np.all(np.abs(got["lppd"] - got["elpd_loo"]) <= 1e-12)
    ph.assert_matches(got, ph.numpy_psis(lnl))


def test_seventy_thousand_samples():
    lnl = ph.near_gaussian(3, 70000, seed=6)
    ph.assert_matches(ph.emul_psis(lnl), ph.numpy_psis(lnl))


@pytest.mark.parametrize("k", [0.2, 0.5, 0.9])
def test_gpd_fit_recovers_a_known_shape(k):
    rng = np.random.default_rng(42)
    x = (rng.uniform(size=4000) ** (-k) - 1.0) / k              # GPD(k, sigma = 1)
    k_hat, sigma = ph.emul_gpd_fit(x)
    assert abs(k_hat - k) < 0.06
    assert abs(sigma - 1.0) < 0.1
    want_k, want_sigma = ph.gpdfit(np.sort(x))
    assert abs(k_hat - want_k) < 1e-10 and abs(sigma - want_sigma) < 1e-10


def test_narrow_posterior_loo_agrees_with_waic():
    lnl = -2.0 + np.random.default_rng(9).normal(scale=0.02, size=(50, 4000))
    got = ph.emul_psis(lnl)
    w = waic_summary(got["lppd"], lnl.var(axis=1, ddof=1), 4000)
    loo = loo_summary(got["elpd_loo"], got["lppd"], got["pareto_k"], 4000)
    assert abs(loo["elpd_loo"] - w["elpd_waic"]) <= 1e-3 * abs(w["elpd_waic"])


def test_loo_summary_by_hand():
    elpd = np.array([-1.2, -2.5, -3.5, -0.75])
    lppd = np.array([-1.0, -2.0, -3.5, -0.5])
    k = np.array([0.1, 0.8, -np.inf, np.inf])
    s = loo_summary(elpd, lppd, k, 4096)
    assert s["elpd_loo"] == pytest.approx(-7.95, abs=1e-14)
    assert s["p_loo"] == pytest.approx(0.95, abs=1e-14)
    assert s["looic"] == pytest.approx(15.9, abs=1e-13)
    assert s["lppd"] == pytest.approx(-7.0, abs=1e-14)
    assert s["se"] == pytest.approx(np.sqrt(4 * np.var(elpd, ddof=1)), rel=1e-13)
    assert s["k_threshold"] == 0.7 and s["n_bad_k"] == 2          # 0.8 and +inf (a tail too short to fit)
    assert s["n_stars"] == 4 and s["n_samples"] == 4096
    assert np.array_equal(s["pointwise"], elpd) and np.array_equal(s["pareto_k"], k)
    assert loo_summary(elpd, lppd, k, 100)["k_threshold"] == pytest.approx(0.5, abs=1e-15)


class _TwoRanks(object):
    """Stands in for the host group: the other rank's totals are `other`."""
    def __init__(self, other):
        self.other = other

    def allreduce(self, a):
        return np.asarray(a) + self.other


def test_loo_totals_are_summed_over_the_ranks():
    rng = np.random.default_rng(3)
    elpd = -rng.uniform(1, 4, 7)
    lppd = elpd + rng.uniform(0, 0.3, 7)
    k = np.array([0.1, 0.9, 0.3, np.inf, 0.2, 0.75, -np.inf])
    whole = loo_summary(elpd, lppd, k, 500)
    e = elpd[4:]
    other = np.array([lppd[4:].sum(), e.sum(), np.dot(e, e), 3.0, float(np.count_nonzero(k[4:] > whole["k_threshold"]))])
    split = loo_summary(elpd[:4], lppd[:4], k[:4], 500, group=_TwoRanks(other))
    for key in ("elpd_loo", "p_loo", "looic", "se", "lppd"):
        assert split[key] == pytest.approx(whole[key], rel=1e-13)
    assert split["n_stars"] == 7 and split["n_bad_k"] == whole["n_bad_k"] == 3 and split["pointwise"].size == 4


def test_elpd_compare_uses_the_paired_standard_error():
    rng = np.random.default_rng(5)
    common = -rng.uniform(1, 5, 200)                              # star-to-star spread shared by both models
    a = {"pointwise": common + rng.normal(scale=0.01, size=200)}
    b = {"pointwise": common - 0.02 + rng.normal(scale=0.01, size=200)}
    c = elpd_compare(a, b)
    d = a["pointwise"] - b["pointwise"]
    assert c["elpd_diff"] == pytest.approx(d.sum(), rel=1e-13)
    assert c["se_diff"] == pytest.approx(np.sqrt(200 * np.var(d, ddof=1)), rel=1e-12)
    se_a = np.sqrt(200 * np.var(a["pointwise"], ddof=1))
    assert c["se_diff"] < 0.05 * se_a                            # far below what subtracting two se's suggests
    # two ranks
    da, db = {"pointwise": a["pointwise"][:120]}, {"pointwise": b["pointwise"][:120]}
    rest = d[120:]
    split = elpd_compare(da, db, group=_TwoRanks(np.array([rest.sum(), np.dot(rest, rest), 80.0])))
    assert split["elpd_diff"] == pytest.approx(c["elpd_diff"], rel=1e-13)
    assert split["se_diff"] == pytest.approx(c["se_diff"], rel=1e-10) and split["n_stars"] == 200
    with pytest.raises(ValueError, match="different stars"):
        elpd_compare(a, {"pointwise": b["pointwise"][:10]})


def test_tile_plan_stays_within_the_budget():
    L = ph.lib()
    MB = 1 << 20
    for n, S, fixed, budget in ((2000, 256, 40000, 1 * MB), (1000000, 4096, 600000, 256 * MB), (10, 70000, 10 ** 7, 64 * MB)):
        t = L.emul_psis_tile_stars(n, S, fixed, budget)
        assert 1 <= t <= n and fixed + t * S * 8 <= budget
        assert t == n or t < 64 or t % 64 == 0
    assert L.emul_psis_tile_stars(100, 70000, 10 ** 6, 1 * MB) == 0

"""CPU check of the per-star posterior summaries of mcd_pointwise_posterior (csrc/mcd_posterior.h compiled for the host by
tests/emul/posterior_emul.cpp): the (star, sample) term, the running log-sum-exp / Welford state and the slice-ordered
merge against a NumPy restatement built from the oracle's per-star functions; the numerical corner cases; the WAIC
arithmetic of Runner.waic; the gfx950 ISA of the sample loop."""
import numpy as np
import pytest

import posterior_helper as ph
from mcmc_dynamics_amd.analysis.runner import waic_summary

MODELS = [0, 1, 2, 3, 4, 5, 6, 7, 8]               # 7, 8: the double Lynden-Bell models, second component live
BG_MODELS = (1, 2, 4, 5, 6, 8)


def rel(got, want):
    return float(np.max(np.abs(got - want) / np.maximum(np.abs(want), 1e-300)))


def var_ok(got, want, scale, rtol=1e-12):
    """Variances to `rtol` relative, or as close as terms of size `scale` that agree to `rtol` relative allow: a term error
    d moves a variance by up to 2 sd d + d^2.  (A star whose mixture is ruled by the fixed background has a variance of
    1e-28, the terms' rounding; the free-centre geometry of the kernels agrees with the reference's arctan2 form to
    ~3e-13 per term, which moves a variance of 0.005 by 5e-12 of itself.)"""
    d = rtol * np.abs(scale)
    return bool(np.all(np.abs(got - want) <= rtol * want + 2.0 * d * np.sqrt(want) + d * d))


@pytest.fixture(scope="module")
def catalogue():
    return ph.model_catalog(300, 0)


@pytest.mark.parametrize("model", MODELS)
@pytest.mark.parametrize("free", [False, True])
def test_emulated_summaries_match_numpy(catalogue, model, free):
    centre = None if free else ph.CENTRE
    table = ph.samples(catalogue, model, free, 200)
    mem = model in BG_MODELS
    got = ph.posterior(catalogue, table, model, centre, mem)
    want = ph.numpy_posterior(catalogue, table, model, centre)
    assert rel(got["lppd"], want["lppd"]) < 1e-12
    assert var_ok(got["lnl_var"], want["lnl_var"], want["lppd"])
    if mem:
        assert np.max(np.abs(got["pmem_mean"] - want["pmem_mean"])) < 1e-12
        assert np.max(np.abs(got["pmem_std"] - want["pmem_std"])) < 1e-12
        assert np.all((got["pmem_mean"] >= 0) & (got["pmem_mean"] <= 1))
    else:
        assert "pmem_mean" not in got


@pytest.mark.parametrize("model", [0, 2, 4])
def test_merge_order_does_not_change_the_result(catalogue, model):
    table = ph.samples(catalogue, model, True, 192, seed=11)
    mem = model in BG_MODELS
    one = ph.posterior(catalogue, table, model, None, mem, n_slices=1)
    for k in (2, 7, 64):
        got = ph.posterior(catalogue, table, model, None, mem, n_slices=k)
        for f in one:
            scale = np.maximum(np.abs(one[f]), 1.0) if f in ("lppd", "lnl_var") else 1.0
            assert np.max(np.abs(got[f] - one[f]) / scale) < 1e-13, (k, f)


def test_slice_plan_fills_the_chip_and_covers_the_samples():
    for n, S in ((10000, 16384), (1000000, 4096), (100000, 4096), (1, 1), (64, 1000), (10000, 100)):
        k, ln = ph.plan(n, S)
        assert k >= 1 and ln >= 1 and (k - 1) * ln < S <= k * ln
        if S >= 64 * k:
            assert ln >= 64 or k == 1
    k, _ = ph.plan(10000, 16384)
    assert k * ((10000 + 63) // 64) >= 4 * 1024          # >= 4 waves per SIMD of 256 CUs x 4 SIMDs
    assert ph.plan(1000000, 4096)[0] == 1


def test_extreme_terms_stay_finite():
    rng = np.random.default_rng(5)
    S = 300
    x = -5e3 + rng.normal(scale=3.0, size=(4, S))
    x[1] = -1e4 + rng.normal(scale=50.0, size=S)
    x[2, 17] = -2e4                                     # one sample far below the rest
    for k in (0, 1, 7):
        got = ph.posterior_terms(x, n_slices=k)
        mx = x.max(axis=1)
        want = mx + np.log(np.exp(x - mx[:, None]).sum(axis=1)) - np.log(S)
        assert np.all(np.isfinite(got["lppd"]))
        assert rel(got["lppd"], want) < 1e-13
        assert rel(got["lnl_var"], x.var(axis=1, ddof=1)) < 1e-11


def test_an_outlier_star_without_background_keeps_a_finite_lppd(catalogue):
    cat = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in catalogue.items()}
    cat["v"][5] = cat["truth"]["v_sys"] + 900.0          # ~ -4e3 in lnL of the model without background
    table = ph.samples(cat, 0, False, 100)
    got = ph.posterior(cat, table, 0, ph.CENTRE, False)
    want = ph.numpy_posterior(cat, table, 0, ph.CENTRE)
    assert want["lppd"][5] < -1e3 and np.isfinite(got["lppd"][5])
    assert rel(got["lppd"], want["lppd"]) < 1e-12


def test_constant_terms_give_exactly_zero_variance():
    x = np.full((3, 257), -1234.5678)
    x[1] = 0.1
    x[2] = -7.0e3
    p = np.full_like(x, 0.3)
    for k in (0, 1, 2, 7):
        got = ph.posterior_terms(x, p, n_slices=k)
        assert np.all(got["lnl_var"] == 0.0) and np.all(got["pmem_std"] == 0.0)
        assert rel(got["lppd"], x[:, 0]) < 1e-15
        assert np.max(np.abs(got["pmem_mean"] - 0.3)) < 1e-16


def test_one_sample_gives_the_term_itself(catalogue):
    for model in (0, 2, 5):
        table = ph.samples(catalogue, model, False, 1)
        got = ph.posterior(catalogue, table, model, ph.CENTRE, model in BG_MODELS)
        x, p = ph.star_terms(catalogue, table[0], model, ph.CENTRE)
        assert rel(got["lppd"], x) < 1e-12
        assert np.all(got["lnl_var"] == 0.0)
        if p is not None:
            assert np.max(np.abs(got["pmem_mean"] - p)) < 1e-12 and np.all(got["pmem_std"] == 0.0)


def test_waic_arithmetic_by_hand():
    lppd = np.array([-1.0, -2.0, -3.5])
    var = np.array([0.1, 0.5, 0.0])
    w = waic_summary(lppd, var, 40)
    elpd = np.array([-1.1, -2.5, -3.5])
    assert w["elpd_waic"] == pytest.approx(-7.1, abs=1e-14)
    assert w["p_waic"] == pytest.approx(0.6, abs=1e-14)
    assert w["waic"] == pytest.approx(14.2, abs=1e-13)
    assert w["lppd"] == pytest.approx(-6.5, abs=1e-14)
    # se = sqrt(N Var_i(elpd_i)): mean -7.1/3, deviations 1.2667, -0.1333, -1.1333, sample variance 2.90667 / 2
    assert w["se"] == pytest.approx(np.sqrt(3 * np.var(elpd, ddof=1)), rel=1e-13)
    assert w["se"] == pytest.approx(np.sqrt(4.36), rel=1e-12)
    assert w["n_stars"] == 3 and w["n_samples"] == 40 and w["n_high_variance"] == 1
    assert np.allclose(w["pointwise"], elpd, rtol=0, atol=1e-15)


def test_waic_totals_are_summed_over_the_ranks():
    class TwoRanks(object):
        """Stands in for the host group: the other rank holds `other`."""
        def __init__(self, other):
            self.other = other

        def allreduce(self, a):
            return np.asarray(a) + self.other

    lppd = np.array([-1.0, -2.0, -3.5, -0.25, -4.0])
    var = np.array([0.1, 0.5, 0.0, 0.45, 0.2])
    whole = waic_summary(lppd, var, 10)
    other = waic_summary(lppd[3:], var[3:], 10)
    e = other["pointwise"]
    totals = np.array([lppd[3:].sum(), var[3:].sum(), e.sum(), np.dot(e, e), 2.0, 1.0])
    split = waic_summary(lppd[:3], var[:3], 10, group=TwoRanks(totals))
    for key in ("elpd_waic", "p_waic", "waic", "se", "lppd"):
        assert split[key] == pytest.approx(whole[key], rel=1e-13)
    assert split["n_stars"] == 5 and split["n_high_variance"] == 2 and split["pointwise"].size == 3


def test_sample_loop_reads_samples_through_the_scalar_cache(tmp_path):
    """posterior_slice_kernel: the sample's derived constants are wave-uniform (s_load inside the loop), the star record
    is loaded once (no vector load inside the loop), no scratch; every model, centre mode, precision and output set."""
    import os
    import sys
    from conftest import ROOT
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import posterior_isa
    rows = posterior_isa.analyse(str(tmp_path))
    assert len(rows) == 2 * 2 * (2 + 5 * 2)
    for r in rows:
        assert r["s_load_in_loop"] >= 1, r
        assert r["vector_loads_in_loop"] == 0, r
        assert r["scratch_in_loop"] == 0, r
    # the budget DESIGN.md section 3.7 quotes: VALU instructions per (star, sample) term of the f64 kernels
    f64 = {(r["model"], r["free_centre"], r["membership"]): r["valu_per_term"] for r in rows if r["precision"] == "f64"}
    assert f64[("BGFIXED", False, True)] <= 320 and f64[("CONST", False, False)] <= 150
    assert max(f64.values()) <= 500

"""CPU: the rules of the exact leave-out refits (csrc/mcd_holdout.h through tests/emul/holdout_emul.cpp), the chunk plan
on range offsets, kfold_summary, reloo's bookkeeping, DataReader.take, the refusals of the Runner layer, and the harness of
the closed-form case that sizes the run of tests/test_gpu_holdout.py."""
import os
import sys

import numpy as np
import pytest

import holdout_helper as hh
from mcmc_dynamics_amd import DataReader, synthetic
from mcmc_dynamics_amd.analysis import BinnedConstantFit, ConstantFit
from mcmc_dynamics_amd.analysis.binned import BinnedSampler
from mcmc_dynamics_amd.analysis.runner import elpd_compare, kfold_summary, loo_summary

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------ offsets, ranges, combine
def test_offsets_validation():
    assert hh.offsets_error([0, 1, 1, 8], 33) is None                     # an empty set is fine
    assert hh.offsets_error([0, 33], 33) is None                          # the sets may cover everything
    assert hh.offsets_error([0, 0], 33) is None
    assert "non-decreasing" in hh.offsets_error([0, 5, 4], 33)
    assert "must be 0" in hh.offsets_error([1, 5], 33)
    assert "exceeds" in hh.offsets_error([0, 5, 34], 33)
    assert "n_sets" in hh.offsets_error([0], 33)


def test_range_table():
    assert hh.ranges([0, 1, 1, 8], 33).tolist() == [0, 1, 1, 8, 33]       # remainder range
    assert hh.ranges([0, 1, 2, 33], 33).tolist() == [0, 1, 2, 33]         # the sets cover all stars: none
    assert hh.ranges([0, 0], 33).tolist() == [0, 0, 33]
    assert hh.ranges([0, 33], 33).tolist() == [0, 33]


@pytest.mark.parametrize("n_sets,n_walkers,remainder", [(1, 2, True), (1, 3, False), (3, 66, True), (5, 7, False)])
def test_combine_rule_against_numpy(n_sets, n_walkers, remainder):
    rng = np.random.default_rng(n_sets * 100 + n_walkers)
    R, rows = n_sets + (1 if remainder else 0), n_sets * n_walkers
    m = rng.normal(scale=1e3, size=(R, rows))
    if n_sets > 1:
        m[1] = 0.0                                                        # a set with no chunks reduces to +0.0
    train, test = hh.combine(m, n_walkers)
    for row in range(rows):
        e = row // n_walkers
        want = 0.0
        for r in range(R):                                                # ascending r, from +0.0
            if r != e:
                want = want + m[r, row]
        assert train[row] == want and test[row] == m[e, row]
        assert not np.signbit(train[row]) or train[row] != 0.0
    if n_sets > 1:
        sl = slice(n_walkers, 2 * n_walkers)
        assert np.all(test[sl] == 0.0) and not np.any(np.signbit(test[sl]))
        assert np.allclose(train[sl], m[:, sl].sum(axis=0), rtol=1e-15)
    if R == 1:                                                            # E = 1, no remainder: nothing to train on
        assert np.all(train == 0.0) and not np.any(np.signbit(train))


@pytest.mark.parametrize("n", [33, 4099])
@pytest.mark.parametrize("sizes,w", [((1,), 2), ((1, 0, 7), 66), ((1, 1, 40, 0, 300), 258)])
def test_plan_on_range_offsets(n, sizes, w):
    offs = hh.sets_of_sizes(sizes, n)
    rng_offs = hh.ranges(offs, n)
    p = hh.plan(offs, n, len(sizes) * w)
    b, c, r = p["begin"], p["count"], p["range"]
    assert np.all(c > 0) and c.sum() == n and b[0] == 0 and np.all(np.diff(b) == c[:-1])
    for j in range(len(b)):                                               # no chunk straddles a boundary
        assert rng_offs[r[j]] <= b[j] and b[j] + c[j] <= rng_offs[r[j] + 1]
    assert np.all(np.diff(r) >= 0)
    for q in range(len(rng_offs) - 1):                                    # plan.offsets: each range's slots
        mine = np.flatnonzero(r == q)
        assert p["offsets"][q + 1] - p["offsets"][q] == mine.size
        if mine.size:
            assert mine[0] == p["offsets"][q]
        size = rng_offs[q + 1] - rng_offs[q]
        if size == 1:
            assert mine.size == 1 and c[mine[0]] == 1                     # singleton sets yield 1-star chunks
        if size == 0:
            assert mine.size == 0
    assert p["max_chunks_per_range"] == max(np.bincount(r, minlength=len(rng_offs) - 1))


def test_limits_are_the_documented_ones():
    assert hh.lib().emul_holdout_max_rows() == 65536
    assert hh.lib().emul_holdout_scratch_bytes() == 256 << 20


def test_new_kernels_use_no_scratch():
    """Every holdout_kernel<MODEL, FREE> and the combine kernel, compiled for gfx950: no scratch, no spills."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import holdout_resources
    rows = holdout_resources.analyse()
    assert sum(r["kernel"] == "holdout" for r in rows) == 14 and sum(r["kernel"] == "combine" for r in rows) == 1
    for r in rows:
        assert r["scratch_bytes_per_lane"] == 0 and r["vgpr_spill"] == 0 and r["sgpr_spill"] == 0, r
        assert r["lds_bytes"] == 0 and r["vgprs"] <= 128, r


# ------------------------------------------------------------------------------------------ summaries and bookkeeping
def test_kfold_summary_against_numpy():
    rng = np.random.default_rng(8)
    elpd = -rng.uniform(1, 6, 37)
    folds = rng.integers(0, 5, 37)
    s = kfold_summary(elpd, folds)
    assert s["elpd_kfold"] == pytest.approx(elpd.sum(), rel=1e-14)
    assert s["se"] == pytest.approx(np.sqrt(37 * np.var(elpd, ddof=1)), rel=1e-12)
    assert s["n_stars"] == 37 and s["n_folds"] == np.unique(folds).size
    assert np.array_equal(s["pointwise"], elpd) and np.array_equal(s["folds"], folds)
    # the se formula is loo_summary's
    assert s["se"] == pytest.approx(loo_summary(elpd, elpd, np.zeros(37), 100)["se"], rel=1e-14)
    assert elpd_compare(s, {"pointwise": elpd - 0.1})["elpd_diff"] == pytest.approx(3.7, rel=1e-12)
    with pytest.raises(ValueError, match="finite"):
        kfold_summary(np.array([1.0, np.nan]))
    with pytest.raises(ValueError, match="one fold id"):
        kfold_summary(elpd, folds[:5])


def _small_fit(n=40, **kwargs):
    c = synthetic.make_catalog(n, config=2, background=False)
    return ConstantFit(DataReader({k: c[k] for k in ("ra", "dec", "v", "verr")}), **kwargs)


def test_reloo_bookkeeping_with_a_stubbed_fit():
    fit = _small_fit()
    rng = np.random.default_rng(4)
    n = fit.n_data
    elpd = -rng.uniform(1, 4, n)
    lppd = elpd + rng.uniform(0, 0.2, n)
    k = rng.uniform(0.0, 0.5, n)
    k[[3, 17, 29, 31]] = [0.9, np.inf, 0.75, 1.4]                          # four bad stars
    loo = loo_summary(elpd, lppd, k, 4096)
    loo["n_eff"] = np.ones(n)
    exact = -rng.uniform(5, 9, n)
    seen = {}

    def stub(sets, **kw):
        seen["sets"], seen["kw"] = [list(s) for s in sets], kw
        out = np.full(n, np.nan)
        idx = np.array([s[0] for s in sets])
        out[idx] = exact[idx]
        return {"elpd": out, "lnl_var": out, "sets": sets, "sampler": None, "tau": np.ones(len(sets)),
                "converged": np.ones(len(sets), dtype=bool), "n_samples": 10}

    fit.holdout_fit = stub
    chain = rng.normal(size=(8, 30, fit.n_fitted_parameters))
    out = fit.reloo(loo, chain, 10, max_refits=3, n_walkers=8, seed=5)
    assert seen["sets"] == [[17], [31], [3]]                              # largest k^ first, at most three
    assert seen["kw"]["pos"].shape == (3, 8, fit.n_fitted_parameters)
    flat = chain[:, 10:, :].reshape(-1, chain.shape[2])                   # starts are post-burn-in rows of the chain
    assert all(np.any(np.all(flat == row, axis=1)) for row in seen["kw"]["pos"].reshape(-1, chain.shape[2]))
    assert np.array_equal(out["refit"], [17, 31, 3]) and out["n_bad_k"] == 1 and loo["n_bad_k"] == 4
    want = elpd.copy()
    want[[17, 31, 3]] = exact[[17, 31, 3]]
    assert np.array_equal(out["pointwise"], want) and np.array_equal(loo["pointwise"], elpd)     # the input is not touched
    assert out["elpd_loo"] == pytest.approx(want.sum(), rel=1e-14)
    assert out["p_loo"] == pytest.approx(lppd.sum() - want.sum(), rel=1e-12)
    assert out["looic"] == pytest.approx(-2 * want.sum(), rel=1e-14)
    assert out["se"] == pytest.approx(np.sqrt(n * np.var(want, ddof=1)), rel=1e-12)
    assert out["lppd"] == loo["lppd"] and out["k_threshold"] == loo["k_threshold"]
    assert elpd_compare(out, loo)["elpd_diff"] == pytest.approx((want - elpd).sum(), rel=1e-12)
    # explicit stars, and none at all
    out = fit.reloo(loo, chain, 10, stars=[5], n_walkers=8)
    assert seen["sets"] == [[5]] and out["n_bad_k"] == 4 and out["pointwise"][5] == exact[5]
    good = loo_summary(elpd, lppd, np.zeros(n), 4096)
    seen.clear()
    out = fit.reloo(good, chain, 10)
    assert not seen and out["refit"].size == 0 and out["elpd_loo"] == pytest.approx(good["elpd_loo"], rel=1e-14)


def test_holdout_layout():
    sets, perm, offs = ConstantFit._holdout_layout([[7, 2], [], [5]], 9)
    assert perm.tolist() == [7, 2, 5, 0, 1, 3, 4, 6, 8] and offs.tolist() == [0, 2, 2, 3]
    with pytest.raises(ValueError, match="disjoint"):
        ConstantFit._holdout_layout([[1, 2], [2]], 9)
    with pytest.raises(ValueError, match="lie in"):
        ConstantFit._holdout_layout([[9]], 9)


def test_data_reader_take_round_trip():
    c = synthetic.make_catalog(25, config=2, background=False)
    data = DataReader({k: c[k] for k in ("ra", "dec", "v", "verr")})
    perm = np.random.default_rng(2).permutation(25)
    taken = data.take(perm)
    assert type(taken) is DataReader and taken.sample_size == 25
    for key in ("ra", "dec", "v", "verr"):
        assert np.array_equal(taken.data[key], data.data[key][perm])
        assert taken.data.unit(key) == data.data.unit(key)
    back = taken.take(np.argsort(perm))
    assert all(np.array_equal(back.data[key], data.data[key]) for key in data.data.columns)
    assert data.take([3, 3, 1]).data["v"].tolist() == [c["v"][3], c["v"][3], c["v"][1]]
    with pytest.raises(IndexError):
        data.take([25])


class _Ranks(object):
    n_ranks, n_devices = 2, 1


def test_refusals_of_the_runner_layer():
    fit = _small_fit(context=_Ranks())
    loo = {"pareto_k": np.zeros(40), "k_threshold": 0.7, "pointwise": np.zeros(40), "lppd": 0.0}
    for call in (lambda: fit.holdout_fit([[1]]), lambda: fit.kfold(4), lambda: fit.reloo(loo, np.zeros((4, 4, 4)), 1, stars=[1])):
        with pytest.raises(NotImplementedError, match="2 ranks"):
            call()
    with pytest.raises(NotImplementedError, match="float64"):
        _small_fit(precision="f32").kfold(4)
    c = synthetic.make_catalog(120, config=2, background=False)
    data = DataReader({k: c[k] for k in ("ra", "dec", "v", "verr")})
    data.make_radial_bins(synthetic.CENTER_RA_DEG, synthetic.CENTER_DEC_DEG, nstars=40)
    binned = BinnedConstantFit(data)
    for call in (lambda: binned.holdout_fit([[1]]), lambda: binned.kfold(4), lambda: binned.reloo(loo, None, 0)):
        with pytest.raises(NotImplementedError, match="un-binned"):
            call()


# ------------------------------------------------------------------------------------------ the closed-form harness
def test_closed_form_harness_sizes_the_run():
    """The closed-form case of tests/test_gpu_holdout.py with a NumPy likelihood inside BinnedSampler (rng='device': the
    numbers the GPU run takes).  Sizes the run: with hh.N_WALKERS x (hh.N_STEPS - hh.N_BURN) samples per refit the
    standard error of the most extreme star's leave-one-out value must be at most half the difference between that value
    and the star's full-posterior lppd -- otherwise the GPU test could not tell a refit from no refit.  Recorded on the
    run below (64 walkers x 600 steps, 200 of them burn-in): difference 0.1765, standard error 0.0136 (ratio 13); z of the
    five stars +0.29, -1.07, -0.27, +1.70, -1.86."""
    cols = hh.closed_form_columns()
    stars = sorted(hh.PLANTED, key=lambda i: -abs(hh.PLANTED[i]))
    sets = [[i] for i in stars]
    exact, full = hh.exact_elpd(cols, sets), hh.exact_full_lppd(cols)
    mu, var = hh.posterior_without(cols, [])
    pos = float(mu) + np.sqrt(float(var)) * np.random.default_rng(1).normal(size=(len(sets), hh.N_WALKERS, 1))
    sampler = BinnedSampler(len(sets), hh.N_WALKERS, 1, hh.numpy_log_prob(cols, sets), seed=77, rng="device")
    sampler.run_mcmc(pos, hh.N_STEPS)
    chain = sampler.chain[:, :, hh.N_BURN:, 0]                            # (E, W, steps)
    z = []
    for e, i in enumerate(stars):
        pooled, se = hh.walker_estimates(chain[e], cols, i)
        z.append(float((pooled - exact[i]) / se))
        if e == 0:
            diff = float(abs(exact[i] - full[i]))
            print("most extreme star %d: exact loo %.6f, full lppd %.6f, difference %.4f, standard error %.4f" %
                  (i, float(exact[i]), float(full[i]), diff, se))
            assert se <= 0.5 * diff
    print("z of the NumPy refits:", z)
    assert np.all(np.abs(z) < 5.0)

"""mcd_psis_loo_expect on the CPU: the per-star arithmetic of csrc/mcd_psis.h / csrc/mcd_predictive.h (compiled by
tests/emul/loo_expect_emul.cpp) against the NumPy oracle of tests/loo_expect_helper.py by its accuracy rule, the two
statistical cases of DESIGN.md section 3.15 (planted star, small-sample calibration), and the resource report of the new
kernels."""
import os
import sys

import numpy as np
import pytest

import loo_expect_helper as lh
import posterior_helper as ph
import predictive_helper as pr
import psis_helper as ps

MATRICES = {"near_gaussian": ps.near_gaussian, "heavy_tailed": ps.heavy_tailed, "repeated_rows": ps.repeated_rows}
SHAPES = (1, 20, 24, 257, 1024)                       # S = 20: M = 4, no tail; S = 24: M = 5, the shortest tail
N = 6


def _rows(n, S, seed):
    """Random rows per star: a PIT-like row in [0, 1] (unit scale) and two rows with an offset far above their spread."""
    rng = np.random.default_rng(seed)
    x = np.empty((n, 3, S))
    x[:, 0] = rng.uniform(size=(n, S))
    x[:, 1] = 300.0 + 0.1 * rng.normal(size=(n, S))
    x[:, 2] = rng.normal(size=(n, S))
    return x, rng.normal(size=(S, 3)) * np.array([1.0, 10.0, 0.01]) + np.array([0.0, -50.0, 2.0])


def test_tail_lengths_of_the_shapes():
    assert [ps.tail_len(S) for S in SHAPES] == [1, 4, 5, 49, 96]


def test_oracle_weights_reproduce_psis_star():
    for name, make in MATRICES.items():
        lnl = make(N, 257)
        want, ref = lh.oracle_expect(lnl), ps.numpy_psis(lnl)
        assert np.all(np.abs(want["elpd_loo"] - ref["elpd_loo"]) <= 1e-12 * np.maximum(1.0, np.abs(ref["elpd_loo"]))), name
        assert np.all(np.abs(want["n_eff"] - ref["n_eff"]) <= 1e-12 * ref["n_eff"]), name
        assert np.array_equal(want["pareto_k"], ref["pareto_k"]), name


@pytest.mark.parametrize("S", SHAPES)
@pytest.mark.parametrize("name", sorted(MATRICES))
def test_emulation_matches_oracle(name, S):
    lnl = MATRICES[name](N, S)
    x, func = _rows(N, S, seed=S)
    got = lh.emul_expect(lnl, x, func)
    lh.check_expect(got, lnl, x, func, unit_rows=(0,), what="{0} S={1}".format(name, S))
    ref = ps.emul_psis(lnl)
    assert np.array_equal(got["pareto_k"], ref["pareto_k"]) and np.array_equal(got["n_eff"], ref["n_eff"])


def test_heavy_tails_have_bad_k():
    """The heavy-tailed matrix exercises the smoothing where it matters: every k^ is above 0.7."""
    assert np.all(lh.emul_expect(ps.heavy_tailed(N, 1024))["pareto_k"] > 0.7)


@pytest.mark.parametrize("S", SHAPES)
def test_constant_column_returns_the_constant(S):
    lnl = ps.heavy_tailed(N, S)
    func = np.tile(np.array([[300.0, -0.125, 1e-3]]), (S, 1))
    got = lh.emul_expect(lnl, None, func)["func"]
    assert np.all(np.abs(got - func[0]) <= 1e-14 * np.abs(func[0]))
    assert np.array_equal(lh.emul_expect(lnl, None, np.zeros((S, 2)))["func"], np.zeros((N, 2)))


def test_one_sample_returns_its_own_values():
    lnl = ps.near_gaussian(N, 1)
    x, func = _rows(N, 1, seed=5)
    got = lh.emul_expect(lnl, x, func)
    assert np.array_equal(got["rows"], x[:, :, 0])
    assert np.array_equal(got["func"], np.tile(func[0], (N, 1)))
    assert np.all(got["n_eff"] == 1.0) and np.all(got["pareto_k"] == np.inf)


@pytest.mark.parametrize("model,free", [(0, False), (2, True), (4, False)])
def test_repeated_row_gives_the_posterior_means(model, free):
    """A chain of one repeated row: every weight is 1 / S, so the expectations are the posterior means of
    predictive_helper.predictive (the emulated mcd_posterior_predictive: the same term arithmetic) to 1e-13."""
    cat = pr.head(ph.model_catalog(80, 0, seed=7), 70)
    centre = None if free else ph.CENTRE
    row = ph.samples(cat, model, free, 1)
    table = np.repeat(row, 48, axis=0)
    mix = model in pr.MIX_MODELS
    got = lh.emul_model(cat, table, model, centre, mix=mix)
    want = pr.predictive(cat, table, model, centre, mix=mix)
    vmax = float(np.max(np.abs(cat["v"])))
    for key, ref, scale in (("pit", "pit", 1.0), ("z", "z_mean", np.maximum(1.0, np.abs(want["z_mean"]))),
                            ("vlos", "vlos_mean", vmax), ("sigma", "sigma_mean", np.maximum(1.0, want["sigma_mean"])),
                            ("pit_mix", "pit_mix", 1.0))[:5 if mix else 4]:
        err = np.abs(got[key] - want[ref])
        assert np.all(err <= 1e-13 * scale), (key, float(np.max(err / scale)))
    assert np.all(got["pareto_k"] == -np.inf)            # a constant tail
    assert np.all(np.abs(got["n_eff"] - 48.0) <= 1e-9)


def _model_against_oracle(model, free):
    centre = None if free else ph.CENTRE
    mix = model in pr.MIX_MODELS
    cat = pr.head(ph.model_catalog(80, 0, seed=7), 65)
    table = ph.samples(cat, model, free, 257)
    if free:
        cat = pr.clear_of_centres(cat, *pr.sample_centres(table, model))
    got = lh.emul_model(cat, table, model, centre, mix=mix)
    lnl = lh.lnl_rows(cat, table, model, centre)
    x, keys = lh.term_rows(cat, table, model, centre, mix=mix)
    rows = {"rows": np.stack([got[k] for k in keys], axis=1), "pareto_k": got["pareto_k"]}
    lh.check_expect(rows, lnl, x, unit_rows=(0, 4) if mix else (0,), what="model {0}".format(model))


def test_model_emulation_matches_oracle():
    """The whole call (terms and weights from the catalogue) against the oracle fed with the emulation's own lnL."""
    _model_against_oracle(2, False)


@pytest.mark.parametrize("free", [False, True])
@pytest.mark.parametrize("model", [7, 8])
def test_double_model_emulation_matches_oracle(model, free):
    """The same for the double Lynden-Bell models with a live second component (posterior_term<7 | 8>, predictive_term<7 | 8,
    ..., MIX>): the oracle's lnL and rows hold both rotation terms."""
    _model_against_oracle(model, free)


def test_tile_plan_with_rows():
    lb = ps.lib()
    for n, S, fixed, budget in ((1000, 256, 4096, 1 << 20), (70, 257, 0, 1 << 30), (10 ** 6, 4096, 10 ** 7, 2048 << 20)):
        assert lh.tile_stars_rows(n, S, 1, fixed, budget) == lb.emul_psis_tile_stars(n, S, fixed, budget)
        for rows in (5, 6):
            t = lh.tile_stars_rows(n, S, rows, fixed, budget)
            assert 1 <= t <= n and (t == n or t % 64 == 0 or t < 64)
            assert fixed + t * rows * S * 8 <= budget
            if t < n:
                assert fixed + (t + 64) * rows * S * 8 > budget
    assert lh.tile_stars_rows(10, 256, 5, 0, 5 * 256 * 8 - 1) == 0
    assert lh.tile_stars_rows(10, 256, 5, 0, 5 * 256 * 8) == 1


def test_planted_star_moves_sigma_max():
    """calibration_case(n=300) with star 7 at +4 sigma: removing it lowers sigma_max by ~0.76 posterior standard
    deviations (k^ 0.33) and no other (star, parameter) pair moves by half as much; for the oracle, then the emulation."""
    cat, table, lnl, z, mean, std = lh.planted_case()
    want = lh.oracle_expect(lnl, None, z)
    lh.planted_property(want["func"])
    assert want["pareto_k"][lh.PLANTED_STAR] < ps.k_threshold(table.shape[0])
    got = lh.emul_expect(lnl, None, z)
    lh.planted_property(got["func"])
    lh.check_expect(got, lnl, None, z, what="planted")


def test_small_sample_calibration():
    """40 data sets of 12 stars drawn from the model itself, 512 Metropolis samples each, the 480 PITs pooled into 10
    bins: the posterior PIT fails the chi^2(9) test at 0.999 (the data are used twice), the LOO-PIT passes it."""
    from mcmc_dynamics_amd.analysis.runner import ppc_summary
    sets = lh.small_sample_sets()
    post = np.concatenate([pit.mean(axis=1) for _, pit in sets])
    loo = np.concatenate([lh.oracle_expect(lnl, pit[:, None, :])["rows"][:, 0] for lnl, pit in sets])
    s_post, s_loo = ppc_summary(post, None, 10), ppc_summary(loo, None, 10)
    print("posterior PIT chi2 {0:.1f} tail {1:.3f}; LOO-PIT chi2 {2:.1f} tail {3:.3f}".format(
        s_post["chi2"], s_post["tail_fraction"], s_loo["chi2"], s_loo["tail_fraction"]))
    assert s_post["n_stars"] == s_loo["n_stars"] == 480
    assert s_post["chi2"] > lh.CHI2_9_Q999
    assert s_loo["chi2"] < lh.CHI2_9_Q999
    # the emulation gives the same LOO-PITs
    lnl, pit = sets[0]
    lh.check_expect(lh.emul_expect(lnl, pit[:, None, :]), lnl, pit[:, None, :], unit_rows=(0,), what="set 0")


def test_new_kernels_meet_the_resource_rule(tmp_path):
    """Every loox_term_kernel<MODEL, FREE, MODE, T> and loox_tail_kernel<XR>, compiled for gfx950: 0 bytes of scratch per
    lane, no spilled VGPR and at most 128 VGPRs (DESIGN.md section 3.12's condition for shipping the device library's
    erfc)."""
    from conftest import ROOT
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import loo_expect_resources
    rows = loo_expect_resources.analyse(str(tmp_path))
    terms = [r for r in rows if r["kernel"] == "term"]
    # two precisions x (7 models x 2 centre modes x {lnL only, predictive rows} + pit_mix for two models)
    assert len(terms) == 2 * (7 * 2 * 2 + 2 * 2)
    assert sorted(r["extra_rows"] for r in rows if r["kernel"] == "tail") == [0, 4, 5]
    assert len(rows) == len(terms) + 3
    for r in rows:
        assert r["scratch_bytes_per_lane"] == 0, r
        assert r["vgpr_spill"] == 0 and r["agprs"] == 0, r
        assert r["vgprs"] <= 128, r

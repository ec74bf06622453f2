"""CPU check of the per-star posterior predictive checks of mcd_posterior_predictive (csrc/mcd_predictive.h compiled for
the host by tests/emul/predictive_emul.cpp): the (star, sample) term, the running state and the slice-ordered merge against
the exact oracle of predictive_helper (the accuracy rule stated there); the planted stars; the PPC arithmetic of
analysis/runner.py: ppc_summary; the calibration case; the gfx950 resource use of every instantiation."""
import mpmath
import numpy as np
import pytest
from scipy import special

import posterior_helper as ph
import predictive_helper as pr
from mcmc_dynamics_amd.analysis.runner import ppc_summary
from test_posterior_cpu import var_ok

MODELS = [0, 1, 2, 3, 4, 5, 6, 7, 8]               # 7, 8: the double Lynden-Bell models, second component live


@pytest.fixture(scope="module")
def catalogue():
    return ph.model_catalog(300, 0)


def _case(catalogue, model, free, S, seed=3):
    table = ph.samples(catalogue, model, free, S, seed=seed)
    cat = pr.clear_of_centres(catalogue, *pr.sample_centres(table, model)) if free else catalogue
    return cat, table, (None if free else ph.CENTRE)


@pytest.mark.parametrize("model", MODELS)
@pytest.mark.parametrize("free", [False, True])
def test_emulated_summaries_follow_the_rule(catalogue, model, free):
    cat, table, centre = _case(catalogue, model, free, 200)
    mix = model in pr.MIX_MODELS
    got = pr.predictive(cat, table, model, centre, mix)
    exact, np64, vmax = pr.Reference(cat, table, model, centre).at()
    assert ("pit_mix" in got) == mix
    pr.check_rule(got, exact, np64, vmax, var_ok, rtol=1e-12, cell=(model, free))
    for f in ("tail_p", "pit") + (("pit_mix",) if mix else ()):
        assert np.all((got[f] >= 0.0) & (got[f] <= 1.0))


def _merge_scale(one, f, vmax):
    if f in ("vlos_mean", "vlos_std"):
        return vmax
    if f in ("z_mean", "z_std"):
        return np.maximum(1.0, np.abs(one["z_mean"]))
    if f in ("sigma_mean", "sigma_std"):
        return np.maximum(1.0, one["sigma_mean"])
    return 1.0


@pytest.mark.parametrize("model", [0, 2, 4, 5])
def test_merge_order_does_not_change_the_result(catalogue, model):
    cat, table, centre = _case(catalogue, model, True, 192, seed=11)
    mix = model in pr.MIX_MODELS
    vmax = float(np.max(np.abs(cat["v"])))
    one = pr.predictive(cat, table, model, None, mix, n_slices=1)
    for k in (2, 7, 64):
        got = pr.predictive(cat, table, model, None, mix, n_slices=k)
        for f in one:
            assert np.max(np.abs(got[f] - one[f]) / _merge_scale(one, f, vmax)) < 1e-13, (k, f)


def _rotation_free(S, f_back=0.3):
    """CONST_BGGAUSS rows without rotation and with one v_sys, so that d = v_i - v_sys exactly; sigma_max varies."""
    rng = np.random.default_rng(2)
    sig = 8.0 * (1.0 + 0.05 * rng.normal(size=S))
    rows = np.zeros((S, 7))                              # v_sys, sigma_max, v_maxx, v_maxy, v_back, sigma_back, f_back
    rows[:, 0], rows[:, 1] = 3.25, sig
    rows[:, 4], rows[:, 5], rows[:, 6] = 20.0, 40.0, f_back
    return rows


def planted_case(S=130):
    """Eight stars under rotation-free samples: 0 on the model exactly, 1 / 2 at z ~ +-45, 3 with verr = 0, 4 with density
    0, the rest ordinary."""
    cat = pr.head(ph.model_catalog(64, 0), 8)
    table = _rotation_free(S)
    norm = np.sqrt(cat["verr"] ** 2 + 64.0)
    cat["v"][0] = 3.25
    cat["v"][1] = 3.25 + 45.0 * norm[1]
    cat["v"][2] = 3.25 - 45.0 * norm[2]
    cat["verr"][3] = 0.0
    cat["density"][4] = 0.0
    return cat, table


def test_planted_stars():
    cat, table = planted_case()
    got = pr.predictive(cat, table, 2, ph.CENTRE, True)
    # v_i exactly on the model: z = 0 in every sample
    assert got["z_mean"][0] == 0.0 and got["z_std"][0] == 0.0 and got["tail_p"][0] == 1.0 and got["pit"][0] == 0.5
    # z ~ +-45: erfc underflows to an exact 0 on the far side; nothing is formed as 1 - (a value near 1)
    assert 40.0 < got["z_mean"][1] < 50.0 and -50.0 < got["z_mean"][2] < -40.0
    assert got["tail_p"][1] == 0.0 and got["pit"][1] == 1.0
    assert got["tail_p"][2] == 0.0 and got["pit"][2] == 0.0
    assert np.isfinite(got["z_std"][1]) and got["z_std"][1] > 0.0
    # verr = 0: n = sigma^2, every output finite; sigma is sigma_max itself
    assert all(np.isfinite(got[f][3]) for f in got)
    assert abs(got["sigma_mean"][3] - table[:, 1].mean()) < 1e-14 * 8.0
    # density = 0: m = 0, pit_mix is the background CDF
    zb = (cat["v"][4] - 20.0) / np.sqrt(cat["verr"][4] ** 2 + 1600.0)
    assert abs(got["pit_mix"][4] - 0.5 * special.erfc(-zb / np.sqrt(2.0))) < 5e-16      # a few ulp of 0.5
    exact, np64, vmax = pr.Reference(cat, table, 2, ph.CENTRE).at()
    pr.check_rule(got, exact, np64, vmax, var_ok, rtol=1e-12, cell="planted")
    # f_back = 0: m = 1, pit_mix equals pit bit for bit (star 4, density 0 / 0, is NaN and alone in that)
    g0 = pr.predictive(cat, _rotation_free(130, f_back=0.0), 2, ph.CENTRE, True)
    keep = np.arange(8) != 4
    assert g0["pit_mix"][keep].tobytes() == g0["pit"][keep].tobytes()
    assert np.isnan(g0["pit_mix"][4]) and np.isfinite(g0["pit"][4])


def test_a_non_finite_term_stays_with_its_star():
    """sigma = 0 with verr = 0: z = d / 0.  That star's outputs are not finite; no other star notices."""
    cat, table = planted_case(70)
    table[:, 1] = 0.0
    cat["verr"][5] = 0.0
    cat["v"][5] = 3.25                                   # 0 / 0
    got = pr.predictive(cat, table, 2, ph.CENTRE, True)
    assert np.isnan(got["z_mean"][5]) and np.isnan(got["pit"][5])
    assert not np.isfinite(got["z_mean"][3])             # verr = 0, v off the model: d / 0
    others = np.arange(8)[[0, 1, 2, 4, 6, 7]]
    for f in got:
        assert np.all(np.isfinite(got[f][others])), f


def test_a_repeated_vector_gives_exactly_zero_spreads(catalogue):
    for model, free in ((0, False), (2, True), (4, False), (5, True)):
        row = ph.samples(catalogue, model, free, 1)
        centre = None if free else ph.CENTRE
        mix = model in pr.MIX_MODELS
        term = pr.predictive(catalogue, row, model, centre, mix)
        for k in (0, 1, 2, 7):
            got = pr.predictive(catalogue, np.tile(row, (257, 1)), model, centre, mix, n_slices=k)
            for f in got:
                if f.endswith("_std"):
                    assert np.all(got[f] == 0.0), (model, k, f)
                else:
                    assert got[f].tobytes() == term[f].tobytes(), (model, k, f)


def test_one_sample_gives_the_term_itself(catalogue):
    for model in (0, 2, 5):
        table = ph.samples(catalogue, model, False, 1)
        mix = model in pr.MIX_MODELS
        got = pr.predictive(catalogue, table, model, ph.CENTRE, mix)
        ref = pr.Reference(catalogue, table, model, ph.CENTRE)
        exact, np64, vmax = ref.at()
        assert np.array_equal(exact["z_mean"], ref.exact["z"][0])             # the oracle's "mean" of one term is the term
        pr.check_rule(got, exact, np64, vmax, var_ok, rtol=1e-12, cell=(model, "S=1"))
        assert all(np.all(got[f] == 0.0) for f in ("z_std", "vlos_std", "sigma_std"))


def test_erfc_against_mpmath():
    """The header's erfc (libm on both sides) on |x| in [0, 40]: a few ulp, and exact zeros only where the true value lies
    below the smallest denormal.  The oracle's (scipy): 1e-15 absolute, a thousandth of the rule's floor for the
    probabilities, which is all the rule asks of it."""
    mpmath.mp.dps = 40
    x = np.concatenate([np.linspace(0.0, 6.0, 121), np.linspace(6.0, 27.0, 85), [27.5, 31.8, 40.0]])
    want = np.array([float(mpmath.erfc(mpmath.mpf(float(v)))) for v in x])
    t, _ = pr.normal_tail_cdf(x * np.sqrt(2.0))          # erfc(|z| / sqrt 2) at z = x sqrt 2: the argument is x to 1 ulp
    arg = np.abs(x * np.sqrt(2.0)) * 0.70710678118654752440
    want_t = np.array([float(mpmath.erfc(mpmath.mpf(float(v)))) for v in arg])
    normal = want_t > 1e-300
    assert np.max(np.abs(t[normal] / want_t[normal] - 1.0)) < 8 * 2.0 ** -52
    assert np.all(t[~normal] <= 1e-300) and t[-1] == 0.0 and t[-2] == 0.0
    sc = special.erfc(x)
    assert np.max(np.abs(sc - want)) < 1e-15


def test_float32_terms_on_the_host_build(catalogue):
    """float32 records and sample rows, float64 after the term: within the per-term float32 tolerance of DESIGN.md
    section 5 (2e-5 of the scale) of the float64 build -- the bound the device test uses."""
    vmax = float(np.max(np.abs(catalogue["v"])))
    for model in (0, 2, 4, 5):
        table = ph.samples(catalogue, model, False, 100)
        mix = model in pr.MIX_MODELS
        a = pr.predictive(catalogue, table, model, ph.CENTRE, mix, f32=True)
        b = pr.predictive(catalogue, table, model, ph.CENTRE, mix)
        for f in b:
            dev = float(np.max(np.abs(a[f] - b[f]) / _merge_scale(b, f, vmax)))
            print(model, f, "%.2e" % dev)
            assert dev < 2e-5, (model, f, dev)


def test_ppc_summary_by_hand():
    pit = np.array([0.01, 0.02, 0.30, 0.55, 0.56, 0.99, 1.0, 0.0])
    s = ppc_summary(pit, n_bins=4)
    assert s["hist"].tolist() == [3.0, 1.0, 2.0, 2.0] and s["n"] == 8.0 and s["n_stars"] == 8
    assert s["chi2"] == pytest.approx((1.0 + 1.0 + 0.0 + 0.0) / 2.0, abs=1e-15)
    assert s["tail_fraction"] == pytest.approx(5.0 / 8.0, abs=1e-15)      # 0.01, 0.02, 0.99, 1.0, 0.0
    w = np.array([1.0, 0.5, 0.25, 1.0, 0.0, 0.25, 0.5, 0.5])
    s = ppc_summary(pit, weights=w, n_bins=4)
    assert s["hist"].tolist() == [2.0, 0.25, 1.0, 0.75] and s["n"] == 4.0
    assert s["chi2"] == pytest.approx(1.0 + 0.5625 + 0.0 + 0.0625, abs=1e-15)
    assert s["tail_fraction"] == pytest.approx(2.75 / 4.0, abs=1e-15)
    # a star without a finite PIT is left out
    s = ppc_summary(np.array([0.1, np.nan, 0.6]), n_bins=2)
    assert s["hist"].tolist() == [1.0, 1.0] and s["n"] == 2.0 and s["n_stars"] == 2 and s["chi2"] == 0.0


def test_ppc_totals_are_summed_over_the_ranks():
    class TwoRanks(object):
        """Stands in for the host group: the other rank holds `other`."""
        def __init__(self, other):
            self.other = other

        def allreduce(self, a):
            return np.asarray(a) + self.other

    rng = np.random.default_rng(4)
    pit, w = rng.uniform(size=50) ** 2, rng.uniform(size=50)
    whole = ppc_summary(pit, w, n_bins=10)
    other = ppc_summary(pit[30:], w[30:], n_bins=10)
    totals = np.concatenate([other["hist"], [other["n"], other["tail_fraction"] * other["n"], 20.0]])
    split = ppc_summary(pit[:30], w[:30], n_bins=10, group=TwoRanks(totals))
    assert np.allclose(split["hist"], whole["hist"], rtol=1e-14, atol=0)
    for key in ("n", "chi2", "tail_fraction"):
        assert split[key] == pytest.approx(whole[key], rel=1e-13)
    assert split["n_stars"] == 50


def calibration_chi2(sigma_factor=1.0):
    """chi2 over 20 PIT bins of the calibration catalogue under its truth vector repeated (host build)."""
    cat, truth = pr.calibration_case()
    row = truth.copy()
    row[1] *= sigma_factor
    got = pr.predictive(cat, np.tile(row, (3, 1)), 0, ph.CENTRE)
    assert np.all(got["z_std"] == 0.0)
    return ppc_summary(got["pit"], n_bins=20)


def test_calibration():
    """Velocities drawn from the model itself: the PIT histogram is flat (chi2 below the 0.999 quantile of chi^2(19));
    with sigma_max halved the model is too narrow and chi2 exceeds ten times that.  (The NumPy restatement gives 12.1 and
    2.0e4 for this seed.)"""
    cat, truth = pr.calibration_case()
    numpy_pit = pr.star_terms(cat, truth, 0, ph.CENTRE)["pit"]
    assert ppc_summary(numpy_pit, n_bins=20)["chi2"] < pr.CHI2_19_Q999
    s = calibration_chi2()
    assert s["n"] == pr.CALIBRATION_N and s["chi2"] < pr.CHI2_19_Q999
    assert abs(s["tail_fraction"] - 0.05) < 0.01
    bad = calibration_chi2(0.5)
    assert bad["chi2"] > 10.0 * pr.CHI2_19_Q999 and bad["tail_fraction"] > 0.2


def test_no_instantiation_uses_scratch(tmp_path):
    """Every predictive_slice_kernel<MODEL, FREE, MIX, T> and both merge kernels, compiled for gfx950: 0 bytes of scratch
    per lane, no spilled VGPR, no LDS, and at most 128 VGPRs (the condition for shipping the device library's erfc,
    DESIGN.md section 3.12)."""
    import os
    import sys
    from conftest import ROOT
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import predictive_resources
    rows = predictive_resources.analyse(str(tmp_path))
    slices = [r for r in rows if r["kernel"] == "slice"]
    assert len(slices) == 2 * (7 * 2 + 2 * 2)            # two precisions x (7 models x 2 centre modes + MIX for two models)
    assert sorted(r["mix"] for r in rows if r["kernel"] == "merge") == [False, True]
    assert len(rows) == len(slices) + 2
    for r in rows:
        assert r["scratch_bytes_per_lane"] == 0, r
        assert r["vgpr_spill"] == 0 and r["lds_bytes"] == 0 and r["agprs"] == 0, r
        assert r["vgprs"] <= 128, r

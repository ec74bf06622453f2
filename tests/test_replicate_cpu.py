"""CPU: the replicated-data predictive checks (csrc/mcd_replicate.h through tests/emul/replicate_emul.cpp): the generator,
the accuracy rule against the NumPy restatement of tests/replicate_helper.py, the invariances of a replicate, the plan and
the validation of the C-ABI, calibration verdicts on synthetic posteriors, replicate_summary, the refusals of the Runner
layer and the compiler's resource report of the kernels."""
import os
import sys

import numpy as np
import pytest

import emul_helper as eh
import posterior_helper as ph
import predictive_helper as pr
import replicate_helper as rh
from mcmc_dynamics_amd import DataReader, _native, synthetic
from mcmc_dynamics_amd.analysis import BinnedConstantFit, ConstantFit
from mcmc_dynamics_amd.analysis.runner import REPLICATE_NAMES, replicate_summary
from mcmc_dynamics_amd.background import Gaussian, SingleStars

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODELS = tuple(range(7))


def numpy_block(counter, key):
    """The four words NumPy's Philox produces for `counter` (four 64-bit words, little end first): NumPy increments the
    counter BEFORE it generates a block, so the generator is started one below."""
    value = (sum(int(x) << (64 * i) for i, x in enumerate(counter)) - 1) % (1 << 256)
    before = [(value >> (64 * i)) & 0xFFFFFFFFFFFFFFFF for i in range(4)]
    return np.random.Philox(counter=np.array(before, dtype=np.uint64), key=np.array(key, dtype=np.uint64)).random_raw(4)


# ------------------------------------------------------------------------------------------ generator
def test_words_match_numpys_philox_for_the_replicate_key():
    key = rh.lib().emul_rep_key()
    assert key == int.from_bytes(b"mcd_rep", "big")
    rng = np.random.default_rng(5)
    for _ in range(100):
        seed, s, i = (int(x) for x in rng.integers(0, 2 ** 62, 3))
        for slot, call in ((0, 0), (0, 3), (1, 0)):
            assert np.array_equal(rh.rep_words(seed, s, i, slot, call), numpy_block([s, i, slot, call], [seed, key]))


def _pairs(seed, s, i, call):
    """The two candidate pairs (u, v, q) of one generator call of the normal, from NumPy's words."""
    w = numpy_block([s, i, 0, call], [seed, rh.lib().emul_rep_key()])
    uni = (w >> np.uint64(11)).astype(np.float64) * (1.0 / 9007199254740992.0)
    x = 2.0 * uni - 1.0
    return [(x[0], x[1], x[0] * x[0] + x[1] * x[1]), (x[2], x[3], x[2] * x[2] + x[3] * x[3])]


def test_normal_of_a_rejected_then_accepted_pair_is_as_written():
    seed, found = 77, 0
    for i in range(400):
        z, used = rh.rep_normal(seed, 3, i)
        (u0, v0, q0), (u1, v1, q1) = _pairs(seed, 3, i, 0)
        if used == 2:
            assert not (0.0 < q0 < 1.0) and 0.0 < q1 < 1.0
            want = u1 * np.sqrt(-2.0 * eh.det_log(np.array([q1]))[0] / q1)
            assert z == want
            found += 1
        elif used == 1:
            assert 0.0 < q0 < 1.0 and z == u0 * np.sqrt(-2.0 * eh.det_log(np.array([q0]))[0] / q0)
    assert found > 20                                             # ~ 17 % of the draws


def test_fallback_after_max_calls():
    seed = 77
    for i in range(2000):
        (_, _, q0), (_, _, q1) = _pairs(seed, 9, i, 0)
        if not (0.0 < q0 < 1.0) and not (0.0 < q1 < 1.0):          # both pairs of call 0 are rejected (4.6 % of the counters)
            assert rh.rep_normal(seed, 9, i, max_calls=1) == (0.0, 2)
            z, used = rh.rep_normal(seed, 9, i)
            assert used >= 3 and z != 0.0
            return
    raise AssertionError("no counter with two rejected pairs among 2000")


def test_moments_of_a_million_draws():
    g, u = rh.numbers(20240917, 0, 1000, 0, 1000)
    n = float(g.size)
    # standard errors of the first four raw moments of N(0, 1): sqrt of 1, 2, 15, 96 over n
    for k, (want, var) in enumerate(((0.0, 1.0), (1.0, 2.0), (0.0, 15.0), (3.0, 96.0)), start=1):
        got = np.mean(g ** k)
        print("moment", k, got)
        assert abs(got - want) <= 5.0 * np.sqrt(var / n)
    assert abs(np.mean(u < 0.3) - 0.3) <= 5.0 * np.sqrt(0.3 * 0.7 / n)
    assert u.min() >= 0.0 and u.max() < 1.0


def test_library_numbers_are_the_emulated_ones():
    """mcd_replicate_numbers (host code of the library) and the harness compile the same header."""
    g, u = _native.replicate_numbers(123456789, 5, 7, 11, 13)
    ge, ue = rh.numbers(123456789, 5, 7, 11, 13)
    assert np.array_equal(g, ge) and np.array_equal(u, ue)
    # a function of (seed, sample, star) alone: any window of the table holds the same numbers
    g2, _ = rh.numbers(123456789, 0, 12, 0, 24)
    assert np.array_equal(g2[5:12, 11:24], ge)


# ------------------------------------------------------------------------------------------ accuracy
@pytest.mark.parametrize("free", [False, True])
@pytest.mark.parametrize("model", MODELS)
def test_emulation_follows_the_rule(model, free):
    """7 models x {fixed, free} x N in {1, 65, 4099} x S in {1, 65, 257} x the three range layouts."""
    rh.check_matrix_cell(model, free, lambda cat, table, centre, offs, order:
                         rh.replicate(cat, table, model, centre, rh.SEED, offs, order))


@pytest.mark.parametrize("free", [False, True])
@pytest.mark.parametrize("model", [7, 8])
def test_double_models_follow_the_rule(model, free):
    """The double Lynden-Bell models with a live second component at the matrix's N = 65, S = 65 cell, the three layouts."""
    cat, table, centre = rh.matrix_case(model, free)
    cat, table = pr.head(cat, 65), table[:65]
    ref = rh.Reference(cat, table, model, centre)
    for kind in rh.LAYOUTS:
        offs, order = rh.layout(kind, 65)
        got = rh.replicate(cat, table, model, centre, rh.SEED, offs, order)
        rh.check_rule(got, *ref.at(offs, order), cell=(model, free, kind))


def test_star_unit_is_the_models_position_angle():
    for model in (0, 3):
        for free in (False, True):
            cat, table, centre = rh.matrix_case(model, free)
            c, s = rh.star_unit(cat, table[0], model, centre)
            t = rh.star_terms(cat, table[0], model, centre, np.zeros(len(c)), np.zeros(len(c)), (0.0, 1.0))
            assert np.max(np.abs(c - t["c"])) < 1e-12 and np.max(np.abs(s - t["s"])) < 1e-12
            assert np.max(np.abs(c * c + s * s - 1.0)) < 1e-14


# ------------------------------------------------------------------------------------------ invariances
def _recombine(got):
    """The ranges of (S, R, 8, 2) fields combined in ascending order, as replicate_summary's "all" row."""
    tot = np.zeros((got.shape[0], 1, 8, 2))
    for r in range(got.shape[1]):
        tot[:, 0, :6] += got[:, r, :6]
        tot[:, 0, 7] += got[:, r, 7]
        tot[:, 0, 6] = np.maximum(tot[:, 0, 6], got[:, r, 6])
    return tot


@pytest.mark.parametrize("model,free", [(0, False), (2, True), (6, False)])
def test_a_replicate_does_not_depend_on_ranges_or_chunks(model, free):
    cat, table, centre = rh.matrix_case(model, free)
    ref = rh.matrix_reference(model, free)
    n = len(cat["v"])
    one, sixteen = rh.layout("one", n), rh.layout("sixteen", n)
    exact, np64, scale = ref.at(*one)
    base = rh.replicate(cat, table, model, centre, rh.SEED, *one)
    combined = _recombine(rh.replicate(cat, table, model, centre, rh.SEED, *sixteen))
    rh.check_rule(combined, exact, np64, scale, cell="16 ranges recombined")
    assert np.array_equal(combined[:, :, 6:], base[:, :, 6:])                  # max and count: exactly
    for forced in (64, 1024):
        assert rh.plan(one[0], table.shape[0], forced)["len"] == forced
        got = rh.replicate(cat, table, model, centre, rh.SEED, *one, forced_len=forced)
        rh.check_rule(got, exact, np64, scale, cell="chunk length {0}".format(forced))
        assert np.array_equal(got[:, :, 6:], base[:, :, 6:])
    # the replicated fields of the shuffled order's first range hold the same stars' replicates whatever precedes them
    offs, order = sixteen
    lone = rh.replicate(cat, table, model, centre, rh.SEED, [0, offs[6] - offs[5]], order[offs[5]:offs[6]])
    assert np.array_equal(lone[:, 0], rh.replicate(cat, table, model, centre, rh.SEED, *sixteen)[:, 5])


def _plain_case(n=300, S=9):
    cat = ph.model_catalog(n, 0, seed=7)
    return pr.clear_of_centres(cat, *ph.CENTRE)


def test_membership_one_is_the_model_without_background():
    cat = _plain_case()
    n = len(cat["v"])
    offs, order = rh.layout("sixteen", n)
    for bg_model, plain in ((1, 0), (6, 3), (2, 0), (4, 3), (5, 3)):
        t_plain = ph.samples(cat, plain, False, 9)
        t_bg = ph.samples(cat, bg_model, False, 9)
        t_bg[:, :t_plain.shape[1]] = t_plain
        c = {k: (x.copy() if isinstance(x, np.ndarray) else x) for k, x in cat.items()}
        if eh.BG_OF[bg_model] == 1:
            c["pmember"] = np.ones(n)
        else:
            t_bg[:, -1] = 0.0                                                  # f_back = 0: m = rho / (rho + 0) = 1
        want = rh.replicate(c, t_plain, plain, ph.CENTRE, 99, offs, order)
        got = rh.replicate(c, t_bg, bg_model, ph.CENTRE, 99, offs, order)
        assert np.array_equal(got, want), bg_model


def test_membership_zero_is_pure_background():
    cat = _plain_case()
    cat["pmember"] = np.zeros(len(cat["v"]))
    table = ph.samples(cat, 1, False, 9)
    ref = rh.Reference(cat, table, 1, ph.CENTRE, seed=99)
    assert np.all(ref.exact["m"] == 0)
    offs, order = rh.layout("three", len(cat["v"]))
    got = rh.replicate(cat, table, 1, ph.CENTRE, 99, offs, order)
    rh.check_rule(got, *ref.at(offs, order), cell="m = 0")
    # the background's residuals against the cluster component are far wider than a standard normal's
    assert np.all(got[:, 2, 1, 1] > 3.0 * got[:, 2, 1, 0])


def test_a_repeated_row_gives_equal_observed_fields():
    cat, table, centre = rh.matrix_case(4, True)
    rows = np.repeat(table[3:4], 5, axis=0)
    offs, order = rh.layout("sixteen", 65)
    got = rh.replicate(pr.head(cat, 65), rows, 4, centre, rh.SEED, offs, order)
    assert all(np.array_equal(got[s, ..., 0], got[0, ..., 0]) for s in range(5))
    assert not np.array_equal(got[1, ..., 1], got[0, ..., 1])                 # the replicates differ from row to row
    # ... and the generator's row index follows row0
    assert np.array_equal(rh.replicate(pr.head(cat, 65), rows[:2], 4, centre, rh.SEED, offs, order, row0=3), got[3:5])


def test_a_non_finite_term_stays_in_its_range_and_row():
    cat = _plain_case(80)
    cat["verr"][7] = 0.0
    table = ph.samples(cat, 0, False, 4)
    table[2, 1] = 0.0                                                          # sigma_max = 0 in row 2: n = 0 for star 7
    offs, order = np.array([0, 40, 80]), np.arange(80)
    got = rh.replicate(cat, table, 0, ph.CENTRE, 5, offs, order)
    assert not np.isfinite(got[2, 0, :, 0]).any()                              # all eight observed fields of (row 2, range 0)
    assert np.isfinite(got[2, 0, :, 1]).all()                                  # its replicates are standard normals
    keep = np.ones(got.shape[:2], bool)
    keep[2, 0] = False
    assert np.isfinite(got[keep]).all()


# ------------------------------------------------------------------------------------------ plan and validation
def test_plan_keeps_the_budget_and_fills_the_device():
    budget = rh.lib().emul_rep_scratch_bytes()
    assert budget == 256 << 20 and rh.lib().emul_rep_max_rows() == 65536
    for n, R, S in ((1000000, 8, 1024), (100000, 1, 4096), (65, 1, 65537), (1000000, 8, 70000), (4099, 16, 257)):
        offs = (np.arange(R + 1, dtype=np.int64) * n) // R
        p = rh.plan(offs, S)
        assert p["pass_rows"] == min(S, 65536)
        assert p["n_chunks"] * p["pass_rows"] * 128 <= budget, (n, R, S, p["n_chunks"])
        assert np.array_equal(np.sort(p["begin"]), p["begin"]) and p["count"].sum() == n
        ends = p["begin"] + p["count"]
        assert all(np.searchsorted(offs, b, side="right") - 1 == r and e <= offs[r + 1]
                   for b, e, r in zip(p["begin"], ends, p["range"]))           # no chunk straddles a range
        if n >= 100000:
            assert p["n_chunks"] * ((p["pass_rows"] + 63) // 64) >= 4 * 1024    # several waves on each of the 1024 SIMDs
    # so many ranges that a 65536-row pass cannot hold one chunk of each: shorter passes
    offs = np.arange(5001, dtype=np.int64) * 3
    p = rh.plan(offs, 65536)
    assert p["pass_rows"] < 65536 and p["pass_rows"] % 64 == 0 and p["n_chunks"] * p["pass_rows"] * 128 <= budget
    # an empty range has no chunk, a singleton a one-star chunk
    p = rh.plan([0, 0, 1, 900], 65)
    assert p["range"].tolist().count(0) == 0 and p["count"][p["range"] == 1].tolist() == [1]


def test_validation_of_ranges_order_and_background():
    nan = float("nan")
    assert rh.validate(0, [0, 2, 2, 5], [4, 0, 1, 3, 2], 5) is None
    assert rh.validate(0, [0, 0], [], 5) is None
    assert "non-decreasing" in rh.validate(0, [0, 3, 2], [0, 1, 2], 5)
    assert "must be 0" in rh.validate(0, [1, 3], [0, 1, 2], 5)
    assert "exceeds" in rh.validate(0, [0, 6], [0, 1, 2, 3, 4, 4], 5)
    assert "outside" in rh.validate(0, [0, 2], [0, 5], 5)
    assert "outside" in rh.validate(0, [0, 2], [-1, 1], 5)
    assert "twice" in rh.validate(0, [0, 1, 3], [2, 4, 2], 5)
    for model in (1, 5, 6):
        assert rh.validate(model, [0, 1], [0], 5, (20.0, 0.0)) is None
        for bad in ((nan, 1.0), (1.0, nan), (1.0, -1.0), (np.inf, 1.0), (1.0, np.inf)):
            assert "fixed-background" in rh.validate(model, [0, 1], [0], 5, bad)
    for model in (0, 2, 3, 4):
        assert rh.validate(model, [0, 1], [0], 5, (nan, nan)) is None


# ------------------------------------------------------------------------------------------ calibration
# data seeds, fixed after checking that the float64 restatement alone satisfies each line (of the seeds 101 .. 106 the
# model-drawn case has every p-value of "all" inside [0.01, 0.99] with 102, 103, 104 and 106; the other three cases gave
# 0 or 1 where the line asks for < 0.01 or > 0.5 with every seed tried)
CAL_SEEDS = {"model": 106, "outer": 102, "rotation": 103, "tails": 104}


def _calibration(kind):
    """replicate_summary of the emulation and of the float64 restatement alone for one calibration case."""
    cat, table, offs, order = rh.calibration_case(kind, CAL_SEEDS[kind])
    got = rh.replicate(cat, table, 0, ph.CENTRE, 31, offs, order)
    g, u = rh.numbers(31, 0, table.shape[0], 0, len(cat["v"]))
    restated, _ = rh.fields_of(rh.sample_terms(cat, table, 0, ph.CENTRE, g, u, (np.nan, np.nan), np.float64), offs, order)
    counts = np.diff(offs)
    return replicate_summary(got, counts), replicate_summary(restated, counts)


def _p(summary, row, name):
    return summary["p_value"][row, REPLICATE_NAMES.index(name)]


def test_calibration_data_drawn_from_the_model():
    for s in _calibration("model"):
        print(dict(zip(REPLICATE_NAMES, s["p_value"][0])))
        assert np.all(s["p_value"][0] >= 0.01) and np.all(s["p_value"][0] <= 0.99)


def test_calibration_dispersion_doubled_in_the_outer_half():
    for s in _calibration("outer"):
        print(s["p_value"][:, 1])
        assert _p(s, rh.CAL_ANNULI, "var_ratio") < 0.01 and _p(s, 1, "var_ratio") > 0.5


def test_calibration_rotation_the_rows_do_not_have():
    for s in _calibration("rotation"):
        assert _p(s, 0, "rot_amp") < 0.01


def test_calibration_heavy_tails():
    for s in _calibration("tails"):
        assert _p(s, 0, "kurt_excess") < 0.01 and _p(s, 0, "max_abs_z") < 0.01


# ------------------------------------------------------------------------------------------ summary and refusals
def test_replicate_summary_on_hand_made_fields():
    # two ranges of 4 and 2 stars, two samples; observed z = (1, -1, 2, -2 | 3.5, 0.5) in both samples
    z = [np.array([1.0, -1.0, 2.0, -2.0]), np.array([3.5, 0.5])]
    c = [np.array([1.0, 0.0, -1.0, 0.0]), np.array([0.6, -0.8])]
    s = [np.array([0.0, 1.0, 0.0, -1.0]), np.array([0.8, 0.6])]

    def fields(zz, k):
        return [zz.sum(), (zz ** 2).sum(), (zz ** 3).sum(), (zz ** 4).sum(), (zz * s[k]).sum(), (zz * c[k]).sum(),
                np.abs(zz).max(), float((np.abs(zz) > 3).sum())]
    out = np.zeros((2, 2, 8, 2))
    for k in range(2):
        out[:, k, :, 0] = fields(z[k], k)
        out[0, k, :, 1] = fields(0.5 * z[k], k)                     # sample 0: the replicate is narrower
        out[1, k, :, 1] = fields(2.0 * z[k], k)                     # sample 1: wider
    res = replicate_summary(out, [4, 2])
    assert res["names"] == REPLICATE_NAMES and res["n_stars"].tolist() == [6, 4, 2]
    assert res["obs"].shape == (2, 3, 7) and res["bands"].shape == (3, 7, 2, 3)
    za = np.concatenate(z)
    m = za.mean()
    want_all = [m, (za ** 2).mean(), ((za - m) ** 3).mean() / za.var() ** 1.5, ((za - m) ** 4).mean() / za.var() ** 2 - 3.0,
                2.0 * np.hypot((za * np.concatenate(s)).sum(), (za * np.concatenate(c)).sum()) / 6.0, 3.5, 1.0]
    assert np.allclose(res["obs"][0, 0], want_all, rtol=1e-13, atol=1e-15)
    assert np.allclose(res["obs"][1, 1], [0.0, 2.5, 0.0, (2 * 1 + 2 * 16) / 4 / 2.5 ** 2 - 3.0, 2.0 * np.hypot(1.0, 1.0) / 4, 2.0, 0.0],
                       rtol=1e-13, atol=1e-15)
    vi = REPLICATE_NAMES.index("var_ratio")
    assert np.allclose(res["rep"][:, 0, vi], [0.25 * want_all[1], 4.0 * want_all[1]])
    assert res["p_value"][:, vi].tolist() == [0.5, 0.5, 0.5] and res["extreme"][:, vi].tolist() == [0.5, 0.5, 0.5]
    ti = REPLICATE_NAMES.index("n_tail3")
    assert res["p_value"][:, ti].tolist() == [0.5, 1.0, 0.5]         # range 0 has no |z| > 3 either way: 0 >= 0 in both
    assert np.allclose(res["bands"][0, vi, 0], want_all[1]) and np.allclose(
        res["bands"][0, vi, 1], np.percentile([0.25 * want_all[1], 4.0 * want_all[1]], [16, 50, 84]))
    # an empty range: NaN throughout, and it does not touch "all"
    out3 = np.concatenate([out, np.zeros((2, 1, 8, 2))], axis=1)
    res3 = replicate_summary(out3, [4, 2, 0])
    assert np.isnan(res3["p_value"][3]).all() and np.array_equal(res3["p_value"][:3], res["p_value"])
    with pytest.raises(ValueError):
        replicate_summary(out, [4, 2, 1])


class _Ranks(object):
    n_ranks, n_devices = 2, 1


def _fit(n=60, **kwargs):
    c = synthetic.make_catalog(n, config=2, background=True)
    cols = ("ra", "dec", "v", "verr") + (("pmember",) if "background" in kwargs else ())
    return ConstantFit(DataReader({k: c[k] for k in cols}), **kwargs)


def test_refusals_of_the_runner_layer():
    chain = np.zeros((4, 6, 4))
    with pytest.raises(NotImplementedError, match="2 ranks"):
        _fit(context=_Ranks()).replicate_check(chain, 1)
    with pytest.raises(NotImplementedError, match="float64"):
        _fit(precision="f32").replicate_check(chain, 1)
    fit = _fit(background=Gaussian(20.0, 40.0))
    assert fit._replicate_background() == (20.0, 40.0)
    fit.background = SingleStars(np.array([1.0, 2.0, 3.0]))
    with pytest.raises(NotImplementedError, match="SingleStars"):
        fit.replicate_check(chain, 1)
    c = synthetic.make_catalog(120, config=2, background=False)
    data = DataReader({k: c[k] for k in ("ra", "dec", "v", "verr")})
    data.make_radial_bins(synthetic.CENTER_RA_DEG, synthetic.CENTER_DEC_DEG, nstars=40)
    with pytest.raises(NotImplementedError, match="un-binned"):
        BinnedConstantFit(data).replicate_check(chain, 1)


def test_groups_of_the_runner_layer():
    fit = _fit(61)
    fit.parameters["ra_center"].set(value=synthetic.CENTER_RA_DEG, fixed=True)
    fit.parameters["dec_center"].set(value=synthetic.CENTER_DEC_DEG, fixed=True)
    offs, order, (key, edges) = fit._replicate_groups(4, None)
    assert key == "edges" and edges.shape == (5,) and np.all(np.diff(edges) > 0)
    assert offs.tolist() == [0, 16, 31, 46, 61] and sorted(order.tolist()) == list(range(61))
    dx, dy = rh.oracle.calc_xy_offset(fit.ra, fit.dec, synthetic.CENTER_RA_DEG, synthetic.CENTER_DEC_DEG)
    r = np.hypot(dx, dy)
    for g in range(4):
        mine = r[order[offs[g]:offs[g + 1]]]
        assert mine.min() >= edges[g] and mine.max() <= edges[g + 1]
    offs2, order2, (key2, _) = fit._replicate_groups(edges[1:4], None)                # explicit edges in arcmin
    assert key2 == "edges" and offs2.tolist() == [0, 15, 30] and set(order2) == set(order[16:46])
    labels = np.full(61, -1)
    labels[[5, 9]] = 2
    labels[7] = 0
    offs3, order3, (key3, names) = fit._replicate_groups(8, labels)
    assert key3 == "groups" and names.tolist() == [0, 1, 2] and offs3.tolist() == [0, 1, 1, 3] and order3.tolist() == [7, 5, 9]
    with pytest.raises(ValueError):
        fit._replicate_groups(8, np.zeros(61))                                       # not an int array


def test_kernels_use_no_scratch():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import replicate_resources
    rows = replicate_resources.analyse()
    assert sum(r["kernel"] == "replicate" for r in rows) == 14 and sum(r["kernel"] == "reduce" for r in rows) == 1
    for r in rows:
        assert r["scratch_bytes_per_lane"] == 0 and r["vgpr_spill"] == 0 and r["sgpr_spill"] == 0, r
        assert r["lds_bytes"] == 0, r

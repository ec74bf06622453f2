"""GPU: mcd_psis_loo_expect -- leave-one-out expectations under the PSIS weights on the device (LOO-PIT, case-deletion
means) -- against the NumPy oracle of tests/loo_expect_helper.py fed with the lnL rows of Catalog.loglike_per_star and the
terms of predictive_helper.sample_terms, by the helper's accuracy rule; its bits, refusals and float32 catalogues; and
through Runner.loo_pit / Runner.loo_influence."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import loo_expect_helper as lh
import posterior_helper as ph
import predictive_helper as pr
import psis_helper as psh
from conftest import ROOT
from test_gpu_psis import CAP_R_EFF, CAP_S, _lnl_matrix, cap_case

pytestmark = pytest.mark.gpu
MODELS = [0, 1, 2, 3, 4, 5, 6]
# (65, 257): one full wave plus one lane, 16-sample chunks with a remainder of 1, five sample slices, M = 49;
# (2000, 256): the catalogue and samples of test_gpu_psis.py
SHAPES = [(65, 257), (2000, 256)]


@pytest.fixture(scope="module")
def ctx():
    from mcmc_dynamics_amd import _native
    return _native.default_context()


@pytest.fixture(scope="module")
def cat2k():
    return ph.model_catalog(2000, 0, seed=17)


def _device_terms(gpu, table, keys):
    """(n, R, S) rows of the device's own (star, sample) terms, one mcd_posterior_predictive call per sample -- the per-row
    entry the library already had, as loglike_per_star is for lnL (over one sample its means are the sample's terms)."""
    name = {"pit": "pit", "z": "z_mean", "vlos": "vlos_mean", "sigma": "sigma_mean", "pit_mix": "pit_mix"}
    per = [gpu.posterior_predictive(row, mixture="pit_mix" in keys) for row in table]
    return np.ascontiguousarray(np.stack([np.array([o[name[k]] for o in per]).T for k in keys], axis=1))


def _clear_of_centres(cat, table, model, centre, limit=0.8):
    """Stars at least `limit` arcmin from every centre of the samples: predictive_helper.clear_of_centres' limit, inside
    which theta = arctan2(dy, dx) is ill-conditioned in the reference's own float64 formula (up to 3.3e-16 / r rad), so
    that NumPy's v_los and z are not known to the rule's 1e-11 of their spread over the samples."""
    from oracle import lnprob_numpy as oracle
    ra_c, dec_c = pr.sample_centres(table, model) if centre is None else centre
    ra_c, dec_c = np.atleast_1d(np.asarray(ra_c, dtype=np.float64)), np.atleast_1d(np.asarray(dec_c, dtype=np.float64))
    dx, dy = oracle.calc_xy_offset(cat["ra"][:, None], cat["dec"][:, None], ra_c[None, :], dec_c[None, :])
    return np.hypot(dx, dy).min(axis=1) >= limit


def _check_device(gpu, cat, table, model, centre, got, what):
    """The device's rows by the rule against the oracle fed with loglike_per_star's lnL rows and (a) the terms of
    predictive_helper.sample_terms, for the stars clear of the centres, (b) the device's own per-sample terms, for every
    star: (b) holds the weights and the sums to the rule where NumPy's own terms are not good enough to.  Returns the
    oracle's result of (a) and the lnL rows."""
    mix = "pit_mix" in got
    lnl = _lnl_matrix(gpu, cat, table, model, centre)
    x, keys = lh.term_rows(cat, table, model, centre, mix=mix)
    rows = np.stack([got[k] for k in keys], axis=1)
    unit = tuple(i for i, k in enumerate(keys) if k in ("pit", "pit_mix"))
    clear = _clear_of_centres(cat, table, model, centre)
    print(what, "stars clear of the centres:", int(clear.sum()), "of", clear.size)
    want = lh.check_expect({"rows": rows[clear], "pareto_k": got["pareto_k"][clear]}, lnl[clear], x[clear], unit_rows=unit,
                           what=what + " (NumPy terms)")
    lh.check_expect({"rows": rows, "pareto_k": got["pareto_k"]}, lnl, _device_terms(gpu, table, keys), unit_rows=unit,
                    what=what + " (device terms)")
    return want, lnl


@pytest.mark.parametrize("n,S", SHAPES)
@pytest.mark.parametrize("model", MODELS)
@pytest.mark.parametrize("free", [False, True])
def test_device_expectations_follow_the_rule(ctx, cat2k, model, free, n, S):
    centre = None if free else ph.CENTRE
    cat = pr.head(cat2k, n)
    table = ph.samples(cat2k, model, free, S)
    gpu = pr.device_catalog(ctx, cat, model, centre)
    mix = model in pr.MIX_MODELS
    got = gpu.psis_loo_expect(table, mixture=mix)
    _check_device(gpu, cat, table, model, centre, got, "model {0} free {1} ({2}, {3})".format(model, free, n, S))
    ref = gpu.psis_loo(table)
    assert np.array_equal(got["pareto_k"], ref["pareto_k"]) and np.array_equal(got["n_eff"], ref["n_eff"])
    gpu.close()


@pytest.mark.parametrize("S", [1, 20, 24])
def test_short_chains(ctx, cat2k, S):
    """S = 20: M = 4, no tail; S = 24: M = 5, the shortest tail; S = 1: w~ = 1.  For S = 1 the rule's scale (the spread of
    x over the samples) is zero, so the device is held to its own single-sample terms, mcd_posterior_predictive's means
    over one sample, bit for bit (the NumPy terms differ from the device's in the last bits); pit by the rule as well."""
    model, centre = 2, ph.CENTRE
    cat = pr.head(cat2k, 65)
    table = ph.samples(cat2k, model, False, 257)[:S]
    gpu = pr.device_catalog(ctx, cat, model, centre)
    func = np.linspace(-1.0, 1.0, 3 * S).reshape(S, 3)
    got = gpu.psis_loo_expect(table, func=func, mixture=True)
    if S == 1:
        own = gpu.posterior_predictive(table, mixture=True)
        for key, ref in (("pit", "pit"), ("z", "z_mean"), ("vlos", "vlos_mean"), ("sigma", "sigma_mean"),
                         ("pit_mix", "pit_mix")):
            assert np.array_equal(got[key], own[ref]), key
        assert np.array_equal(got["func"], np.tile(func[0], (65, 1)))
        assert np.all(got["n_eff"] == 1.0) and np.all(got["pareto_k"] == np.inf)
        lnl = _lnl_matrix(gpu, cat, table, model, centre)
        x, keys = lh.term_rows(cat, table, model, centre, mix=True)
        for i in (0, 4):
            lh.rule_ok(got[keys[i]], lh.oracle_expect(lnl, x)["rows"][:, i], 1.0, 0.0, keys[i] + " S=1")
    else:
        _, lnl = _check_device(gpu, cat, table, model, centre, got, "S={0}".format(S))
        lh.check_expect({"func": got["func"], "pareto_k": got["pareto_k"]}, lnl, None, func, what="S={0}".format(S))
        assert np.all(np.isinf(got["pareto_k"])) == (S == 20)
    gpu.close()


def test_bits_repeat_and_do_not_depend_on_tiles(ctx, cat2k):
    table = ph.samples(cat2k, 2, False, 512, seed=4)
    gpu = pr.device_catalog(ctx, cat2k, 2, ph.CENTRE)
    cols = table[:, :5]
    std = cols.std(axis=0)
    func = np.concatenate([(cols - cols.mean(axis=0)) / std, np.zeros((512, 1))], axis=1)   # a standardised constant: zeros
    a = gpu.psis_loo_expect(table, r_eff=0.7, func=func, mixture=True)
    b = gpu.psis_loo_expect(table, r_eff=0.7, func=func, mixture=True)
    gpu.set_option("loo_scratch_mb", 1)                  # 1 MiB: tiles of fewer than 64 stars of 6 rows
    c = gpu.psis_loo_expect(table, r_eff=0.7, func=func, mixture=True)
    gpu.set_option("loo_scratch_mb", 2048)
    for k in a:
        assert np.array_equal(a[k], b[k]) and np.array_equal(a[k], c[k]), k
    assert np.all(a["func"][:, 5] == 0.0)
    ref = gpu.psis_loo(table, r_eff=0.7)
    assert np.array_equal(a["pareto_k"], ref["pareto_k"]) and np.array_equal(a["n_eff"], ref["n_eff"])
    # what is asked for does not change what comes back
    only = gpu.psis_loo_expect(table, r_eff=0.7, func=func, predictive=False)
    assert np.array_equal(only["func"], a["func"]) and np.array_equal(only["n_eff"], a["n_eff"])
    pred = gpu.psis_loo_expect(table, r_eff=0.7)
    for k in ("pit", "z", "vlos", "sigma", "pareto_k"):
        assert np.array_equal(pred[k], a[k]), k
    gpu.set_option("posterior_pass", 100)                # six upload passes
    d = gpu.psis_loo_expect(table, r_eff=0.7, func=func, mixture=True)
    for k in a:
        assert np.array_equal(a[k], d[k]), k
    gpu.set_option("timing", 1)
    gpu.psis_loo_expect(table, r_eff=0.7)
    assert gpu.last_kernel_ms > 0.0
    gpu.close()


def test_heavy_tails_and_ties(ctx, cat2k):
    """The catalogue of test_gpu_psis.test_heavy_tails_and_ties: repeated rows (ties at the cutoff) and stars far out in
    velocity (k^ > 0.7)."""
    cat = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in cat2k.items()}
    cat["v"][:40] += 60.0
    table = ph.samples(cat, 0, False, 400, seed=8)
    reps = np.repeat(np.arange(400), np.random.default_rng(2).integers(1, 6, size=400))[:400]
    table = np.ascontiguousarray(table[reps])
    gpu = pr.device_catalog(ctx, cat, 0, ph.CENTRE)
    func = (table - table.mean(axis=0)) / table.std(axis=0)
    got = gpu.psis_loo_expect(table, func=func)
    _, lnl = _check_device(gpu, cat, table, 0, ph.CENTRE, got, "heavy")
    lh.check_expect({"func": got["func"], "pareto_k": got["pareto_k"]}, lnl, None, func, what="heavy")
    assert np.count_nonzero(got["pareto_k"] > 0.7) >= 5
    gpu.close()


def near_tie_table(cat, S, seed):
    """Runs of repeated rows (rejected moves) interleaved with rows whose v_sys differs from the run's by 1 to 32 ulps (one
    ulp of v_sys moves lnL by well under one of its own, so fewer would only make more exact ties): every star's lnL row has
    exact ties, and most have entries a few ulps apart, at the cutoff as anywhere else."""
    rng = np.random.default_rng(seed)
    base = ph.samples(cat, 2, False, S, seed=seed)
    table = np.ascontiguousarray(base[np.repeat(np.arange(S), rng.integers(1, 6, size=S))[:S]])
    col = ph.abi_names(2, False).index("v_sys")
    odd = np.arange(S) % 2 == 1
    table[odd, col] += rng.integers(1, 33, size=int(odd.sum())) * rng.choice([-1.0, 1.0], size=int(odd.sum())) * \
        np.spacing(table[odd, col])
    return table


@pytest.mark.parametrize("S", [63, 65, 400])
def test_ties_and_near_ties_reach_the_second_copy_of_the_selection(ctx, cat2k, S):
    """loox_tail_kernel carries its own copy of psis_row's select, scan, gather and rank sort: on rows with ties and
    near-ties its k^ and n_eff are mcd_psis_loo's bit for bit, and the expectation of the sample index under its weights --
    which sees who is in the tail and at which rank -- follows the rule."""
    cat = pr.head(cat2k, 65)
    table = near_tie_table(cat2k, S, seed=31 + S)
    gpu = pr.device_catalog(ctx, cat, 2, ph.CENTRE)
    index = np.arange(S, dtype=np.float64)[:, None]
    got = gpu.psis_loo_expect(table, func=index, predictive=False)
    ref = gpu.psis_loo(table)
    assert np.array_equal(got["pareto_k"], ref["pareto_k"]) and np.array_equal(got["n_eff"], ref["n_eff"])
    lnl = _lnl_matrix(gpu, cat, table, 2, ph.CENTRE)
    gaps = [np.diff(np.sort(row)) / np.spacing(np.abs(row).max()) for row in lnl]
    ties = np.array([np.count_nonzero(g == 0.0) for g in gaps])
    near = np.array([np.count_nonzero((g > 0.0) & (g <= 8.0)) for g in gaps])
    print("S", S, "neighbours per star that are equal:", ties.min(), "..", ties.max(), "; 1 to 8 ulps apart:", near.min(),
          "..", near.max(), "in", int(np.count_nonzero(near)), "stars")
    assert np.all(ties >= S // 8) and np.count_nonzero(near) >= 8
    lh.check_expect({"func": got["func"], "pareto_k": got["pareto_k"]}, lnl, None, index, what="near ties S={0}".format(S))
    gpu.close()


def test_the_largest_tail_is_accepted_and_the_next_refused(ctx, cat2k):
    """S = 12 800 with r_eff = 0.0175: M = kPsisMaxTail = 2 560, the largest dynamic LDS of loox_tail_kernel."""
    cat, table, lnl = cap_case(ctx, cat2k)
    gpu = pr.device_catalog(ctx, cat, 2, ph.CENTRE)
    func = np.ascontiguousarray((table - table.mean(axis=0)) / table.std(axis=0))
    got = gpu.psis_loo_expect(table, r_eff=CAP_R_EFF, func=func, predictive=False)
    ref = gpu.psis_loo(table, r_eff=CAP_R_EFF)
    assert np.array_equal(got["pareto_k"], ref["pareto_k"]) and np.array_equal(got["n_eff"], ref["n_eff"])
    want = lh.check_expect({"func": got["func"], "pareto_k": got["pareto_k"]}, lnl, None, func, r_eff=CAP_R_EFF, what="cap")
    k_tol = np.maximum(1e-10, 10.0 * psh.k_noise(lnl, CAP_R_EFF))
    fin = np.isfinite(want["pareto_k"])
    assert np.all(np.abs(got["pareto_k"][fin] - want["pareto_k"][fin]) <= k_tol[fin])
    assert np.all(np.abs(got["n_eff"] - want["n_eff"]) <= 1e-9 * want["n_eff"])
    more = np.ascontiguousarray(ph.samples(cat2k, 2, False, 12805, seed=23))
    dp = ctypes.POINTER(ctypes.c_double)
    outs = [np.full(70, -7.0), np.full(70, -7.0), np.full(4 * 70, -7.0)]
    pk, ne, lp = (o.ctypes.data_as(dp) for o in outs)
    rc = gpu.lib.mcd_psis_loo_expect(gpu.handle, 12805, more.shape[1], more.ctypes.data_as(dp), CAP_R_EFF, 0, None, None, lp,
                                     None, pk, ne)
    assert rc == -1 and b"S / r_eff too large" in gpu.lib.mcd_last_error()
    for o in outs:
        assert np.all(o == -7.0)
    gpu.close()


@pytest.mark.parametrize("model,precision", [(0, "f32acc64"), (2, "f32")])
def test_float32_catalogue(ctx, cat2k, model, precision):
    table = ph.samples(cat2k, model, False, 256)
    mix = model in pr.MIX_MODELS
    g32 = pr.device_catalog(ctx, cat2k, model, ph.CENTRE, precision)
    g64 = pr.device_catalog(ctx, cat2k, model, ph.CENTRE)
    a, b = g32.psis_loo_expect(table, mixture=mix), g64.psis_loo_expect(table, mixture=mix)
    for k in ("pit",) + (("pit_mix",) if mix else ()):
        err = float(np.max(np.abs(a[k] - b[k])))
        print(k, precision, err)
        assert err < 2e-5
    g32.close()
    g64.close()


def test_refusals(ctx, cat2k):
    from mcmc_dynamics_amd import _native
    small = {k: (v[:200] if isinstance(v, np.ndarray) else v) for k, v in cat2k.items()}
    const = pr.device_catalog(ctx, small, 0, ph.CENTRE)
    lib = const.lib
    dp = ctypes.POINTER(ctypes.c_double)
    row = np.ascontiguousarray(ph.samples(small, 0, False, 30))
    rowp = row.ctypes.data_as(dp)
    func = np.ascontiguousarray(np.random.default_rng(1).normal(size=(30, 17)))
    fp = func.ctypes.data_as(dp)
    outs = [np.full(17 * 200, -7.0), np.full(4 * 200, -7.0), np.full(200, -7.0), np.full(200, -7.0), np.full(200, -7.0)]
    lf, lp, lm, pk, ne = (o.ctypes.data_as(dp) for o in outs)

    def refused(rc, word=None):
        assert rc == -1
        if word:
            assert word in lib.mcd_last_error(), lib.mcd_last_error()
        for o in outs:
            assert np.all(o == -7.0)
    call = lib.mcd_psis_loo_expect
    refused(call(const.handle, 30, 4, rowp, 0.0, 0, None, None, lp, None, pk, ne), b"r_eff")
    refused(call(const.handle, 30, 4, rowp, float("inf"), 0, None, None, lp, None, pk, ne), b"r_eff")
    refused(call(const.handle, 0, 4, rowp, 1.0, 0, None, None, lp, None, pk, ne), b"n_samples")
    refused(call(const.handle, 30, 5, rowp, 1.0, 0, None, None, lp, None, pk, ne), b"columns")
    refused(call(const.handle, 30, 4, rowp, 1.0, 17, fp, lf, lp, None, pk, ne), b"n_func")
    refused(call(const.handle, 30, 4, rowp, 1.0, -1, fp, lf, lp, None, pk, ne), b"n_func")
    refused(call(const.handle, 30, 4, rowp, 1.0, 3, None, lf, lp, None, pk, ne), b"func")
    refused(call(const.handle, 30, 4, rowp, 1.0, 3, fp, None, lp, None, pk, ne), b"loo_func")
    refused(call(const.handle, 30, 4, rowp, 1.0, 0, None, None, lp, lm, pk, ne), b"Gaussian background")
    binned = _native.Catalog(ctx, small["ra"], small["dec"], small["v"], small["verr"], centre=ph.CENTRE,
                             bin_offsets=[0, 80, 200])
    refused(call(binned.handle, 30, 4, rowp, 1.0, 0, None, None, lp, None, pk, ne), b"un-binned")
    # the tail rule of mcd_psis_loo: M = min(ceil(0.2 S), ceil(3 sqrt(S / r_eff))) = 6000 > 2560
    big = np.ascontiguousarray(ph.samples(small, 0, False, 30000))
    refused(call(const.handle, 30000, 4, big.ctypes.data_as(dp), 1e-3, 0, None, None, lp, None, pk, ne), b"Pareto tail")
    const.set_option("loo_scratch_mb", 1)
    refused(call(const.handle, 30000, 4, big.ctypes.data_as(dp), 1.0, 0, None, None, lp, None, pk, ne), b"loo_scratch_mb")
    const.set_option("loo_scratch_mb", 2048)
    # all outputs NULL: MCD_OK without work
    assert call(const.handle, 30, 4, rowp, 1.0, 0, None, None, None, None, None, None) == 0
    for o in outs:
        assert np.all(o == -7.0)
    assert call(const.handle, 30, 4, rowp, 1.0, 16, fp, lf, lp, None, pk, ne) == 0      # (the first 480 values as [30][16])
    assert np.all(np.isfinite(outs[1])) and np.all(outs[2] == -7.0)
    assert lib.mcd_abi_version() == 1
    const.close()
    binned.close()


def test_a_star_with_non_finite_terms_touches_no_other(ctx, cat2k):
    cat = pr.head(cat2k, 130)
    cat["verr"][70] = 0.0
    table = ph.samples(cat2k, 0, False, 64)
    table[:, 1] = 0.0                                    # sigma_max = 0: star 70 has n = 0
    bad = pr.device_catalog(ctx, cat, 0, ph.CENTRE)
    got = bad.psis_loo_expect(table)
    assert not np.isfinite(got["pit"][70]) and not np.isfinite(got["z"][70])
    keep = np.arange(130) != 70
    assert np.all(np.isfinite(got["pit"][keep])) and np.all(np.isfinite(got["z"][keep]))
    bad.close()


def _fit(cls, cat, columns):
    from mcmc_dynamics_amd import DataReader
    fit = cls(DataReader({k: cat[k] for k in columns}))
    fit.parameters["ra_center"].set(value=ph.CENTRE[0], fixed=True)
    fit.parameters["dec_center"].set(value=ph.CENTRE[1], fixed=True)
    return fit


def test_runner_loo_pit_on_the_calibration_catalogue():
    """A chain of one repeated vector: every weight is 1 / S, so the LOO-PIT is ppc()'s posterior PIT."""
    from mcmc_dynamics_amd.analysis import ConstantFit
    cat, truth = pr.calibration_case()
    fit = _fit(ConstantFit, cat, ("ra", "dec", "v", "verr"))
    names = ph.abi_names(0, False)
    vec = np.array([truth[names.index(n)] for n in fit.fitted_parameters])
    chain = np.tile(vec, (4, 3, 1))
    out, want = fit.loo_pit(chain, n_burn=1), fit.ppc(chain, n_burn=1)
    assert np.all(np.abs(out["loo_pit"] - want["pit"]) <= 1e-13)
    assert abs(out["chi2"] - want["chi2"]) <= 1e-9 * want["chi2"]
    assert out["n_stars"] == pr.CALIBRATION_N and out["n_samples"] == 8 and out["hist"].size == 20
    # eight samples: M = 2, a tail too short to fit -- k^ = +inf counts as unreliable, as in loo()
    assert np.all(out["weight"] == 1.0) and np.all(out["pareto_k"] == np.inf) and out["n_bad_k"] == pr.CALIBRATION_N
    for k, ref in (("z", "z_mean"), ("vlos", "vlos_mean"), ("sigma", "sigma_mean")):
        assert np.all(np.abs(out[k] - want[ref]) <= 1e-13 * np.maximum(1.0, np.abs(want[ref]))), k
    fit.close()


def test_runner_loo_influence_finds_the_planted_star():
    from mcmc_dynamics_amd.analysis import ConstantFit
    cat, table, lnl, z, mean, std = lh.planted_case()
    fit = _fit(ConstantFit, cat, ("ra", "dec", "v", "verr"))
    names = ph.abi_names(0, False)
    keep = [names.index(n) for n in fit.fitted_parameters]
    chain = table[:, keep].reshape(1, table.shape[0], len(keep))
    out = fit.loo_influence(chain, n_burn=0)
    assert out["names"] == list(fit.fitted_parameters) and out["n_samples"] == 1024
    shift = np.empty_like(out["shift"])
    shift[:, keep] = out["shift"]                        # in the oracle's column order
    # (MODEL_CONST has no per-star entry: the oracle runs on NumPy's lnL rows, whose k^ noise the rule carries)
    lh.check_expect({"func": shift, "pareto_k": out["pareto_k"]}, lnl, None, z, what="influence")
    lh.planted_property(shift)
    assert out["ranking"][0] == lh.PLANTED_STAR
    assert np.allclose(out["mean"], mean[keep], rtol=1e-14) and np.allclose(out["std"], std[keep], rtol=1e-13)
    assert np.array_equal(out["loo_mean"], out["mean"] + out["std"] * out["shift"])
    # a derived function: the rotation amplitude; and a constant one
    ix, iy = (list(fit.fitted_parameters).index(n) for n in ("v_maxx", "v_maxy"))
    fns = {"v_rot": lambda t: np.hypot(t[:, ix], t[:, iy]), "one": lambda t: np.ones(t.shape[0])}
    der = fit.loo_influence(chain, n_burn=0, functions=fns)
    amp = np.hypot(table[:, names.index("v_maxx")], table[:, names.index("v_maxy")])
    zc = ((amp - amp.mean()) / amp.std())[:, None]
    lh.check_expect({"func": der["shift"][:, :1], "pareto_k": der["pareto_k"]}, lnl, None, zc, what="v_rot")
    assert der["names"] == ["v_rot", "one"] and np.all(der["shift"][:, 1] == 0.0) and der["std"][1] == 0.0
    # more than 16 functions run in batches of 16
    many = {"f{0}".format(q): (lambda t, q=q: t[:, q % 4] * (1.0 + q)) for q in range(18)}
    res = fit.loo_influence(chain, n_burn=0, functions=many)
    assert res["shift"].shape == (300, 18)
    for q in range(18):
        assert np.allclose(res["shift"][:, q], out["shift"][:, q % 4], rtol=0, atol=1e-12), q
    fit.close()


def test_runner_loo_pit_of_the_background_models(cat2k):
    from mcmc_dynamics_amd.analysis import ConstantFitGB
    from mcmc_dynamics_amd.analysis.binned import BinnedConstantFit
    from mcmc_dynamics_amd.analysis.runner import ppc_summary
    from mcmc_dynamics_amd import DataReader
    fit = _fit(ConstantFitGB, cat2k, ("ra", "dec", "v", "verr", "density"))
    table = ph.samples(cat2k, 2, False, 16 * 16, seed=12)
    names = ph.abi_names(2, False)
    chain = table[:, [names.index(n) for n in fit.fitted_parameters]].reshape(16, 16, -1)
    out = fit.loo_pit(chain, n_burn=0, n_bins=10)
    want = fit._catalog.psis_loo_expect(table, mixture=True)
    assert np.array_equal(out["loo_pit"], want["pit_mix"]) and np.array_equal(out["pit"], want["pit"])
    assert np.array_equal(out["pareto_k"], want["pareto_k"]) and np.array_equal(out["n_eff"], want["n_eff"])
    summary = ppc_summary(want["pit_mix"], None, 10)
    assert out["chi2"] == summary["chi2"] and out["n"] == 2000.0 and out["hist"].size == 10
    assert np.array_equal(out["weight"], fit.posterior_membership_probabilities(chain, 0)[0])
    assert out["k_threshold"] == pytest.approx(psh.k_threshold(256))
    assert out["n_bad_k"] == int(np.count_nonzero(want["pareto_k"] > out["k_threshold"]))
    fit.close()
    reader = DataReader({k: cat2k[k] for k in ("ra", "dec", "v", "verr")})
    reader.make_radial_bins(ph.CENTRE[0], ph.CENTRE[1], nstars=500)
    bf = BinnedConstantFit(reader)
    with pytest.raises(NotImplementedError, match="un-binned"):
        bf.loo_pit(chain, 1)
    with pytest.raises(NotImplementedError, match="un-binned"):
        bf.loo_influence(chain, 1)
    bf.close()


def test_loo_pit_of_two_ranks_on_one_device():
    """Two ranks (one process each, one device, tests/fake_rccl for the collective): the per-rank arrays concatenate to
    the single-rank result bit for bit and the summaries are equal on both ranks."""
    subprocess.run(["make", "-C", os.path.join(ROOT, "tests", "fake_rccl")], check=True, capture_output=True)
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", OMP_NUM_THREADS="1")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr",
           "127.0.0.1", "--master-port", "29593", os.path.join(ROOT, "tests", "loo_expect_rank_worker.py")]
    res = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-3000:]
    assert "LOO_EXPECT_RANKS_OK world=2" in res.stdout

"""GPU: the simulated catalogues (csrc/mcd_simulated.hip, csrc/mcd_api_simulated.hip) and the lock-stepped fits on them
(Runner.simulated_fits, sbc, recovery).

Catalogues and models: simulated_helper.make_case, 9 models x {fixed, free centre}.  Shapes: N in {1, 33, 1027} x E in
{1, 3, 70} (70 simulations give a second, ragged lane tile) x rows in {1, 65, 257} (257: the XCD-grouped branch of
wave_task).

  1. mcd_simulate against the longdouble restatement of the velocity rule from _native.replicate_numbers
     (simulated_helper.check_velocities: the bound of tests/test_simulated_cpu.py and its asserted |u - m*| margin); the
     sim0 split and a forced chunk_len give the same bits; the returned array is what a call with velocities = NULL
     followed by an identical call returns;
  2. mcd_simulated_loglike against this device's own plain path (option fast_path = 0) on a fresh catalogue per
     simulation that holds the simulated velocities (lnlike_bg recomputed from the Gaussian for the fixed-background
     families): 1e-12 on max(|lnL|, N); a row under the wrong simulation differs by more than 1e-6 relative;
  3. mcd_simulated_set: simulate's own output reproduces 2's values bit for bit; the observed velocities give the plain
     path's sum to 1e-12;
  4. every refusal with its status and message, the resident set answering as before after each; MCD_ERR_NONFINITE leaves
     no set resident;
  5. the runs fixed by tests/test_simulated_cpu.py::test_closed_form_harness_sizes_the_run end to end, the chain's bits
     twice, the stored lnprobability, and recovery's coverage;
  6. lnprob_simulated_batch: shapes, prior masking with a donor row, structured priors."""
import ctypes

import numpy as np
import pytest

import holdout_helper as hh
import simulated_helper as sh
import variant_helper as vh

pytestmark = pytest.mark.gpu

CELLS = [(m, f) for m in sh.MODELS for f in (False, True)]
STARS, SIMS, ROWS = (1, 33, 1027), (1, 3, 70), (1, 65, 257)
_I64P = ctypes.POINTER(ctypes.c_int64)
_F64P = ctypes.POINTER(ctypes.c_double)
NAN = float("nan")


@pytest.fixture(scope="module")
def native():
    from mcmc_dynamics_amd import _native
    return _native


@pytest.fixture(scope="module")
def ctx(native):
    return native.default_context()


def within(got, want, scale_n):
    """The project's bound for kernel families: 1e-12 on the scale max(|lnL|, N)."""
    return np.abs(got - want) <= 1e-12 * np.maximum(np.abs(want), float(scale_n))


def plain_values(native, ctx, case, table, velocities):
    """(R,) values of the rows `table` on the velocities (N,) through the plain path of a fresh catalogue."""
    fresh = vh.catalog(native, ctx, dict(case, cat=sh.substituted(case, velocities)))
    try:
        fresh.set_option("fast_path", 0)
        return fresh.loglike(table)
    finally:
        fresh.close()


# ------------------------------------------------------------------------------------------ 1
@pytest.mark.skipif(not vh.HAVE_LONGDOUBLE, reason="numpy.longdouble is not wider than float64 here")
@pytest.mark.parametrize("model,free", CELLS)
def test_simulate_follows_the_velocity_rule(native, ctx, model, free):
    worst = 0.0
    for n in STARS:
        case = sh.make_case(model, free, n)
        bg = sh.background_of(case)
        cat = vh.catalog(native, ctx, case)
        try:
            for n_sims in SIMS:
                truths = case["params"][:n_sims]
                got = cat.simulate(truths, sh.SEED, bg_mean=bg[0], bg_sigma=bg[1])
                assert got.shape == (n_sims, n) and cat.simulated_sims == n_sims
                worst = max(worst, sh.check_velocities(got, case, truths, label=(model, free, n, n_sims),
                                                       numbers=native.replicate_numbers))
            # (the 70-simulation set is resident) the split of a call, a forced chunk length, a call without the copy
            full = got
            for s0, s1 in ((3, 4), (64, 70), (1, 70)):
                part = cat.simulate(truths[s0:s1], sh.SEED, sim0=s0, bg_mean=bg[0], bg_sigma=bg[1])
                assert part.tobytes() == full[s0:s1].tobytes(), (model, free, n, s0, s1)
            cat.set_option("chunk_len", 96)
            assert cat.simulate(truths, sh.SEED, bg_mean=bg[0], bg_sigma=bg[1]).tobytes() == full.tobytes()
            cat.set_option("chunk_len", 0)
            assert cat.simulate(truths, sh.SEED, bg_mean=bg[0], bg_sigma=bg[1], want_velocities=False) is None
            assert cat.simulated_sims == 70
            assert cat.simulate(truths, sh.SEED, bg_mean=bg[0], bg_sigma=bg[1]).tobytes() == full.tobytes()
            assert not np.array_equal(cat.simulate(truths, sh.SEED + 1, bg_mean=bg[0], bg_sigma=bg[1]), full)
        finally:
            cat.close()
    print("model", model, "free" if free else "fixed", "largest velocity error", worst)


# ------------------------------------------------------------------------------------------ 2, 3
@pytest.mark.parametrize("model,free", CELLS)
def test_simulated_loglike_against_the_plain_path_and_the_uploaded_set(native, ctx, model, free):
    worst = 0.0
    for n in STARS:
        case = sh.make_case(model, free, n)
        bg = sh.background_of(case)
        cat = vh.catalog(native, ctx, case)
        try:
            n_sims = 3
            vel = cat.simulate(case["params"][:n_sims], sh.SEED, bg_mean=bg[0], bg_sigma=bg[1])
            values = {}
            for rows in ROWS:
                table = np.ascontiguousarray(case["params"][:rows])
                sim = sh.row_sims(rows, n_sims)
                got = cat.simulated_loglike(table, sim)
                assert got.shape == (rows,) and np.all(np.isfinite(got))
                assert cat.simulated_loglike(table, sim).tobytes() == got.tobytes()
                want = np.empty(rows)
                for e in range(n_sims):
                    if np.any(sim == e):
                        want[sim == e] = plain_values(native, ctx, case, table[sim == e], vel[e])
                ok = within(got, want, n)
                worst = max(worst, float(np.max(np.abs(got - want) / np.maximum(np.abs(want), n))))
                assert ok.all(), (model, free, n, rows, got[~ok], want[~ok])
                values[rows] = got
                if n > 1:
                    # a row under the wrong simulation
                    other = cat.simulated_loglike(table, (sim + 1) % n_sims)
                    assert np.all(np.abs(other - got) > 1e-6 * np.abs(got)), (model, free, n, rows)
            # a forced chunk length keeps the resident set, and moves the sums by rounding at the most
            cat.set_option("chunk_len", 96)
            assert cat.simulated_sims == n_sims
            again = cat.simulated_loglike(np.ascontiguousarray(case["params"][:65]), sh.row_sims(65, n_sims))
            assert within(again, values[65], n).all()
            cat.set_option("chunk_len", 0)
            # 3. the uploaded set: simulate's own output, then the observed velocities
            cat.simulated_set(vel + 1.0, bg_mean=bg[0], bg_sigma=bg[1])
            assert not np.array_equal(cat.simulated_loglike(np.ascontiguousarray(case["params"][:65]), sh.row_sims(65, n_sims)),
                                      values[65])
            cat.simulated_set(vel, bg_mean=bg[0], bg_sigma=bg[1])
            for rows in ROWS:
                got = cat.simulated_loglike(np.ascontiguousarray(case["params"][:rows]), sh.row_sims(rows, n_sims))
                assert got.tobytes() == values[rows].tobytes(), (model, free, n, rows)
            cat.simulated_set(np.stack([case["cat"]["v"] + 1.0, case["cat"]["v"]]), bg_mean=bg[0], bg_sigma=bg[1])
            assert cat.simulated_sims == 2
            table = np.ascontiguousarray(case["params"][:65])
            got = cat.simulated_loglike(table, np.ones(65, dtype=np.int64))
            cat.set_option("fast_path", 0)
            want = cat.loglike(table)
            assert within(got, want, n).all(), (model, free, n, "observed velocities")
            if sh.eh.BG_OF[model]:                               # (per-star outputs exist for the background models)
                assert within(got[7], cat.loglike_per_star(table[7]).sum(), n)
        finally:
            cat.close()
    print("model", model, "free" if free else "fixed", "largest error against the plain path", worst)


# ------------------------------------------------------------------------------------------ 4
def _raw_loglike(cat, table, sim, n_rows=None, k=None):
    out = np.full(table.shape[0], -7.25)
    sim = None if sim is None else np.ascontiguousarray(sim, dtype=np.int64)
    rc = cat.lib.mcd_simulated_loglike(cat.handle, table.shape[0] if n_rows is None else n_rows, table.shape[1] if k is None else k,
                                       table.ctypes.data_as(_F64P), None if sim is None else sim.ctypes.data_as(_I64P),
                                       out.ctypes.data_as(_F64P))
    return rc, out


def _raw_simulate(cat, truths, n_sims=None, k=None, seed=1, sim0=0, bg=(NAN, NAN), want=True):
    out = np.full((truths.shape[0], cat.n_stars), -7.25)
    rc = cat.lib.mcd_simulate(cat.handle, truths.shape[0] if n_sims is None else n_sims, truths.shape[1] if k is None else k,
                              truths.ctypes.data_as(_F64P), seed, sim0, bg[0], bg[1], out.ctypes.data_as(_F64P) if want else None)
    return rc, out


def _raw_set(cat, vel, n_sims=None, bg=(NAN, NAN)):
    vel = np.ascontiguousarray(vel, dtype=np.float64)
    return cat.lib.mcd_simulated_set(cat.handle, vel.shape[0] if n_sims is None else n_sims, vel.ctypes.data_as(_F64P), bg[0], bg[1])


def test_refusals_leave_the_outputs_and_the_resident_set_untouched(native, ctx):
    n = 33
    case = sh.make_case(0, False, n)
    cat = vh.catalog(native, ctx, case)
    table = np.ascontiguousarray(case["params"][:4])
    sim = np.array([0, 2, 1, 2], dtype=np.int64)
    assert cat.simulated_sims == 0
    rc, out = _raw_loglike(cat, table, sim)
    assert rc == -1 and np.all(out == -7.25) and "no simulated set is resident" in cat.lib.mcd_last_error().decode()
    vel = cat.simulate(table[:3], 5)
    before = cat.simulated_loglike(table, sim)

    def still():
        assert cat.simulated_sims == 3 and cat.simulated_loglike(table, sim).tobytes() == before.tobytes()

    def refused(call, name, what, rc, out=None, status=-1):
        assert rc == status, (what, rc)
        if out is not None:
            assert np.all(out == -7.25), what
        message = cat.lib.mcd_last_error().decode()
        assert what in message and message.startswith(name + ":"), (what, message)
        still()
    # mcd_simulated_loglike
    refused("loglike", "mcd_simulated_loglike", "columns", *_raw_loglike(cat, table, sim, k=5))
    refused("loglike", "mcd_simulated_loglike", "65536", *_raw_loglike(cat, table, sim, n_rows=0))
    big = np.ascontiguousarray(np.broadcast_to(table[0], (65537, table.shape[1])))
    refused("loglike", "mcd_simulated_loglike", "65536", *_raw_loglike(cat, big, np.zeros(65537, dtype=np.int64)))
    refused("loglike", "mcd_simulated_loglike", "outside [0, 3)", *_raw_loglike(cat, table, [0, 3, 1, 2]))
    refused("loglike", "mcd_simulated_loglike", "outside [0, 3)", *_raw_loglike(cat, table, [0, -1, 1, 2]))
    refused("loglike", "mcd_simulated_loglike", "null", *_raw_loglike(cat, table, None))
    # mcd_simulate
    refused("simulate", "mcd_simulate", "columns", *_raw_simulate(cat, table, k=5))
    refused("simulate", "mcd_simulate", "at least one simulation", *_raw_simulate(cat, table, n_sims=0))
    refused("simulate", "mcd_simulate", "sim0", *_raw_simulate(cat, table, sim0=-1))
    too_many = (1 << 30) // 8 // n + 1
    refused("simulate", "mcd_simulate", "1024 MiB", *_raw_simulate(cat, table, n_sims=too_many))
    # mcd_simulated_set
    refused("set", "mcd_simulated_set", "at least one simulation", _raw_set(cat, vel, n_sims=0))
    refused("set", "mcd_simulated_set", "1024 MiB", _raw_set(cat, vel, n_sims=too_many))
    for bad in (np.nan, np.inf, -np.inf):
        v = vel.copy()
        v[2, 17] = bad
        refused("set", "mcd_simulated_set", "velocity [2][17] is not finite", _raw_set(cat, v))
    assert cat.lib.mcd_simulated_set(cat.handle, 3, None, NAN, NAN) == -1
    still()
    # out NULL: MCD_OK without work
    assert cat.lib.mcd_simulated_loglike(cat.handle, 4, table.shape[1], table.ctypes.data_as(_F64P), sim.ctypes.data_as(_I64P), None) == 0
    # binned and float32 catalogues
    c = case["cat"]
    for more, what in (({"bin_offsets": np.array([0, 10, 33], dtype=np.int64)}, "un-binned"), ({"precision": "f32"}, "MCD_F64")):
        other = native.Catalog(ctx, c["ra"], c["dec"], c["v"], c["verr"], model=0, centre=case["centre"], **more)
        for rc in (_raw_simulate(other, table)[0], _raw_set(other, vel), _raw_loglike(other, table, sim)[0]):
            assert rc == -1 and what in other.lib.mcd_last_error().decode()
        other.close()
    still()
    cat.close()


def test_a_fixed_background_model_needs_its_gaussian(native, ctx):
    for model in (1, 5, 6):
        case = sh.make_case(model, False, 33)
        bg = sh.background_of(case)
        cat = vh.catalog(native, ctx, case)
        table = np.ascontiguousarray(case["params"][:3])
        vel = cat.simulate(table, 5, bg_mean=bg[0], bg_sigma=bg[1])
        before = cat.simulated_loglike(table, [0, 1, 2])
        for bad in ((NAN, NAN), (bg[0], -1.0), (np.inf, bg[1]), (bg[0], NAN)):
            rc, out = _raw_simulate(cat, table, bg=bad)
            assert rc == -1 and np.all(out == -7.25) and "fixed-background model needs" in cat.lib.mcd_last_error().decode()
            assert _raw_set(cat, vel, bg=bad) == -1 and "fixed-background model needs" in cat.lib.mcd_last_error().decode()
            assert cat.simulated_loglike(table, [0, 1, 2]).tobytes() == before.tobytes()
        # the set's Gaussian is part of the set: another width moves the values
        cat.simulated_set(vel, bg_mean=bg[0], bg_sigma=2.0 * bg[1])
        assert not np.array_equal(cat.simulated_loglike(table, [0, 1, 2]), before)
        cat.close()


def test_a_non_finite_generated_velocity_leaves_no_set_resident(native, ctx):
    """A truth outside the model's domain: the Plummer profile with a scale radius a < 0 has a negative dispersion
    squared, so a star of verr = 0 has n* < 0 and its velocity is NaN.  (sigma_max < 0 alone is inside the domain of every
    family: it enters as sigma_max^2.)  The message names the first simulation with such a star and its first star, which
    the CPU build of the rule tells."""
    import re
    case = sh.make_case(3, False, 33)
    case["cat"]["verr"][[11, 20]] = 0.0
    cat = vh.catalog(native, ctx, case)
    table = np.ascontiguousarray(case["params"][:70])
    cat.simulate(table[:3], 5)
    assert cat.simulated_sims == 3
    bad = table.copy()
    bad[[2, 66], 2] *= -1.0
    host = sh.simulate(case, bad, seed=5)
    assert np.all(np.isfinite(host[[0, 1]])) and not np.isfinite(host[2, 11]) and not np.isfinite(host[66, 20])
    first = int(np.flatnonzero(~np.isfinite(host[2]))[0])
    rc, out = _raw_simulate(cat, bad, seed=5)
    assert rc == -5, rc
    message = cat.lib.mcd_last_error().decode()
    assert message.startswith("mcd_simulate:") and "not finite" in message, message
    assert re.search(r"simulation 2, star (\d+) ", message) and int(re.search(r"star (\d+) ", message).group(1)) == first, message
    assert cat.simulated_sims == 0
    rc, out = _raw_loglike(cat, table[:4], [0, 0, 0, 0])
    assert rc == -1 and np.all(out == -7.25) and "no simulated set is resident" in cat.lib.mcd_last_error().decode()
    # a later simulation alone is named with its own index in the call
    rc, out = _raw_simulate(cat, bad[60:], seed=5, sim0=60)
    assert rc == -5 and "simulation 6, star" in cat.lib.mcd_last_error().decode()
    # and the catalogue still works
    assert np.all(np.isfinite(cat.simulate(table[:3], 5))) and cat.simulated_sims == 3
    cat.close()


def test_a_communicator_is_refused(native, ctx):
    import os
    case = sh.make_case(0, False, 33)
    os.environ["MCD_FORCE_RCCL"] = "1"
    try:
        ctx1 = native.Context(n_devices=1)
    finally:
        del os.environ["MCD_FORCE_RCCL"]
    other = vh.catalog(native, ctx1, case)
    try:
        table = np.ascontiguousarray(case["params"][:4])
        rc, out = _raw_simulate(other, table)
        assert rc == -1 and np.all(out == -7.25) and "one device per process" in other.lib.mcd_last_error().decode()
        assert _raw_set(other, np.zeros((2, 33))) == -1 and "one device per process" in other.lib.mcd_last_error().decode()
        rc, out = _raw_loglike(other, table, [0, 0, 0, 0])
        assert rc == -1 and np.all(out == -7.25) and "one device per process" in other.lib.mcd_last_error().decode()
    finally:
        other.close()


# ------------------------------------------------------------------------------------------ 5
@pytest.fixture(scope="module")
def cols():
    return hh.closed_form_columns()


@pytest.fixture(scope="module")
def fit(cols):
    f = sh.closed_form_fit(cols)
    yield f
    f.close()


_RUNS = {}


def _run(fit, run):
    """The fixed run, made once for the whole module."""
    if run not in _RUNS:
        _RUNS[run] = fit.sbc(seed=sh.RUN_SEED, n_bins=sh.N_BINS, **sh.RUNS[run])
    return _RUNS[run]


@pytest.mark.parametrize("run", sorted(sh.RUNS))
def test_every_fit_samples_the_posterior_of_its_own_catalogue(native, fit, cols, run):
    from mcmc_dynamics_amd.analysis.runner import sbc_summary
    cfg = sh.RUNS[run]
    out = _run(fit, run)
    fits = out["fits"]
    n_e, n_w, t_kept = cfg["n_sims"], cfg["n_walkers"], cfg["n_steps"] - cfg["n_burn"]
    assert fits["sampler"].chain.shape == (n_e, n_w, cfg["n_steps"], 1) and out["seed"] == sh.RUN_SEED and out["names"] == ["v_sys"]
    assert np.array_equal(out["truths"], fit.sample_prior(n_e, seed=sh.RUN_SEED))
    # the device's velocities are the rule's at those truths, from the replayed numbers
    want = sh.host_velocities(cols, out["truths"], sh.RUN_SEED)
    assert np.all(np.abs(fits["velocities"] - want) <= 1e-12 * np.maximum(np.abs(want), 1.0))
    mu, lam = sh.closed_form_posteriors(cols, fits["velocities"])
    sh.check_fits(fits, mu, lam, "device, " + run, n_w, t_kept)
    sh.check_ranks(out, "device, " + run)
    # the bounds tell the catalogues apart: fit e against catalogue e + 1
    with pytest.raises(AssertionError):
        sh.check_fits(fits, np.roll(mu, -1), lam, "(expected to miss)", n_w, t_kept)
    with pytest.raises(AssertionError):
        sh.check_ranks(sbc_summary(fits["sampler"].chain, np.roll(out["truths"], -1, axis=0), cfg["n_burn"], thin=out["thin"],
                                   n_bins=sh.N_BINS), "(expected to miss)")


def test_stored_lnprobability_and_the_chains_bits(fit):
    cfg = sh.RUNS["ragged"]
    out = _run(fit, "ragged")
    sampler, truths = out["fits"]["sampler"], out["truths"]
    chain, lnp = sampler.chain, sampler.lnprobability
    assert lnp.shape == chain.shape[:3]
    # (the set of the run is made resident again: the tiled run may have replaced it)
    fit.simulate(truths, sh.RUN_SEED)
    for e, w, t in ((0, 0, 0), (3, 17, 1), (7, 31, 299), (63, 5, cfg["n_steps"] - 1), (40, 9, 1000)):
        got = fit.lnprob_simulated_batch(chain[e, w, t], [e])
        assert got.shape == ()
        assert abs(float(got) - lnp[e, w, t]) <= 1e-12 * max(abs(lnp[e, w, t]), hh.N_STARS), (e, w, t, float(got), lnp[e, w, t])
        other = fit.lnprob_simulated_batch(chain[e, w, t], [(e + 1) % 64])
        assert abs(float(other) - lnp[e, w, t]) > 1e-6 * abs(lnp[e, w, t])
    # the first 200 steps again: the chain is a function of the seed
    again = fit.simulated_fits(truths, n_walkers=cfg["n_walkers"], n_steps=200, n_burn=50, seed=sh.RUN_SEED)["sampler"]
    assert again.chain.tobytes() == np.ascontiguousarray(chain[:, :, :200]).tobytes()
    assert again.lnprobability.tobytes() == np.ascontiguousarray(lnp[:, :, :200]).tobytes()
    other = fit.simulated_fits(truths, n_walkers=cfg["n_walkers"], n_steps=20, n_burn=5, seed=sh.RUN_SEED + 1)["sampler"]
    assert not np.array_equal(other.chain[:, :, 19], chain[:, :, 19])


def test_recovery_covers_the_truth(fit):
    """64 catalogues at v_sys = 1: the share of 68.27 % intervals that hold the truth, within 3 binomial standard errors."""
    n_e = 64
    r = fit.recovery([1.0], n_sims=n_e, n_walkers=32, n_steps=700, n_burn=200, seed=sh.RUN_SEED,
                     functions={"speed": lambda t: np.abs(t[:, 0])}, null=[0.0])
    se = np.sqrt(0.6827 * 0.3173 / n_e)
    print("recovery at v_sys = 1: coverage", r["coverage"][68][0], r["coverage"][95][0], "bias", r["bias"][0], "rmse", r["rmse"][0],
          "z", r["z_mean"][0], r["z_std"][0], "exceeds", r["functions"]["speed"]["exceeds"])
    assert abs(r["coverage"][68][0] - 0.6827) <= 3.0 * se, r["coverage"][68]
    assert r["n_sims"] == n_e and r["functions"]["speed"]["truth"] == 1.0 and 0.0 <= r["functions"]["speed"]["exceeds"] <= 1.0
    # the posterior of one catalogue is N(mu_e, 1 / Lambda), Lambda about 2: the means scatter by about 0.7 about a point
    # shrunk towards the prior's 0 by 1 / (4 Lambda)
    assert 0.4 < r["rmse"][0] < 1.0 and abs(r["bias"][0]) < 0.5


# ------------------------------------------------------------------------------------------ 6
def test_lnprob_simulated_batch_shapes_prior_and_structured_priors(fit, cols):
    rng = np.random.default_rng(8)
    truths = np.array([[0.5], [-1.0], [2.0]])
    vel = fit.simulate(truths, 4)
    assert vel.shape == (3, hh.N_STARS)
    values = rng.normal(size=(3, 5, 1))
    sim = np.repeat(np.arange(3), 5)
    got = fit.lnprob_simulated_batch(values, sim)
    assert got.shape == (3, 5) and np.all(np.isfinite(got))
    stand_in = sh.NumpySimulated(cols)
    stand_in.simulated_set(vel)
    want = stand_in(values, sim)                                  # the likelihood and the structured prior N(0, 2^2)
    assert np.all(np.abs(got - want) <= 1e-10 * np.abs(want))
    # rows outside the box are -inf and leave the others as they were (the donor row stands in for them in the launch)
    outside = values.copy()
    outside[1, 2, 0] = 5000.0
    outside[0, 0, 0] = -5000.0
    masked = fit.lnprob_simulated_batch(outside, sim)
    bad = np.zeros((3, 5), dtype=bool)
    bad[1, 2] = bad[0, 0] = True
    assert np.all(masked[bad] == -np.inf) and np.array_equal(masked[~bad], got[~bad])
    assert np.all(fit.lnprob_simulated_batch(np.full((2, 1), 5000.0), [0, 1]) == -np.inf)
    # the caller's own velocities
    assert fit.simulated_set(vel[::-1]).shape == (3, hh.N_STARS)
    assert np.array_equal(fit.lnprob_simulated_batch(values, 2 - sim), got)
    with pytest.raises(ValueError):
        fit.lnprob_simulated_batch(values, sim[:-1])
    with pytest.raises(ValueError):
        fit.lnprob_simulated_batch(np.zeros((4, 2)), np.zeros(4))
    with pytest.raises(ValueError):
        fit.simulate(np.array([[5000.0]]), 1)

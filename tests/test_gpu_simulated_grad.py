"""GPU: value and gradient on simulated catalogues (csrc/mcd_simulated_grad.hip, mcd_simulated_loglike_grad) and the MAP fits
built on them (Runner.lnprob_simulated_grad_batch, simulated_maximize, lrt).

Catalogues and models: simulated_helper.make_case, 9 models x {fixed, free centre} x N in {1, 33, 1027} (a single star that
sets every scale; fewer stars than a chunk; several chunks) x rows in {1, 65, 257} (one wave with idle lanes; a ragged
second tile; the XCD-grouped branch of wave_task), on the 3-simulation set of simulated_grad_helper.velocities with rows
mapped by simulated_helper.row_sims.

  1. the matrix: every column under |got - exact| / S_k <= 2 err_np64 + floor (simulated_grad_helper: the longdouble
     restatements and the floors measured with the host build), the value field with mcd_simulated_loglike's bits, two calls
     with identical bytes, out = NULL with the same gradient bytes, and for N > 1 a row under the wrong simulation moving a
     column by more than 1e-6 of S_k;
  2. option chunk_len = 96 keeps the resident set and moves the results by rounding only (the same rule);
  3. a set that holds the observed velocities: value and gradient under the rule against the observed catalogue, as
     mcd_loglike_grad_batch's are;
  4. every refusal with its status and message, prefilled out / grad untouched, the resident set answering as before; a
     communicator;
  5. end to end on holdout_helper's closed-form catalogue, 64 simulations: simulated_maximize against the exact posterior
     modes, lrt against the weighted-least-squares closed form of every statistic;
  6. lnprob_simulated_grad_batch on a ConstantFitGB: shapes, prior masking with a donor row, structured priors."""
import ctypes

import numpy as np
import pytest

import holdout_helper as hh
import simulated_grad_helper as sg
import simulated_helper as sh
import variant_helper as vh

pytestmark = pytest.mark.gpu

_I64P = ctypes.POINTER(ctypes.c_int64)
_F64P = ctypes.POINTER(ctypes.c_double)
L = vh.L


@pytest.fixture(scope="module")
def native():
    from mcmc_dynamics_amd import _native
    return _native


@pytest.fixture(scope="module")
def ctx(native):
    return native.default_context()


# ------------------------------------------------------------------------------------------ 1, 2, 3
@pytest.mark.skipif(not vh.HAVE_LONGDOUBLE, reason="numpy.longdouble is not wider than float64 here")
@pytest.mark.parametrize("model,free", sg.CELLS)
def test_matrix_against_the_longdouble_gradient(native, ctx, model, free):
    worst_v = worst_g = 0.0
    k = sg.n_columns(model, free)
    for n in sg.STARS:
        case = sh.make_case(model, free, n)
        bg = sh.background_of(case)
        vel = sg.velocities(case)
        floor = sg.floor(model, free, n)
        cat = vh.catalog(native, ctx, case)
        try:
            cat.simulated_set(vel, bg_mean=bg[0], bg_sigma=bg[1])
            kept = {}
            for rows in sg.ROWS:
                table = np.ascontiguousarray(case["params"][:rows])
                sim = sh.row_sims(rows, sg.N_SIMS)
                value, grad = cat.simulated_loglike_grad(table, sim)
                assert value.shape == (rows,) and grad.shape == (rows, k) and np.all(np.isfinite(grad))
                assert value.tobytes() == cat.simulated_loglike(table, sim).tobytes(), ("value bits", model, free, n, rows)
                again = cat.simulated_loglike_grad(table, sim)
                assert again[0].tobytes() == value.tobytes() and again[1].tobytes() == grad.tobytes(), ("not repeatable", model, free, n, rows)
                none, only = cat.simulated_loglike_grad(table, sim, want_value=False)
                assert none is None and only.tobytes() == grad.tobytes(), ("out = NULL", model, free, n, rows)
                other = cat.simulated_loglike_grad(table, (sim + 1) % sg.N_SIMS)[1] if n > 1 else None
                for j in vh.sample_rows(rows):
                    ref = sg.reference(case, j, int(sim[j]), vel)
                    cell = (model, free, n, rows, j)
                    v_err, g_err = sg.check_row(value[j], grad[j], ref, n, cell, floor)
                    worst_v, worst_g = max(worst_v, v_err), max(worst_g, g_err)
                    if other is not None:
                        assert sg.gh.col_err(other[j], ref["g"], ref["s"]).max() > 1e-6, ("wrong simulation", cell)
                kept[rows] = (value, grad)
            # 2. a forced chunk length keeps the resident set, and moves the sums by rounding at the most
            cat.set_option("chunk_len", 96)
            assert cat.simulated_sims == sg.N_SIMS
            sim = sh.row_sims(65, sg.N_SIMS)
            value, grad = cat.simulated_loglike_grad(np.ascontiguousarray(case["params"][:65]), sim)
            for j in vh.sample_rows(65):
                sg.check_row(value[j], grad[j], sg.reference(case, j, int(sim[j]), vel), n, (model, free, n, "chunk_len", j), floor)
            assert np.all(np.abs(value - kept[65][0]) <= 2e-12 * np.maximum(np.abs(value), n))
            cat.set_option("chunk_len", 0)
            again = cat.simulated_loglike_grad(np.ascontiguousarray(case["params"][:65]), sim)
            assert again[0].tobytes() == kept[65][0].tobytes() and again[1].tobytes() == kept[65][1].tobytes()
            # 3. the observed velocities
            obs = np.stack([case["cat"]["v"] + 1.0, case["cat"]["v"]])
            cat.simulated_set(obs, bg_mean=bg[0], bg_sigma=bg[1])
            table = np.ascontiguousarray(case["params"][:65])
            value, grad = cat.simulated_loglike_grad(table, np.ones(65, dtype=np.int64))
            plain_value, plain_grad = cat.loglike_grad(table)
            for j in vh.sample_rows(65):
                ref = sg.reference(case, j, 1, obs)
                sg.check_row(value[j], grad[j], ref, n, (model, free, n, "observed", j), floor)
                sg.check_row(plain_value[j], plain_grad[j], ref, n, (model, free, n, "loglike_grad", j), floor)
        finally:
            cat.close()
    print("model", model, "free" if free else "fixed", "largest value error", worst_v, "largest column error", worst_g)


# ------------------------------------------------------------------------------------------ 4
def _raw(cat, table, sim, n_rows=None, k=None, want_out=True, want_grad=True):
    out, grad = np.full(table.shape[0], -7.25), np.full(table.shape, -7.25)
    sim = None if sim is None else np.ascontiguousarray(sim, dtype=np.int64)
    rc = cat.lib.mcd_simulated_loglike_grad(cat.handle, table.shape[0] if n_rows is None else n_rows,
                                            table.shape[1] if k is None else k, table.ctypes.data_as(_F64P),
                                            None if sim is None else sim.ctypes.data_as(_I64P),
                                            out.ctypes.data_as(_F64P) if want_out else None,
                                            grad.ctypes.data_as(_F64P) if want_grad else None)
    return rc, out, grad


def test_refusals_leave_the_outputs_and_the_resident_set_untouched(native, ctx):
    n = 33
    case = sh.make_case(0, False, n)
    cat = vh.catalog(native, ctx, case)
    table = np.ascontiguousarray(case["params"][:4])
    sim = np.array([0, 2, 1, 2], dtype=np.int64)
    name = "mcd_simulated_loglike_grad"
    rc, out, grad = _raw(cat, table, sim)
    assert rc == -1 and np.all(out == -7.25) and np.all(grad == -7.25) and "no simulated set is resident" in cat.lib.mcd_last_error().decode()
    cat.simulate(table[:3], 5)
    before = cat.simulated_loglike_grad(table, sim)

    def still():
        after = cat.simulated_loglike_grad(table, sim)
        assert cat.simulated_sims == 3 and after[0].tobytes() == before[0].tobytes() and after[1].tobytes() == before[1].tobytes()

    def refused(what, rc, out, grad, who=cat):
        assert rc == -1, (what, rc)
        assert np.all(out == -7.25) and np.all(grad == -7.25), what
        message = who.lib.mcd_last_error().decode()
        assert what in message and message.startswith(name + ":"), (what, message)
        if who is cat:
            still()
    refused("columns", *_raw(cat, table, sim, k=5))
    refused("65536", *_raw(cat, table, sim, n_rows=0))
    big = np.ascontiguousarray(np.broadcast_to(table[0], (65537, table.shape[1])))
    refused("65536", *_raw(cat, big, np.zeros(65537, dtype=np.int64)))
    refused("outside [0, 3)", *_raw(cat, table, [0, 3, 1, 2]))
    refused("outside [0, 3)", *_raw(cat, table, [0, -1, 1, 2]))
    refused("null", *_raw(cat, table, None))
    refused("null", *_raw(cat, table, sim, want_grad=False))
    rc = cat.lib.mcd_simulated_loglike_grad(cat.handle, 4, table.shape[1], None, sim.ctypes.data_as(_I64P), None, before[1].ctypes.data_as(_F64P))
    assert rc == -1 and "null" in cat.lib.mcd_last_error().decode()
    still()
    assert cat.lib.mcd_simulated_loglike_grad(None, 4, table.shape[1], table.ctypes.data_as(_F64P), sim.ctypes.data_as(_I64P), None,
                                              before[1].ctypes.data_as(_F64P)) == -1
    # out NULL: the gradient alone
    rc, out, grad = _raw(cat, table, sim, want_out=False)
    assert rc == 0 and np.all(out == -7.25) and grad.tobytes() == before[1].tobytes()
    # binned and float32 catalogues
    c = case["cat"]
    for more, what in (({"bin_offsets": np.array([0, 10, 33], dtype=np.int64)}, "un-binned"), ({"precision": "f32"}, "MCD_F64")):
        other = native.Catalog(ctx, c["ra"], c["dec"], c["v"], c["verr"], model=0, centre=case["centre"], **more)
        refused(what, *_raw(other, table, sim), who=other)
        other.close()
    still()
    # the plans go with option chunk_len, the set stays; a new set replaces the old one
    cat.set_option("chunk_len", 96)
    still()
    cat.set_option("chunk_len", 0)
    cat.simulate(table[:2], 6)
    rc, out, grad = _raw(cat, table, sim)
    assert rc == -1 and np.all(out == -7.25) and np.all(grad == -7.25) and "outside [0, 2)" in cat.lib.mcd_last_error().decode()
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
        rc, out, grad = _raw(other, table, [0, 0, 0, 0])
        assert rc == -1 and np.all(out == -7.25) and np.all(grad == -7.25)
        assert "one device per process" in other.lib.mcd_last_error().decode()
    finally:
        other.close()


# ------------------------------------------------------------------------------------------ 5
@pytest.fixture(scope="module")
def cols():
    return hh.closed_form_columns()


@pytest.mark.skipif(not vh.HAVE_LONGDOUBLE, reason="numpy.longdouble is not wider than float64 here")
def test_simulated_maximize_finds_every_posterior_mode(cols):
    """Only v_sys free under N(0, 2^2): catalogue e has the exact posterior mode mu_e and curvature Lambda_e.  All 64 fits
    converge and |x_e - mu_e| <= (gtol / scale + (2 err_np64 + 1e-12) S) / Lambda_e: the optimiser's stopping rule (scale =
    max(|start|, 1) over the starts, optimize.maximize_batch) plus the gradient rule, divided by the curvature.  S and
    err_np64 are those of the gradient sum at x_e: S = sum_i |v'_i - x_e| / n_i + |x_e| / 4."""
    fit = sh.closed_form_fit(cols)
    try:
        truths = fit.sample_prior(sg.N_E, seed=sg.RUN_SEED)
        out = fit.simulated_maximize(truths, seed=sg.RUN_SEED, gtol=sg.GTOL)
        assert out["converged"].all() and out["x"].shape == (sg.N_E, 1) and out["velocities"].shape == (sg.N_E, hh.N_STARS)
        mu, lam = sh.closed_form_posteriors(cols, out["velocities"])
        n80 = sg.variances(cols)
        x = out["x"][:, 0]
        terms80 = (out["velocities"].astype(L) - x.astype(L)[:, None]) / n80
        s = np.abs(terms80).sum(axis=1) + np.abs(x.astype(L)) / L(sh.PRIOR_SD) ** 2
        g80 = terms80.sum(axis=1) - x.astype(L) / L(sh.PRIOR_SD) ** 2
        g64 = ((out["velocities"] - x[:, None]) / n80.astype(np.float64)).sum(axis=1) - x / sh.PRIOR_SD ** 2
        err64 = np.abs(g64.astype(L) - g80) / s
        scale = max(float(np.abs(truths).max()), 1.0)
        bound = ((sg.GTOL / scale + (2 * err64 + L(1e-12)) * s) / lam).astype(np.float64)
        err = np.abs(x.astype(L) - mu).astype(np.float64)
        print("largest |x - mu| %.3g, smallest bound %.3g, iterations %d .. %d" % (err.max(), bound.min(), out["n_iter"].min(), out["n_iter"].max()))
        assert np.all(err <= bound), (err.tolist(), bound.tolist())
        # the bound tells the catalogues apart
        assert np.all(np.abs(x.astype(L) - np.roll(mu, 1)).astype(np.float64) > bound)
        again = fit.simulated_maximize(truths, seed=sg.RUN_SEED, gtol=sg.GTOL)
        assert again["x"].tobytes() == out["x"].tobytes() and again["lnprob"].tobytes() == out["lnprob"].tobytes()
        assert again["velocities"].tobytes() == out["velocities"].tobytes()
    finally:
        fit.close()


@pytest.mark.skipif(not vh.HAVE_LONGDOUBLE, reason="numpy.longdouble is not wider than float64 here")
def test_lrt_against_the_weighted_least_squares_closed_form(cols):
    """full = {v_sys, v_maxx free}, null = {v_sys free}, flat wide boxes: linear in both, so every statistic is
    2 (lnL_full - lnL_null) of two weighted-least-squares fits, in longdouble with sin(theta_i) from the oracle's rotation
    model.  |stat - exact| <= 4e-12 max(|lnL|, N) -- twice the value rule on each of the two maxima -- plus what the
    optimiser's stopping rule leaves (tests/test_simulated_grad_cpu.py::test_lrt_on_the_linear_stand_in_sizes_the_gpu_run:
    2.4e-16)."""
    full, null = sg.lrt_fits(cols)
    try:
        out = full.lrt(null, n_sims=sg.N_E, seed=sg.RUN_SEED, gtol=sg.GTOL)
        assert out["used"].all() and out["n_used"] == sg.N_E and out["df"] == 1 and out["n_negative"] == 0
        vel = out["velocities"]
        _, f1, a1 = sg.least_squares(cols, ["v_sys", "v_maxx"], vel)
        _, f0, a0 = sg.least_squares(cols, ["v_sys"], vel)
        exact = 2 * (f1 - f0)
        room = sg.optimiser_room(a1.astype(float), np.ones(2)) + sg.optimiser_room(a0.astype(float), np.ones(1))
        bound = 4e-12 * max(float(np.abs(f1).max()), float(np.abs(f0).max()), hh.N_STARS) + room
        err = np.abs(out["stat"].astype(L) - exact).astype(np.float64)
        _, g1, _ = sg.least_squares(cols, ["v_sys", "v_maxx"], cols["v"][None, :])
        _, g0, _ = sg.least_squares(cols, ["v_sys"], cols["v"][None, :])
        obs = 2 * (g1[0] - g0[0])
        print("largest |stat - exact| %.3g (bound %.3g), stat_obs %.6g (exact %.6g), p %.4f, iterations %d .. %d" %
              (err.max(), bound, out["stat_obs"], float(obs), out["p_value"], out["fits_full"]["n_iter"].min(),
               out["fits_full"]["n_iter"].max()))
        assert np.all(err <= bound), (err.max(), bound)
        assert abs(float(L(out["stat_obs"]) - obs)) <= bound
        assert out["p_value"] == (1.0 + np.count_nonzero(exact >= obs)) / (1.0 + sg.N_E)
        # the statistic tells the catalogues apart
        assert np.all(np.abs(out["stat"].astype(L) - np.roll(exact, 1)).astype(np.float64) > bound)
    finally:
        full.close()
        null.close()


# ------------------------------------------------------------------------------------------ 6
def test_lnprob_simulated_grad_batch_shapes_prior_and_structured_priors(native):
    from mcmc_dynamics_amd import DataReader, synthetic
    from mcmc_dynamics_amd.analysis import ConstantFitGB
    c = synthetic.make_catalog(300, config=2, background=True)
    fit = ConstantFitGB(DataReader({k: c[k] for k in ("ra", "dec", "v", "verr", "density")}))
    fit.parameters["ra_center"].set(value=synthetic.CENTER_RA_DEG, fixed=True)
    fit.parameters["dec_center"].set(value=synthetic.CENTER_DEC_DEG, fixed=True)
    fit.parameters["v_sys"].set(min=-100.0, max=100.0, prior=("normal", 0.0, 5.0))
    fit.parameters["sigma_max"].set(prior=("lognormal", np.log(6.0), 0.6))
    try:
        n_p = fit.n_fitted_parameters
        rows = fit.get_initials(10)
        fit.simulate(rows[:2], 4)
        sim = np.arange(10, dtype=np.int64) % 2
        value, grad = fit.lnprob_simulated_grad_batch(rows, sim)
        assert value.shape == (10,) and grad.shape == (10, n_p) and np.all(np.isfinite(value)) and np.all(np.isfinite(grad))
        # the likelihood's own value and gradient plus prior_eval's
        plan = fit._grad_plan()
        ll, g_ll = fit._lnlike_grad_rows(rows, lambda cat, table: cat.simulated_loglike_grad(table, sim))
        lp, g_lp = native.prior_eval(plan.prior, rows, want_grad=True)
        assert np.array_equal(value, ll + lp) and np.array_equal(grad, g_ll + g_lp) and np.any(g_lp != 0.0)
        # the value is lnprob_simulated_batch's, and the gradient its central difference
        want = fit.lnprob_simulated_batch(rows, sim)
        assert np.all(np.abs(value - want) <= 1e-12 * np.maximum(np.abs(want), 300.0))
        for j in range(n_p):
            h = 1e-5 * max(abs(rows[0, j]), 1.0)
            up, down = rows.copy(), rows.copy()
            up[:, j] += h
            down[:, j] -= h
            numeric = (fit.lnprob_simulated_batch(up, sim) - fit.lnprob_simulated_batch(down, sim)) / (up[:, j] - down[:, j])
            assert np.all(np.abs(numeric - grad[:, j]) <= 1e-5 * np.maximum(np.abs(grad[:, j]), 1.0)), (j, numeric, grad[:, j])
        # a row under the other simulation differs
        assert not np.array_equal(fit.lnprob_simulated_grad_batch(rows, 1 - sim)[1], grad)
        # rows outside the box are (-inf, zero row) and leave the others as they were (a donor row stands in for them)
        outside = rows.copy()
        outside[3, 0], outside[0, 1] = 1e9, -1.0
        m_value, m_grad = fit.lnprob_simulated_grad_batch(outside, sim)
        bad = np.zeros(10, dtype=bool)
        bad[[0, 3]] = True
        assert np.all(m_value[bad] == -np.inf) and np.all(m_grad[bad] == 0.0)
        assert np.array_equal(m_value[~bad], value[~bad]) and np.array_equal(m_grad[~bad], grad[~bad])
        with pytest.raises(ValueError):
            fit.lnprob_simulated_grad_batch(rows, sim[:-1])
        with pytest.raises(ValueError):
            fit.lnprob_simulated_grad_batch(np.zeros((4, n_p + 1)), np.zeros(4))
        assert fit.simulated_sims() == 2
    finally:
        fit.close()

"""CPU: MAP fits of simulated catalogues -- the value-and-gradient loop of csrc/mcd_simulated_grad.h through
tests/emul/simulated_grad_emul.cpp, the host layer (analysis/runner.py: lnprob_simulated_grad_batch's callers
simulated_maximize, parametric_bootstrap, lrt and the pure summaries) and the compiler's resource report
(profiles/simulated_grad_resources.json).

  1. chunk_simulated_grad against the longdouble restatements on the substituted velocities
     (simulated_grad_helper.reference): 9 models x {fixed, free} x N in {1, 33, 1027}, E = 3, rows under
     simulated_helper.row_sims; |got - exact| / S_k <= 2 err_np64 + floor per column with the floors of
     simulated_grad_helper.SIM_FLOOR, values 1e-12 on max(|sum l|, N);
  2. bits: the value field is simulated_helper.value's at the same chunk_len, in every cell; with the observed velocities as
     the simulation the no-background and Gaussian-background families give chunk_grad's bits in every field (see
     test_observed_velocities_give_the_plain_gradient_loops_bits for the two cells where those two demands exclude each
     other);
  3. the host logic on NumPy stand-ins (simulated_grad_helper.NumpyLinear): simulated_maximize reaches the closed-form
     maxima, best-of-S selection, the summaries on hand-made arrays, every ValueError of lrt, and the sizing of the
     end-to-end GPU run;
  4. no instantiation of the kernel uses scratch memory or LDS, and the committed report is today's."""
import json
import os

import numpy as np
import pytest

import holdout_helper as hh
import simulated_grad_helper as sg
import simulated_helper as sh
import variant_helper as vh
from mcmc_dynamics_amd.analysis.runner import lrt_summary, parametric_bootstrap_summary

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
needs_longdouble = pytest.mark.skipif(not vh.HAVE_LONGDOUBLE, reason="numpy.longdouble is not wider than float64 here")


# ------------------------------------------------------------------------------------------ 1. the loop against the truth
@needs_longdouble
@pytest.mark.parametrize("model,free", sg.CELLS)
def test_emulation_follows_the_gradient_rule(model, free):
    worst_v = worst_g = 0.0
    for n in sg.STARS:
        case = sh.make_case(model, free, n)
        vel = sg.velocities(case)
        for n_rows in sg.ROWS:
            sim = sh.row_sims(n_rows, sg.N_SIMS)
            values, grad = sg.emul(case, list(range(n_rows)), sim, vel)
            assert values.shape == (n_rows,) and grad.shape == (n_rows, sg.n_columns(model, free)) and np.all(np.isfinite(grad))
            for j in vh.sample_rows(n_rows):                     # the longdouble reference costs: a sample of the rows
                ref = sg.reference(case, j, int(sim[j]), vel)
                v_err, g_err = sg.check_row(values[j], grad[j], ref, n, (model, free, n, n_rows, j), sg.floor(model, free, n))
                worst_v, worst_g = max(worst_v, v_err), max(worst_g, g_err)
    print("model", model, "free" if free else "fixed", "largest value error", worst_v, "largest column error", worst_g)


@needs_longdouble
def test_a_row_under_the_wrong_simulation_misses_the_rule():
    case = sh.make_case(4, True, 33)
    vel = sg.velocities(case)
    values, grad = sg.emul(case, [0, 1, 2], [1, 2, 0], vel)
    for j in range(3):
        ref = sg.reference(case, j, j, vel)
        assert sg.gh.col_err(grad[j], ref["g"], ref["s"]).max() > 1e-6
        with pytest.raises(AssertionError):
            sg.check_row(values[j], grad[j], ref, 33, "wrong simulation", sg.floor(4, True, 33))


def test_floor_table_names_cells_of_the_matrix_only():
    assert all((m, f) in sg.CELLS and n in sg.STARS and v > sg.FLOOR for (m, f, n), v in sg.SIM_FLOOR.items())


# ------------------------------------------------------------------------------------------ 2. bits
@pytest.mark.parametrize("model,free", sg.CELLS)
def test_value_field_has_the_value_loops_bits(model, free):
    for n, chunk_len in ((1, 96), (33, 96), (1027, 96), (1027, 7)):
        case = sh.make_case(model, free, n)
        vel = sg.velocities(case)
        rows = list(range(65))
        sim = sh.row_sims(65, sg.N_SIMS)
        values, _ = sg.emul(case, rows, sim, vel, chunk_len=chunk_len)
        assert values.tobytes() == sh.value(case, rows, sim, vel, chunk_len=chunk_len).tobytes(), (model, free, n, chunk_len)


# The cells whose plain gradient loop rounds the residual otherwise than the value loop: the constant-rotation models with a
# free centre.  grad_term forms it as (v - v_sys) - (v_maxx sin - v_maxy cos) from the sine and cosine the derivatives need;
# the value path (free_centre_residual) as fma(-cross, 1 / r, v - v_sys).  The simulated term returns the value path's bits
# (test_value_field_has_the_value_loops_bits), so it cannot also return chunk_grad's there: on rows 0 .. 64 of the
# no-background cell chunk_grad's own value field differs from the value loop's by up to 9.1e-13 at 1027 stars.
RESIDUAL_ROUNDED_TWICE = {(0, True), (2, True)}


@pytest.mark.parametrize("model,free", [(m, f) for m, f in sg.CELLS if sh.eh.BG_OF[m] in (0, 2)])
def test_observed_velocities_give_the_plain_gradient_loops_bits(model, free):
    """With the observed velocities as the simulation the loop gives the value loop's bits in the value field and
    chunk_grad's bits in every field -- except in the two cells of RESIDUAL_ROUNDED_TWICE, where chunk_grad itself does not
    return the value loop's residual: there the value field is still the value loop's, bit for bit, and every gradient field
    agrees with chunk_grad's to the rounding of that residual, 1e-12 of the column's largest entry."""
    for n, chunk_len in ((33, 96), (1027, 96), (1027, 7)):
        case = sh.make_case(model, free, n)
        rows = [0, 1, 2, 64, 256]
        vel = np.stack([case["cat"]["v"], case["cat"]["v"] + 1.0])
        zero, one = np.zeros(len(rows), dtype=np.int64), np.ones(len(rows), dtype=np.int64)
        got_v, got_g = sg.emul(case, rows, zero, vel, chunk_len=chunk_len)
        plain_v, plain_g = sg.plain(case, rows, chunk_len=chunk_len)
        assert got_v.tobytes() == sh.plain_value(case, rows, chunk_len=chunk_len).tobytes(), (model, free, n, chunk_len)
        if (model, free) not in RESIDUAL_ROUNDED_TWICE:
            assert got_v.tobytes() == plain_v.tobytes() and got_g.tobytes() == plain_g.tobytes(), (model, free, n, chunk_len)
        else:
            assert np.all(np.abs(got_g - plain_g) <= 1e-12 * np.abs(plain_g).max(axis=0)), (model, free, n, chunk_len)
        other_v, other_g = sg.emul(case, rows, one, vel, chunk_len=chunk_len)
        assert not np.array_equal(other_v, plain_v) and not np.array_equal(other_g, plain_g)


# ------------------------------------------------------------------------------------------ 3. host logic on stand-ins
def _one_parameter_fit(monkeypatch):
    cols = hh.closed_form_columns()
    fit = sh.closed_form_fit(cols)                               # only v_sys free, N(0, 2^2)
    stub = sg.NumpyLinear(cols, ["v_sys"], prior_sd=sh.PRIOR_SD).attach(monkeypatch, fit)
    return fit, stub, cols


def test_simulated_maximize_reaches_the_closed_form_maxima(monkeypatch):
    fit, stub, cols = _one_parameter_fit(monkeypatch)
    truths = np.linspace(-3.0, 4.0, sg.N_E)[:, None]
    out = fit.simulated_maximize(truths, seed=sg.RUN_SEED, gtol=sg.GTOL)
    assert out["x"].shape == (sg.N_E, 1) and out["lnprob"].shape == out["converged"].shape == out["n_iter"].shape == (sg.N_E,)
    assert out["all_x"].shape == (sg.N_E, 1, 1) and out["all_lnprob"].shape == (sg.N_E, 1) and out["names"] == ["v_sys"]
    assert out["converged"].all() and out["seed"] == sg.RUN_SEED
    assert len(stub.simulate_calls) == 1 and np.array_equal(out["velocities"], sh.host_velocities(cols, truths, sg.RUN_SEED))
    mu, lam = sh.closed_form_posteriors(cols, out["velocities"])
    # the stopping rule, |g| scale <= gtol with scale = max(|x0|, 1) = 4, divided by the curvature; NumPy's own gradient
    # rounds at 1e-13 of sum |d_i / n_i| <= 200 x 0.4
    bound = (sg.GTOL / 4.0 + 1e-13 * 80.0) / lam.astype(float)
    err = np.abs(out["x"][:, 0] - mu.astype(float))
    print("largest |x - mu| %.3g (bound %.3g), iterations %d .. %d" % (err.max(), bound.min(), out["n_iter"].min(), out["n_iter"].max()))
    assert np.all(err <= bound)
    beta, value, _ = sg.least_squares(cols, ["v_sys"], out["velocities"], prior_sd=sh.PRIOR_SD)
    assert np.all(np.abs(out["lnprob"] - value.astype(float)) <= 1e-12 * np.abs(value.astype(float)))
    # every trial step is ONE call with all E rows, row e on simulation e
    assert all(c["rows"] == sg.N_E and np.array_equal(c["sim"], np.arange(sg.N_E)) for c in stub.calls)
    # the resident set, fitted again from one shared start, and the caller's own velocities
    n_sim = len(stub.simulate_calls)
    again = fit.simulated_maximize(x0=np.array([0.5]))
    assert len(stub.simulate_calls) == n_sim and "velocities" not in again and np.all(np.abs(again["x"][:, 0] - mu.astype(float)) <= bound)
    own = fit.simulated_maximize(velocities=out["velocities"][:5], x0=truths[:5])
    assert own["x"].shape == (5, 1) and np.all(np.abs(own["x"][:, 0] - mu.astype(float)[:5]) <= bound[:5])
    for bad in (dict(x0=np.zeros((3, 1))), dict(x0=np.zeros((5, 2, 2))), dict(x0=np.zeros(2))):
        with pytest.raises(ValueError):
            fit.simulated_maximize(velocities=out["velocities"][:5], **bad)
    with pytest.raises(ValueError):
        fit.simulated_maximize(velocities=out["velocities"][:5])              # no truths to start from
    with pytest.raises(ValueError):
        fit.simulated_maximize(np.array([[5000.0]]), seed=1)                  # a truth outside the box
    with pytest.raises(ValueError):
        fit.simulated_maximize(truths[:3], velocities=np.zeros((2, hh.N_STARS)))


def test_default_start_is_strictly_inside_the_box(monkeypatch):
    fit, stub, cols = _one_parameter_fit(monkeypatch)
    seen = []
    import mcmc_dynamics_amd.optimize as opt
    real = opt.maximize_batch

    def spy(value_and_grad, x0, lo, hi, **kw):
        seen.append(x0.copy())
        return real(value_and_grad, x0, lo, hi, **kw)
    monkeypatch.setattr(opt, "maximize_batch", spy)
    fit.simulated_maximize(np.array([[-1000.0], [1000.0], [0.25]]), seed=3)
    assert np.all(seen[0] > -1000.0) and np.all(seen[0] < 1000.0) and seen[0][2, 0] == 0.25


def test_best_of_s_selection(monkeypatch):
    """Per simulation the best CONVERGED start wins, whatever an unconverged one reached; the best of all where none
    converged; -inf and NaN values never win."""
    fit, stub, cols = _one_parameter_fit(monkeypatch)
    stub.simulated_set(np.zeros((3, hh.N_STARS)))
    f = np.array([[1.0, 5.0, 2.0], [3.0, 4.0, np.nan], [-np.inf, 2.0, 7.0]])
    conv = np.array([[True, False, True], [False, False, False], [True, True, False]])
    x = np.arange(9, dtype=float).reshape(9, 1)
    import mcmc_dynamics_amd.optimize as opt

    def fake(value_and_grad, x0, lo, hi, **kw):
        assert x0.shape == (9, 1)
        return {"x": x, "f": f.reshape(-1), "grad": np.zeros((9, 1)), "n_iter": np.arange(9), "converged": conv.reshape(-1), "n_calls": 1}
    monkeypatch.setattr(opt, "maximize_batch", fake)
    out = fit.simulated_maximize(x0=np.zeros((3, 3, 1)))
    assert out["x"][:, 0].tolist() == [2.0, 4.0, 7.0] and out["lnprob"].tolist() == [2.0, 4.0, 2.0]
    assert out["converged"].tolist() == [True, False, True] and out["n_iter"].tolist() == [2, 4, 7]
    assert out["all_lnprob"][1, 2] == -np.inf and out["all_converged"].tolist() == conv.tolist()


def test_parametric_bootstrap_summary_on_hand_made_arrays():
    x = np.array([[1.0, 10.0], [3.0, 14.0], [100.0, -100.0], [2.0, 12.0]])
    conv = np.array([True, True, False, True])
    with pytest.warns(UserWarning):
        s = parametric_bootstrap_summary(x, [1.5, 12.5], conv, ["a", "b"], laplace_covariance=np.diag([4.0, 1.0]))
    assert s["n_converged"] == 3 and s["n_sims"] == 4 and s["names"] == ["a", "b"] and "n_replicates" not in s
    assert np.allclose(s["mean"], [2.0, 12.0]) and np.allclose(s["bias"], [0.5, -0.5])
    assert np.allclose(s["covariance"], [[1.0, 2.0], [2.0, 4.0]]) and np.allclose(s["std"], [1.0, 2.0])
    assert np.allclose(s["std_ratio"], [0.5, 2.0]) and np.allclose(s["percentiles"][50.0], [2.0, 12.0])
    with pytest.raises(ValueError):
        parametric_bootstrap_summary(x, [1.0], conv, ["a"])


def test_lrt_summary_on_hand_made_arrays():
    from scipy import stats
    l0 = np.array([0.0, 0.0, 0.0, 0.0, 0.0, 0.0])
    l1 = np.array([0.5, 2.0, 1.0, 50.0, -1e-3, 0.25])
    c0 = np.array([True, True, True, True, True, False])
    c1 = np.array([True, True, True, False, True, True])
    with pytest.warns(UserWarning):                              # 4 of 6 used
        s = lrt_summary(l0, l1, c0, c1, stat_obs=2.0, df=1, tolerance=1e-6)
    assert np.array_equal(s["stat"], 2.0 * l1) and s["used"].tolist() == [True, True, True, False, True, False]
    assert s["n_used"] == 4 and s["n_sims"] == 6 and s["df"] == 1
    # used statistics 1, 4, 2, -2e-3: two are >= 2 -> (1 + 2) / (1 + 4); the unconverged 100 does not count
    assert s["p_value"] == 3.0 / 5.0 and np.isclose(s["p_se"], np.sqrt(0.6 * 0.4 / 5.0))
    assert np.isclose(s["p_asymptotic"], stats.chi2(1).sf(2.0), rtol=1e-12) and s["n_negative"] == 1
    assert np.isclose(s["quantiles"][50.0], np.percentile([1.0, 4.0, 2.0, -2e-3], 50.0)) and sorted(s["quantiles"]) == [50.0, 90.0, 95.0, 99.0, 99.9]
    assert lrt_summary(l0, l1, c0, c1, 2.0, 1, tolerance=1e-2)["n_negative"] == 0
    # no simulation reaches the observed statistic: 1 / (1 + n_used), never 0; df = 2 in the asymptotic tail
    big = lrt_summary(l0[:3], l1[:3], c0[:3], c1[:3], stat_obs=30.0, df=2)
    assert big["p_value"] == 0.25 and np.isclose(big["p_asymptotic"], np.exp(-15.0), rtol=1e-12)
    for bad in (dict(df=0), dict(lnprob_full=l1[:2])):
        with pytest.raises(ValueError):
            lrt_summary(**dict(dict(lnprob_null=l0, lnprob_full=l1, converged_null=c0, converged_full=c1, stat_obs=1.0, df=1), **bad))


def _lrt_pair(monkeypatch, cols=None):
    cols = hh.closed_form_columns() if cols is None else cols
    full, null = sg.lrt_fits(cols)
    stubs = (sg.NumpyLinear(cols, ["v_sys", "v_maxx"]).attach(monkeypatch, full), sg.NumpyLinear(cols, ["v_sys"]).attach(monkeypatch, null))
    return full, null, stubs, cols


def test_every_refusal_of_lrt():
    from mcmc_dynamics_amd.analysis import ConstantFit
    cols = hh.closed_form_columns()
    full, null = sg.lrt_fits(cols)

    class Other(ConstantFit):
        pass
    other = Other(full.data)
    with pytest.raises(ValueError, match="null fit is a"):
        full.lrt(other)
    with pytest.raises(ValueError, match="same class"):
        full.lrt("null")
    fewer = sg.lrt_fits({k: v[:150] for k, v in cols.items()})[1]
    with pytest.raises(ValueError, match="150 stars"):
        full.lrt(fewer)
    moved = sg.lrt_fits(dict(cols, v=cols["v"] + 1.0))[1]
    with pytest.raises(ValueError, match="data column 'v'"):
        full.lrt(moved)
    with pytest.raises(ValueError, match="'v_maxx' is free in the null fit"):
        null.lrt(full)
    with pytest.raises(ValueError, match="fixes no parameter"):
        full.lrt(sg.lrt_fits(cols)[0])
    outside = sg.lrt_fits(cols)[1]
    outside.parameters["v_maxx"].set(value=5000.0)
    with pytest.raises(ValueError, match="outside this fit's box"):
        full.lrt(outside)
    differs = sg.lrt_fits(cols)[1]
    differs.parameters["sigma_max"].set(value=hh.SIGMA + 1.0)
    with pytest.raises(ValueError, match="'sigma_max' is fixed at"):
        full.lrt(differs)
    with pytest.raises(ValueError, match="n_sims"):
        full.lrt(null, n_sims=0)


def test_lrt_on_the_linear_stand_in_sizes_the_gpu_run(monkeypatch):
    """Runner.lrt around the NumPy stand-ins with the run of tests/test_gpu_simulated_grad.py: 64 catalogues of 200 stars
    drawn under the null, seed 20261024.  Every statistic against its weighted-least-squares closed form in longdouble.
    What the optimiser's stopping rule leaves of a maximum, g' A^-1 g <= P gtol^2 / lambda_min(A) (its scale is >= 1, so
    every |g_j| <= gtol), summed over the two fits, is 2.4e-16 here: nothing beside the 4e-12 max(|lnL|, N) = 3.1e-9 of the
    value rule, to which the GPU test adds it.  Recorded on this run: largest |stat - exact| 1.7e-12, 4 .. 6 iterations per
    fit, stat_obs 0.881 with p_value 0.369, null quantiles 50 % 0.42, 90 % 2.19, 95 % 2.98 against chi2(1)'s 0.45, 2.71,
    3.84 (64 draws).  The test prints the run's figures."""
    full, null, (stub1, stub0), cols = _lrt_pair(monkeypatch)
    out = full.lrt(null, n_sims=sg.N_E, seed=sg.RUN_SEED, gtol=sg.GTOL)
    assert out["used"].all() and out["n_used"] == sg.N_E and out["df"] == 1 and out["seed"] == sg.RUN_SEED and out["n_negative"] == 0
    # the sets: drawn once, by the null at its own maximum, and handed to the full fit
    assert len(stub0.simulate_calls) == 1 and len(stub1.simulate_calls) == 0
    assert np.array_equal(stub0.simulate_calls[0]["truths"], np.tile(out["x_null"], (sg.N_E, 1)))
    assert np.array_equal(stub1.velocities, out["velocities"]) and np.array_equal(stub0.velocities, out["velocities"])
    # two starts per simulation in the full fit: the embedded null maximum and the full maximum
    assert out["fits_full"]["all_x"].shape == (sg.N_E, 2, 2) and out["fits_null"]["all_x"].shape == (sg.N_E, 1, 1)
    assert all(c["rows"] == 2 * sg.N_E and np.array_equal(c["sim"], np.repeat(np.arange(sg.N_E), 2)) for c in stub1.calls)
    b1, f1, a1 = sg.least_squares(cols, ["v_sys", "v_maxx"], out["velocities"])
    b0, f0, a0 = sg.least_squares(cols, ["v_sys"], out["velocities"])
    exact = (2 * (f1 - f0)).astype(float)
    o1, g1, _ = sg.least_squares(cols, ["v_sys", "v_maxx"], cols["v"][None, :])
    o0, g0, _ = sg.least_squares(cols, ["v_sys"], cols["v"][None, :])
    room = sg.optimiser_room(a1.astype(float), np.ones(2)) + sg.optimiser_room(a0.astype(float), np.ones(1))
    bound = 4e-12 * max(float(np.abs(f1).max()), float(np.abs(f0).max()), hh.N_STARS) + room
    err = np.abs(out["stat"] - exact)
    print("largest |stat - exact| %.3g (bound %.3g, of which the optimiser's %.3g), iterations %d .. %d, stat_obs %.6g, p %.4f, "
          "quantiles %s" % (err.max(), bound, room, out["fits_full"]["n_iter"].min(), out["fits_full"]["n_iter"].max(), out["stat_obs"],
                            out["p_value"], {q: round(v, 3) for q, v in out["quantiles"].items()}))
    assert room < 1e-12 and np.all(err <= bound)
    assert abs(out["stat_obs"] - float(2 * (g1[0] - g0[0]))) <= bound
    assert np.all(np.abs(out["x_full"] - o1[0].astype(float)) <= 1e-6) and np.all(np.abs(out["x_null"] - o0[0].astype(float)) <= 1e-6)
    want_p = (1.0 + np.count_nonzero(exact >= float(2 * (g1[0] - g0[0])))) / (1.0 + sg.N_E)
    assert out["p_value"] == want_p
    assert out["tolerance"] == 4e-12 * max(np.abs(out["fits_null"]["lnprob"]).max(), np.abs(out["fits_full"]["lnprob"]).max(), hh.N_STARS)


def test_parametric_bootstrap_on_the_stand_in(monkeypatch):
    fit, stub, cols = _one_parameter_fit(monkeypatch)
    monkeypatch.setattr(fit, "laplace", lambda x: {"covariance": np.array([[1.0 / float(sh.closed_form_posteriors(cols, cols["v"][None, :])[1][0])]])})
    out = fit.parametric_bootstrap(n_sims=256, seed=5)
    assert out["n_sims"] == 256 and out["n_converged"] == 256 and out["x"].shape == (256, 1) and out["seed"] == 5
    assert np.array_equal(stub.simulate_calls[-1]["truths"], np.tile(out["x_hat"], (256, 1)))
    # the estimator is mu = sum(v / n) / Lambda with v ~ N(x_hat, n): variance (Lambda - 1/4) / Lambda^2, a shade below the
    # Laplace 1 / Lambda, and bias -x_hat / (4 Lambda) from the prior's pull
    lam = float(sh.closed_form_posteriors(cols, cols["v"][None, :])[1][0])
    want_std = np.sqrt((lam - 0.25) / lam ** 2)
    assert abs(out["std"][0] / want_std - 1.0) < 5.0 / np.sqrt(2 * 256) and abs(out["std_ratio"][0] - want_std * np.sqrt(lam)) < 0.25
    assert abs(out["bias"][0] + out["x_hat"][0] / (4.0 * lam)) < 5.0 * want_std / np.sqrt(256)
    again = fit.parametric_bootstrap(n_sims=256, seed=5, x_hat=out["x_hat"])
    assert again["x"].tobytes() == out["x"].tobytes()
    with pytest.raises(ValueError):
        fit.parametric_bootstrap(n_sims=0)
    with pytest.raises(ValueError):
        fit.parametric_bootstrap(n_sims=4, x_hat=[1.0, 2.0])


def test_binned_fit_raises():
    from mcmc_dynamics_amd import DataReader, synthetic
    from mcmc_dynamics_amd.analysis import BinnedConstantFit
    c = synthetic.make_catalog(120, config=2, background=False)
    data = DataReader({k: c[k] for k in ("ra", "dec", "v", "verr")})
    data.make_radial_bins(synthetic.CENTER_RA_DEG, synthetic.CENTER_DEC_DEG, nstars=40)
    fit = BinnedConstantFit(data)
    for call in (lambda: fit.simulated_maximize(np.zeros((1, 1)), seed=1), lambda: fit.parametric_bootstrap(n_sims=2, x_hat=[0.0]),
                 lambda: fit.lnprob_simulated_grad_batch(np.zeros((1, 1)), [0]), lambda: fit.lrt(fit)):
        with pytest.raises(NotImplementedError):
            call()


# ------------------------------------------------------------------------------------------ 4. resources
def _committed():
    with open(os.path.join(ROOT, "profiles", "simulated_grad_resources.json")) as fh:
        return json.load(fh)["rows"]


def test_no_simulated_grad_kernel_uses_scratch_or_lds():
    rows = _committed()
    assert len(rows) == 18
    assert {(r["kernel"], r["model_id"], r["free_centre"]) for r in rows} == \
        {("simulated_grad", m, f) for m in range(9) for f in (False, True)}
    for r in rows:
        assert r["scratch_bytes_per_lane"] == 0 and r["vgpr_spill"] == 0 and r["lds_bytes"] == 0, r


def test_resource_report_is_what_the_compiler_says_today():
    """The committed JSON against a fresh run of tools/simulated_grad_resources.py (hipcc for gfx950; no device needed)."""
    import shutil
    import sys
    if shutil.which("hipcc") is None:
        pytest.skip("no hipcc on this machine")
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import simulated_grad_resources
    assert simulated_grad_resources.analyse() == _committed()


def test_the_plain_gradient_loop_rounds_a_free_constant_residual_otherwise():
    """Why RESIDUAL_ROUNDED_TWICE exists: chunk_grad's own value field is not the value loop's there."""
    case = sh.make_case(0, True, 1027)
    rows = list(range(65))
    assert sg.plain(case, rows)[0].tobytes() != sh.plain_value(case, rows).tobytes()
    case = sh.make_case(0, False, 1027)
    assert sg.plain(case, rows)[0].tobytes() == sh.plain_value(case, rows).tobytes()

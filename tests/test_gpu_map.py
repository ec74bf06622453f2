"""GPU: the first-order methods of Runner on the device gradient -- lnprob_grad_batch (host chain rule, prior handling,
refusal of constrained parameters), maximize (MAP) and laplace.

The MAP fits use a 2 000-star synthetic catalogue with the centre fixed and the 64 starts of get_initials under seed 13.
That seed was checked beforehand on the CPU (float64 oracle value + the test-side gradient through maximize_batch, gtol =
1e-8 on the scaled projected gradient): 64 of 64 starts converge for ConstantFit, 41 of 64 for ConstantFitGB -- the rest run
away on the all-background plateau f_back = 1, where the cluster component turns into a second, ever broader background
and the likelihood has no maximum.  (Seeds 1, 2, 3, 7, 11, 12 gave 34, 41, 34, 33, 39, 37 for ConstantFitGB.)"""
import numpy as np
import pytest

import grad_helper as gh
import variant_helper as vh

pytestmark = pytest.mark.gpu
L = vh.L
SEED = 13


def _fit(kind):
    from mcmc_dynamics_amd import DataReader, synthetic
    from mcmc_dynamics_amd.analysis import ConstantFit, ConstantFitGB
    bg = kind == "gb"
    cat = synthetic.make_catalog(2000, config=2, background=bg)
    cols = ("ra", "dec", "v", "verr") + (("density",) if bg else ())
    fit = (ConstantFitGB if bg else ConstantFit)(DataReader({k: cat[k] for k in cols}), seed=SEED)
    # the `initials` recipes draw from the parameter set's own generator, which a default set seeds from the system's
    # entropy: without this line every process had other starts (11 .. 63 of 64 converged from run to run for ConstantFit)
    fit.parameters.rng.bit_generator.state = np.random.default_rng(SEED).bit_generator.state
    centre = (synthetic.CENTER_RA_DEG, synthetic.CENTER_DEC_DEG)
    fit.parameters["ra_center"].set(value=centre[0], fixed=True)
    fit.parameters["dec_center"].set(value=centre[1], fixed=True)
    truth = np.array([cat["truth"][n] for n in fit.fitted_parameters])
    return fit, {k: cat[k] for k in cols}, centre, truth, (2 if bg else 0)


_FITS = {}


def fitted(kind):
    """(fit, catalogue columns, centre, truth, model id, maximize() result), one fit per kind for the whole module."""
    if kind not in _FITS:
        fit, cat, centre, truth, model = _fit(kind)
        _FITS[kind] = (fit, cat, centre, truth, model, fit.maximize(n_starts=64, max_iter=200, gtol=1e-8))
    return _FITS[kind]


@pytest.mark.parametrize("kind", ["constant", "gb"])
def test_map_fit(kind):
    fit, cat, centre, truth, model, res = fitted(kind)
    print(kind, "converged", int(res["all_converged"].sum()), "of 64; x =", res["x"], "lnprob", res["lnprob"])
    assert res["all_converged"].sum() >= 32 and res["converged"]
    assert res["all_x"].shape == (64, truth.size) and res["all_lnprob"].shape == (64,)
    assert res["lnprob"] >= fit.lnprob_batch(truth[None])[0]
    assert res["lnprob"] == fit.lnprob_batch(res["x"][None])[0] or \
        abs(res["lnprob"] - fit.lnprob_batch(res["x"][None])[0]) < 1e-12 * 2000
    value, grad = fit.lnprob_grad_batch(res["x"][None])
    _, s = gh.grad(model, cat, res["x"], centre, L)                   # (every column free: x is the kernel row)
    print(kind, "|grad| / S_k =", np.abs(grad[0] / s.astype(np.float64)))
    assert np.all(np.abs(grad[0]) <= 1e-6 * s.astype(np.float64))


@pytest.mark.parametrize("kind", ["constant", "gb"])
def test_laplace(kind):
    fit, cat, centre, truth, model, res = fitted(kind)
    x = res["x"]
    lap = fit.laplace(x)
    hess = lap["hessian"]
    assert np.array_equal(hess, hess.T)
    assert np.all(np.linalg.eigvalsh(-hess) > 0)
    assert np.allclose(lap["covariance"] @ (-hess), np.eye(x.size), atol=1e-8)
    # the same Hessian from central differences of the longdouble test-side gradient
    want = np.empty((x.size, x.size), dtype=L)
    for j in range(x.size):
        h = L(1e-4) * max(abs(x[j]), 1e-3)
        up, dn = x.astype(L), x.astype(L)
        up[j] += h
        dn[j] -= h
        want[j] = (gh.grad(model, cat, up, centre, L)[0] - gh.grad(model, cat, dn, centre, L)[0]) / (up[j] - dn[j])
    want = (0.5 * (want + want.T)).astype(np.float64)
    scale = np.sqrt(np.outer(np.diag(hess), np.diag(hess)))
    err = np.abs(hess - want) / scale
    print(kind, "Hessian: worst |device - exact| / sqrt(H_jj H_kk) =", err.max())
    assert err.max() < 1e-5
    ball = fit.get_initials_laplace(32, x, lap["covariance"])
    assert ball.shape == (32, x.size) and np.all(np.isfinite(fit.lnprob_batch(ball)))
    sd = np.sqrt(np.diag(lap["covariance"]))
    assert np.all(np.abs(ball - x) < 8 * sd)
    with pytest.raises(ValueError):
        fit.laplace(truth + 100 * sd)                                  # far from the maximum in every direction: -H indefinite or ...
    lo = fit._plan().lo[fit._plan().free_idx]
    on_bound = x.copy()
    on_bound[1] = lo[1]                                                # sigma_max = 0: on the bound
    with pytest.raises(ValueError, match="bound"):
        fit.laplace(on_bound)


def _model_fit():
    """ModelFit with the centre and r_peak fixed (a fixed parameter feeds a kernel column) and `a` in arcmin."""
    from mcmc_dynamics_amd import DataReader
    from mcmc_dynamics_amd.analysis import ModelFit
    from mcmc_dynamics_amd.analysis import model as model_module
    from mcmc_dynamics_amd.parameter import Parameter, Parameters
    case = vh.make_case(3, False, 500)
    pars = Parameters()
    for name in model_module._MODEL_ORDER:
        n, unit, lo, hi, label, initials = model_module._ROW[name]
        pars.add(Parameter(n, unit="arcmin" if name == "a" else unit, min=lo, max=hi, label=label, initials=initials))
    fit = ModelFit(DataReader({k: case["cat"][k] for k in ("ra", "dec", "v", "verr")}), parameters=pars, seed=SEED)
    fit.parameters["ra_center"].set(value=vh.CENTRE[0], fixed=True)
    fit.parameters["dec_center"].set(value=vh.CENTRE[1], fixed=True)
    fit.parameters["r_peak"].set(value=40.0, fixed=True)
    return fit, case


def test_host_chain_rule_with_a_fixed_column_and_a_unit_factor():
    fit, case = _model_fit()
    assert fit.fitted_parameters == ["v_sys", "sigma_max", "a", "v_maxx", "v_maxy"]
    rows = case["params"][:9, :5].copy()                               # C-ABI head: v_sys, sigma_max, a [arcsec], v_maxx, v_maxy
    values = rows.copy()
    values[:, 2] = rows[:, 2] / 60.0                                   # the sampler's vector carries a in arcmin
    value, grad = fit.lnprob_grad_batch(values)
    table = np.column_stack([rows, np.full(len(rows), 40.0)])          # ... the kernel's table a in arcsec and the fixed r_peak
    raw_value, raw_grad = fit._catalog.loglike_grad(table)
    assert np.array_equal(value, raw_value)
    want = raw_grad[:, :5].copy()                                      # the r_peak column is dropped
    want[:, 2] *= 60.0                                                 # d a[arcsec] / d a[arcmin]
    assert np.array_equal(grad, want)
    assert np.all(raw_grad[:, 5] != 0.0)
    # and it is the derivative of what lnprob_batch returns: central difference in a [arcmin].  h = 1e-3 a: truncation
    # ~h^2 |third derivative| / 6 ~ 1e-6 of the derivative's scale, round-off ~1e-13 |lnL| / h ~ 1e-6 -- both inside 1e-4
    h = 1e-3 * values[0, 2]
    up, dn = values[:1].copy(), values[:1].copy()
    up[0, 2] += h
    dn[0, 2] -= h
    fd = (fit.lnprob_batch(up)[0] - fit.lnprob_batch(dn)[0]) / (up[0, 2] - dn[0, 2])
    assert abs(fd - grad[0, 2]) < 1e-4 * max(abs(grad[0, 2]), 1.0)


def test_rows_outside_the_prior():
    fit, case = _model_fit()
    values = case["params"][:6, :5].copy()
    values[:, 2] /= 60.0
    values[1, 1] = -1.0                                                # sigma_max < 0
    values[4, 2] = -0.5                                                # a < 0
    value, grad = fit.lnprob_grad_batch(values)
    inside = np.array([True, False, True, True, False, True])
    assert np.all(np.isneginf(value[~inside])) and np.all(grad[~inside] == 0.0)
    assert np.all(np.isfinite(value[inside])) and np.all(np.any(grad[inside] != 0.0, axis=1))
    assert np.array_equal(value, fit.lnprob_batch(values)) or np.all(vh.scaled_err(value[inside], fit.lnprob_batch(values)[inside], 500) < 1e-12)
    value, grad = fit.lnprob_grad_batch(values[[1, 4]])                # no row inside: nothing is launched
    assert np.all(np.isneginf(value)) and np.all(grad == 0.0)


def test_constrained_parameter_is_refused():
    fit, case = _model_fit()
    fit.parameters["v_maxy"].set(expr="v_maxx * 0.5 - 1.0")
    with pytest.raises(NotImplementedError, match="v_maxy"):
        fit.lnprob_grad_batch(case["params"][:2, :4])
    with pytest.raises(NotImplementedError, match="v_maxy"):
        fit.maximize(n_starts=4)

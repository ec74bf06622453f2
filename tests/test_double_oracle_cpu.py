"""The test-side restatement of the double Lynden-Bell models (tests/double_helper.py) against the reference.

* float64 restatement vs the four golden vectors (tools/make_golden_double.py: the reference's own rotation_model twice,
  its dispersion, likelihood, priors): 1e-13 relative, as test_oracle_golden.py pins the ModelFit family (NumPy 2.2 here
  against NumPy 1.26 there differ in SIMD sin / cos / log by an ulp); per-star membership of the GB goldens 1e-13 absolute.
* zero second amplitudes: the restatement IS the oracle's ModelFit / ModelFitGB value, 1e-15 relative.
* the longdouble gradient against central differences of the longdouble value, by the rule of test_grad_oracle_cpu.py:
  two steps h = 1e-4 x column scale and h / 2, |g - FD(h/2)| <= 4 |FD(h) - FD(h/2)| + 1e-9 S_k."""
import os

import numpy as np
import pytest

import double_helper as dh
import variant_helper as vh
from oracle import lnprob_numpy as oracle

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CASES = {"double_model": (dh.DOUBLE, False), "double_model_free": (dh.DOUBLE, True),
         "double_model_gb": (dh.DOUBLE_GB, False), "double_model_gb_free": (dh.DOUBLE_GB, True)}
L = vh.L


def load(name):
    g = dict(np.load(os.path.join(GOLDEN, name + ".npz"), allow_pickle=False))
    model, free = CASES[name]
    cat = {k: g[k] for k in ("ra", "dec", "v", "verr", "density") if k in g}
    centre = None if free else (float(g["ra_center"]), float(g["dec_center"]))
    return g, model, free, cat, centre, dh.abi_columns(g["names"], g["values"], model, free)


@pytest.mark.parametrize("name", sorted(CASES))
def test_float64_restatement_matches_the_goldens(name):
    g, model, free, cat, centre, table = load(name)
    ok = np.isfinite(g["lnprob"])
    assert np.array_equal(ok, np.isfinite(g["lnprior"]))
    assert g["values"].shape[0] == 24 and len(cat["v"]) == 1500 and ok.sum() >= 16 and (~ok).sum() >= 4
    got = np.array([dh.value(model, cat, row, centre) for row in table[ok]])
    want = g["lnprob"][ok] - g["lnprior"][ok]
    assert np.max(np.abs(got - want) / np.abs(want)) <= 1e-13
    # the rejected rows are outside the box this package gives the parameters (analysis/double_model.py)
    names = [str(n) for n in g["names"]]
    lo = {"sigma_max": 0.0, "a": 0.0, "r_peak": 0.0, "v_maxx_c": -50.0, "v_maxy_c": -50.0, "r_peak_ratio": 1e-3,
          "sigma_back": 0.0, "f_back": 0.0, "ra_center": 0.0, "dec_center": -90.0}
    hi = {"v_maxx_c": 50.0, "v_maxy_c": 50.0, "r_peak_ratio": 1.0, "f_back": 1.0, "ra_center": 360.0, "dec_center": 90.0}
    inside = np.array([all(lo.get(n, -np.inf) <= x <= hi.get(n, np.inf) for n, x in zip(names, row)) for row in g["values"]])
    assert np.array_equal(inside, ok)


@pytest.mark.parametrize("name", ["double_model_gb", "double_model_gb_free"])
def test_membership_matches_the_goldens(name):
    g, model, free, cat, centre, table = load(name)
    for i, want in zip(g["membership_rows"].astype(int), g["membership"]):
        got = dh.per_star(model, cat, table[i], centre, np.float64)[1]
        assert np.max(np.abs(got - want)) <= 1e-13


@pytest.mark.parametrize("free", [False, True])
@pytest.mark.parametrize("model", dh.MODELS)
def test_zero_second_amplitudes_are_the_single_component_oracle(model, free):
    case = dh.make_case(model, free, 4099)
    rows, base_rows = dh.nested_rows(case["params"][:8])
    for row, base in zip(rows, base_rows):
        got = dh.value(model, case["cat"], row, case["centre"])
        want = vh.value(dh.BASE[model], case["cat"], base, case["centre"])
        assert abs(got - want) <= 1e-15 * abs(want)


@pytest.mark.skipif(not vh.HAVE_LONGDOUBLE, reason="numpy.longdouble is not wider than float64 here")
@pytest.mark.parametrize("free", [False, True])
@pytest.mark.parametrize("model", dh.MODELS)
def test_gradient_matches_differences_of_the_value(model, free):
    case = dh.make_case(model, free, 33)
    for w in (0, 3):
        row = case["params"][w].astype(L)
        g, s = dh.grad(model, case["cat"], row, case["centre"], L)
        scales = dh.column_scales(model, free, case["params"][w], case["scale"])
        for k in range(len(row)):
            fd = []
            for h in (L(1e-4) * L(scales[k]), L(0.5e-4) * L(scales[k])):
                up, dn = row.copy(), row.copy()
                up[k] += h
                dn[k] -= h
                fd.append((dh.value(model, case["cat"], up, case["centre"], L) -
                           dh.value(model, case["cat"], dn, case["centre"], L)) / (2 * h))
            assert abs(g[k] - fd[1]) <= 4 * abs(fd[0] - fd[1]) + L(1e-9) * s[k], (model, free, w, k)


@pytest.mark.skipif(not vh.HAVE_LONGDOUBLE, reason="numpy.longdouble is not wider than float64 here")
def test_float64_run_tracks_the_longdouble_run():
    case = dh.make_case(dh.DOUBLE_GB, True, 4099)
    ref = dh.reference(case, 1)
    assert np.all(ref["err64"] < 1e-9)
    v64 = dh.value(dh.DOUBLE_GB, case["cat"], case["params"][1], case["centre"])
    assert vh.scaled_err(v64, ref["value"], 4099) < 1e-12

"""The test-side gradient (tests/grad_helper.py) against central differences of the 80-bit value oracle
(variant_helper.exact), for every model x {fixed, free centre}.

Two step sizes, h = 1e-4 x column scale and h / 2.  The bound is
    |g - FD(h/2)| <= 4 |FD(h) - FD(h/2)| + 1e-9 S_k:
the first term is the truncation error the differences themselves exhibit (FD(h) - FD(h/2) is 3/4 of the h^2 term, of
which FD(h/2) keeps 1/4), the second is far above the 80-bit round-off of a difference, ~1e-19 sum |lnL_i| / h."""
import numpy as np
import pytest

import grad_bounds as gb
import grad_helper as gh
import variant_helper as vh

pytestmark = pytest.mark.skipif(not vh.HAVE_LONGDOUBLE, reason="numpy.longdouble is not wider than float64 here")
L = vh.L


def central(model, cat, row, centre, k, h):
    up, dn = np.array(row, dtype=L), np.array(row, dtype=L)
    up[k] += L(h)
    dn[k] -= L(h)
    return (vh.exact(model, cat, up, centre) - vh.exact(model, cat, dn, centre)) / (up[k] - dn[k])


@pytest.mark.parametrize("free", [False, True])
@pytest.mark.parametrize("model", range(7))
def test_helper_gradient_matches_differences_of_the_oracle(model, free):
    case = vh.make_case(model, free, 33)
    for w in (0, 3):
        row = case["params"][w]
        g, s = gh.grad(model, case["cat"], row, case["centre"], L)
        scales = gh.column_scales(model, free, row, case["scale"])
        for k, name in enumerate(gh.column_names(model, free)):
            h = 1e-4 * scales[k]
            fd1, fd2 = central(model, case["cat"], row, case["centre"], k, h), central(model, case["cat"], row, case["centre"], k, h / 2)
            bound = 4 * abs(fd1 - fd2) + L(1e-9) * s[k]
            print(model, free, w, name, float(g[k]), float(abs(g[k] - fd2)), float(bound))
            assert abs(g[k] - fd2) <= bound, (model, free, w, name, float(g[k]), float(fd2), float(bound))


def test_float64_run_tracks_the_longdouble_run():
    case = vh.make_case(4, True, 33)
    g64, _ = gh.grad(4, case["cat"], case["params"][0], None, np.float64)
    g80, s80 = gh.grad(4, case["cat"], case["params"][0], None, L)
    assert g64.dtype == np.float64 and g80.dtype == L
    assert np.all(gh.col_err(g64, g80, s80) < 1e-9)


@pytest.mark.parametrize("model,free", [(1, False), (4, True)])
def test_prefix_reference_is_the_reference_of_the_sliced_catalogue(model, free):
    """grad_bounds.prefix_reference serves every prefix catalogue from one evaluation of the term matrix: at two prefix
    lengths (one of them no multiple of numpy's pairwise-summation blocks) it gives the gradient, S_k and err_np64 of
    grad_bounds.reference on the sliced catalogue, exactly."""
    case = vh.make_case(model, free, 4099)
    lengths = (51, 2611)
    for w in (0, 3):
        got = gb.prefix_reference(case, w, lengths + (4099,))
        assert sorted(got) == [51, 2611, 4099]
        for n in lengths:
            want = gb.reference(gb.sub_case(case, slice(0, n)), w)
            assert got[n]["g"].dtype == L and got[n]["s"].dtype == L
            for key in ("g", "s", "err64"):
                assert np.array_equal(got[n][key], want[key]), (model, free, w, n, key)
        whole = gb.reference(case, w)
        assert np.array_equal(got[4099]["g"], whole["g"]) and np.array_equal(got[4099]["s"], whole["s"])

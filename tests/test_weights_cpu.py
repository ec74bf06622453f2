"""CPU: the star weights of the weighted-likelihood bootstrap (csrc/mcd_weights.h) and the weighted gradient loop
(csrc/mcd_weighted.h through tests/emul/weighted_emul.cpp).

  1. the generator: mcd_bootstrap_weights (host code of the library) against numpy.random.Philox with key
     (seed, kWeightKey1) and counter (star >> 2, replicate, 0, 0); exponential weights against -log(u) to 4 ulp (det_log is
     good to ~2 ulp); Poisson weights against numpy.searchsorted on the header's literals, and their mean and variance
     over 2e5 draws within 5 standard errors of 1 (Poisson(1): Var = 1, fourth central moment 4, so the sample variance
     has variance (4 - 1) / n); any window of a larger table holds the same numbers;
  2. the loop against sum_i w_i t_i in longdouble under the rule of tests/weighted_helper.py, 7 models x {fixed, free} x
     N in {1, 33, 4099} x rows in {1, 65, 257}, both generated schemes and explicit weights, with a non-monotone replicate
     map that repeats and holds one id of 2^40;
  3. the zero-weight rule on a star whose term is -inf;
  4. chunk-start independence: chunks of 5 and of 7 stars see the weights of the generator's table, recovered one star at
     a time, bit for bit."""
import numpy as np
import pytest

import double_helper as dh
import grad_bounds as gb
import variant_helper as vh
import weighted_helper as wh
from mcmc_dynamics_amd import _native

SEEDS = np.random.default_rng(11).integers(0, 2 ** 63, 6)
REPLICATES = (0, 1, 77, 1 << 40)
STAR_WINDOWS = ((0, 10), ((1 << 32) + 5, 7))


# ------------------------------------------------------------------------------------------ 1. generator
def test_key_names_this_use_of_the_generator():
    assert wh.lib().emul_weight_key() == int.from_bytes(b"mcd_wgh", "big")


def test_words_and_weights_match_numpys_philox():
    c = wh.poisson_thresholds()
    for seed in SEEDS:
        for rep in REPLICATES:
            for star0, n in STAR_WINDOWS:
                u = wh.numpy_uniforms(seed, rep, star0, n)
                assert np.all(u > 0.0) and np.all(u < 1.0)
                expo = _native.bootstrap_weights("exponential", seed, rep, 1, star0, n)[0]
                want = -np.log(u.astype(np.longdouble))
                assert np.all(np.isfinite(expo)) and np.all(expo > 0.0)
                assert np.all(np.abs(expo - want) <= 4 * np.spacing(want.astype(np.float64)))
                pois = _native.bootstrap_weights("poisson", seed, rep, 1, star0, n)[0]
                assert np.array_equal(pois, np.searchsorted(c, u, side="right").astype(np.float64))


def test_library_weights_are_the_emulated_ones():
    for scheme in ("exponential", "poisson"):
        assert np.array_equal(_native.bootstrap_weights(scheme, 987654321, 3, 5, 6, 29), wh.weights(scheme, 987654321, 3, 5, 6, 29))


def test_poisson_literals_are_the_cumulative_probabilities():
    from math import factorial
    c = wh.poisson_thresholds()
    assert c[-1] == 1.0 and np.all(c[:-1] < 1.0) and np.all(np.diff(c) >= 0)
    L = np.longdouble
    exact = np.cumsum([L(1) / L(factorial(m)) for m in range(c.size)]) / np.exp(L(1))
    assert np.all(np.abs(c - exact) <= 0.5000001 * np.spacing(c))


def test_poisson_count_at_every_threshold():
    """Head, gate and tail of the count: at each literal, one ulp below it and one above, and on a grid."""
    c = wh.poisson_thresholds()
    u = np.concatenate([c, np.nextafter(c, 0.0), np.nextafter(c[:-1], 2.0), np.linspace(2.0 ** -54, 1.0, 4001)])
    assert np.array_equal(wh.poisson_count(u), np.searchsorted(c, u, side="right").astype(np.float64))
    assert wh.poisson_count([1.0])[0] == c.size == 19


def test_poisson_moments_over_2e5_draws():
    w = _native.bootstrap_weights("poisson", 20261020, 0, 200, 0, 1000)
    n = float(w.size)
    assert n == 2e5 and np.array_equal(w, np.round(w)) and w.min() == 0.0
    print("poisson mean", w.mean(), "variance", w.var(ddof=1))
    assert abs(w.mean() - 1.0) <= 5.0 * np.sqrt(1.0 / n)
    assert abs(w.var(ddof=1) - 1.0) <= 5.0 * np.sqrt(3.0 / n)


def test_exponential_moments_over_2e5_draws():
    w = _native.bootstrap_weights("exponential", 20261020, 0, 200, 0, 1000)
    n = float(w.size)
    # Exp(1): Var = 1; the sample variance has variance (mu4 - 1) / n = 8 / n
    assert abs(w.mean() - 1.0) <= 5.0 * np.sqrt(1.0 / n)
    assert abs(w.var(ddof=1) - 1.0) <= 5.0 * np.sqrt(8.0 / n)


@pytest.mark.parametrize("scheme", ["exponential", "poisson"])
def test_window_independence(scheme):
    big = _native.bootstrap_weights(scheme, 5150, 0, 9, 0, 40)
    for rep0 in (0, 2, 7):
        for star0 in (0, 1, 2, 3, 5):
            assert np.array_equal(_native.bootstrap_weights(scheme, 5150, rep0, 2, star0, 11), big[rep0:rep0 + 2, star0:star0 + 11])


def test_host_entry_refuses_bad_arguments():
    lib = _native.load_library()
    w = np.full(4, -7.25)
    for args in ((2, 1, 0, 2, 0, 2), (7, 1, 0, 2, 0, 2), (0, 1, -1, 2, 0, 2), (0, 1, 0, 2, -1, 2)):
        assert lib.mcd_bootstrap_weights(*args, _native._ptr(w)) == -1
        assert np.all(w == -7.25)


# ------------------------------------------------------------------------------------------ 2. the loop
needs_longdouble = pytest.mark.skipif(not vh.HAVE_LONGDOUBLE, reason="numpy.longdouble is not wider than float64 here")


def _check_cell(model, free, n, n_rows, scheme):
    case = dh.make_case(model, free, n) if model in dh.MODELS else vh.make_case(model, free, n)
    rows = list(range(n_rows))
    rep = wh.row_replicates(n_rows) if n_rows > 1 else np.array([3], dtype=np.int64)
    explicit = None
    if scheme == "explicit":
        # five replicates of weights with exact zeros, integers and fractions; the 2^40 id is mapped into the table
        rep = rep % 5
        explicit = np.random.default_rng(n + n_rows).choice([0.0, 0.0, 1.0, 2.0, 0.375, 1.625], size=(5, n))
        w_rows = explicit[rep]
    else:
        w_rows = wh.weights_of_rows(scheme, wh.SEED, rep, n)
    value, grad = wh.emul_weighted(case, rows, rep, scheme, explicit=explicit)
    floors = dh.floors(model, free, n) if model in dh.MODELS else gb.floors(model, free, n)
    worst = 0.0
    for j in vh.sample_rows(n_rows):                            # the longdouble reference costs: a sample of the rows
        ref = wh.reference(model, case["cat"], case["params"][j], case["centre"], w_rows[j])
        worst = max(worst, wh.check_row(value[j], grad[j], ref, (model, free, n, n_rows, scheme, j), floors)[1])
    return worst


@needs_longdouble
@pytest.mark.parametrize("free", [False, True])
@pytest.mark.parametrize("model", range(7))
def test_emulation_follows_the_rule(model, free):
    for n in (1, 33, 4099):
        for n_rows in (1, 65, 257):
            for scheme in ("exponential", "poisson", "explicit"):
                _check_cell(model, free, n, n_rows, scheme)


@needs_longdouble
@pytest.mark.parametrize("free", [False, True])
@pytest.mark.parametrize("model", dh.MODELS)
def test_emulation_follows_the_rule_for_the_double_models(model, free):
    """chunk_weighted<7 | 8> with a live second component against double_helper's longdouble terms: the matrix's smallest
    cell, and N = 33 stars under 65 rows."""
    for n, n_rows in ((1, 1), (33, 65)):
        for scheme in ("exponential", "poisson", "explicit"):
            print(model, free, n, n_rows, scheme, "largest column error", _check_cell(model, free, n, n_rows, scheme))


def test_unit_weights_give_the_unweighted_gradient_bits():
    """Explicit weights of 1 multiply by one and select every star in: the bits of the unweighted loop (csrc/mcd_grad.h)."""
    from test_grad_emul_cpu import emul_grad
    for model, free in ((0, False), (2, True), (4, True), (6, False)):
        case = vh.make_case(model, free, 33)
        rows = [0, 1, 2]
        v0, g0 = emul_grad(case, rows)
        v1, g1 = wh.emul_weighted(case, rows, np.zeros(3, dtype=np.int64), "explicit", explicit=np.ones((1, 33)))
        assert v0.tobytes() == v1.tobytes() and g0.tobytes() == g1.tobytes()


# ------------------------------------------------------------------------------------------ 3. zero weights
def test_zero_weight_selects_a_star_out_even_where_its_term_is_not_finite():
    case = vh.make_case(0, False, 33)
    cat = case["cat"]
    cat["verr"][7] = 0.0                                        # sigma = 0 and verr = 0 off the model velocity: l = -inf
    case["params"] = np.ascontiguousarray(case["params"][:2])
    case["params"][:, 1] = 0.0
    explicit = np.ones((2, 33))
    explicit[0, 7] = 0.0
    value, grad = wh.emul_weighted(case, [0, 0], [0, 1], "explicit", explicit=explicit)
    assert np.isfinite(value[0]) and np.all(np.isfinite(grad[0])) and not np.any(np.isnan(grad[0]))
    assert not np.isfinite(value[1])
    without = {k: np.delete(v, 7) for k, v in cat.items()}
    v_ref, g_ref = wh.emul_weighted(dict(case, cat=without), [0], [0], "explicit", explicit=np.ones((1, 32)), chunk_len=4099)
    v_one, g_one = wh.emul_weighted(case, [0], [0], "explicit", explicit=explicit, chunk_len=4099)
    assert v_one.tobytes() == v_ref.tobytes() and g_one.tobytes() == g_ref.tobytes()
    # generated Poisson weights: a replicate that draws 0 for the star stays finite, one that draws it does not
    w = wh.weights("poisson", wh.SEED, 0, 40, 7, 1)[:, 0]
    zero, some = int(np.flatnonzero(w == 0)[0]), int(np.flatnonzero(w > 0)[0])
    value, grad = wh.emul_weighted(case, [0, 0], [zero, some], "poisson")
    assert np.isfinite(value[0]) and np.all(np.isfinite(grad[0])) and not np.isfinite(value[1])


# ------------------------------------------------------------------------------------------ 4. chunk starts
@pytest.mark.parametrize("scheme", ["exponential", "poisson"])
def test_chunks_of_5_and_7_stars_see_the_generators_weights(scheme):
    """CONST, v_maxx = v_maxy = v_sys = 0, sigma = 1, verr = 0: n = 1 and d = v exactly, so with v = e_i the v_sys column
    of the gradient is sum_j w_j v_j = w_i itself, bit for bit."""
    n, rows = 23, 9
    case = vh.make_case(0, False, n)
    case["cat"]["verr"][:] = 0.0
    case["params"] = np.tile(np.array([0.0, 1.0, 0.0, 0.0]), (rows, 1))
    rep = wh.row_replicates(rows)
    want = wh.weights_of_rows(scheme, wh.SEED, rep, n)
    for chunk_len in (5, 7, n):
        got = np.empty_like(want)
        for i in range(n):
            case["cat"]["v"][:] = 0.0
            case["cat"]["v"][i] = 1.0
            got[:, i] = wh.emul_weighted(case, list(range(rows)), rep, scheme, chunk_len=chunk_len)[1][:, 0]
        assert np.array_equal(got, want), chunk_len

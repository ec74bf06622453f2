"""CPU: the weighted value loop of mcd_weighted_loglike (csrc/mcd_weighted_value.h through
tests/emul/weighted_value_emul.cpp) and the compiler's resource report of its kernels
(profiles/weighted_value_resources.json).

  1. the loop against sum_i w_i t_i in longdouble with selected-out zeros (weighted_helper.reference), 7 models x {fixed,
     free} x N in {1, 33, 4099} x rows in {1, 65, 257}, both generated schemes and explicit weights, with a non-monotone
     replicate map that repeats and holds one id of 2^40: |got - exact| <= 1e-12 max(|sum w l|, sum w);
  2. unit explicit weights give chunk_holdout's bits (the same term, the same order, 1.0 l selected in, from +0.0);
  3. explicit weights filled from the generator reproduce the generated call bit for bit, for both schemes (host code
     computes the weight the same way in both places; the device's exponential need not, tests/test_gpu_weighted_value.py);
  4. chunk starts: forced chunks of 5, 7 and 23 stars against one chunk, and zero-weight stars whose term is not finite;
  5. no instantiation of weighted_value_kernel uses scratch memory or LDS, and the committed report is today's."""
import json
import os

import numpy as np
import pytest

import double_helper as dh
import variant_helper as vh
import weighted_helper as wh
import weighted_value_helper as wv

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
needs_longdouble = pytest.mark.skipif(not vh.HAVE_LONGDOUBLE, reason="numpy.longdouble is not wider than float64 here")


# ------------------------------------------------------------------------------------------ 1. the loop
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
    value = wv.emul_weighted_value(case, rows, rep, scheme, explicit=explicit)
    worst = 0.0
    for j in vh.sample_rows(n_rows):                            # the longdouble reference costs: a sample of the rows
        ref = wh.reference(model, case["cat"], case["params"][j], case["centre"], w_rows[j])
        err = wv.value_error(value[j], ref)
        assert err <= 1e-12, (model, free, n, n_rows, scheme, j, float(value[j]), float(ref["value"]), err)
        worst = max(worst, err)
    return worst


@needs_longdouble
@pytest.mark.parametrize("free", [False, True])
@pytest.mark.parametrize("model", range(7))
def test_emulation_follows_the_value_rule(model, free):
    worst = 0.0
    for n in (1, 33, 4099):
        for n_rows in (1, 65, 257):
            for scheme in ("exponential", "poisson", "explicit"):
                worst = max(worst, _check_cell(model, free, n, n_rows, scheme))
    print("model", model, "free" if free else "fixed", "largest value error", worst)


@needs_longdouble
@pytest.mark.parametrize("free", [False, True])
@pytest.mark.parametrize("model", dh.MODELS)
def test_emulation_follows_the_value_rule_for_the_double_models(model, free):
    """chunk_weighted_value<7 | 8> with a live second component against double_helper's longdouble terms: the matrix's
    smallest cell, and N = 33 stars under 65 rows."""
    for n, n_rows in ((1, 1), (33, 65)):
        for scheme in ("exponential", "poisson", "explicit"):
            print(model, free, n, n_rows, scheme, "largest value error", _check_cell(model, free, n, n_rows, scheme))


# ------------------------------------------------------------------------------------------ 2, 3. bits
@pytest.mark.parametrize("model,free", [(m, f) for m in range(7) for f in (False, True)])
def test_unit_weights_give_the_unweighted_loops_bits(model, free):
    for n, chunk_len in ((33, 96), (4099, 96), (4099, 7)):
        case = vh.make_case(model, free, n)
        rows = [0, 1, 2, 64, 519]
        plain = wv.emul_plain_value(case, rows, chunk_len=chunk_len)
        unit = wv.emul_weighted_value(case, rows, np.zeros(len(rows), dtype=np.int64), "explicit", explicit=np.ones((1, n)),
                                      chunk_len=chunk_len)
        assert plain.tobytes() == unit.tobytes(), (model, free, n, chunk_len)


@pytest.mark.parametrize("scheme", ["exponential", "poisson"])
def test_explicit_weights_from_the_generator_reproduce_the_generated_call(scheme):
    for model, free, n in ((0, False, 33), (1, False, 4099), (2, True, 4099), (4, True, 33), (5, False, 4099), (6, True, 33)):
        case = vh.make_case(model, free, n)
        rows = list(range(65))
        rep = (7 * np.arange(65, dtype=np.int64) + 3) % 5
        generated = wv.emul_weighted_value(case, rows, rep, scheme)
        explicit = wv.emul_weighted_value(case, rows, rep, "explicit", explicit=wh.weights(scheme, wh.SEED, 0, 5, 0, n))
        assert generated.tobytes() == explicit.tobytes(), (model, free, n)
        other = wv.emul_weighted_value(case, rows, rep, scheme, seed=wh.SEED + 1)
        assert not np.array_equal(other, generated)


# ------------------------------------------------------------------------------------------ 4. chunk starts, zero weights
def _const_case(n, rows):
    """CONST, sigma = 1, verr = 0, no rotation: rows that differ in v_sys only."""
    case = vh.make_case(0, False, n)
    case["cat"]["verr"][:] = 0.0
    case["params"] = np.tile(np.array([0.0, 1.0, 0.0, 0.0]), (rows, 1))
    case["params"][:, 0] = np.linspace(-2.0, 2.0, rows)
    return case


@needs_longdouble
@pytest.mark.parametrize("scheme", ["exponential", "poisson"])
def test_chunk_starts_do_not_change_the_sums(scheme):
    n, rows = 47, 9                                             # chunks of 23 start at stars 23 and 46: words 3 and 2
    case = _const_case(n, rows)
    rep = wh.row_replicates(rows)
    w_rows = wh.weights_of_rows(scheme, wh.SEED, rep, n)
    one = wv.emul_weighted_value(case, list(range(rows)), rep, scheme, chunk_len=4099)
    refs = [wh.reference(0, case["cat"], case["params"][j], case["centre"], w_rows[j]) for j in range(rows)]
    for j in range(rows):
        assert wv.value_error(one[j], refs[j]) <= 1e-12
    for chunk_len in (5, 7, 23):
        got = wv.emul_weighted_value(case, list(range(rows)), rep, scheme, chunk_len=chunk_len)
        for j in range(rows):
            scale = float(max(abs(refs[j]["value"]), refs[j]["sum_w"]))
            assert abs(got[j] - one[j]) <= 1e-12 * scale, (scheme, chunk_len, j, got[j], one[j])
    # (the bound has teeth: a chunk start that read its neighbour's weight would move the sum by about one term)
    moved = wv.emul_weighted_value(case, list(range(rows)), rep % 5, "explicit", explicit=np.roll(wh.weights(scheme, wh.SEED, 0, 5, 0, n), 1, axis=1))
    assert np.all(np.abs(moved - one)[rep < 5] > 1e-6)


def test_zero_weight_stars_with_a_non_finite_term_add_exactly_zero():
    """verr = 0 and sigma = 0 off the model velocity: the term is -inf (or NaN).  A zero weight selects it out: the sum
    equals, bit for bit, that of the catalogue without the star; a non-zero weight lets it through."""
    n = 33
    case = _const_case(n, 2)
    case["params"][:, 1] = 0.0
    case["cat"]["verr"][:] = 1.0
    case["cat"]["verr"][[7, 20]] = 0.0
    explicit = np.random.default_rng(3).choice([1.0, 2.0, 0.375], size=(2, n))
    explicit[0, [7, 20]] = 0.0
    explicit[1, 7] = -0.0                                        # -0.0 is a zero weight too; star 20 stays in
    value = wv.emul_weighted_value(case, [0, 1], [0, 1], "explicit", explicit=explicit, chunk_len=4099)
    assert np.isfinite(value[0]) and not np.isfinite(value[1])
    without = dict(case, cat={k: np.delete(v, [7, 20]) for k, v in case["cat"].items()})
    ref = wv.emul_weighted_value(without, [0], [0], "explicit", explicit=np.delete(explicit[:1], [7, 20], axis=1), chunk_len=4099)
    assert value[:1].tobytes() == ref.tobytes()
    # a chunk that holds nothing but such stars is +0.0, sign and all
    only = dict(case, cat={k: v[[7, 20]] for k, v in case["cat"].items()})
    zero = wv.emul_weighted_value(only, [0], [0], "explicit", explicit=np.zeros((1, 2)), chunk_len=4099)
    assert zero[0] == 0.0 and not np.signbit(zero[0])
    # generated Poisson weights: a replicate that draws 0 for the star stays finite, one that draws it does not
    case["cat"]["verr"][20] = 1.0
    w = wh.weights("poisson", wh.SEED, 0, 40, 7, 1)[:, 0]
    zero, some = int(np.flatnonzero(w == 0)[0]), int(np.flatnonzero(w > 0)[0])
    value = wv.emul_weighted_value(case, [0, 0], [zero, some], "poisson")
    assert np.isfinite(value[0]) and not np.isfinite(value[1])


# ------------------------------------------------------------------------------------------ 5. resources
def _committed():
    with open(os.path.join(ROOT, "profiles", "weighted_value_resources.json")) as fh:
        return json.load(fh)["rows"]


def test_no_weighted_value_kernel_uses_scratch_or_lds():
    rows = _committed()
    cells = {(r["model_id"], r["free_centre"], r["scheme"]) for r in rows}
    assert len(rows) == 54
    assert cells == {(m, f, s) for m in range(9) for f in (False, True) for s in ("exponential", "poisson", "explicit")}
    for r in rows:
        assert r["scratch_bytes_per_lane"] == 0 and r["vgpr_spill"] == 0 and r["lds_bytes"] == 0, r


def test_resource_report_is_what_the_compiler_says_today():
    """The committed JSON against a fresh run of tools/weighted_value_resources.py (hipcc for gfx950; no device needed)."""
    import shutil
    import sys
    if shutil.which("hipcc") is None:
        pytest.skip("no hipcc on this machine")
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import weighted_value_resources
    assert weighted_value_resources.analyse() == _committed()

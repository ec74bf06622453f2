"""GPU: mcd_weighted_loglike (csrc/mcd_weighted_value.hip, csrc/mcd_api_weighted.hip), the weighted value without its
gradient.

Catalogues and models: the three setups of tests/test_gpu_hmc.py.  Shapes: N in {33, 4099} x rows in {2, 66, 258} -- one
ragged row tile, a ragged second tile, more than four tiles (the XCD-grouped branch of wave_task); N = 4099 = 3 mod 4
leaves a ragged generator block.  (The device's chunk tables start every chunk on a multiple of 8 stars; starts off a
multiple of 4 are the CPU build's part, tests/test_weighted_value_cpu.py.)

  1. the three schemes against sum_i w_i t_i in longdouble (tests/weighted_helper.py): 1e-12 on max(|sum w l|, sum w);
  2. integer (Poisson) weights against the UNWEIGHTED value path on the catalogue with star i repeated w_i times
     (Catalog.loglike: code from before this call, another summation order): 1e-12 on max(|lnL|, sum w);
  3. explicit weights filled from mcd_bootstrap_weights against the generated call: Poisson bit for bit, exponential
     within 1e-12 (whether its bits match is printed);
  4. 0 / 1 explicit weights on the prefix sets {1, 0, 7} against mcd_holdout_loglike's train; unit weights against
     mcd_loglike_batch and against mcd_weighted_loglike_grad's value: 1e-12 on max(|lnL|, N) (bit equality is printed);
  5. bit repeatability across a differently shaped call, another seed, forced chunk lengths;
  6. refusals on sentinel-filled output, the one-rank communicator, out = NULL."""
import ctypes

import numpy as np
import pytest

import holdout_helper as hh
import variant_helper as vh
import weighted_helper as wh
import weighted_value_helper as wv
from test_gpu_hmc import MODELS, setup as model_setup

pytestmark = pytest.mark.gpu

ROWS = (2, 66, 258)
STARS = (33, 4099)
SEED = wh.SEED
_I64P = ctypes.POINTER(ctypes.c_int64)
_F64P = ctypes.POINTER(ctypes.c_double)


@pytest.fixture(scope="module")
def native():
    from mcmc_dynamics_amd import _native
    return _native


@pytest.fixture(scope="module")
def ctx(native):
    return native.default_context()


_CASES = {}


def case(native, ctx, kind, n):
    """One catalogue per (model, N) for the whole module: the device catalogue, what it was made of, a table maker and
    the columns in the form the test-side restatements take (as tests/test_gpu_weighted.py builds them)."""
    if (kind, n) not in _CASES:
        kw, plan, x, scale, _ = model_setup(kind, n)
        cols = [kw.pop(k) for k in ("ra", "dec", "v", "verr")]
        cat = native.Catalog(ctx, *cols, **kw)

        def table(rows, seed):
            pos = x + 0.5 * scale * np.random.default_rng(seed).normal(size=(rows, x.size))
            pos = np.clip(pos, plan["lo"], plan["hi"])
            return np.ascontiguousarray(np.stack(
                [pos[:, s] * plan["col_factor"][j] if s >= 0 else np.full(rows, plan["col_const"][j])
                 for j, s in enumerate(plan["col_source"])], axis=1))
        host = dict(zip(("ra", "dec", "v", "verr"), cols))
        host.update({k: kw[k] for k in ("lnlike_bg", "pmember", "density") if k in kw})
        _CASES[(kind, n)] = {"cat": cat, "cols": cols, "kw": kw, "table": table, "host": host, "model": kw["model"],
                             "centre": kw["centre"], "free": kw["centre"] is None}
    return _CASES[(kind, n)]


def within(got, want, scale_n):
    """The project's bound for kernel families: 1e-12 on the scale max(|lnL|, N)."""
    return np.abs(got - want) <= 1e-12 * np.maximum(np.abs(want), float(scale_n))


# ------------------------------------------------------------------------------------------ 1
@pytest.mark.skipif(not vh.HAVE_LONGDOUBLE, reason="numpy.longdouble is not wider than float64 here")
@pytest.mark.parametrize("scheme", ["exponential", "poisson", "explicit"])
@pytest.mark.parametrize("rows", ROWS)
@pytest.mark.parametrize("n", STARS)
@pytest.mark.parametrize("kind", MODELS)
def test_three_schemes_against_the_longdouble_weighted_sums(native, ctx, kind, n, rows, scheme):
    """The reference is sum_i w_i t_i in longdouble with w from mcd_bootstrap_weights, for all three schemes: the explicit
    scheme is handed the generator's own weights (the Poisson and then the exponential ones of replicates 0 .. 4, which
    its row map indexes; the 2^40 id of the generated cases cannot index a table)."""
    c = case(native, ctx, kind, n)
    table = c["table"](rows, seed=1000 + rows)
    for source in (("poisson", "exponential") if scheme == "explicit" else (scheme,)):
        rep = wh.row_replicates(rows)
        explicit = None
        if scheme == "explicit":
            rep, explicit = rep % 5, native.bootstrap_weights(source, SEED, 0, 5, 0, n)
            w_rows = explicit[rep]
        else:
            w_rows = np.stack([native.bootstrap_weights(scheme, SEED, int(b), 1, 0, n)[0] for b in rep])
        value = c["cat"].weighted_loglike(table, rep, scheme=scheme, seed=SEED, weights=explicit)
        assert value.shape == (rows,)
        errs = {j: wv.value_error(value[j], wh.reference(c["model"], c["host"], table[j], c["centre"], w_rows[j]))
                for j in vh.sample_rows(rows)}
        print(kind, n, rows, scheme, source, "largest value error %.3e" % max(errs.values()))
        for j, err in errs.items():
            assert err <= 1e-12, (kind, n, rows, scheme, source, j, float(value[j]), err)


# ------------------------------------------------------------------------------------------ 2
@pytest.mark.parametrize("rows", ROWS)
@pytest.mark.parametrize("n", STARS)
@pytest.mark.parametrize("kind", MODELS)
def test_poisson_weights_against_the_unweighted_value_path_on_the_expanded_catalogue(native, ctx, kind, n, rows):
    c = case(native, ctx, kind, n)
    table = c["table"](rows, seed=rows)
    rep = wh.row_replicates(rows)
    value = c["cat"].weighted_loglike(table, rep, scheme="poisson", seed=SEED)
    worst = 0.0
    for j in sorted({0, rows // 2, rows - 1}):
        w = native.bootstrap_weights("poisson", SEED, int(rep[j]), 1, 0, n)[0].astype(np.int64)
        if not w.any():
            continue
        host = {k: np.repeat(v, w) for k, v in c["host"].items()}
        extra = {k: host[k] for k in host if k not in ("ra", "dec", "v", "verr")}
        big = native.Catalog(ctx, host["ra"], host["dec"], host["v"], host["verr"], model=c["model"], centre=c["centre"], **extra)
        try:
            v_ref = big.loglike(table[j:j + 1])
        finally:
            big.close()
        n_big = int(w.sum())
        worst = max(worst, float(abs(value[j] - v_ref[0]) / max(abs(v_ref[0]), n_big)))
        assert within(value[j], v_ref[0], n_big), (kind, n, rows, j, value[j], v_ref[0])
    print(kind, n, rows, "against the expanded catalogue: value", worst)


# ------------------------------------------------------------------------------------------ 3
@pytest.mark.parametrize("rows", ROWS)
@pytest.mark.parametrize("n", STARS)
@pytest.mark.parametrize("kind", MODELS)
def test_explicit_weights_from_the_generator_reproduce_the_generated_call(native, ctx, kind, n, rows):
    c = case(native, ctx, kind, n)
    table = c["table"](rows, seed=2000 + rows)
    rep = (7 * np.arange(rows, dtype=np.int64) + 3) % 5
    for scheme in ("poisson", "exponential"):
        generated = c["cat"].weighted_loglike(table, rep, scheme=scheme, seed=SEED)
        explicit = c["cat"].weighted_loglike(table, rep, scheme="explicit", weights=native.bootstrap_weights(scheme, SEED, 0, 5, 0, n))
        same = generated.tobytes() == explicit.tobytes()
        print(kind, n, rows, scheme, "explicit == generated bit for bit:", same)
        if scheme == "poisson":
            assert same
        else:
            assert np.all(within(explicit, generated, n))


# ------------------------------------------------------------------------------------------ 4
@pytest.mark.parametrize("n", STARS)
@pytest.mark.parametrize("kind", MODELS)
def test_zero_one_weights_against_the_holdout_call_and_unit_weights_against_the_value_paths(native, ctx, kind, n):
    c = case(native, ctx, kind, n)
    offs = hh.sets_of_sizes((1, 0, 7), n)
    E, W = 3, 22
    table = c["table"](E * W, seed=7)
    train, _ = c["cat"].holdout_loglike(offs, table.reshape(E, W, -1))
    weights = np.ones((E, n))
    for e in range(E):
        weights[e, int(offs[e]):int(offs[e + 1])] = 0.0
    value = c["cat"].weighted_loglike(table, np.repeat(np.arange(E), W), scheme="explicit", weights=weights)
    print(kind, n, "0 / 1 weights == holdout train bit for bit:", value.tobytes() == train.reshape(-1).tobytes(),
          "largest error", float(np.max(np.abs(value - train.reshape(-1)) / np.maximum(np.abs(train.reshape(-1)), n))))
    assert np.all(within(value, train.reshape(-1), n))
    zeros, ones = np.zeros(E * W, dtype=np.int64), np.ones((1, n))
    unit = c["cat"].weighted_loglike(table, zeros, scheme="explicit", weights=ones)
    plain = c["cat"].loglike(table)
    v_grad, _ = c["cat"].weighted_loglike_grad(table, zeros, scheme="explicit", weights=ones, want_grad=False)
    print(kind, n, "unit weights == loglike bit for bit:", unit.tobytes() == plain.tobytes(), "== the gradient call's value:",
          unit.tobytes() == v_grad.tobytes())
    assert np.all(within(unit, plain, n)) and np.all(within(unit, v_grad, n))


# ------------------------------------------------------------------------------------------ 5
@pytest.mark.parametrize("scheme", ["exponential", "poisson", "explicit"])
@pytest.mark.parametrize("kind", MODELS)
def test_bitwise_repeatable(native, ctx, kind, scheme):
    c = case(native, ctx, kind, 4099)
    table = c["table"](66, seed=5)
    rep = wh.row_replicates(66) % (5 if scheme == "explicit" else (1 << 41))
    weights = np.random.default_rng(9).choice([0.0, 0.0, 1.0, 2.0, 0.375, 1.625], size=(5, 4099)) if scheme == "explicit" else None
    first = c["cat"].weighted_loglike(table, rep, scheme=scheme, seed=SEED, weights=weights)
    c["cat"].weighted_loglike(c["table"](258, seed=6), np.arange(258), scheme="poisson", seed=3)
    c["cat"].weighted_loglike_grad(table[:7], np.arange(7), scheme="explicit", weights=np.ones((7, 4099)))   # (another table kept)
    again = c["cat"].weighted_loglike(table, rep, scheme=scheme, seed=SEED, weights=weights)
    assert first.tobytes() == again.tobytes()
    # another seed is another set of weights
    if scheme != "explicit":
        other = c["cat"].weighted_loglike(table, rep, scheme=scheme, seed=SEED + 1)
        assert not np.any(other == first)


@pytest.mark.parametrize("scheme", ["exponential", "poisson"])
def test_forced_chunk_lengths_agree(native, ctx, scheme):
    """Forced chunk lengths move the chunk starts: the generator's weights do not move with them."""
    n, rows = 4099, 66
    c = vh.make_case(0, False, n)
    rep = wh.row_replicates(rows)
    table = np.ascontiguousarray(c["params"][:rows])
    cat = vh.catalog(native, ctx, c)
    try:
        got = {}
        for forced in (0, 64, 96):
            cat.set_option("chunk_len", forced)
            got[forced] = cat.weighted_loglike(table, rep, scheme=scheme, seed=SEED)
        sum_w = np.array([native.bootstrap_weights(scheme, SEED, int(b), 1, 0, n)[0].sum() for b in rep])
        for forced in (64, 96):
            err = np.abs(got[forced] - got[0]) / np.maximum(np.abs(got[0]), sum_w)
            print(scheme, "chunk_len", forced, "against the default plan:", float(err.max()))
            assert np.all(err <= 1e-12)
    finally:
        cat.close()


# ------------------------------------------------------------------------------------------ 6
def _raw(native, cat, table, rep, scheme=0, seed=1, weights=None, n_replicates=0, k=None, n_rows=None, desc=True):
    """The C entry point itself, on sentinel-filled output: (status, out)."""
    rows, K = table.shape
    out = np.full(rows, -7.25)
    d = native.WeightDesc()
    d.scheme, d.seed, d.n_replicates = scheme, seed, n_replicates
    rep = None if rep is None else np.ascontiguousarray(rep, dtype=np.int64)
    d.row_replicate = None if rep is None else rep.ctypes.data_as(_I64P)
    d.weights = None if weights is None else weights.ctypes.data_as(_F64P)
    rc = cat.lib.mcd_weighted_loglike(cat.handle, rows if n_rows is None else n_rows, K if k is None else k,
                                      table.ctypes.data_as(_F64P), ctypes.byref(d) if desc else None, out.ctypes.data_as(_F64P))
    return rc, out


def test_refusals_leave_the_output_untouched(native, ctx):
    c = case(native, ctx, "const", 33)
    cat, n = c["cat"], 33
    table = c["table"](4, seed=2)
    rep = np.arange(4, dtype=np.int64)
    ones = np.ones((4, n))

    def refused(what, catalogue=cat, **kw):
        args = dict(table=table, rep=rep)
        args.update(kw)
        rc, out = _raw(native, catalogue, **args)
        assert rc == -1, (what, rc)
        assert np.all(out == -7.25), what
        message = catalogue.lib.mcd_last_error().decode()
        assert what in message and message.startswith("mcd_weighted_loglike:"), (what, message)
    for more, what in (({"bin_offsets": np.array([0, 10, 33], dtype=np.int64)}, "un-binned"), ({"precision": "f32"}, "MCD_F64")):
        other = native.Catalog(ctx, *c["cols"], **dict(c["kw"], **more))
        refused(what, catalogue=other)
        other.close()
    refused("columns", k=5)
    refused("65536", n_rows=0)
    big = np.ascontiguousarray(np.broadcast_to(table[0], (65537, table.shape[1])))
    refused("65536", table=big, rep=np.zeros(65537, dtype=np.int64))
    refused("unknown weight scheme", scheme=3)
    refused("unknown weight scheme", scheme=-1)
    refused("row_replicate is null", rep=None)
    refused("negative", rep=np.array([0, 1, -1, 2]))
    refused("null", desc=False)
    refused("outside [0, n_replicates)", scheme=2, weights=ones, n_replicates=4, rep=np.array([0, 1, 4, 2]))
    refused("outside [0, n_replicates)", scheme=2, weights=ones, n_replicates=4, rep=np.array([0, -1, 3, 2]))
    refused("explicit weights are null", scheme=2, n_replicates=4)
    for bad in (-1.0, np.nan, np.inf):
        w = ones.copy()
        w[2, 17] = bad
        refused("negative or not finite", scheme=2, weights=w, n_replicates=4)
    too_many = (256 << 20) // 8 // n + 1
    refused("256 MiB", scheme=2, weights=ones, n_replicates=too_many)
    # out NULL: MCD_OK without work
    d = native.WeightDesc()
    d.scheme, d.seed, d.row_replicate = 0, 1, rep.ctypes.data_as(_I64P)
    assert cat.lib.mcd_weighted_loglike(cat.handle, 4, table.shape[1], table.ctypes.data_as(_F64P), ctypes.byref(d), None) == 0
    # a weight of -0.0 is a zero weight, and the catalogue still works after the refusals
    w = ones.copy()
    w[0, 3] = -0.0
    rc, out = _raw(native, cat, table, rep, scheme=2, weights=w, n_replicates=4)
    assert rc == 0 and np.all(np.isfinite(out))


def test_a_communicator_is_refused(native, ctx):
    """A one-rank communicator (MCD_FORCE_RCCL=1, as tests/test_gpu_device_chain.py makes one) stands for several devices
    or ranks: the context then has a collective path, which this call does not take."""
    import os
    c = case(native, ctx, "const", 33)
    os.environ["MCD_FORCE_RCCL"] = "1"
    try:
        ctx1 = native.Context(n_devices=1)
    finally:
        del os.environ["MCD_FORCE_RCCL"]
    other = native.Catalog(ctx1, *c["cols"], **c["kw"])
    try:
        table = c["table"](4, seed=2)
        rc, out = _raw(native, other, table, np.arange(4))
        assert rc == -1 and np.all(out == -7.25)
        assert "one device per process" in other.lib.mcd_last_error().decode()
    finally:
        other.close()

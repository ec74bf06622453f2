"""GPU: mcd_weighted_loglike_grad (csrc/mcd_weighted.hip, csrc/mcd_api_weighted.hip) and Runner.bootstrap.

Catalogues and models: the three setups of tests/test_gpu_hmc.py.  Shapes: N in {33, 4099} x rows in {2, 66, 258} -- one
ragged row tile, a ragged second tile, more than four tiles (the XCD-grouped branch of wave_task); N = 4099 = 3 mod 4
leaves a ragged generator block.  (The device's chunk tables start every chunk on a multiple of 8 stars; starts off a
multiple of 4 are the CPU build's part, tests/test_weights_cpu.py.)

  1. integer (Poisson) weights against the UNWEIGHTED gradient kernel on the catalogue with star i repeated w_i times:
     code from before this feature, another summation order; rule of DESIGN 3.9 on the expanded catalogue's S_k,
     2 err_np64 + 1e-12;
  2. the three schemes against sum_i w_i t_i in longdouble (tests/weighted_helper.py), the CPU test's bounds;
  3. explicit weights filled from mcd_bootstrap_weights against the generated call: Poisson bit for bit, exponential
     within 1e-12 (whether its bits match is printed);
  4. 0 / 1 explicit weights on the prefix sets {1, 0, 7} against mcd_holdout_loglike's train, unit weights against
     mcd_loglike_grad_batch, within 1e-12 on max(|lnL|, N);
  5. determinism, and the out = NULL / grad = NULL variants;
  6. refusals on sentinel-filled outputs;
  7. Runner.bootstrap end to end against the closed-form weighted maxima of a one-parameter fit."""
import ctypes

import numpy as np
import pytest

import grad_bounds as gb
import grad_helper as gh
import holdout_helper as hh
import variant_helper as vh
import weighted_helper as wh
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
    the columns in the form the test-side restatements take."""
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
@pytest.mark.parametrize("rows", ROWS)
@pytest.mark.parametrize("n", STARS)
@pytest.mark.parametrize("kind", MODELS)
def test_poisson_weights_against_the_unweighted_kernel_on_the_expanded_catalogue(native, ctx, kind, n, rows):
    c = case(native, ctx, kind, n)
    table = c["table"](rows, seed=rows)
    rep = wh.row_replicates(rows)
    value, grad = c["cat"].weighted_loglike_grad(table, rep, scheme="poisson", seed=SEED)
    worst_v = worst_g = 0.0
    for j in sorted({0, rows // 2, rows - 1}):
        w = native.bootstrap_weights("poisson", SEED, int(rep[j]), 1, 0, n)[0].astype(np.int64)
        if not w.any():
            continue
        host = {k: np.repeat(v, w) for k, v in c["host"].items()}
        extra = {k: host[k] for k in host if k not in ("ra", "dec", "v", "verr")}
        big = native.Catalog(ctx, host["ra"], host["dec"], host["v"], host["verr"], model=c["model"], centre=c["centre"], **extra)
        try:
            v_ref, g_ref = big.loglike_grad(table[j:j + 1])
        finally:
            big.close()
        n_big = int(w.sum())
        assert within(value[j], v_ref[0], n_big), (kind, n, rows, j, value[j], v_ref[0])
        g80, s80 = gh.grad(c["model"], host, table[j], c["centre"], vh.L)
        g64, _ = gh.grad(c["model"], host, table[j], c["centre"], np.float64)
        bound = 2 * gh.col_err(g64, g80, s80) + 1e-12
        err = gh.col_err(grad[j], g_ref[0], s80)
        assert np.all(err <= bound), (kind, n, rows, j, err.tolist(), bound.tolist())
        worst_v = max(worst_v, float(abs(value[j] - v_ref[0]) / max(abs(v_ref[0]), n_big)))
        worst_g = max(worst_g, float(err.max()))
    print(kind, n, rows, "against the expanded catalogue: value", worst_v, "gradient / S_k", worst_g)


# ------------------------------------------------------------------------------------------ 2, 3
def _explicit_table(n, seed):
    """Five replicates of weights with exact zeros, integers and fractions (the determinism test's)."""
    return np.random.default_rng(seed).choice([0.0, 0.0, 1.0, 2.0, 0.375, 1.625], size=(5, n))


@pytest.mark.skipif(not vh.HAVE_LONGDOUBLE, reason="numpy.longdouble is not wider than float64 here")
@pytest.mark.parametrize("scheme", ["exponential", "poisson", "explicit"])
@pytest.mark.parametrize("rows", ROWS)
@pytest.mark.parametrize("n", STARS)
@pytest.mark.parametrize("kind", MODELS)
def test_three_schemes_against_the_longdouble_weighted_sums(native, ctx, kind, n, rows, scheme):
    """The reference is sum_i w_i terms[:, i] in longdouble with w from mcd_bootstrap_weights, for all three schemes: the
    explicit scheme is handed the generator's own weights (the Poisson and then the exponential ones of replicates 0 .. 4,
    which its row map indexes; the 2^40 id of the generated cases cannot index a table).

    The free-centre cell at N = 33 (PROFILE_BGGAUSS) has no entry in grad_bounds.FREE_FLOOR and is held to 1e-12, which is
    about what the free-centre record format allows there (grad_bounds.py: the offsets cancel to ~1e-12 relative, and few
    stars set S_k): over ALL 66 rows of the 66-row table the host build of the UNWEIGHTED loop reaches err - 2 err_np64 =
    1.12e-12 (row 13, ra_center), exponential weights 1.40e-12 and Poisson weights 2.06e-12, on rows this test does not
    sample.  An earlier version of this test gave the explicit scheme a table of its own making (weights drawn from {0, 0,
    1, 2, 0.375, 1.625}) instead of the generator's: row 1 of the two-row table then missed the bound in the r_peak
    column, 2.37e-12 on the device and 2.42e-12 in the host build of the same loop against 1.46e-12 -- the arithmetic of
    csrc/mcd_grad.h on free-centre records, host and device alike, not the kernel.  DESIGN 3.20 keeps the figures."""
    c = case(native, ctx, kind, n)
    table = c["table"](rows, seed=1000 + rows)
    floors = gb.floors(c["model"], c["free"], n)
    for source in (("poisson", "exponential") if scheme == "explicit" else (scheme,)):
        rep = wh.row_replicates(rows)
        explicit = None
        if scheme == "explicit":
            rep, explicit = rep % 5, native.bootstrap_weights(source, SEED, 0, 5, 0, n)
            w_rows = explicit[rep]
        else:
            w_rows = np.stack([native.bootstrap_weights(scheme, SEED, int(b), 1, 0, n)[0] for b in rep])
        value, grad = c["cat"].weighted_loglike_grad(table, rep, scheme=scheme, seed=SEED, weights=explicit)
        refs = {j: wh.reference(c["model"], c["host"], table[j], c["centre"], w_rows[j]) for j in vh.sample_rows(rows)}
        errs = [(float(abs(value[j] - r["value"]) / max(abs(r["value"]), r["sum_w"])),
                 float((gh.col_err(grad[j], r["g"], r["s"]) - 2 * r["err64"]).max())) for j, r in refs.items()]
        print(kind, n, rows, scheme, source, "largest value error %.3e, largest column err - 2 err_np64 %.3e" % tuple(np.max(errs, axis=0)))
        for j, r in refs.items():
            wh.check_row(value[j], grad[j], r, (kind, n, rows, scheme, source, j), floors)


@pytest.mark.parametrize("rows", ROWS)
@pytest.mark.parametrize("n", STARS)
@pytest.mark.parametrize("kind", MODELS)
def test_explicit_weights_from_the_generator_reproduce_the_generated_call(native, ctx, kind, n, rows):
    c = case(native, ctx, kind, n)
    table = c["table"](rows, seed=2000 + rows)
    rep = (7 * np.arange(rows, dtype=np.int64) + 3) % 5
    for scheme in ("poisson", "exponential"):
        generated = c["cat"].weighted_loglike_grad(table, rep, scheme=scheme, seed=SEED)
        explicit = c["cat"].weighted_loglike_grad(table, rep, scheme="explicit", weights=native.bootstrap_weights(scheme, SEED, 0, 5, 0, n))
        same = generated[0].tobytes() == explicit[0].tobytes() and generated[1].tobytes() == explicit[1].tobytes()
        print(kind, n, rows, scheme, "explicit == generated bit for bit:", same)
        if scheme == "poisson":
            assert same
        else:
            assert np.all(within(explicit[0], generated[0], n))
            for j in vh.sample_rows(rows):
                w = native.bootstrap_weights(scheme, SEED, int(rep[j]), 1, 0, n)[0]
                scale = wh.reference(c["model"], c["host"], table[j], c["centre"], w)["s"]
                assert np.all(gh.col_err(explicit[1][j], generated[1][j], scale) <= 1e-12), (kind, n, rows, j)


# ------------------------------------------------------------------------------------------ 4
@pytest.mark.parametrize("n", STARS)
@pytest.mark.parametrize("kind", MODELS)
def test_zero_one_weights_against_the_holdout_call_and_unit_weights_against_the_gradient(native, ctx, kind, n):
    c = case(native, ctx, kind, n)
    offs = hh.sets_of_sizes((1, 0, 7), n)
    E, W = 3, 22
    table = c["table"](E * W, seed=7)
    train, _ = c["cat"].holdout_loglike(offs, table.reshape(E, W, -1))
    weights = np.ones((E, n))
    for e in range(E):
        weights[e, int(offs[e]):int(offs[e + 1])] = 0.0
    value, _ = c["cat"].weighted_loglike_grad(table, np.repeat(np.arange(E), W), scheme="explicit", weights=weights)
    err = np.abs(value - train.reshape(-1)) / np.maximum(np.abs(train.reshape(-1)), n)
    print(kind, n, "largest |weighted - train| / max(|lnL|, N):", err.max())
    assert np.all(within(value, train.reshape(-1), n))
    v_ref, g_ref = c["cat"].loglike_grad(table)
    value, grad = c["cat"].weighted_loglike_grad(table, np.zeros(E * W, dtype=np.int64), scheme="explicit", weights=np.ones((1, n)))
    assert np.all(within(value, v_ref, n))
    for j in vh.sample_rows(E * W):
        s = wh.reference(c["model"], c["host"], table[j], c["centre"], np.ones(n))["s"]
        assert np.all(gh.col_err(grad[j], g_ref[j], s) <= 1e-12), (kind, n, j)


# ------------------------------------------------------------------------------------------ 5
@pytest.mark.parametrize("scheme", ["exponential", "poisson", "explicit"])
@pytest.mark.parametrize("kind", MODELS)
def test_bitwise_repeatable_and_null_outputs(native, ctx, kind, scheme):
    c = case(native, ctx, kind, 4099)
    table = c["table"](66, seed=5)
    rep = wh.row_replicates(66) % (5 if scheme == "explicit" else (1 << 41))
    weights = _explicit_table(4099, 9) if scheme == "explicit" else None
    first = c["cat"].weighted_loglike_grad(table, rep, scheme=scheme, seed=SEED, weights=weights)
    c["cat"].weighted_loglike_grad(c["table"](258, seed=6), np.arange(258), scheme="poisson", seed=3)
    c["cat"].loglike_grad(table[:7])
    again = c["cat"].weighted_loglike_grad(table, rep, scheme=scheme, seed=SEED, weights=weights)
    assert first[0].tobytes() == again[0].tobytes() and first[1].tobytes() == again[1].tobytes()
    only_v, none = c["cat"].weighted_loglike_grad(table, rep, scheme=scheme, seed=SEED, weights=weights, want_grad=False)
    assert none is None and only_v.tobytes() == first[0].tobytes()
    none, only_g = c["cat"].weighted_loglike_grad(table, rep, scheme=scheme, seed=SEED, weights=weights, want_value=False)
    assert none is None and only_g.tobytes() == first[1].tobytes()
    # another seed is another set of weights
    if scheme != "explicit":
        other = c["cat"].weighted_loglike_grad(table, rep, scheme=scheme, seed=SEED + 1)
        assert not np.array_equal(other[0], first[0])


def test_chunk_plan_does_not_change_a_generated_weight(native, ctx):
    """Forced chunk lengths move the chunk starts; the sums agree to rounding, and with CONST rows whose v_sys column reads
    one star's weight (tests/test_weights_cpu.py) the weights themselves are recovered bit for bit."""
    n, rows = 203, 66
    c = vh.make_case(0, False, n)
    c["cat"]["verr"][:] = 0.0
    rep = wh.row_replicates(rows)
    table = np.tile(np.array([0.0, 1.0, 0.0, 0.0]), (rows, 1))
    for scheme in ("exponential", "poisson"):
        want = np.stack([native.bootstrap_weights(scheme, SEED, int(b), 1, 0, n)[0] for b in rep])
        for star in (0, 63, 64, 67, 129, 202):                   # around the starts of 64-star chunks, and the ragged end
            c["cat"]["v"][:] = 0.0
            c["cat"]["v"][star] = 1.0
            cat = vh.catalog(native, ctx, c)
            try:
                for forced in (0, 64, 96):
                    cat.set_option("chunk_len", forced)
                    grad = cat.weighted_loglike_grad(table, rep, scheme=scheme, seed=SEED)[1]
                    assert np.array_equal(grad[:, 0], want[:, star]), (scheme, star, forced)
            finally:
                cat.close()


# ------------------------------------------------------------------------------------------ 6
def _raw(native, cat, table, rep, scheme=0, seed=1, weights=None, n_replicates=0, k=None, n_rows=None, desc=True):
    """The C entry point itself, on sentinel-filled outputs: (status, out, grad)."""
    rows, K = table.shape
    out, grad = np.full(rows, -7.25), np.full((rows, K), -7.25)
    d = native.WeightDesc()
    d.scheme, d.seed, d.n_replicates = scheme, seed, n_replicates
    rep = None if rep is None else np.ascontiguousarray(rep, dtype=np.int64)
    d.row_replicate = None if rep is None else rep.ctypes.data_as(_I64P)
    d.weights = None if weights is None else weights.ctypes.data_as(_F64P)
    rc = cat.lib.mcd_weighted_loglike_grad(cat.handle, rows if n_rows is None else n_rows, K if k is None else k,
                                           table.ctypes.data_as(_F64P), ctypes.byref(d) if desc else None,
                                           out.ctypes.data_as(_F64P), grad.ctypes.data_as(_F64P))
    return rc, out, grad


def test_refusals_leave_the_outputs_untouched(native, ctx):
    c = case(native, ctx, "const", 33)
    cat, n = c["cat"], 33
    table = c["table"](4, seed=2)
    rep = np.arange(4, dtype=np.int64)
    ones = np.ones((4, n))

    def refused(what, catalogue=cat, **kw):
        args = dict(table=table, rep=rep)
        args.update(kw)
        rc, out, grad = _raw(native, catalogue, **args)
        assert rc == -1, (what, rc)
        assert np.all(out == -7.25) and np.all(grad == -7.25), what
        assert what in catalogue.lib.mcd_last_error().decode(), (what, catalogue.lib.mcd_last_error().decode())
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
    # both outputs NULL: MCD_OK without work
    d = native.WeightDesc()
    d.scheme, d.seed, d.row_replicate = 0, 1, rep.ctypes.data_as(_I64P)
    assert cat.lib.mcd_weighted_loglike_grad(cat.handle, 4, table.shape[1], table.ctypes.data_as(_F64P), ctypes.byref(d), None, None) == 0
    # a weight of -0.0 is a zero weight, and the catalogue still works after the refusals
    w = ones.copy()
    w[0, 3] = -0.0
    rc, out, grad = _raw(native, cat, table, rep, scheme=2, weights=w, n_replicates=4)
    assert rc == 0 and np.all(np.isfinite(out)) and np.all(np.isfinite(grad))


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
        rc, out, grad = _raw(native, other, table, np.arange(4))
        assert rc == -1 and np.all(out == -7.25) and np.all(grad == -7.25)
        assert "one device per process" in other.lib.mcd_last_error().decode()
    finally:
        other.close()


# ------------------------------------------------------------------------------------------ 7
def test_bootstrap_against_the_closed_form():
    """ConstantFit on 200 synthetic stars, no background, only v_sys free in a wide box: replicate b's weighted maximum is
    mu_b = sum w_i v_i / n_i / sum w_i / n_i, n_i = verr_i^2 + sigma^2 (long double, from the catalogue's columns and
    mcd_bootstrap_weights).  Every replicate converges (tests/test_bootstrap_cpu.py checks that condition on the NumPy
    quadratic) to within the stopping rule's own bound: |g| scale <= gtol with scale >= 1 and g = Lambda_b (mu_b - x)."""
    from mcmc_dynamics_amd import _native
    cols = hh.closed_form_columns()
    fit = hh.closed_form_fit(cols)
    try:
        x_hat = fit.maximize()["x"]
        for scheme in ("exponential", "poisson"):
            out = fit.bootstrap(n_replicates=64, scheme=scheme, seed=1, x_hat=x_hat)
            w = _native.bootstrap_weights(scheme, 1, 0, 64, 0, hh.N_STARS)
            mu, lam = wh.closed_form_maximum(cols["v"], cols["verr"], hh.SIGMA, w)
            assert out["converged"].all() and out["n_converged"] == 64
            err = np.abs(out["x"][:, 0] - mu)
            bound = 1e-8 / lam + 1e-12 * np.abs(mu)
            print(scheme, "largest |x_b - mu_b| / bound:", float(np.max(err / bound)), "iterations", int(out["n_iter"].max()),
                  "std", out["std"][0], "std_ratio", out["std_ratio"][0])
            assert np.all(err <= bound)
            assert abs(out["std"][0] - float(np.std(mu.astype(np.float64), ddof=1))) <= float(np.max(bound))
            again = fit.bootstrap(n_replicates=64, scheme=scheme, seed=1, x_hat=x_hat)
            assert again["x"].tobytes() == out["x"].tobytes()
            if scheme == "poisson":
                # a replicate that draws weight 0 for a star: the closed form without that star
                b = int(np.argmax((w == 0).any(axis=1)))
                keep = w[b] != 0
                assert not keep.all()
                mu_b, lam_b = wh.closed_form_maximum(cols["v"][keep], cols["verr"][keep], hh.SIGMA, w[b][keep])
                assert mu_b[0] == mu[b] or abs(mu_b[0] - mu[b]) <= 1e-18 * abs(mu[b])
                assert abs(out["x"][b, 0] - mu_b[0]) <= 1e-8 / lam_b[0] + 1e-12 * abs(mu_b[0])
        # the covariance is accepted where laplace()'s is
        start = fit.get_initials_laplace(8, x_hat, out["covariance"])
        assert start.shape == (8, 1) and np.all(np.isfinite(start))
    finally:
        fit.close()

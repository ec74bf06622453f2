"""GPU: mcd_loglike_grad_batch (csrc/mcd_grad.hip) against the 80-bit test-side gradient (tests/grad_helper.py).

Matrix: model 0 .. 6 x fixed / free centre x N in {1, 33, 4099} x W in {1, 65, 257}, plus planted certain members at
N = 4099 for the mixture models.  N = 4099 in chunks of 96 stars crosses chunk and multi-round plan boundaries, N = 1 and
33 are where few terms set the scale; W = 1 leaves 63 idle lanes, 65 has a ragged second tile, 257 takes the XCD-grouped
grid.  Per cell and per column, for up to six walker rows (row 0 and row W - 1 among them):
    err = |device - exact| / S_k <= 2 err_np64 + floor            (grad_bounds.py; the rule of test_grad_emul_cpu.py)
with the floors of the host-build test (grad_bounds.floors: 1e-12, more for the free-centre cells at N = 1 and 33, whose
record format cancels; the table and its reason are there).  Also: the value output against the plain value kernels,
bitwise repeatability, binned catalogues against un-binned ones, edge rows and error paths."""
import numpy as np
import pytest

import grad_bounds as gb
import grad_helper as gh
import variant_helper as vh

pytestmark = pytest.mark.gpu

STARS = (1, 33, 4099)
WALKERS = (1, 65, 257)

@pytest.fixture(scope="module")
def native():
    from mcmc_dynamics_amd import _native
    return _native


@pytest.fixture(scope="module")
def ctx(native):
    return native.default_context()


def open_catalog(native, ctx, case, sl=slice(None), **more):
    cat = vh.catalog(native, ctx, case, sl, **more)
    cat.set_option("balance", 0)
    cat.set_option("chunk_len", vh.CHUNK_LEN)
    return cat


def check_cell(cat, case, w, log):
    """One (catalogue, W) cell: functional assertions, then the accuracy of up to six rows.  Appends (N, W, row, planted,
    largest err - 2 err_np64, its column) per row to `log` and returns the rows that miss their bound."""
    model, free, n = case["model"], case["free"], case["n"]
    params = np.ascontiguousarray(case["params"][:w])
    value, grad = cat.loglike_grad(params)
    assert value.shape == (w,) and grad.shape == (w, params.shape[1])
    assert np.all(np.isfinite(grad)) and np.all(np.isfinite(value))
    value2, grad2 = cat.loglike_grad(params)
    assert value.tobytes() == value2.tobytes() and grad.tobytes() == grad2.tobytes(), ("not repeatable", model, free, n, w)
    cat.set_option("fast_path", 0)
    plain = cat.loglike(params)
    assert np.all(vh.scaled_err(value, plain, n) < 1e-12), ("value output", model, free, n, w)
    if case["planted"] == [] and n > 1:
        assert cat.launch_info()["chunks"] == -(-n // vh.CHUNK_LEN)
    failures = []
    for r in vh.sample_rows(w):
        ref = gb.reference(case, r)
        err = gh.col_err(grad[r], ref["g"], ref["s"])
        excess = err - 2 * ref["err64"]
        log.append((n, w, r, bool(case["planted"]), float(np.max(excess)), int(np.argmax(excess))))
        bound = 2 * ref["err64"] + gb.floors(model, free, n)
        if np.any(err > bound):
            failures.append((n, w, r, err.tolist(), bound.tolist()))
    return failures


@pytest.mark.parametrize("free", [False, True])
@pytest.mark.parametrize("model", range(7))
def test_device_gradient_against_the_80_bit_truth(native, ctx, model, free):
    log, failures = [], []
    cases = [vh.make_case(model, free, n) for n in STARS]
    if model in vh.MIXTURE_MODELS:
        cases.append(vh.make_case(model, free, 4099, plant=True))
    for case in cases:
        cat = open_catalog(native, ctx, case)
        for w in WALKERS:
            failures += check_cell(cat, case, w, log)
        cat.close()
    for n in STARS:                                     # (the figures a floor would be judged by, before the assertion)
        top = max((t for t in log if t[0] == n), key=lambda t: t[4])
        print("model {0} free {1} N = {2}: worst err - 2 err_np64 = {3:.3e} (W = {4}, row {5}, planted {6}, "
              "column {7})".format(model, int(free), n, top[4], top[1], top[2], top[3], top[5]))
    assert not failures, failures


@pytest.mark.parametrize("model", [0, 1])
def test_binned_catalogue_matches_unbinned_bins(native, ctx, model):
    case = vh.make_case(model, False, 4099)
    offs = [0, 5, 705, 4099]
    w = 65
    params = np.ascontiguousarray(np.stack([case["params"][b * w:(b + 1) * w] for b in range(3)]))
    binned = open_catalog(native, ctx, case, bin_offsets=offs)
    value, grad = binned.loglike_grad(params)
    assert value.shape == (3, w) and grad.shape == (3, w, 4)
    for b in range(3):
        sl = slice(offs[b], offs[b + 1])
        sub = dict(case, cat={k: v[sl] for k, v in case["cat"].items()}, n=offs[b + 1] - offs[b], params=params[b])
        one = open_catalog(native, ctx, sub)
        v1, g1 = one.loglike_grad(params[b])
        one.close()
        assert np.all(vh.scaled_err(value[b], v1, sub["n"]) < 1e-12)
        for r in vh.sample_rows(w):
            ref = gb.reference(sub, r)
            gb.check_columns(grad[b, r], ref, (model, "bin", b, r))
            gb.check_columns(g1[r], ref, (model, "un-binned", b, r))
    binned.close()


def test_sigma_zero_f_back_zero_and_certain_membership(native, ctx):
    case = vh.make_case(2, False, 33)
    case["params"][0, 1] = 0.0                        # sigma_max = 0, verr > 0
    case["params"][1, -1] = 0.0                       # f_back = 0
    cat = open_catalog(native, ctx, case)
    _, grad = cat.loglike_grad(case["params"][:2])
    cat.close()
    assert np.all(np.isfinite(grad)) and grad[0, 1] == 0.0
    gb.check_columns(grad[1], gb.reference(case, 1), "f_back = 0")
    case = vh.make_case(1, False, 33)
    case["cat"]["pmember"][:4] = [0.0, 1.0, 0.0, 1.0]
    cat = open_catalog(native, ctx, case)
    _, grad = cat.loglike_grad(case["params"][:3])
    cat.close()
    assert np.all(np.isfinite(grad))
    gb.check_columns(grad[0], gb.reference(case, 0), "pmember in {0, 1}")


@pytest.mark.parametrize("model", [0, 2])
def test_star_on_a_free_centre_adds_nothing_to_the_centre_columns(native, ctx, model):
    """ra = dec = 0 gives the record (A, B, sin dec) = (0, 1, 0) exactly, and the walker centre (0, 0) then has x = y = 0
    exactly: the position angle is undefined, the value path takes numpy's arctan2 convention and the gradient gives that
    star no centre derivative -- the centre columns equal those of the catalogue without the star, bit for bit."""
    case = vh.make_case(model, True, 33)
    c = case["cat"]
    c["ra"] = c["ra"] - vh.CENTRE[0]
    c["dec"] = c["dec"] - vh.CENTRE[1]
    params = np.ascontiguousarray(case["params"][:3])
    params[:, 4:6] -= np.array(vh.CENTRE)
    params[0, 4:6] = 0.0
    c["ra"][-1], c["dec"][-1] = 0.0, 0.0
    with_star = open_catalog(native, ctx, case)
    v1, g1 = with_star.loglike_grad(params)
    without = open_catalog(native, ctx, case, slice(0, 32))
    v0, g0 = without.loglike_grad(params)
    with_star.close()
    without.close()
    assert np.all(np.isfinite(g1)) and np.all(np.isfinite(v1))
    assert g1[0, 4] == g0[0, 4] and g1[0, 5] == g0[0, 5]          # (one chunk: the star is the last term of each sum)
    assert g1[0, 0] != g0[0, 0] and v1[0] != v0[0]                  # ... while it does count elsewhere
    assert g1[1, 4] != g0[1, 4]                                     # and for walkers whose centre is somewhere else


def test_profile_star_on_a_free_centre_keeps_its_true_derivative(native, ctx):
    """The profile models are smooth at r = 0 (v_los and sigma_los are polynomials in dx, dy there): no special case, the
    star's centre derivative is the true, non-zero one, and the row matches the 80-bit gradient like any other."""
    case = vh.make_case(3, True, 33)
    c = case["cat"]
    c["ra"], c["dec"] = c["ra"] - vh.CENTRE[0], c["dec"] - vh.CENTRE[1]
    case["params"] = np.ascontiguousarray(case["params"][:3])
    case["params"][:, 6:8] -= np.array(vh.CENTRE)
    case["params"][0, 6:8] = 0.0
    c["ra"][-1], c["dec"][-1] = 0.0, 0.0
    with_star = open_catalog(native, ctx, case)
    _, g1 = with_star.loglike_grad(case["params"])
    without = open_catalog(native, ctx, case, slice(0, 32))
    _, g0 = without.loglike_grad(case["params"])
    with_star.close()
    without.close()
    assert np.all(np.isfinite(g1))
    assert g1[0, 6] != g0[0, 6] and g1[0, 7] != g0[0, 7]
    gb.check_columns(g1[0], gb.reference(case, 0), "profile, star on the centre", gb.floors(3, True, 33))


def test_error_paths(native, ctx):
    case = vh.make_case(0, False, 33)
    cat = open_catalog(native, ctx, case)
    value, grad = cat.loglike_grad(case["params"][:5], want_value=False)           # out = NULL is accepted
    assert value is None and np.all(np.isfinite(grad))
    out, g = np.empty(5), np.empty((5, 3))
    bad = np.ascontiguousarray(case["params"][:5, :3])
    rc = cat.lib.mcd_loglike_grad_batch(cat.handle, 5, 3, native._ptr(bad), native._ptr(out), native._ptr(g))
    assert rc == -1, rc                                                            # MCD_ERR_INVALID: wrong k
    cat.close()
    c = case["cat"]
    f32 = native.Catalog(ctx, c["ra"], c["dec"], c["v"], c["verr"], model=0, centre=case["centre"], precision="f32")
    p = np.ascontiguousarray(case["params"][:5])
    g = np.empty((5, 4))
    rc = f32.lib.mcd_loglike_grad_batch(f32.handle, 5, 4, native._ptr(p), native._ptr(out), native._ptr(g))
    assert rc == -1, rc                                                            # MCD_ERR_INVALID: float32 catalogue
    with pytest.raises(native.NativeError):
        f32.loglike_grad(p)
    f32.close()

"""GPU: the float32 instantiations of the main kernel (csrc/mcd_kernels.hip: launch_precision, precision "f32acc64" and
"f32") against the reference's formulas in numpy.longdouble, at small and ragged shapes.

Matrix: model 0 .. 6 x fixed / free centre (the parametrisation) x precision x N in f32_helper.F32_STARS (every tail branch
of chunk_const_f32 / chunk_mixture_f32: singles, the lone 4-star tree, 16 + 4 + 3, 43 chunks of 96 with a last one of 67) x
W in (1, 65, 257) (idle lanes, a ragged second tile, the grid above 256 walkers) x plain / fast kernels, the fast ones with
the record prefetch off and on.  The inputs (tests/f32_helper.py) are inside the float32 accuracy domain and get the fast
formulations from the guard: tests/test_f32_emul_cpu.py asserts that for every cell on the host, this file on the device.

Per cell: what ran (kernel family, no re-run, chunks, prefetch, the domain verdict); two evaluations and prefetch on / off
bitwise equal; the finite pattern of the oracle; and |device - exact| / max(|exact|, N, 32) within the tolerance that
csrc/mcd_guard.h states -- fixed centre 1e-6 (f32acc64) / 2e-5 (f32), free centre 2e-5 / 1e-4.  The host build of the same
arithmetic (tests/emul/f32_emul.cpp) has libm where the device has v_rcp_f32 / v_rsq_f32 / v_exp_f32: no agreement between
the two is asserted, the largest difference is printed."""
import numpy as np
import pytest

import emul_helper as emul
import f32_helper as fh
import variant_helper as vh

pytestmark = pytest.mark.gpu

CELLS = [(m, f) for m in range(7) for f in (False, True)]
IDS = ["{0}-{1}".format(m, "free" if f else "fixed") for m, f in CELLS]
FAMILIES = (("plain", 0, (0,)), ("fast", 1, (0, 1)))         # name, option "fast_path" = expected level, prefetch settings


@pytest.fixture(scope="module")
def native():
    from mcmc_dynamics_amd import _native
    return _native


@pytest.fixture(scope="module")
def ctx(native):
    return native.default_context()


def open_catalog(native, ctx, case, precision, sl=slice(None), **more):
    cat = vh.catalog(native, ctx, case, sl, precision=precision, **more)
    cat.set_option("balance", 0)
    cat.set_option("chunk_len", fh.CHUNK_LEN)
    return cat


def assert_ran(cat, level, prefetch, n, cell):
    """What the last launch was.  A cell that was not admitted as demanded fails."""
    assert cat.fast_level == level, ("kernel family", cat.fast_level, cell)
    assert cat.rerun_count == 0, ("re-run", cell)
    assert cat.f32_in_domain, ("outside the float32 accuracy domain", cat.f32_condition, cell)
    assert cat.last_prefetch == int(bool(prefetch) and level != 0), ("prefetch", cat.last_prefetch, cell)
    assert cat.launch_info()["chunks"] == -(-n // fh.CHUNK_LEN), ("chunks", cat.launch_info(), cell)


@pytest.mark.skipif(not vh.HAVE_LONGDOUBLE, reason="no extended-precision long double on this platform")
@pytest.mark.parametrize("model,free", CELLS, ids=IDS)
def test_float32_kernels_against_the_80_bit_oracle(native, ctx, model, free):
    worst, host_diff, failures, cells = {}, {}, [], 0
    for precision in fh.PRECISIONS:
        tol = fh.tolerance(free, precision)
        for n in fh.stars(free):
            case, oracle = fh.cached_case(model, free, n)
            g = open_catalog(native, ctx, case, precision)        # option "f32_domain" stays at its default of 1: enforced
            for w in fh.F32_WALKERS:
                params = np.ascontiguousarray(case["params"][:w])
                rows = vh.sample_rows(w)
                want = oracle.rows(rows)
                for family, level, prefetches in FAMILIES:
                    first = None
                    for prefetch in prefetches:
                        cell = (precision, n, w, family, prefetch)
                        g.set_option("fast_path", level)
                        g.set_option("prefetch", prefetch)
                        reruns = g.rerun_count
                        got = g.loglike(params)
                        assert got.shape == (w,)
                        assert_ran(g, level, prefetch, n, cell)
                        assert g.rerun_count == reruns, ("rerun_count moved", cell)
                        assert got.tobytes() == g.loglike(params).tobytes(), ("not bitwise repeatable", cell)
                        cells += 1
                        if first is not None:
                            assert got.tobytes() == first.tobytes(), ("prefetch changed the bits", cell)
                            continue
                        first = got
                        assert np.array_equal(np.isfinite(got), np.ones(w, bool)), (cell, got)
                        assert np.array_equal(np.isfinite(got[rows]), np.isfinite(want.astype(np.float64))), (cell, got[rows], want)
                        err = fh.scaled_err(got[rows], want, n)
                        i = int(np.argmax(err))
                        key = (family, precision)
                        if key not in worst or err[i] > worst[key][0]:
                            worst[key] = (float(err[i]), n, w, rows[i])
                        if not err[i] <= tol:
                            failures.append((cell, rows[i], float(err[i]), tol))
                        host = emul.loglike_f32(case["cat"], case["params"][rows], model, case["centre"], level,
                                                precision == "f32acc64", fh.CHUNK_LEN)
                        host_diff[key] = max(host_diff.get(key, 0.0), float(fh.scaled_err(got[rows], host, n).max()))
            g.close()
    for (family, precision), (err, n, w, row) in sorted(worst.items()):
        tol = fh.tolerance(free, precision)
        print("F32_ACCURACY model {0} {1} {2} {3}: worst {4:.3e} at N = {5}, W = {6}, row {7}: {8:.4f} of the tolerance {9:g}; "
              "largest |device - host build| {10:.3e}".format(model, "free" if free else "fixed", family, precision, err, n, w,
                                                              row, err / tol, tol, host_diff[(family, precision)]))
    print("F32_CELLS model {0} {1}: {2}".format(model, "free" if free else "fixed", cells))
    assert set(worst) == {(f[0], p) for f in FAMILIES for p in fh.PRECISIONS}
    assert cells == len(fh.PRECISIONS) * len(fh.stars(free)) * len(fh.F32_WALKERS) * 3
    assert not failures, failures


BIN_OFFSETS, BIN_WALKERS = list(fh.BIN_OFFSETS), fh.BIN_WALKERS


@pytest.mark.skipif(not vh.HAVE_LONGDOUBLE, reason="no extended-precision long double on this platform")
@pytest.mark.parametrize("precision", fh.PRECISIONS)
@pytest.mark.parametrize("model", [0, 1])
def test_binned_float32_catalogue_against_its_bins(native, ctx, model, precision):
    """Bins of 5, 700 and 3394 stars inside ONE launch (1, 8 and 36 chunks of 96), each with walkers of its own, against the
    three un-binned float32 catalogues of the same stars and against the oracle: both sides within the stated tolerance,
    and -- with the chunk length pinned -- bit for bit equal to each other."""
    case, _ = fh.cached_case(model, False, BIN_OFFSETS[-1])
    tol = fh.tolerance(False, precision)
    n_bins = len(BIN_OFFSETS) - 1
    params = fh.binned_params(case)
    rows = vh.sample_rows(BIN_WALKERS)
    for family, level, _ in FAMILIES:
        g = open_catalog(native, ctx, case, precision, bin_offsets=BIN_OFFSETS)
        g.set_option("fast_path", level)
        got = g.loglike(params)
        assert got.shape == (n_bins, BIN_WALKERS) and np.all(np.isfinite(got))
        assert g.fast_level == level and g.rerun_count == 0 and g.f32_in_domain
        assert g.launch_info()["chunks"] == sum(-(-(b1 - b0) // fh.CHUNK_LEN) for b0, b1 in zip(BIN_OFFSETS, BIN_OFFSETS[1:]))
        assert got.tobytes() == g.loglike(params).tobytes()
        g.close()
        for b in range(n_bins):
            sl = slice(BIN_OFFSETS[b], BIN_OFFSETS[b + 1])
            nb = sl.stop - sl.start
            sub = {k: v[sl] for k, v in case["cat"].items()}
            want = np.array([vh.exact(model, sub, params[b][r], case["centre"]) for r in rows], dtype=vh.L)
            alone = open_catalog(native, ctx, case, precision, sl)
            alone.set_option("fast_path", level)
            one = alone.loglike(params[b])
            assert alone.fast_level == level and alone.f32_in_domain and alone.launch_info()["chunks"] == -(-nb // fh.CHUNK_LEN)
            alone.close()
            e_bin, e_one = fh.scaled_err(got[b][rows], want, nb).max(), fh.scaled_err(one[rows], want, nb).max()
            print("F32_BINNED model {0} {1} {2} bin of {3}: binned {4:.3e} un-binned {5:.3e} (tolerance {6:g}), bitwise equal: {7}".format(
                model, family, precision, nb, e_bin, e_one, tol, got[b].tobytes() == one.tobytes()))
            assert e_bin <= tol and e_one <= tol, (family, b, e_bin, e_one)
            assert got[b].tobytes() == one.tobytes(), (family, b, np.abs(got[b] - one).max())


@pytest.mark.parametrize("precision", fh.PRECISIONS)
@pytest.mark.parametrize("model", range(7))
def test_one_star_with_a_free_centre_is_refused(native, ctx, model, precision):
    """The star is the catalogue's centroid (sep_harm has nothing to average): outside the domain, refused with the
    tangent-plane reason; with the enforcement off the call evaluates, finite, and the verdict stays on record."""
    case = fh.f32_case(model, True, 1)
    g = open_catalog(native, ctx, case, precision)
    params = np.ascontiguousarray(case["params"][:65])
    with pytest.raises(native.NativeError, match="float32 accuracy domain.*tangent-plane"):
        g.loglike(params)
    g.set_option("f32_domain", 0)
    got = g.loglike(params)
    assert got.shape == (65,) and np.all(np.isfinite(got))
    assert not g.f32_in_domain and g.launch_info()["chunks"] == 1
    if vh.HAVE_LONGDOUBLE:
        rows = vh.sample_rows(65)
        want = np.array([vh.exact(model, case["cat"], params[r], None) for r in rows], dtype=vh.L)
        print("F32_ONE_STAR_FREE model {0} {1}: level {2}, error {3:.3e} (outside the domain: not asserted)".format(
            model, precision, g.fast_level, fh.scaled_err(got[rows], want, 1).max()))
    g.close()


@pytest.mark.parametrize("precision", fh.PRECISIONS)
@pytest.mark.parametrize("model", [1, 6])
def test_a_certain_member_is_refused_and_takes_the_plain_kernels_when_forced(native, ctx, model, precision):
    """pmember = 1 planted at N = 33 (the last star: a single of the tail) leaves the float32 mixture ranges: refused with
    the reason; with the enforcement off the plain float32 kernels evaluate it (level 0), finite, verdict on record -- what
    tests/test_gpu_baseline_shapes.py::test_float32_fast_mixtures_against_float64 expects at 50 000 stars."""
    case, _ = fh.cached_case(model, False, 33)
    planted = dict(case, cat=dict(case["cat"], pmember=case["cat"]["pmember"].copy()))
    planted["cat"]["pmember"][32] = 1.0
    params = np.ascontiguousarray(case["params"][:65])
    g = open_catalog(native, ctx, planted, precision)
    with pytest.raises(native.NativeError, match="float32 accuracy domain.*pmember <= 1 - 2\\^-20"):
        g.loglike(params)
    g.set_option("f32_domain", 0)
    got = g.loglike(params)
    assert g.fast_level == 0 and not g.f32_in_domain and g.rerun_count == 0
    assert got.shape == (65,) and np.all(np.isfinite(got))
    if vh.HAVE_LONGDOUBLE:
        rows = vh.sample_rows(65)
        want = np.array([vh.exact(model, planted["cat"], params[r], planted["centre"]) for r in rows], dtype=vh.L)
        print("F32_CERTAIN_MEMBER model {0} {1}: error {2:.3e} (outside the domain: not asserted)".format(
            model, precision, fh.scaled_err(got[rows], want, 33).max()))
    g.close()

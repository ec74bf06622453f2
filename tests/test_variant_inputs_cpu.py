"""CPU: the inputs of the device variant matrix (tests/variant_helper.py) select what tests/test_gpu_variant_matrix.py will
demand -- checked through the host build of the library's own guard and chunk planner (tests/emul_helper.py) -- and the
oracles it compares with are what they claim to be: numpy.longdouble throughout, and the float64 oracle itself within the
accuracy bound of the device test."""
import ctypes
import subprocess

import numpy as np
import pytest

import emul_helper as emul
import variant_helper as H

CELLS = [(model, free) for model in range(7) for free in (False, True)]
TARGET_WAVES, TAIL_SPLIT = 10240, 1               # the library's defaults (csrc/mcd_host.h)

# Literal expectations, derived once from csrc/mcd_guard.h (level_verdict, bounded_rescale) and csrc/mcd_kernels.hip
# (launch_precision, launch_one) -- NOT computed from the code under test:
#   (model, free centre): (narrow-range variant exists, bounded loop's rescale interval R or 0)
VARIANT_TABLE = {
    (0, False): (False, 0), (0, True): (False, 0),      # MODEL_CONST: the fraction tree has no narrow form
    (1, False): (True, 32), (1, True): (True, 0),       # MODEL_BGFIXED: bounded loop for a fixed centre only
    (2, False): (True, 0), (2, True): (True, 0),        # MODEL_BGGAUSS
    (3, False): (True, 0), (3, True): (False, 0),       # MODEL_PROFILE: ProfileNarrowAcc needs the fixed centre's r_max
    (4, False): (True, 0), (4, True): (True, 0),        # MODEL_PROFILE_BGGAUSS
    (5, False): (True, 0), (5, True): (True, 0),        # MODEL_PROFILE_BGDENS
    (6, False): (False, 0), (6, True): (False, 0),      # MODEL_PROFILE_BGFIXED: the guard never answers 2
}
# balanced one-round plans the matrix can reach: (N, W) -> workgroup sizes beyond 4 waves (G = 256 m 4 / tiles chunks of
# >= 16 stars: 20011 stars give 512 x 32 (m = 2) and 1024 x 16 (m = 4) for four walker tiles, 1024 x 16 (m = 2) for two)
PARAM_COUNT = {0: 4, 1: 4, 2: 7, 3: 6, 4: 9, 5: 7, 6: 6}      # include/mcd.h: mcd_catalog_param_count, fixed centre
COMBINE_CELLS = {(20011, 65): (8,), (20011, 256): (8, 16)}


def test_the_helper_tables_are_the_literal_expectations():
    assert {k: v[0] for k, v in VARIANT_TABLE.items()} == H.HAS_NARROW
    assert {k: v[1] for k, v in VARIANT_TABLE.items() if v[1]} == H.BOUNDED_R
    for n in H.STARS:
        for w in H.WALKERS:
            assert H.combine_cells(n, w) == COMBINE_CELLS.get((n, w), ()), (n, w)
    assert H.expected_waves(2, "narrow", 16) == 8 and H.expected_waves(4, "general", 16) == 8     # BG_GAUSS: no 16-wave case
    assert H.expected_waves(1, "narrow", 16) == 16 and H.expected_waves(1, "plain", 16) == 4
    assert H.sample_rows(1) == [0] and H.sample_rows(520) == [0, 1, 2, 260, 518, 519]


@pytest.fixture(scope="module")
def bounded_lib(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("variant_inputs") / "libbgfixed_bounded.so")
    subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-I", emul.INC,
                    emul.os.path.join(emul.ROOT, "tests", "emul", "bgfixed_bounded_emul.cpp"), "-o", out], check=True)
    lib = ctypes.CDLL(out)
    lib.emul_bounded_verdict.argtypes = [ctypes.c_int64] + [ctypes.c_void_p] * 5 + [ctypes.c_int64, ctypes.c_void_p]
    return lib


def _bounded_verdict(lib, cat, params):
    cols = [np.ascontiguousarray(cat[k], dtype=np.float64) for k in ("v", "verr", "lnlike_bg", "pmember")]
    params = np.ascontiguousarray(params, dtype=np.float64)
    info = np.zeros(6)
    return lib.emul_bounded_verdict(len(cols[0]), *[c.ctypes.data for c in cols], params.ctypes.data, len(params),
                                    info.ctypes.data)


@pytest.mark.parametrize("model,free", CELLS)
def test_inputs_select_the_demanded_family(model, free, bounded_lib):
    """Every (N, W, planted) of the matrix: the guard's level is 2 exactly where the table says a narrow variant exists
    (so "fast_path" 1 / 2 / 0 give narrow / general / plain), the bounded verdict is the table's R, and the planted
    exceptions flag the expected chunks without switching the narrow variant off."""
    narrow, r = VARIANT_TABLE[(model, free)]
    for n in H.STARS:
        for plant in (False, True) if model in H.MIXTURE_MODELS and n in H.PLANT_STARS else (False,):
            case = H.make_case(model, free, n, plant)
            cat, centre = case["cat"], case["centre"]
            assert case["params"].shape == (max(H.WALKERS), PARAM_COUNT[model] + 2 * int(free))
            exc = emul.narrow_exceptions(cat, model) if model in H.MIXTURE_MODELS else np.empty(0, np.int64)
            assert exc is not None and list(exc) == case["planted"], (n, plant, exc)
            for w in H.WALKERS:
                params = case["params"][:w]
                assert emul.fast_level_at(cat, params, model, centre) == (2 if narrow else 1), (n, w, plant)
                if model == 1 and not free:                        # (the emulated verdict is the fixed-centre one)
                    want_r = r if not plant else 0                 # a certain member has no lower bound on the product
                    assert _bounded_verdict(bounded_lib, cat, params) == want_r, (n, w, plant)
                # chunk tables: the multi-round plan has ceil(N / 96) chunks, the balanced ones exist where combine_cells says
                plan = emul.plan_chunks([0, n], 0, n, w, TARGET_WAVES, TAIL_SPLIT, exc, balance=0)
                chunks, _ = H.expected_launch(model, "general", n, w, 4)
                assert len(plan["count"]) == chunks and plan["len"] == H.CHUNK_LEN and plan["uniform_len"] == H.CHUNK_LEN
                if plant:
                    # star 0's chunk, the interior chunk and its successor, the last chunk
                    c = (n // H.CHUNK_LEN) // 2
                    assert list(np.flatnonzero(plan["general"])) == [0, c, c + 1, chunks - 1]
                else:
                    assert not plan["has_general"]
                for waves, m in ((8, 2), (16, 4)):
                    bal = emul.plan_chunks([0, n], 0, n, w, TARGET_WAVES, TAIL_SPLIT, exc, balance=m)
                    if waves in H.combine_cells(n, w):
                        assert bal["balanced_m"] == m and len(bal["count"]) == H.expected_launch(model, "general", n, w, waves)[0]
                    elif H.n_wtiles(w) in (1, 2, 4):
                        assert bal["balanced_m"] == 0, (n, w, m)


@pytest.mark.parametrize("model", range(7))
def test_the_oracle_keeps_longdouble_throughout(model):
    """oracle.faithful_* with numpy.longdouble inputs: every intermediate and the result stay longdouble (a float64
    constant or a dtype= argument inside would silently make "exact" the float64 value)."""
    if not H.HAVE_LONGDOUBLE:
        pytest.skip("no extended-precision long double on this platform")
    from oracle import lnprob_numpy as oracle
    for free in (False, True):
        case = H.make_case(model, free, 33)
        cat, centre = case["cat"], case["centre"]
        cL = {k: v.astype(H.L) for k, v in cat.items()}
        row = case["params"][3]
        head, rc, dc, tail = H._split(model, row, centre, H.L)
        pieces = [oracle.calc_xy_offset(cL["ra"], cL["dec"], rc, dc)[1]]
        if model in H.PROFILE_MODELS:
            pieces += [oracle.model_rotation(cL["ra"], cL["dec"], head[0], head[3], head[4], head[5], rc, dc),
                       oracle.model_dispersion(cL["ra"], cL["dec"], head[1], head[2], rc, dc)]
        else:
            pieces += [oracle.rotation_model(cL["ra"], cL["dec"], head[0], head[2], head[3], rc, dc),
                       oracle.dispersion_model(33, head[1])]
        if H.BG_OF[model] == H.BG_GAUSS:
            pieces.append(oracle.gaussian_background(cL["v"], cL["verr"], tail[0], tail[1]))
        assert all(p.dtype == H.L for p in pieces)
        ex = H.exact(model, cat, row, centre)
        f64 = H.value(model, cat, row, centre)
        assert isinstance(ex, H.L) and isinstance(f64, np.float64)
        # the two differ below float64 resolution of the sum's terms, and they do differ: 33 terms of 11 extra bits
        assert 0 < abs(ex - H.L(f64)) < 1e-12 * abs(ex)
        if model in H.MIXTURE_MODELS:
            lnl, mem = H.per_star(model, cat, row, centre)
            assert lnl.dtype == H.L and mem.dtype == H.L
            assert abs(lnl.sum() - ex) < 1e-16 * abs(ex) * 33            # the same terms, summed in another order
            assert np.all((mem > 0) & (mem < 1))


@pytest.mark.parametrize("model,free", CELLS)
def test_float64_oracle_is_within_the_accuracy_bound(model, free):
    """err_np64 = |float64 oracle - exact| on the scale max(|lnL|, N) is finite and < 5e-12 for the rows the device test
    compares: the yardstick `err_dev <= 2 err_np64 + floor` is a tight one for every cell."""
    if not H.HAVE_LONGDOUBLE:
        pytest.skip("no extended-precision long double on this platform")
    worst = 0.0
    for n in H.STARS:
        for plant in (False, True) if model in H.MIXTURE_MODELS and n in H.PLANT_STARS else (False,):
            case = H.make_case(model, free, n, plant)
            rows = sorted({r for w in H.WALKERS for r in H.sample_rows(w)})
            if n == max(H.STARS):
                rows = rows[::3]                                  # (the longest catalogue: a third of the rows keeps this quick)
            for r in rows:
                ex = H.exact(model, case["cat"], case["params"][r], case["centre"])
                f64 = H.value(model, case["cat"], case["params"][r], case["centre"])
                assert np.isfinite(ex) and np.isfinite(f64), (n, plant, r)
                err = float(H.scaled_err(f64, ex, n))
                assert err < 5e-12, (n, plant, r, err)
                worst = max(worst, err)
    print("err_np64 model {0} free {1}: worst {2:.2e}".format(model, int(free), worst))


@pytest.mark.parametrize("free", [False, True], ids=["fixed", "free"])
def test_the_float64_error_at_small_n_is_the_geometry(free):
    """Why the device test carries a geometry floor: with the line-of-sight model velocity computed in longdouble (exact
    tangent-plane geometry) and everything after it in float64, the reference's formula is within 4e-16 of the exact value
    on the scale max(|lnL|, N); with its own float64 geometry it is 5 to 200 times further off at N <= 33 -- the position
    angle of stars 0.01 deg (free centre: 0.003 deg) from the centre is ill-conditioned, and nothing else in the sum is."""
    if not H.HAVE_LONGDOUBLE:
        pytest.skip("no extended-precision long double on this platform")
    from oracle import lnprob_numpy as oracle
    for n in (1, 7, 33):
        case = H.make_case(0, free, n)
        cat = case["cat"]
        cL = {k: v.astype(H.L) for k, v in cat.items()}
        full = exact_geometry = 0.0
        for r in sorted({r for w in H.WALKERS for r in H.sample_rows(w)}):
            row = case["params"][r]
            head, rc, dc, _ = H._split(0, row, case["centre"], H.L)
            ex = H.exact(0, cat, row, case["centre"])
            v_los = oracle.rotation_model(cL["ra"], cL["dec"], head[0], head[2], head[3], rc, dc).astype(np.float64)
            mixed = oracle.calculate_lnlike(cat["v"], cat["verr"], v_los, oracle.dispersion_model(n, row[1]))
            full = max(full, float(H.scaled_err(H.value(0, cat, row, case["centre"]), ex, n)))
            exact_geometry = max(exact_geometry, float(H.scaled_err(mixed, ex, n)))
        print("N", n, "free", int(free), "float64 %.2e, float64 on exact geometry %.2e" % (full, exact_geometry))
        assert exact_geometry < 4e-16 and full > 5.0 * exact_geometry, (n, full, exact_geometry)

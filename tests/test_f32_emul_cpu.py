"""CPU: the float32 instantiations of the main kernel's arithmetic (csrc/mcd_math.h: chunk_loglike<.., float, float | double,
0 | 1>, built for the host in tests/emul/f32_emul.cpp) against the reference's formulas in numpy.longdouble, at the small,
ragged star counts where a tail branch decides the value (tests/f32_helper.py: F32_STARS).

The bound is the tolerance csrc/mcd_guard.h STATES for the float32 modes inside their accuracy domain, on the scale
max(|lnL|, N, 32): fixed centre 1e-6 (f32acc64) / 2e-5 (f32), free centre 2e-5 / 1e-4.  They are the project's published
numbers, not fitted to this build; every cell is asserted to be inside the domain and to be given the fast formulations by the
guard, so the bound applies.  A star lost or counted twice at N <= 33 is an error of ~3e-2 on that scale:
test_a_lost_tail_star_is_far_above_the_bound shows the bound can see it."""
import re

import numpy as np
import pytest

import emul_helper as emul
import f32_helper as fh
import variant_helper as vh

pytestmark = pytest.mark.skipif(not vh.HAVE_LONGDOUBLE, reason="no extended-precision long double on this platform")

CELLS = [(m, f) for m in range(7) for f in (False, True)]
IDS = ["{0}-{1}".format(m, "free" if f else "fixed") for m, f in CELLS]
ROWS = vh.sample_rows(fh.CPU_WALKERS)
FAMILIES = (("plain", 0), ("fast", 1))


def host(case, fast, precision, chunk_len=fh.CHUNK_LEN, rows=ROWS):
    return emul.loglike_f32(case["cat"], case["params"][rows], case["model"], case["centre"], fast,
                            precision == "f32acc64", chunk_len)


def test_stated_tolerances_are_the_headers():
    """f32_helper.TOLERANCE against the sentence in csrc/mcd_guard.h that states them, and DESIGN section 5 against both."""
    with open(emul.os.path.join(emul.INC, "mcd_guard.h")) as f:
        text = " ".join(f.read().replace("//", " ").split())
    m = re.search(r"Stated tolerances inside the domain: fixed centre (\S+) \(MCD_F32_ACC64\) / (\S+) \(MCD_F32[^)]*\); "
                  r"free centre (\S+) / (\S+)\.", text)
    assert m, "the header no longer states the float32 tolerances in this form"
    stated = [float(x) for x in m.groups()]
    assert stated == [fh.TOLERANCE[(False, True)], fh.TOLERANCE[(False, False)], fh.TOLERANCE[(True, True)],
                      fh.TOLERANCE[(True, False)]] == [1e-6, 2e-5, 2e-5, 1e-4]
    with open(emul.os.path.join(emul.ROOT, "DESIGN.md")) as f:
        design = f.read()
    assert "1e-5 / 1e-4" not in design, "DESIGN states the free-centre float32 tolerance as 1e-5 / 1e-4 (header: 2e-5 / 1e-4)"
    assert "2e-5 / 1e-4" in design


@pytest.mark.parametrize("model,free", CELLS, ids=IDS)
def test_every_cell_is_inside_the_domain_and_gets_the_fast_kernels(model, free):
    """The conditions under which the stated tolerances apply, for every table either test evaluates: the first 1, 65 and
    257 rows (device) and the sampled rows (host build).  No cell is skipped."""
    for n in fh.stars(free):
        case, _ = fh.cached_case(model, free, n)
        assert case["params"].shape[0] == fh.N_ROWS and len(case["cat"]["v"]) == n
        tables = [case["params"][:w] for w in fh.F32_WALKERS] + [case["params"][ROWS]]
        for p in tables:
            inside, kv, kt, sep, why = emul.f32_domain(case["cat"], p, model, case["centre"])
            assert inside and why == "", (model, free, n, len(p), kv, kt, sep, why)
            assert kv <= 96.0 and kt <= 2e-5
            assert emul.fast_level(case["cat"], p, model, case["centre"], f32=True) == 1, (model, free, n, len(p))


@pytest.mark.parametrize("model", [0, 1])
def test_the_binned_cells_are_inside_the_domain(model):
    """tests/test_gpu_f32_matrix.py: one catalogue with bins of 5, 700 and 3394 stars (the verdict is taken over the tables
    of all bins together) and the three un-binned catalogues of those stars, each with its bin's table."""
    case, _ = fh.cached_case(model, False, fh.BIN_OFFSETS[-1])
    params = fh.binned_params(case)
    tables = [(case["cat"], params.reshape(-1, params.shape[-1]))]
    for b, (b0, b1) in enumerate(zip(fh.BIN_OFFSETS, fh.BIN_OFFSETS[1:])):
        tables.append(({k: v[b0:b1] for k, v in case["cat"].items()}, params[b]))
    for cat, p in tables:
        inside, kv, kt, sep, why = emul.f32_domain(cat, p, model, case["centre"])
        assert inside and why == "", (len(cat["v"]), kv, why)
        assert emul.fast_level(cat, p, model, case["centre"], f32=True) == 1


@pytest.mark.parametrize("model", range(7))
def test_one_star_with_a_free_centre_is_outside_the_domain(model):
    """The star is the centroid: no separation to divide by.  The free-centre matrix starts at N = 2; the device test
    checks the refusal."""
    case = fh.f32_case(model, True, 1)
    inside, kv, kt, sep, why = emul.f32_domain(case["cat"], case["params"], model, None)
    assert not inside and "tangent-plane" in why and kv <= 96.0, (kv, kt, sep, why)


def test_the_double_models_are_refused():
    case, _ = fh.cached_case(0, False, 7)
    rec = emul.pack_records(case["cat"], 0, case["centre"])
    wp = emul.pack_walkers(case["params"][:2], 0, False)
    out = np.full(2, 123.0)
    for model in (7, 8, 9, -1):
        for free in (0, 1):
            assert emul.lib_f32().emul_loglike_f32(model, free, 1, 1, rec.shape[0], rec.ctypes.data, wp.ctypes.data, 2, 96,
                                                   out.ctypes.data) == -1
    assert np.all(out == 123.0)


@pytest.mark.parametrize("model,free", CELLS, ids=IDS)
def test_host_build_is_within_the_stated_tolerance_of_the_exact_value(model, free):
    """Every N x {plain, fast} x {f32acc64, f32}, six walker rows each."""
    failures = []
    for family, fast in FAMILIES:
        for precision in fh.PRECISIONS:
            tol = fh.tolerance(free, precision)
            worst = (-1.0, None)
            for n in fh.stars(free):
                case, oracle = fh.cached_case(model, free, n)
                want = oracle.rows(ROWS)
                got = host(case, fast, precision)
                assert np.all(np.isfinite(want.astype(np.float64))) and np.all(np.isfinite(got)), (family, precision, n)
                err = fh.scaled_err(got, want, n)
                if err.max() > worst[0]:
                    worst = (float(err.max()), n)
                if not err.max() <= tol:
                    failures.append((family, precision, n, float(err.max()), tol))
            print("F32_HOST_ACCURACY model {0} {1} {2} {3}: worst {4:.3e} at N = {5}, {6:.4f} of the tolerance {7:g}".format(
                model, "free" if free else "fixed", family, precision, worst[0], worst[1], worst[0] / tol, tol))
    assert not failures, failures


@pytest.mark.parametrize("model,free", CELLS, ids=IDS)
def test_a_lost_tail_star_is_far_above_the_bound(model, free):
    """The same call on the catalogue without its last star -- what a loop that loses the tail star would return -- differs
    by more than 100 x the tolerance at every N <= 33, and is itself far outside the bound against the exact value."""
    for n in (n for n in fh.stars(free) if n <= 33):
        case, oracle = fh.cached_case(model, free, n)
        short = fh.drop_last_star(case)
        want = oracle.rows(ROWS)
        for family, fast in FAMILIES:
            for precision in fh.PRECISIONS:
                tol = fh.tolerance(free, precision)
                full, lost = host(case, fast, precision), host(short, fast, precision)
                moved = fh.scaled_err(lost, full, n)
                assert moved.min() > 100.0 * tol, (family, precision, n, moved.min())
                assert fh.scaled_err(lost, want, n).min() > 99.0 * tol, (family, precision, n)


@pytest.mark.parametrize("model,free", CELLS, ids=IDS)
def test_chunk_length_moves_the_value_within_the_tolerance_only(model, free):
    """chunk_len 96, 104 and 4096 (43, 40 and 2 chunks of 4099 stars: other tails), and 8 / 16 / 24, which send the stars of
    the small catalogues through other branches (23 = 16 + 4 + 3 becomes 8 + 8 + 4 + 3 or 16 + 4 + 3 in two chunks):
    every value within the tolerance of the exact one and of the value at 96.  Chunk lengths are multiples of 8."""
    for n in fh.stars(free):
        case, oracle = fh.cached_case(model, free, n)
        want = oracle.rows(ROWS)
        for family, fast in FAMILIES:
            for precision in fh.PRECISIONS:
                tol = fh.tolerance(free, precision)
                base = host(case, fast, precision, 96)
                for chunk_len in (104, 4096, 8, 16, 24):
                    got = host(case, fast, precision, chunk_len)
                    cell = (family, precision, n, chunk_len)
                    assert fh.scaled_err(got, base, n).max() <= tol, cell
                    assert fh.scaled_err(got, want, n).max() <= tol, cell

"""Host build of the double Lynden-Bell models' arithmetic (tests/emul/double_emul.cpp: star_d_n plain and fast general
through chunk_loglike, star_components, grad_term of csrc/mcd_math.h and csrc/mcd_grad.h) against the longdouble
restatement of tests/double_helper.py, models 7 and 8, fixed and free centre, N = 1, 33 and 4099 in chunks of 96 stars.

Value: 1e-12 on the scale max(|lnL|, N) (variant_helper.scaled_err), plain and fast general.  Gradient: the rule of
test_grad_emul_cpu.py, err <= 2 err_np64 + floor per column with the floors grad_bounds gives PROFILE / PROFILE_BGGAUSS at
the same cell.  A cell that misses is a finding."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import double_helper as dh
import emul_helper as eh
import grad_bounds as gb
import grad_helper as gh
import variant_helper as vh

pytestmark = pytest.mark.skipif(not vh.HAVE_LONGDOUBLE, reason="numpy.longdouble is not wider than float64 here")

SRC = os.path.join(eh.ROOT, "tests", "emul", "double_emul.cpp")
OUT = os.path.join(eh.ROOT, "tests", "emul", "libmcd_double_emul.so")
_lib = None
P, I64, I = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int


def lib():
    global _lib
    if _lib is None:
        deps = [SRC] + [os.path.join(eh.INC, h) for h in ("mcd_grad.h", "mcd_math.h", "mcd_exp_table.h", "mcd_dispatch.h",
                                                          "mcd_guard.h")]
        if not os.path.exists(OUT) or any(os.path.getmtime(d) > os.path.getmtime(OUT) for d in deps):
            subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-I", eh.INC, SRC,
                            "-o", OUT], check=True)
        _lib = ctypes.CDLL(OUT)
        _lib.double_emul_loglike.argtypes = [I, I, I, I64, P, P, I64, I64, P]
        _lib.double_emul_d_n.argtypes = [I, I, I, I64, P, P, P, P]
        _lib.double_emul_per_star.argtypes = [I, I, I, I64, P, P, P]
        _lib.double_emul_grad.argtypes = [I, I, I64, P, P, P, I64, I64, P]
        _lib.double_emul_level.argtypes = [I, I, I64, P, P, P, P, P, ctypes.c_double, ctypes.c_double, I, P, I64]
    return _lib


def packed(case, rows):
    model, free = case["model"], case["free"]
    params = np.ascontiguousarray(case["params"][rows])
    rec = dh.pack_records(case["cat"], model, case["centre"])
    assert rec.shape[1] == lib().double_emul_record_doubles(model, int(free))
    assert params.shape[1] == lib().double_emul_columns(model, int(free)) == dh.n_columns(model, free)
    return params, rec, dh.pack_walkers(params, model, free, lib().double_emul_kd())


def emul_value(case, rows, fast, chunk_len=96):
    params, rec, wp = packed(case, rows)
    out = np.empty(len(rows))
    assert lib().double_emul_loglike(case["model"], int(case["free"]), int(fast), rec.shape[0], rec.ctypes.data, wp.ctypes.data,
                                     len(rows), chunk_len, out.ctypes.data) == 0
    return out


def emul_grad(case, rows, chunk_len=96):
    params, rec, wp = packed(case, rows)
    out = np.empty((len(rows), 1 + params.shape[1]))
    assert lib().double_emul_grad(case["model"], int(case["free"]), rec.shape[0], rec.ctypes.data, wp.ctypes.data,
                                  params.ctypes.data, len(rows), chunk_len, out.ctypes.data) == 0
    return out[:, 0], out[:, 1:]


def level(case, rows):
    c, params = case["cat"], np.ascontiguousarray(case["params"][rows])
    cols = [np.ascontiguousarray(c[k]) if k in c else None for k in ("ra", "dec", "v", "verr", "density")]
    rc, dc = (0.0, 0.0) if case["centre"] is None else case["centre"]
    return lib().double_emul_level(case["model"], int(case["free"]), len(c["v"]), *[a.ctypes.data if a is not None else None
                                                                                     for a in cols],
                                   rc, dc, params.shape[1], params.ctypes.data, params.shape[0])


def check(case, rows, cell):
    model, free, n = case["model"], case["free"], case["n"]
    plain, fast = emul_value(case, rows, 0), emul_value(case, rows, 1)
    value, grad = emul_grad(case, rows)
    assert level(case, rows) == 1                                 # the fast general form is what the library would run
    for j, w in enumerate(rows):
        ref = dh.reference(case, w)
        for name, got in (("plain", plain[j]), ("fast", fast[j]), ("gradient's value", value[j])):
            assert vh.scaled_err(got, ref["value"], n) < 1e-12, (cell, w, name)
        gb.check_columns(grad[j], ref, (cell, w), dh.floors(model, free, n))


@pytest.mark.parametrize("n", [1, 33, 4099])
@pytest.mark.parametrize("free", [False, True])
@pytest.mark.parametrize("model", dh.MODELS)
def test_host_build_matches_the_longdouble_helper(model, free, n):
    check(dh.make_case(model, free, n), vh.sample_rows(8), (model, free, n))


@pytest.mark.parametrize("free", [False, True])
@pytest.mark.parametrize("model", dh.MODELS)
def test_star_on_the_centre_and_the_ratio_at_its_bounds(model, free):
    """Star 32 sits exactly on the centre (r = 0: both components vanish there, the centre derivative does not); row 0 has
    r_peak_ratio = 1 (both peaks at one radius), row 1 r_peak_ratio = 1e-3."""
    case = dh.make_case(model, free, 33)
    c = case["cat"]
    case["params"] = np.ascontiguousarray(case["params"][:3])
    case["params"][0, 8], case["params"][1, 8] = 1.0, 1e-3
    if free:
        # ra = dec = 0 packs to (A, B, sin dec) = (0, 1, 0) and a centre (0, 0) then has x = y = 0 exactly
        c["ra"], c["dec"] = c["ra"] - vh.CENTRE[0], c["dec"] - vh.CENTRE[1]
        case["params"][:, 9:11] -= np.array(vh.CENTRE)
        case["params"][0, 9:11] = 0.0
        c["ra"][-1], c["dec"][-1] = 0.0, 0.0
    else:
        c["ra"][-1], c["dec"][-1] = vh.CENTRE
    check(case, [0, 1, 2], (model, free, "r = 0, ratio bounds"))
    params, rec, wp = packed(case, [0])
    d, nn = np.empty(33), np.empty(33)
    for fast in (0, 1):
        assert lib().double_emul_d_n(model, int(free), fast, 33, rec.ctypes.data, wp.ctypes.data, d.ctypes.data, nn.ctypes.data) == 0
        assert d[-1] == c["v"][-1] - params[0, 0]                 # v - v_sys exactly: no rotation on the centre
        assert np.all(np.isfinite(d)) and np.all(nn > 0)


@pytest.mark.parametrize("free", [False, True])
def test_membership_and_per_star_terms(free):
    case = dh.make_case(dh.DOUBLE_GB, free, 33)
    params, rec, wp = packed(case, [2])
    want_l, want_m = dh.per_star(dh.DOUBLE_GB, case["cat"], case["params"][2], case["centre"])
    out = np.empty(33)
    for mode, want in ((1, want_l), (0, want_m)):
        assert lib().double_emul_per_star(dh.DOUBLE_GB, int(free), mode, 33, rec.ctypes.data, wp.ctypes.data, out.ctypes.data) == 0
        assert np.max(np.abs(out - want.astype(np.float64)) / np.maximum(np.abs(want.astype(np.float64)), 1.0)) < 1e-11


@pytest.mark.parametrize("model", dh.MODELS)
def test_zero_second_amplitudes_give_the_single_component_gradient(model):
    """The six shared columns (and the background's) equal PROFILE's to rounding; the two `_c` amplitude columns do not
    vanish: they are the second component's own sensitivities at zero amplitude."""
    case = dh.make_case(model, False, 4099)
    rows, base_rows = dh.nested_rows(case["params"][:4])
    case["params"] = rows
    value, grad = emul_grad(case, [0, 1, 2, 3])
    base = dict(case, model=dh.BASE[model], params=base_rows)
    for j in range(4):
        want_v = vh.exact(dh.BASE[model], case["cat"], base_rows[j], case["centre"])
        assert vh.scaled_err(value[j], want_v, 4099) < 1e-12
        ref = gb.reference(base, j)
        shared = [k for k in range(grad.shape[1]) if k not in (6, 7, 8)]
        gb.check_columns(grad[j][shared], ref, (model, "nested", j))
        own = dh.reference(case, j)
        assert np.all(grad[j][[6, 7]] != 0.0)
        gb.check_columns(grad[j], own, (model, "nested, all columns", j))


def test_the_level_is_never_two():
    """No narrow-range variant: a table inside MODEL_PROFILE's level-2 domain still gets level 1, NaN rows level 0."""
    case = dh.make_case(dh.DOUBLE, False, 4099)
    single = vh.make_case(3, False, 4099)
    assert eh.fast_level_at(single["cat"], single["params"][:64], 3, single["centre"]) == 2
    assert level(case, np.arange(64)) == 1
    case["params"][5, 8] = np.nan
    assert level(case, np.arange(64)) == 0


@pytest.mark.parametrize("free", [0, 1])
@pytest.mark.parametrize("model", range(9))
def test_the_launchers_dispatcher_reaches_every_model_with_its_own_constants(model, free):
    """dispatch_any_model (csrc/mcd_dispatch.h): the seven models of dispatch_model and the two double models."""
    assert lib().double_emul_num_all_models() == 9
    calls = ctypes.c_int(0)
    assert lib().double_emul_dispatch(model, free, -7, ctypes.byref(calls)) == model * 2 + free and calls.value == 1


@pytest.mark.parametrize("model", [-1, 9, 10])
def test_the_launchers_dispatcher_calls_nothing_for_an_unknown_model(model):
    calls = ctypes.c_int(0)
    assert lib().double_emul_dispatch(model, 0, -7, ctypes.byref(calls)) == -7 and calls.value == 0

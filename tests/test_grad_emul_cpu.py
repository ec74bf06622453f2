"""Host build of csrc/mcd_grad.h (tests/emul/grad_emul.cpp) against the 80-bit test-side gradient, for every model x
{fixed, free centre} at N = 1 (the size the GPU matrix adds), 33 and 4099, in chunks of 96 stars.

Per column err = |emul - exact| / S_k (grad_helper.grad), and the rule of test_gpu_variant_matrix.py:
    err <= 2 err_np64 + FLOOR,
err_np64 being the float64 run of the test-side restatement against its own longdouble run -- what float64 arithmetic on
these inputs costs in any formulation.  FLOOR is 1e-12, and more for the free-centre cells where few stars set the scale:
grad_bounds.py holds the rule and the table of floors with their reason and measurements, shared with the GPU tests."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import emul_helper as eh
import grad_bounds as gb
import grad_helper as gh
import variant_helper as vh

pytestmark = pytest.mark.skipif(not vh.HAVE_LONGDOUBLE, reason="numpy.longdouble is not wider than float64 here")

SRC = os.path.join(eh.ROOT, "tests", "emul", "grad_emul.cpp")
OUT = os.path.join(eh.ROOT, "tests", "emul", "libmcd_grad_emul.so")
_lib = None


def lib():
    global _lib
    if _lib is None:
        deps = [SRC] + [os.path.join(eh.INC, h) for h in ("mcd_grad.h", "mcd_math.h", "mcd_exp_table.h", "mcd_dispatch.h")]
        if not os.path.exists(OUT) or any(os.path.getmtime(d) > os.path.getmtime(OUT) for d in deps):
            subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-I", eh.INC, SRC,
                            "-o", OUT], check=True)
        _lib = ctypes.CDLL(OUT)
        _lib.emul_grad.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_int64, ctypes.c_void_p, ctypes.c_void_p,
                                   ctypes.c_void_p, ctypes.c_int64, ctypes.c_int64, ctypes.c_void_p]
    return _lib


def emul_grad(case, rows, chunk_len=96):
    model, free = case["model"], case["free"]
    params = np.ascontiguousarray(case["params"][rows])
    rec = eh.pack_records(case["cat"], model, case["centre"])
    wp = eh.pack_walkers(params, model, free)
    k = lib().emul_grad_columns(model, int(free))
    assert k == params.shape[1] == gh.n_columns(model, free)
    out = np.empty((len(rows), 1 + k))
    assert lib().emul_grad(model, int(free), rec.shape[0], rec.ctypes.data, wp.ctypes.data, params.ctypes.data, len(rows),
                           chunk_len, out.ctypes.data) == 0
    return out[:, 0], out[:, 1:]


@pytest.mark.parametrize("n", [1, 33, 4099])
@pytest.mark.parametrize("free", [False, True])
@pytest.mark.parametrize("model", range(7))
def test_host_build_matches_the_80_bit_gradient(model, free, n):
    case = vh.make_case(model, free, n)
    rows = vh.sample_rows(8)
    value, grad = emul_grad(case, rows)
    for j, w in enumerate(rows):
        ref = gb.reference(case, w)
        gb.check_columns(grad[j], ref, (model, free, n, w), gb.floors(model, free, n))
        assert vh.scaled_err(value[j], vh.exact(model, case["cat"], case["params"][w], case["centre"]), n) < 1e-12


def test_sigma_zero_gives_an_exactly_zero_sigma_column():
    case = vh.make_case(2, False, 33)
    case["params"][0, 1] = 0.0
    _, grad = emul_grad(case, [0])
    assert np.all(np.isfinite(grad)) and grad[0, 1] == 0.0


def test_f_back_zero_and_certain_members_are_finite():
    for model in (2, 4, 5):
        case = vh.make_case(model, False, 33)
        case["params"][0, -1] = 0.0
        _, grad = emul_grad(case, [0])
        ref = gb.reference(case, 0)
        assert np.all(np.isfinite(grad))
        gb.check_columns(grad[0], ref, (model, "f_back = 0"))
    case = vh.make_case(1, False, 33)
    case["cat"]["pmember"][:4] = [0.0, 1.0, 0.0, 1.0]
    _, grad = emul_grad(case, [0])
    assert np.all(np.isfinite(grad))
    gb.check_columns(grad[0], gb.reference(case, 0), (1, "pmember in {0, 1}"))


@pytest.mark.parametrize("model", [0, 2])
def test_star_on_a_free_centre_adds_nothing_to_the_centre_columns(model):
    """ra = dec = 0 packs to (A, B, sin dec) = (0, 1, 0) and the centre (0, 0) then has x = y = 0 exactly: the star adds
    +0 to the two centre columns (the same bits as without it) and counts everywhere else."""
    case = vh.make_case(model, True, 33)
    c = case["cat"]
    c["ra"], c["dec"] = c["ra"] - vh.CENTRE[0], c["dec"] - vh.CENTRE[1]
    case["params"] = np.ascontiguousarray(case["params"][:3])
    case["params"][:, 4:6] -= np.array(vh.CENTRE)
    case["params"][0, 4:6] = 0.0
    c["ra"][-1], c["dec"][-1] = 0.0, 0.0
    _, g1 = emul_grad(case, [0, 1])
    _, g0 = emul_grad(dict(case, cat={k: v[:32] for k, v in c.items()}), [0, 1])
    assert np.all(np.isfinite(g1))
    assert g1[0, 4] == g0[0, 4] and g1[0, 5] == g0[0, 5]
    assert g1[0, 0] != g0[0, 0] and g1[1, 4] != g0[1, 4]


def test_profile_star_on_a_free_centre_keeps_its_true_derivative():
    """The profile models are smooth at r = 0: the star on the centre contributes its true, non-zero centre derivative."""
    case = vh.make_case(3, True, 33)
    c = case["cat"]
    c["ra"], c["dec"] = c["ra"] - vh.CENTRE[0], c["dec"] - vh.CENTRE[1]
    case["params"] = np.ascontiguousarray(case["params"][:3])
    case["params"][:, 6:8] -= np.array(vh.CENTRE)
    case["params"][0, 6:8] = 0.0
    c["ra"][-1], c["dec"][-1] = 0.0, 0.0
    _, g1 = emul_grad(case, [0])
    _, g0 = emul_grad(dict(case, cat={k: v[:32] for k, v in c.items()}), [0])
    assert np.all(np.isfinite(g1)) and g1[0, 6] != g0[0, 6] and g1[0, 7] != g0[0, 7]
    gb.check_columns(g1[0], gb.reference(case, 0), "profile, star on the centre", gb.floors(3, True, 33))

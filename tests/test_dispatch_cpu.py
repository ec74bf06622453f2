"""Host build of csrc/mcd_dispatch.h (tests/emul/dispatch_emul.cpp): every runtime (model, free_centre) pair and every
precision must reach the functor with its own compile-time constants, and a model outside the list must reach nothing."""
import ctypes
import os
import subprocess

import pytest

import emul_helper as eh

SRC = os.path.join(eh.ROOT, "tests", "emul", "dispatch_emul.cpp")
OUT = os.path.join(eh.ROOT, "tests", "emul", "libdispatch_emul.so")
_lib = None


def lib():
    global _lib
    if _lib is None:
        deps = [SRC] + [os.path.join(eh.INC, h) for h in ("mcd_dispatch.h", "mcd_math.h", "mcd_exp_table.h")]
        if not os.path.exists(OUT) or any(os.path.getmtime(d) > os.path.getmtime(OUT) for d in deps):
            subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-I", eh.INC, SRC,
                            "-o", OUT], check=True)
        _lib = ctypes.CDLL(OUT)
    return _lib


def dispatch(model, free, fallback=-7):
    calls = ctypes.c_int(0)
    got = lib().emul_dispatch_model(int(model), int(free), fallback, ctypes.byref(calls))
    return got, calls.value


def test_model_count():
    assert lib().emul_num_models() == 7


@pytest.mark.parametrize("free", [0, 1])
@pytest.mark.parametrize("model", range(7))
def test_every_pair_reaches_its_own_constants(model, free):
    assert dispatch(model, free) == (model * 2 + free, 1)


@pytest.mark.parametrize("free", [0, 1])
@pytest.mark.parametrize("model", [-1, 7])
def test_unknown_model_returns_the_fallback_without_a_call(model, free):
    assert model in (-1, lib().emul_num_models())
    assert dispatch(model, free, fallback=-7) == (-7, 0)


def test_term_type():
    assert [lib().emul_dispatch_term_bytes(p) for p in (0, 1, 2)] == [8, 4, 4]

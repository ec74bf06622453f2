"""The guard's verdicts for models 0 .. 8 are what they were before the error-scale models (no GPU).

guard_verdict's variance bounds became fma(es2_min, e2_min, ...) / fma(es2_max, e2_max, ...) with es2_min = es2_max = 1 for
every model but the two new ones, and ParamRanges grew by two fields.  PINNED holds, for models 0 .. 8 x fixed / free centre x
48 seeded random tables each, what tests/emul/guard_pin_emul.cpp returned when it was built against csrc/mcd_guard.h and
csrc/mcd_math.h of the commit BEFORE the error-scale models (the source uses no name that commit lacked; `pins()` below is
the function that made the table, called with that commit's csrc directory): guard_verdict, level_verdict and a SHA-256 of the
bytes of GuardRanges.n_min / n_max.  The test builds the same source against the tree's headers and compares with equality:
levels and verdicts digit for digit, n_min / n_max bit for bit.

The tables are made to land on both sides of the guard: the catalogue's verr is rescaled by a power of ten from
{0, 0, -30, 28, 110} and one random column of the walker table by 10^U(-40, 40) in three tables of four, so that every cell
sees refusals (level 0) next to admitted tables, and the cells with a narrow-range variant level 2 as well."""
import ctypes
import hashlib
import os
import subprocess

import numpy as np
import pytest

import double_helper as dh
import emul_helper as eh
import variant_helper as vh

SRC = os.path.join(eh.ROOT, "tests", "emul", "guard_pin_emul.cpp")
N_TABLES, N_ROWS, N_STARS = 48, 16, 33
CELLS = [(m, f) for m in range(9) for f in (False, True)]
_libs = {}


def lib(inc=eh.INC, out=None):
    out = os.path.join(eh.ROOT, "tests", "emul", "libmcd_guard_pin_emul.so") if out is None else out
    if out not in _libs:
        deps = [SRC] + [os.path.join(inc, h) for h in ("mcd_guard.h", "mcd_math.h", "mcd_exp_table.h")]
        if not os.path.exists(out) or any(os.path.getmtime(d) > os.path.getmtime(out) for d in deps):
            subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-I", inc, SRC, "-o", out], check=True)
        handle = ctypes.CDLL(out)
        handle.guard_pin.restype = None
        handle.guard_pin.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_int64] + [ctypes.c_void_p] * 7 + \
            [ctypes.c_double, ctypes.c_double, ctypes.c_int, ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p]
        _libs[out] = handle
    return _libs[out]


def tables(model, free):
    """(catalogue columns, (N_ROWS, K) table) x N_TABLES of one cell, seeded by the cell."""
    case = dh.make_case(model, free, N_STARS) if model in dh.MODELS else vh.make_case(model, free, N_STARS)
    rng = np.random.default_rng(31000 + 100 * model + int(free))
    for t in range(N_TABLES):
        cat = {k: np.array(v, copy=True) for k, v in case["cat"].items()}
        cat["verr"] = cat["verr"] * 10.0 ** float(rng.choice([0, 0, -30, 28, 110]))
        rows = np.array(case["params"][t:t + N_ROWS], copy=True)
        if t % 4:
            rows[:, rng.integers(rows.shape[1])] *= 10.0 ** rng.uniform(-40.0, 40.0)
        yield cat, np.ascontiguousarray(rows)


def cell(handle, model, free):
    """(levels as a string of digits, verdicts likewise, SHA-256 of the n_min / n_max bytes) of one cell."""
    centre = None if free else vh.CENTRE
    levels, verdicts, digest = "", "", hashlib.sha256()
    for cat, rows in tables(model, free):
        cols = [np.ascontiguousarray(cat[k], dtype=np.float64) if k in cat else None
                for k in ("ra", "dec", "v", "verr", "lnlike_bg", "pmember", "density")]
        out = np.zeros(4)
        rc, dc = (0.0, 0.0) if centre is None else centre
        handle.guard_pin(model, int(free), len(cat["v"]), *[a.ctypes.data if a is not None else None for a in cols], rc, dc,
                         rows.shape[1], rows.ctypes.data, rows.shape[0], out.ctypes.data)
        verdicts += str(int(out[0]))
        levels += str(int(out[1]))
        digest.update(out[2:].tobytes())
    return levels, verdicts, digest.hexdigest()[:16]


def pins(inc, out):
    """The table PINNED for the headers under `inc` (how it was made: inc = csrc of the commit before the new models)."""
    return {(m, f): cell(lib(inc, out), m, f) for m, f in CELLS}


PINNED = {
    (0, False): ("101110101000011011011000000111011000110011000001", "101110101000011011011000000111011000110011000001", "bb9e2192dbe9e9fd"),
    (0, True): ("111100111000100110011001111101000010100111101000", "111100111000100110011001111101000010100111101000", "4d313122b0965d6a"),
    (1, False): ("202202022200200022020202222220120022000022002202", "101101011100100011010101111110110011000011001101", "863efb2c47811274"),
    (1, True): ("200022002022220020202222200222020202222222002220", "100011001011110010101111100111010101111111001110", "b28156e3d095f3be"),
    (2, False): ("020100012111022122012111210021002201010120102100", "010100011111011111011111110011001101010110101100", "60b1ab10b1ba2659"),
    (2, True): ("122222021022000021002001210000002012220021200010", "111111011011000011001001110000001011110011100010", "0b6b315455ea1c3b"),
    (3, False): ("000220000020200200100001020022200202002000002000", "000110000010100100100001010011100101001000001000", "730876acbd39dd9a"),
    (3, True): ("100110011000111000000000000100101000100000100100", "100110011000111000000000000100101000100000100100", "4a6fc9cbd6b51d73"),
    (4, False): ("000020020001012002002021101010120001022120200000", "000010010001011001001011101010110001011110100000", "0360da729f5f68f4"),
    (4, True): ("110121012102122012200001002011102120111020111220", "110111011101111011100001001011101110111010111110", "ac5b3572a2633b79"),
    (5, False): ("200020012100202220022020220222000021202200022000", "100010011100101110011010110111000011101100011000", "1b2c791910c3ecf2"),
    (5, True): ("002000002020020220202012022022222221220020222000", "001000001010010110101011011011111111110010111000", "c7f8e44dc076ba40"),
    (6, False): ("010110011010011101101001011100101000000101000000", "010110011010011101101001011100101000000101000000", "cd564d22640ad9c5"),
    (6, True): ("101101100010011111000000100111110111001011100101", "101101100010011111000000100111110111001011100101", "49a94d0fe6d8fdc2"),
    (7, False): ("000100001100011110011011100001000001110100001000", "000100001100011110011011100001000001110100001000", "774164711db502e4"),
    (7, True): ("101010010000010001010010100010111000011110101000", "101010010000010001010010100010111000011110101000", "fd0892522ccc6831"),
    (8, False): ("101010100110000110011000110011111111001111001100", "101010100110000110011000110011111111001111001100", "76fea51fda358718"),
    (8, True): ("010100111010110011100010101010011111001101000001", "010100111010110011100010101010011111001101000001", "f7ad3c62f94efcab"),
}


@pytest.mark.parametrize("model, free", CELLS)
def test_verdicts_levels_and_variance_bounds_of_models_0_to_8_are_unchanged(model, free):
    got = cell(lib(), model, free)
    assert got == PINNED[(model, free)], (model, free, got, PINNED[(model, free)])


def test_the_pinned_tables_land_on_both_sides_of_the_guard():
    assert sorted(PINNED) == sorted(CELLS)
    for (model, free), (levels, verdicts, _) in PINNED.items():
        assert len(levels) == len(verdicts) == N_TABLES
        assert "0" in levels and ("1" in levels or "2" in levels), (model, free, levels)
        assert all((v == "0") == (l == "0") for v, l in zip(verdicts, levels))
    assert any("2" in levels for levels, _, _ in PINNED.values()) and any("1" in levels for levels, _, _ in PINNED.values())

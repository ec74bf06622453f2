"""Test helper: the accuracy rule of the gradient tests, shared by the host-build test (test_grad_emul_cpu.py) and the GPU
tests (test_gpu_grad*.py).  Test infrastructure only.

Per column, err = |got - exact| / S_k with exact and S_k from the longdouble run of grad_helper, and
    err <= 2 err_np64 + FLOOR
where err_np64 is the float64 run of the SAME restatement against its longdouble run (the rule of
test_gpu_variant_matrix.py): what float64 costs on these inputs in any formulation, with a factor 2 for the different
order of operations.  FLOOR = 1e-12 for every cell unless FREE_FLOOR names it: ~5e3 ulps of S_k, the room a sum of up
to 4099 float64 terms and libm (log, exp: a few ulps each) may take where err_np64 happens to be tiny.

FREE_FLOOR: free-centre cells whose floor is larger, for ONE cause.  The free-centre record holds A = cos(dec) sin(ra),
B = cos(dec) cos(ra), and the offsets are x = B sin(ra_c) - A cos(ra_c), y = ...: differences of O(0.4) products that cancel
to the stars' separations of 5e-5 .. 2e-4 rad (0.003 .. 0.01 deg from the walkers' centres in make_case), so x and y carry
~1e-12 relative error in float64 whatever follows.  The restatement in grad_helper.py forms sin(ra - ra_c) from the
difference of the angles and does not have that error, so err_np64 does not cover it.  The GEOMETRY columns (v_maxx, v_maxy,
r_peak, the centre) take it through sin / cos(theta) and their 1 / r conditioning; the other columns only through the
residual d, an order of magnitude less.  With N = 1 (N = 33) one star (a few stars) set S_k: a derivative that itself nearly
cancels has nothing to be measured against.  The fixed-centre cells run the same arithmetic on records without that
cancellation and stay below 2e-15 over the same rows, which isolates the cause.

Measured with the host build of csrc/mcd_grad.h as the largest err - 2 err_np64 over ALL 257 walker rows of make_case that
the GPU matrix can reach, free centre, models 0 .. 6 (`python tests/grad_floor_sweep.py` prints these two tables; at
N = 4099, planted cases included, every figure is below 2.4e-13):
    geometry columns   N = 1:  2.02e-11  3.09e-12  7.06e-10  1.23e-11  1.78e-10  1.01e-10  3.11e-10
                       N = 33: 4.59e-13  6.35e-13  6.90e-13  1.53e-12  4.51e-13  7.07e-13  7.35e-13
    other columns      N = 1:  1.92e-13  1.09e-12  3.15e-11  5.30e-13  2.03e-11  1.11e-11  2.47e-12
                       N = 33: 8.14e-14  1.93e-13  9.52e-14  1.66e-13  3.56e-13  3.18e-13  1.80e-13
Each floor is max(1e-12, 2 x measured); the device is held to the same table (its libm draws other roundings of the same
sines and cosines)."""
import hashlib

import numpy as np

import grad_helper as gh
import variant_helper as vh

FLOOR = 1e-12
GEOMETRY_COLUMNS = ("v_maxx", "v_maxy", "r_peak", "ra_center", "dec_center")
# (model, N) -> (floor of the geometry columns, floor of the other columns), free centre
FREE_FLOOR = {(0, 1): (4.1e-11, FLOOR), (1, 1): (6.2e-12, 2.2e-12), (2, 1): (1.5e-9, 6.4e-11), (3, 1): (2.5e-11, 1.1e-12),
              (4, 1): (3.6e-10, 4.1e-11), (5, 1): (2.1e-10, 2.3e-11), (6, 1): (6.3e-10, 5.0e-12),
              (1, 33): (1.3e-12, FLOOR), (2, 33): (1.4e-12, FLOOR), (3, 33): (3.1e-12, FLOOR), (5, 33): (1.5e-12, FLOOR),
              (6, 33): (1.5e-12, FLOOR)}
_cache = {}


def is_geometry(model, free):
    """Boolean per column: does it read sin / cos(theta) or the offsets themselves?"""
    return np.array([name in GEOMETRY_COLUMNS for name in gh.column_names(model, free)])


def floors(model, free, n):
    """The floor of every column of cell (model, free centre, N stars)."""
    geometry, other = FREE_FLOOR.get((model, n), (FLOOR, FLOOR)) if free else (FLOOR, FLOOR)
    return np.where(is_geometry(model, free), geometry, other)


def reference(case, w):
    """{"g": longdouble gradient, "s": S_k, "err64": err_np64 per column} of walker row w of `case` (computed once)."""
    digest = hashlib.sha1()
    for name in sorted(case["cat"]):
        digest.update(np.ascontiguousarray(case["cat"][name]).tobytes())
    key = (case["model"], case["free"], w, case["params"][w].tobytes(), digest.hexdigest())
    if key not in _cache:
        args = (case["model"], case["cat"], case["params"][w], case["centre"])
        g80, s80 = gh.grad(*args, vh.L)
        g64, _ = gh.grad(*args, np.float64)
        _cache[key] = {"g": g80, "s": s80, "err64": gh.col_err(g64, g80, s80)}
    return _cache[key]


def check_columns(got, ref, cell, column_floor=FLOOR):
    """`column_floor`: one number, or one per column (floors() above)."""
    err = gh.col_err(got, ref["g"], ref["s"])
    bound = 2 * ref["err64"] + column_floor
    bad = err > bound
    assert not bad.any(), (cell, "columns", np.nonzero(bad)[0].tolist(), "err", err[bad].tolist(), "bound",
                           bound[bad].tolist())
    return err

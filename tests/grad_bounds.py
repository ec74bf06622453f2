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
sines and cosines).

LARGE_FLOOR: the catalogues of test_gpu_grad_plans.py have up to 5.2e5 stars, 128 x the 4099 terms FLOOR was argued for, so
every floor used beyond 4099 stars is listed per (model, centre) with the size up to which it was measured; floors() refuses
a larger catalogue or an unlisted model instead of assuming 1e-12.  Measured as above (host build of csrc/mcd_grad.h in
chunks of 64 stars, added in chunk order; largest err - 2 err_np64) over EVERY walker row that module can reach and at every
prefix length it uses (`python tests/grad_floor_sweep.py plans`; plan_cells() below lists the catalogues):
    slot counts, rows 0 .. 129      model 0 fixed   N = 16307 .. 524339:  geometry 2.36e-15   other 3.17e-15  (at 524339)
                                    model 1 fixed   N = 16307 .. 262195:  geometry 1.49e-15   other 2.15e-15
                                    model 4 free    N = 16307 .. 262195:  geometry 1.73e-13   other 3.56e-14  (at 16307;
                                                    1.60e-13 / 3.52e-14 at 262195: the cancellation, not the length)
                                    model 4 free    N = 51:               geometry 4.02e-13   other 1.77e-13
    balanced, rows 0 .. 129         model 0 fixed   N = 140009:           geometry 5.56e-16   other 1.78e-15
                                    model 2 fixed   N = 140009:           geometry 8.89e-16   other 2.86e-15
    sorted, rows 0 .. 256           model 1 fixed   N = 20011:            geometry 1.23e-16   other 5.66e-16
                                    ... planted     N = 20011:            geometry 1.08e-16   other 5.77e-16
    long bin (stars 65 .. 19170     model 2 fixed   N = 19106:            geometry 3.46e-16   other 8.93e-16
    of 24001), rows 0 .. 319        model 5 fixed   N = 19106:            geometry 8.57e-17   other 7.18e-16
                                    model 3 free    N = 19106:            geometry 1.80e-13   other 1.09e-13
2 x measured is below 1e-12 in every line: each floor of LARGE_FLOOR is 1e-12.  The length of the sum does not show: the
fixed-centre figures grow from 3e-16 at 1.6e4 stars to 3e-15 at 5.2e5, and the free-centre ones are the record format's
cancellation at any length.  (N = 51, model 4 free: below the 1e-12 that floors() gives an N without an entry in FREE_FLOOR.)

The one-star bin of that module (star 0 of make_case(model, centre, 24001)) takes the N = 1 floors above.  For the free-
centre model 3 that star lies 0.0100 deg from CENTRE, the star of make_case(3, True, 1) 0.0227 deg, and the N = 1 figures
depend on the star: over all 320 rows of the bin's walker table the host build reaches 2.17e-9 (geometry) and 1.63e-10
(other columns), above the (3, 1) entry, on rows whose centre derivative nearly cancels.  At the twelve rows the module
samples (vh.sample_rows of W = 65 and 320) it stays at 6.06e-12 and 6.93e-13, inside the entry, which is held unchanged;
fixed centre, models 2 and 5: 3.78e-15 and 1.87e-15 over all 320 rows."""
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
# (model, free centre) -> (largest N measured, floor of the geometry columns, floor of the other columns), N > 4099
LARGE_FLOOR = {(0, False): (524339, FLOOR, FLOOR), (1, False): (262195, FLOOR, FLOOR), (2, False): (140009, FLOOR, FLOOR),
               (5, False): (19106, FLOOR, FLOOR), (3, True): (19106, FLOOR, FLOOR), (4, True): (262195, FLOOR, FLOOR)}
LARGE_N = 4099                                            # the largest N that FLOOR itself was argued and measured for
_cache = {}

# ---- the catalogues of test_gpu_grad_plans.py: the sizes beyond the 4099 stars FLOOR was argued for ----------------------
PLAN_CHUNK = 64                                           # option "chunk_len": the smallest nominal length the planner accepts
PLAN_SLOTS = (1, 255, 256, 257, 1023, 1024, 1025, 4095, 4096, 4097)
PLAN_SLOTS_EXTRA = {0: (8193,)}                           # model -> further slot counts (three rounds of the several-round shape)
PLAN_SLOT_MODELS = ((0, False), (1, False), (4, True))
PLAN_SLOT_WALKERS = (3, 9, 64, 130)
PLAN_BALANCED_N, PLAN_BALANCED_MODELS, PLAN_BALANCED_WALKERS = 140009, ((0, False), (2, False)), (64, 9, 130)
PLAN_SORTED_N, PLAN_SORTED_WALKERS = 20011, (1, 65, 257)  # model 1, fixed centre, plain and planted
PLAN_BINNED_MODELS, PLAN_BINNED_WALKERS = ((2, False), (5, False), (3, True)), (65, 320)
PLAN_BIN_OFFSETS = (0, 0, 1, 65, PLAN_CHUNK * 300 - 29, 24001)     # empty, one star, one chunk, 299 chunks, the rest (76)
PLAN_LONG_BIN, PLAN_STAR_BIN = 3, 1


def plan_slot_counts(model):
    return PLAN_SLOTS + PLAN_SLOTS_EXTRA.get(model, ())


def plan_prefix(slots):
    """Stars of the prefix catalogue with exactly `slots` chunks of PLAN_CHUNK stars, the last one ragged."""
    return PLAN_CHUNK * slots - 13


def sub_case(case, sl, params=None):
    """The stars `sl` of `case` as a case of their own (optionally with another walker table)."""
    cat = {k: v[sl] for k, v in case["cat"].items()}
    return dict(case, cat=cat, n=len(cat["v"]), planted=[], params=case["params"] if params is None else params)


def plan_cells():
    """(name, case, prefix lengths, walker rows the GPU module can reach) of every catalogue of test_gpu_grad_plans.py:
    what grad_floor_sweep.py measures LARGE_FLOOR on.  The cases are built on demand (the largest has 5.2e5 stars)."""
    for model, free in PLAN_SLOT_MODELS:
        lengths = [plan_prefix(s) for s in plan_slot_counts(model)]
        yield ("slots", model, free), (lambda m=model, f=free, n=max(lengths): vh.make_case(m, f, n)), lengths, \
            range(max(PLAN_SLOT_WALKERS))
    for model, free in PLAN_BALANCED_MODELS:
        yield ("balanced", model, free), (lambda m=model, f=free: vh.make_case(m, f, PLAN_BALANCED_N)), [PLAN_BALANCED_N], \
            range(max(PLAN_BALANCED_WALKERS))
    for plant in (False, True):
        yield ("sorted, planted" if plant else "sorted", 1, False), \
            (lambda p=plant: vh.make_case(1, False, PLAN_SORTED_N, plant=p)), [PLAN_SORTED_N], range(max(PLAN_SORTED_WALKERS))
    for model, free in PLAN_BINNED_MODELS:
        for b, name in ((PLAN_LONG_BIN, "long bin"), (PLAN_STAR_BIN, "one-star bin")):
            lo, hi = PLAN_BIN_OFFSETS[b], PLAN_BIN_OFFSETS[b + 1]
            yield (name, model, free), \
                (lambda m=model, f=free, lo=lo, hi=hi: sub_case(vh.make_case(m, f, PLAN_BIN_OFFSETS[-1]), slice(lo, hi))), \
                [hi - lo], range(max(PLAN_BINNED_WALKERS))


def is_geometry(model, free):
    """Boolean per column: does it read sin / cos(theta) or the offsets themselves?"""
    return np.array([name in GEOMETRY_COLUMNS for name in gh.column_names(model, free)])


def floors(model, free, n):
    """The floor of every column of cell (model, free centre, N stars)."""
    if n > LARGE_N:
        assert (model, bool(free)) in LARGE_FLOOR, ("no host-build figure behind a floor of this model beyond 4099 stars", model, free)
        n_max, geometry, other = LARGE_FLOOR[(model, bool(free))]
        assert n <= n_max, ("no host-build figure behind a floor at this size", model, free, n, n_max)
    else:
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


def prefix_reference(case, w, lengths):
    """{n: reference(first n stars of `case`, w)} for every n of `lengths`, from ONE evaluation of the (K, N) term matrix
    per number format: every term of grad_helper.per_star depends on its own star alone, so the first n columns ARE the
    term matrix of the prefix catalogue.  Each prefix is summed on its own slice with the summation of grad_helper.grad
    (numpy's pairwise sum) rather than read off a running sum: the results then equal reference() of the sliced catalogue
    bit for bit (test_grad_oracle_cpu.py), and err_np64 stays what the float64 restatement costs -- a sequential float64
    running sum of 5e5 terms would lose more and WIDEN the bound."""
    lengths = sorted({int(n) for n in lengths})
    assert lengths and 0 < lengths[0] and lengths[-1] <= case["n"]
    digest = hashlib.sha1()
    for name in sorted(case["cat"]):
        digest.update(np.ascontiguousarray(case["cat"][name]).tobytes())
    key = ("prefix", case["model"], case["free"], w, case["params"][w].tobytes(), digest.hexdigest())
    missing = [n for n in lengths if key + (n,) not in _cache]
    if missing:
        sl = slice(0, missing[-1])
        args = (case["model"], {k: v[sl] for k, v in case["cat"].items()}, case["params"][w], case["centre"])
        t80, t64 = gh.per_star(*args, vh.L), gh.per_star(*args, np.float64)
        for n in missing:
            g80, s80 = t80[:, :n].sum(axis=1), np.abs(t80[:, :n]).sum(axis=1)
            _cache[key + (n,)] = {"g": g80, "s": s80, "err64": gh.col_err(t64[:, :n].sum(axis=1), g80, s80)}
    return {n: _cache[key + (n,)] for n in lengths}


def check_columns(got, ref, cell, column_floor=FLOOR):
    """`column_floor`: one number, or one per column (floors() above)."""
    err = gh.col_err(got, ref["g"], ref["s"])
    bound = 2 * ref["err64"] + column_floor
    bad = err > bound
    assert not bad.any(), (cell, "columns", np.nonzero(bad)[0].tolist(), "err", err[bad].tolist(), "bound",
                           bound[bad].tolist())
    return err

"""GPU: mcd_loglike_grad_batch on the work sets the value path plans for it -- chunk tables, record order and reduction
shapes that tests/test_gpu_grad.py (balance 0, chunk_len 96, at most 43 chunks, catalogue order) never reaches.

The gradient kernel (csrc/mcd_grad.hip) plans nothing itself: it runs on the chunk table and the record array of the value
path's work set for that walker count and hands its 1 + K fields to the value path's launch_reduce as (1 + K) x
roundup64(W) pseudo-walkers with one slot per chunk.  Every cell below names the plan it means to run and checks through
launch_info() of a value call on the same work set that it did: a planner change that moves a cell off its boundary fails
the cell instead of emptying it.

The accuracy rule is grad_bounds.py's: per column err = |device - exact| / S_k <= 2 err_np64 + floor, exact / S_k / err_np64
from the longdouble and float64 runs of grad_helper, the floors from the host build of csrc/mcd_grad.h
(grad_bounds.floors; LARGE_FLOOR for the sizes beyond 4099 stars, measured by grad_floor_sweep.py, never on a device).

  1. test_slot_counts_on_the_reduction_shape_boundaries -- multi-round table, catalogue order (balance 0, combine 0,
     tail_split 0, chunk_len 64), the first 64 slots - 13 stars of one make_case, slots in {1, 255, 256, 257, 1023, 1024,
     1025, 4095, 4096, 4097} x W in {3, 9, 64, 130}, rows 0, W // 2, W - 1, for model 0 fixed centre (5 fields; also 8193
     slots), model 1 fixed centre (the value field carries lnL_bg itself: the gradient's reduction gets no pset_const) and
     model 4 free centre (12 fields, the widest).  Reduction shapes: reduce_group_kernel<8, 16, one round> up to 256
     slots, <32, 16, one round> up to 1024, <128, 16, one round> up to 4096, <128, 16, several rounds> beyond (two rounds
     at 4097, three at 8193).  W = 3 and 9 leave padding lanes in the only walker tile, 130 has a ragged third tile.
  2. test_balanced_one_round_plans -- N = 140009, balance in {2, 4, 8} x combine in {0, 8, 16} x W in {64, 9, 130}, models
     0 and 2 fixed centre: the arithmetic one-round table (1024 m chunks for one walker tile, ceil(1024 m / 3) for three),
     whose value launch combines chunks in 8- / 16-wave workgroups and reduces one slot per workgroup while the gradient
     keeps one slot per chunk -- 2048, 4096 and 8192 of them (the <128, 16> shapes, one round and two).  combine must not
     change a bit of the gradient.  test_default_plan runs one cell with every option at its default (balance -1).
  3. test_verr_sorted_records -- model 1 fixed centre, N = 20011, plain and with planted certain members, verr_sorted 1
     (forced: the catalogue is below the 8 MiB of records from which it is the default) x chunk_len in {0, 64} x W in {1,
     65, 257}: the gradient must read records_sorted with the chunk table planned on it.  chunk_len 64: 313 chunks, the
     four-wave reduction; chunk_len 0: the balanced table (1024 / 1024 / 512 chunks).  1 -> 0 -> 1 on one open catalogue.
  4. test_binned_catalogue_of_very_unequal_bins -- models 2 and 5 fixed centre, 3 free centre, bin_offsets [0, 0, 1, 65,
     64 x 300 - 29, 24001] (empty, one star, one chunk, 299 chunks, 76 chunks), chunk_len 64, W in {65, 320}, another
     walker table per bin: launch_reduce with several parameter sets (slot ranges from the offsets array, the shape chosen
     by the longest set: four waves, inside which the shorter sets must keep the one-wave order of a launch of their own --
     the bin of 76 chunks did not before this module), W = 320 on the XCD-grouped grid.
  5. test_hmc_block_on_sorted_records -- bgfixed, N = 20011, W = 65, n_leap 3, verr_sorted 1, chunk_len 64 (313 chunks):
     the resident block's own launches of the gradient and its reduction on that work set.

Host time is dominated by the longdouble references: one evaluation of the (K, N) term matrix per (case, row) serves
every prefix (grad_bounds.prefix_reference); model 4 at 4097 slots takes about half a second per row, so all three rows
stay.  The whole module runs in under half a minute."""
import numpy as np
import pytest

import grad_bounds as gb
import grad_helper as gh
import variant_helper as vh

pytestmark = pytest.mark.gpu

CHUNK = gb.PLAN_CHUNK
VALUE_TOL = 1e-12


@pytest.fixture(scope="module")
def native():
    from mcmc_dynamics_amd import _native
    return _native


@pytest.fixture(scope="module")
def ctx(native):
    return native.default_context()


def set_options(cat, **options):
    for key, value in options.items():
        cat.set_option(key, value)


def evaluate(cat, params, cell):
    """Value and gradient, called twice: finite and the same bytes."""
    value, grad = cat.loglike_grad(params)
    again = cat.loglike_grad(params)
    assert np.all(np.isfinite(value)) and np.all(np.isfinite(grad)), ("not finite", cell)
    assert value.tobytes() == again[0].tobytes() and grad.tobytes() == again[1].tobytes(), ("not repeatable", cell)
    return value, grad


def value_launch(cat, params, fast):
    """A value call on the gradient's work set (same walker count, same plan options): its output and launch_info()."""
    cat.set_option("fast_path", 1 if fast else 0)
    out = cat.loglike(params)
    info = cat.launch_info()
    if fast:
        assert cat.fast_level > 0 and cat.rerun_count == 0, ("the fast kernels were meant to run", cat.fast_level)
    cat.set_option("fast_path", 1)
    return out, info


def main_grid(chunks, w):
    """mcd_chunks.h: main_grid -- workgroups of a launch that does not combine its chunks."""
    t = vh.n_wtiles(w)
    return -(-chunks * t // 4) if t <= 4 else -(-chunks // 8) * 8 * -(-t // 4)


class Rule:
    """Collects err - 2 err_np64 per checked row, prints the worst figure per group, fails at the end with every miss."""

    def __init__(self):
        self.log, self.failures = {}, []

    def check(self, group, cell, got, ref, floor, factor=1.0, other=None):
        """`got` against the reference under `factor` x (2 err_np64 + floor); with `other`: |got - other| / S_k instead."""
        want = ref["g"] if other is None else other
        err = gh.col_err(got, want, ref["s"])
        bound = factor * (2 * ref["err64"] + floor)
        excess = float(np.max(err - factor * 2 * ref["err64"]))
        if group not in self.log or excess > self.log[group][0]:
            self.log[group] = (excess, cell, int(np.argmax(err - factor * 2 * ref["err64"])))
        if np.any(err > bound):
            self.failures.append((group, cell, err.tolist(), bound.tolist()))

    def finish(self):
        for group, (excess, cell, column) in self.log.items():
            print("{0}: worst err - 2 err_np64 = {1:.3e} at {2}, column {3}".format(group, excess, cell, column))
        assert not self.failures, self.failures


# ---------------------------------------------------------------------------------- 1. slot counts on the shape boundaries
@pytest.mark.parametrize("model,free", gb.PLAN_SLOT_MODELS, ids=["const", "bgfixed", "profile_bggauss_free"])
def test_slot_counts_on_the_reduction_shape_boundaries(native, ctx, model, free):
    counts = gb.plan_slot_counts(model)
    lengths = [gb.plan_prefix(s) for s in counts]
    case = vh.make_case(model, free, max(lengths))
    rows = sorted({r for w in gb.PLAN_SLOT_WALKERS for r in (0, w // 2, w - 1)})
    refs = {r: gb.prefix_reference(case, r, lengths) for r in rows}
    rule = Rule()
    for slots, n in zip(counts, lengths):
        cat = vh.catalog(native, ctx, case, slice(0, n))
        set_options(cat, balance=0, combine=0, tail_split=0, chunk_len=CHUNK)
        floor = gb.floors(model, free, n)
        for w in gb.PLAN_SLOT_WALKERS:
            cell = (model, slots, w)
            params = np.ascontiguousarray(case["params"][:w])
            value, grad = evaluate(cat, params, cell)
            assert value.shape == (w,) and grad.shape == (w, gh.n_columns(model, free))
            plain, info = value_launch(cat, params, fast=False)
            assert (info["chunks"], info["workgroups"]) == (slots, main_grid(slots, w)), (cell, info)
            # every row, the padding rows of every walker group beside them, against the plain value kernels on this plan
            assert np.all(vh.scaled_err(value, plain, n) < VALUE_TOL), (cell, float(np.max(vh.scaled_err(value, plain, n))))
            for r in (0, w // 2, w - 1):
                rule.check("slots {0}".format(slots), cell + (r,), grad[r], refs[r][n], floor)
        cat.close()
    rule.finish()


# ---------------------------------------------------------------------------------- 2. balanced one-round plans
def balanced_launch(model, w, m, combine):
    """(chunks, workgroups of the fast value launch) of the one-round plan with m workgroups per CU (mcd_chunks.h:
    balanced_chunk_count; mcd_api_catalog.hip: build_workset): 8-wave workgroups for an even m and 1, 2 or 4 walker tiles,
    16-wave ones for combine 16 and m % 4 == 0 except for the per-walker Gaussian background (more than 128 VGPRs)."""
    t = vh.n_wtiles(w)
    chunks = (1024 * m + 2) // 3 if t == 3 else 256 * m * (4 // t)
    waves = 4
    if combine and t in (1, 2, 4) and m % 2 == 0:
        waves = 16 if combine == 16 and m % 4 == 0 and vh.BG_OF[model] != vh.BG_GAUSS else 8
    return chunks, -(-chunks * t // waves)


@pytest.mark.parametrize("model,free", gb.PLAN_BALANCED_MODELS, ids=["const", "const_bggauss"])
def test_balanced_one_round_plans(native, ctx, model, free):
    n = gb.PLAN_BALANCED_N
    case = vh.make_case(model, free, n)
    floor = gb.floors(model, free, n)
    cat = vh.catalog(native, ctx, case)
    rule = Rule()
    for m in (2, 4, 8):
        bits = {}
        for combine in (0, 8, 16):
            set_options(cat, balance=m, combine=combine)
            for w in gb.PLAN_BALANCED_WALKERS:
                cell = (model, m, combine, w)
                params = np.ascontiguousarray(case["params"][:w])
                value, grad = evaluate(cat, params, cell)
                _, info = value_launch(cat, params, fast=True)
                assert (info["chunks"], info["workgroups"]) == balanced_launch(model, w, m, combine), (cell, info)
                if w == 64:
                    assert info["chunks"] == 1024 * m                      # 2048, 4096, 8192 slots of the gradient
                    if combine:
                        assert 4 * info["workgroups"] < info["chunks"], ("the value launch did not combine", cell, info)
                plain, info = value_launch(cat, params, fast=False)
                assert info["chunks"] == balanced_launch(model, w, m, combine)[0], (cell, info)
                assert np.all(vh.scaled_err(value, plain, n) < VALUE_TOL), cell
                # combine changes the value launch only: the gradient writes and adds one slot per chunk as before
                first = bits.setdefault(w, (combine, value.tobytes(), grad.tobytes()))
                assert (value.tobytes(), grad.tobytes()) == first[1:], ("combine changed the gradient", cell, first[0])
                for r in vh.sample_rows(w):
                    rule.check("balance {0}".format(m), cell + (r,), grad[r], gb.reference(case, r), floor)
    cat.close()
    rule.finish()


@pytest.mark.parametrize("model,free", gb.PLAN_BALANCED_MODELS, ids=["const", "const_bggauss"])
def test_default_plan(native, ctx, model, free):
    """Every option at its default (balance -1, combine 1): mcd_api_catalog.hip: balance_auto_m gives 140009 stars x 64
    walkers m = 2 for MODEL_CONST (3.5e4 units of work, below 6e4) and m = 4 for MODEL_CONST_BGGAUSS (45 / 8.5 as much)."""
    n, w = gb.PLAN_BALANCED_N, 64
    case = vh.make_case(model, free, n)
    cat = vh.catalog(native, ctx, case)
    params = np.ascontiguousarray(case["params"][:w])
    value, grad = evaluate(cat, params, (model, "defaults"))
    _, info = value_launch(cat, params, fast=True)
    m = {0: 2, 2: 4}[model]
    assert (info["chunks"], info["workgroups"]) == balanced_launch(model, w, m, 16 if m == 4 else 8), info
    plain, _ = value_launch(cat, params, fast=False)
    cat.close()
    assert np.all(vh.scaled_err(value, plain, n) < VALUE_TOL)
    rule = Rule()
    for r in vh.sample_rows(w):
        rule.check("defaults", (model, w, r), grad[r], gb.reference(case, r), gb.floors(model, free, n))
    rule.finish()


# ---------------------------------------------------------------------------------- 3. verr-sorted records
# chunk_len 0: the balanced table.  balance_auto_m gives m = 2, 2, 4 for W = 1, 65, 257 (24 / 8.5 x 20011 x tiles / 4 units
# of work); 2048 chunks for one walker tile would hold 8 stars each, fewer than 16, so the planner halves m to 1.
SORTED_CHUNKS = {(0, 1): 1024, (0, 65): 1024, (0, 257): 512, (CHUNK, 1): 313, (CHUNK, 65): 313, (CHUNK, 257): 313}


@pytest.mark.parametrize("plant", [False, True], ids=["plain", "planted"])
def test_verr_sorted_records(native, ctx, plant):
    model, free, n = 1, False, gb.PLAN_SORTED_N
    case = vh.make_case(model, free, n, plant=plant)
    floor = gb.floors(model, free, n)
    cat = vh.catalog(native, ctx, case)
    rule = Rule()
    for chunk_len in (0, CHUNK):
        cat.set_option("chunk_len", chunk_len)
        for w in gb.PLAN_SORTED_WALKERS:
            params = np.ascontiguousarray(case["params"][:w])
            runs = []
            for order in (1, 0, 1):
                cell = (plant, chunk_len, w, "sorted" if order else "catalogue order")
                cat.set_option("verr_sorted", order)
                value, grad = evaluate(cat, params, cell)
                fast, info = value_launch(cat, params, fast=True)
                assert info["chunks"] == SORTED_CHUNKS[(chunk_len, w)], (cell, info)
                plain, _ = value_launch(cat, params, fast=False)
                assert np.all(vh.scaled_err(value, plain, n) < VALUE_TOL), cell
                runs.append((value, grad, fast, info))
            (v1, g1, f1, i1), (v0, g0, f0, i0), (v2, g2, _, _) = runs
            assert v1.tobytes() == v2.tobytes() and g1.tobytes() == g2.tobytes(), ("1 -> 0 -> 1", plant, chunk_len, w)
            # the sorted plan really ran: the series root and the split exponent exist on sorted records only
            marks = {k: (i1[k], i0[k]) for k in ("series_chunks", "direct_chunks", "exp_split")}
            assert all(off == 0 for _, off in marks.values()), (marks, plant, chunk_len, w)
            ran = any(on > 0 for on, _ in marks.values())
            print("plant {0} chunk_len {1} W = {2}: sorted indicators (on, off) {3}".format(int(plant), chunk_len, w, marks))
            assert ran or (v1.tobytes() != v0.tobytes() and f1.tobytes() != f0.tobytes()), \
                ("nothing shows that the sorted plan ran", marks, plant, chunk_len, w)
            assert np.all(vh.scaled_err(v1, v0, n) < 2 * VALUE_TOL), (plant, chunk_len, w)
            for r in vh.sample_rows(w):
                ref = gb.reference(case, r)
                cell = (plant, chunk_len, w, r)
                rule.check("sorted", cell, g1[r], ref, floor)
                rule.check("catalogue order", cell, g0[r], ref, floor)
                rule.check("sorted against catalogue order", cell, g1[r], ref, floor, factor=2.0, other=g0[r])
    cat.close()
    rule.finish()


# ---------------------------------------------------------------------------------- 4. binned catalogues
@pytest.mark.parametrize("w", gb.PLAN_BINNED_WALKERS)
@pytest.mark.parametrize("model,free", gb.PLAN_BINNED_MODELS, ids=["const_bggauss", "profile_bgconst", "profile_free"])
def test_binned_catalogue_of_very_unequal_bins(native, ctx, model, free, w):
    offs = list(gb.PLAN_BIN_OFFSETS)
    sizes = np.diff(offs)
    case = vh.make_case(model, free, offs[-1])
    k = gh.n_columns(model, free)
    # another walker table per bin, of the rows 0 .. W - 1 the floors were measured on
    params = np.ascontiguousarray(np.stack([np.roll(case["params"][:w], 11 * b, axis=0) for b in range(len(sizes))]))
    binned = vh.catalog(native, ctx, case, bin_offsets=offs)
    binned.set_option("chunk_len", CHUNK)
    value, grad = evaluate(binned, params, (model, w, "binned"))
    assert value.shape == (len(sizes), w) and grad.shape == (len(sizes), w, k)
    plain, info = value_launch(binned, params, fast=False)
    chunks = int(sum(-(-s // CHUNK) for s in sizes))
    assert chunks == 377 and -(-sizes[gb.PLAN_LONG_BIN] // CHUNK) == 299            # the four-wave reduction shape
    assert (info["chunks"], info["workgroups"]) == (chunks, main_grid(chunks, w)), info
    binned.close()
    rule = Rule()
    for b, size in enumerate(sizes):
        if size == 0:
            assert np.all(value[b] == 0.0) and np.all(grad[b] == 0.0) and np.all(plain[b] == 0.0), (b, value[b], grad[b])
            continue
        sl = slice(offs[b], offs[b + 1])
        one = vh.catalog(native, ctx, case, sl)
        one.set_option("chunk_len", CHUNK)
        v1, g1 = evaluate(one, params[b], (model, w, "stand-alone", b))
        p1, info = value_launch(one, params[b], fast=False)
        one.close()
        assert plain[b].tobytes() == p1.tobytes(), ("plain value kernels", model, w, b)
        assert info["chunks"] == -(-size // CHUNK), (b, info)
        assert value[b].tobytes() == v1.tobytes(), (model, w, b, float(np.max(np.abs(value[b] - v1))))
        assert grad[b].tobytes() == g1.tobytes(), (model, w, b, float(np.max(np.abs(grad[b] - g1))))
        assert np.all(vh.scaled_err(value[b], plain[b], size) < VALUE_TOL), (model, w, b)
        if b in (gb.PLAN_LONG_BIN, gb.PLAN_STAR_BIN):
            sub = gb.sub_case(case, sl, params[b])
            for r in vh.sample_rows(w):
                rule.check("bin of {0}".format(size), (model, w, b, r), grad[b, r], gb.reference(sub, r),
                           gb.floors(model, free, int(size)))
    rule.finish()


# ---------------------------------------------------------------------------------- 5. HMC on sorted records
def mapped_numpy_step(cols, plan, chol, eps, n_leap, pos, z, r, jitter, walkers):
    """numpy_step of test_gpu_hmc.py for MODEL_BGFIXED behind a column map: kernel column j is col_const[j] or
    col_factor[j] x free parameter col_source[j], the force on a free parameter its columns' gradients times their
    factors.  Returns the signed H1 - H0 of `walkers`, in longdouble; diagonal metric, no bound met."""
    import test_gpu_hmc as th
    L = vh.L
    diag = np.diag(chol).copy()
    assert np.count_nonzero(chol - np.diag(diag)) == 0
    source, const, factor = plan["col_source"], plan["col_const"].astype(L), plan["col_factor"].astype(L)

    def table_row(q):
        return np.array([q[s] * factor[j] if s >= 0 else const[j] for j, s in enumerate(source)], dtype=L)

    def force(q):
        g, _ = gh.grad(1, cols, table_row(q), th.CENTRE, L)
        out = np.zeros(q.size, dtype=L)
        for j, s in enumerate(source):
            if s >= 0:
                out[s] += factor[j] * g[j]
        return out

    def energy(q, p):
        y = diag.astype(L) * p
        return -vh.exact(1, cols, table_row(q), th.CENTRE) + L(0.5) * (y @ y)

    minv = (diag * diag).astype(L)
    out = np.empty(len(walkers), dtype=L)
    for i, w in enumerate(walkers):
        q = pos[w].astype(L)
        p = (z[w] / diag).astype(L)
        e = L(eps) * (L(1) + L(jitter) * L(r[w]))
        h0 = energy(q, p)
        p = p + L(0.5) * e * force(q)
        for leap in range(1, n_leap + 1):
            q = q + e * (minv * p)
            assert np.all(q >= plan["lo"]) and np.all(q <= plan["hi"])
            p = p + (e if leap < n_leap else L(0.5) * e) * force(q)
        out[i] = energy(q, p) - h0
    return out


def test_hmc_block_on_sorted_records(native, ctx):
    """bgfixed, N = 20011, W = 65, n_leap = 3 on verr-sorted records in 313 chunks (the four-wave reduction): the resident
    block equals the host-driven block bit for bit, and the first step's |dH| is that of the NumPy restatement within the
    bound of test_energy_error_is_the_numpy_gradients_energy_error (1e-9 relative to |dH|, every |dH| > 0.1), for every
    fourth walker and the last (17 of 65: each costs six longdouble passes over the catalogue)."""
    import test_gpu_hmc as th
    n, w, n_leap = 20011, 65, 3
    kw, plan, x, scale, _ = th.setup("bgfixed", n)
    cols = {key: kw[key] for key in ("ra", "dec", "v", "verr", "lnlike_bg", "pmember")}
    cat = native.Catalog(ctx, kw.pop("ra"), kw.pop("dec"), kw.pop("v"), kw.pop("verr"), **kw)
    set_options(cat, verr_sorted=1, chunk_len=CHUNK)
    chol = np.diag(scale)
    # the plan the blocks will run on: a value call with the same walker count
    pos = th.start(x, scale, plan, w)
    table = np.ascontiguousarray(np.stack([pos[:, s] * plan["col_factor"][j] if s >= 0 else np.full(w, plan["col_const"][j])
                                           for j, s in enumerate(plan["col_source"])], axis=1))
    _, info = value_launch(cat, table, fast=True)
    assert info["chunks"] == 313 and (info["series_chunks"] > 0 or info["direct_chunks"] > 0 or info["exp_split"] > 0), info
    dev = th.run(cat, plan, chol, 0.6, n_leap, pos, 31, 2, 4, resident=True)
    host = th.run(cat, plan, chol, 0.6, n_leap, pos, 31, 2, 4, resident=False)
    assert (dev["device_blocks"], dev["host_blocks"]) == (1, 0) and (host["device_blocks"], host["host_blocks"]) == (0, 1)
    for key in th.KEYS:
        assert dev[key].tobytes() == host[key].tobytes(), key
    assert np.all(np.isfinite(dev["chain"])) and dev["accepted"].sum() > 0 and not np.array_equal(dev["pos"], pos)
    # the energy error of one step from far out (test_gpu_hmc.py: DRIVE), against the restatement.  Three points of 1.6
    # widths: with DRIVE's 1.2 the NumPy side has a |dH| of 0.034 among these walkers, with 1.6 it gives 2.8 .. 83, median 33
    d = dict(th.DRIVE, eps=1.6)
    rng = np.random.default_rng(3)
    far = np.ascontiguousarray(x + d["spread"] * scale * rng.choice([-1.0, 1.0], size=(w, x.size)) *
                               rng.uniform(0.8, 1.2, size=(w, x.size)))
    z, thr, r = native.hmc_numbers(d["seed"], 0, 1, w, x.size)
    walkers = sorted(set(range(0, w, 4)) | {w - 1})
    want = mapped_numpy_step(cols, plan, chol, d["eps"], n_leap, far, z[0], r[0], d["jitter"], walkers)
    got = th.run(cat, plan, chol, d["eps"], n_leap, far, d["seed"], 0, 1, resident=True, jitter=d["jitter"])
    cat.close()
    want_abs = np.abs(want).astype(np.float64)
    err = np.abs(got["energy_error"][0][walkers] - want_abs) / want_abs
    print("min / median |dH| (NumPy):", want_abs.min(), np.median(want_abs), " largest relative difference:", err.max())
    assert want_abs.min() > 0.1, "the configuration is meant to keep every |dH| away from 0"
    assert np.all(err <= 1e-9), (err.max(), int(np.argmax(err)))

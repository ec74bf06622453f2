"""GPU: the final reduction (csrc/mcd_kernels.hip: reduce_group_kernel, csrc/mcd_reduce.h) at the boundaries of its four
launch shapes (<= 256, <= 1024, <= 4096 slots, several rounds beyond), with parameter sets of very unequal length, on a
partial-sum buffer reused across calls of different shape, and its twin fused into the resident chain's step kernel
(csrc/mcd_stretch.hip).  One dropped or doubled 64-star slot moves a sum by >= 1e-5 of it; the bar is 1e-12 against the
numpy.longdouble oracle, and bit-identity wherever two routes add the same slots in the same order."""
import numpy as np
import pytest

import variant_helper as H

pytestmark = pytest.mark.gpu

RTOL = 1e-12
CHUNK = 64                                   # option "chunk_len": the smallest nominal length the planner accepts
SLOT_COUNTS = (1, 255, 256, 257, 1023, 1024, 1025, 4095, 4096, 4097, 10000)
WALKERS = (3, 9, 64, 130)
N_MAX = CHUNK * max(SLOT_COUNTS) - 13


@pytest.fixture(scope="module")
def native():
    from mcmc_dynamics_amd import _native
    return _native


@pytest.fixture(scope="module")
def ctx(native):
    return native.default_context()


def _plain_plan(cat, chunk_len=CHUNK):
    for key, value in (("balance", 0), ("combine", 0), ("tail_split", 0), ("chunk_len", chunk_len)):
        cat.set_option(key, value)


def _prefix_sums(case, rows):
    """Exact log-likelihood of every prefix of the catalogue for the given walker rows: cumulative longdouble sums of the
    per-star terms (sequential longdouble summation of 6.4e5 terms: <= 6.4e5 x 2^-64 = 3.5e-14 relative, far below 1e-12)."""
    dtype = H.L if H.HAVE_LONGDOUBLE else np.float64
    out = {}
    for r in rows:
        terms, _ = H.per_star(case["model"], case["cat"], case["params"][r], case["centre"], dtype)
        out[r] = np.cumsum(terms)
    return out


@pytest.mark.parametrize("model", [0, 1], ids=["const", "bgfixed"])
def test_slot_counts_on_the_shape_boundaries(native, ctx, model):
    """MODEL_CONST and MODEL_BGFIXED (whose fast kernels leave the sum of lnL_bg to the reduction: pset_const) with exactly
    1, 255, 256, 257, 1023, 1024, 1025, 4095, 4096, 4097 and 10000 partial sums per walker, for walker counts that fill part
    of a group of 8, several groups, a tile, and three tiles."""
    case = H.make_case(model, False, N_MAX)
    rows = sorted({r for w in WALKERS for r in (0, w // 2, w - 1)})
    exact = _prefix_sums(case, rows)
    for slots in SLOT_COUNTS:
        n = CHUNK * slots - 13
        g = H.catalog(native, ctx, case, slice(0, n))
        _plain_plan(g)
        for w in WALKERS:
            params = np.ascontiguousarray(case["params"][:w])
            got = g.loglike(params)
            info = g.launch_info()
            assert info["chunks"] == slots, (slots, w, info)
            assert g.fast_level == (2 if model == 1 else 1) and g.rerun_count == 0
            assert np.array_equal(got, g.loglike(params)), ("not bitwise repeatable", slots, w)
            for r in (0, w // 2, w - 1):
                want = exact[r][n - 1]
                err = float(abs(H.L(got[r]) - want) / abs(want))
                assert err < RTOL, (slots, w, r, got[r], want, err)
            # every row against the plain kernels on the same chunk table (no pset_const there): all walker groups, padding included
            g.set_option("fast_path", 0)
            plain = g.loglike(params)
            g.set_option("fast_path", 1)
            assert np.max(np.abs(got - plain) / np.abs(plain)) < 2 * RTOL, (slots, w)
        g.close()


@pytest.mark.parametrize("model", [0, 1], ids=["const", "bgfixed"])
def test_combining_plans_slots_equal_workgroups(native, ctx, model):
    """One-round plans whose workgroups add up their chunks themselves: the reduction reads one slot per workgroup --
    256, 512 and 1024 of them -- and the rest of the partial-sum buffer (sized for the chunks) must not enter."""
    n = 140009
    case = H.make_case(model, False, n)
    rows = (0, 4, 8, 31, 63)
    exact = _prefix_sums(case, rows)
    g = H.catalog(native, ctx, case)
    # (workgroups per CU, waves at most) -> slots: 1024 m chunks for one walker tile, `waves` of them per workgroup
    for (m, combine), slots in {(2, 8): 256, (4, 8): 512, (4, 16): 256, (8, 8): 1024, (8, 16): 512}.items():
        g.set_option("balance", m)
        g.set_option("combine", combine)
        for w in (64, 9, 3):
            params = np.ascontiguousarray(case["params"][:w])
            got = g.loglike(params)
            info = g.launch_info()
            assert (info["chunks"], info["workgroups"]) == (1024 * m, slots), (m, combine, w, info)
            assert np.array_equal(got, g.loglike(params))
            for r in rows:
                if r < w:
                    want = exact[r][n - 1]
                    assert float(abs(H.L(got[r]) - want) / abs(want)) < RTOL, (m, combine, w, r)
    g.close()


@pytest.mark.parametrize("model", [0, 1], ids=["const", "bgfixed"])
@pytest.mark.parametrize("where", ["first", "middle", "last"])
def test_parameter_sets_of_very_unequal_length(native, ctx, model, where):
    """bin_offsets with one bin of 5000 chunks beside bins of one chunk, of one star and of no star at all, the long bin
    first, in the middle and last: every bin equals a stand-alone catalogue of its stars (same chunks, same order of
    additions: the same bits), the empty bin is exactly 0 for every walker."""
    long_bin = CHUNK * 5000 - 29
    sizes = {"first": [long_bin, 40, 1, 0, 64, 1], "middle": [1, 40, 0, long_bin, 1, 64], "last": [64, 1, 0, 40, 1, long_bin]}[where]
    offs = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    n = int(offs[-1])
    case = H.make_case(model, False, n, seed=77 + model)
    w = 21
    rng = np.random.default_rng(5)
    params = np.stack([case["params"][rng.permutation(520)[:w]] for _ in sizes])       # per-bin walker tables
    g = H.catalog(native, ctx, case, bin_offsets=offs)           # an empty bin is accepted (offsets non-decreasing)
    _plain_plan(g)
    got = g.loglike(params)
    assert got.shape == (len(sizes), w)
    assert g.launch_info()["chunks"] == sum(-(-s // CHUNK) for s in sizes)
    assert np.array_equal(got, g.loglike(params))
    g.close()
    for b, size in enumerate(sizes):
        if size == 0:
            assert np.all(got[b] == 0.0) and not np.any(np.signbit(got[b])), got[b]
            continue
        sl = slice(int(offs[b]), int(offs[b + 1]))
        one = H.catalog(native, ctx, case, sl)
        _plain_plan(one)
        alone = one.loglike(params[b])
        one.close()
        assert np.array_equal(got[b], alone), (where, b, size, np.max(np.abs(got[b] - alone)))
        if size <= 64:
            dtype = H.L if H.HAVE_LONGDOUBLE else np.float64
            sub = dict(case, cat={k: v[sl] for k, v in case["cat"].items()})
            for r in (0, w - 1):
                want = H.per_star(model, sub["cat"], params[b][r], case["centre"], dtype)[0].sum()
                assert float(abs(H.L(got[b][r]) - want) / abs(want)) < RTOL, (where, b, r)


def test_partial_sum_buffer_reuse_across_shapes(native, ctx):
    """One live catalogue through a sequence of calls that change the walker count, the slot count, the combining and the
    call style: each result is bitwise what a fresh catalogue with the same options gives."""
    n = 70001
    case = H.make_case(1, False, n)
    live = H.catalog(native, ctx, case)
    state = {}

    def step(w, style="blocking", **options):
        state.update(options)
        for k, v in options.items():
            live.set_option(k, v)
        params = np.ascontiguousarray(case["params"][:w])
        if style == "blocking":
            got = live.loglike(params)
        else:
            live.upload_params(params)
            live.enqueue()
            live.enqueue()
            got = live.fetch()
        fresh = H.catalog(native, ctx, case)
        for k, v in state.items():
            fresh.set_option(k, v)
        want = fresh.loglike(params)
        slots = fresh.launch_info()
        fresh.close()
        assert np.all(np.isfinite(want))
        assert np.array_equal(got, want), (w, style, state, np.max(np.abs(got - want)))
        return slots

    _plain_plan(live)
    state.update(balance=0, combine=0, tail_split=0, chunk_len=CHUNK)
    assert step(520)["chunks"] == 1094                       # walker count 520 -> 3 -> 257 on many slots
    step(3)
    step(257)
    assert step(257, chunk_len=4096)["chunks"] == 18         # many slots -> few
    step(3)
    step(520)
    assert step(64, chunk_len=0, balance=2, combine=8)["workgroups"] == 256      # combining on (2048 chunks, 256 slots) ...
    assert step(64, combine=0)["workgroups"] == 512                              # ... and off (2048 slots)
    step(64, style="pipelined", combine=8)                   # blocking call against upload / enqueue x 2 / fetch
    step(64, style="blocking")
    step(257, style="pipelined", balance=0, combine=0, chunk_len=CHUNK)
    step(3, style="pipelined")
    live.close()


@pytest.mark.parametrize("slots", [255, 256, 257])
def test_fused_reduction_of_the_resident_chain(native, ctx, slots):
    """The step kernel's own sum of the main kernel's partial sums (option "fused_reduce", launches of <= 256 slots) against
    the reduction kernel: a seeded resident chain gives the same positions and log-probabilities bit for bit, at 255 and
    256 slots (fused) and at 257 (where both settings run the reduction kernel)."""
    n = CHUNK * slots - 13
    case = H.make_case(0, False, n, seed=4242)
    w, steps = 48, 6
    pos0 = np.ascontiguousarray(case["params"][:w])
    lo, hi = np.full(4, -np.inf), np.full(4, np.inf)
    lo[1] = 0.0
    plan = {"col_source": np.arange(4, dtype=np.int32), "col_const": np.zeros(4), "col_factor": np.ones(4), "lo": lo, "hi": hi,
            "fixed_ok": True}
    out = {}
    for fused in (1, 0):
        g = H.catalog(native, ctx, case)
        _plain_plan(g)
        g.set_option("fused_reduce", fused)
        half = g.loglike(pos0[: w // 2])                     # the chain evaluates W / 2 proposals per half step: this table
        assert g.launch_info()["chunks"] == slots
        lnp = g.loglike(pos0)
        assert np.array_equal(lnp[: w // 2], half)          # (one walker tile either way: the same chunk table)
        pos = pos0.copy()
        chain, lnpc, acc = np.empty((steps, w, 4)), np.empty((steps, w)), np.zeros(w, dtype=np.int64)
        before = g.stretch_info()
        g.stretch_move_seeded(plan, pos, lnp, 20261016, 0, steps, chain, lnpc, acc)
        info = g.stretch_info()
        assert info["device_blocks"] == before["device_blocks"] + 1 and info["discarded_blocks"] == 0 and \
            info["host_blocks"] == before["host_blocks"], info
        assert 0 < acc.sum() < steps * w and np.all(np.isfinite(lnpc))
        # the chain's log-probabilities are the library's own values of the positions it holds
        assert np.array_equal(g.loglike(pos[: w // 2]), lnp[: w // 2])
        out[fused] = (pos, lnp, chain, lnpc, acc)
        g.close()
    for a, b in zip(out[1], out[0]):
        assert np.array_equal(a, b)

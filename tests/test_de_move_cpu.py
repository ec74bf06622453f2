"""The differential-evolution move (csrc/mcd_de.h) without a GPU: its random numbers, the uniformity of its partner pairs,
the host-driven block against the samplers' NumPy loop bit for bit, stationarity and mixing against the stretch move on a
correlated Gaussian, and the samplers' argument checks.  The library's host code (``mcd_de_numbers``, ``mcd_prior_eval``)
needs no device."""
import numpy as np
import pytest

import de_helper as dh
from mcmc_dynamics_amd.analysis.binned import BinnedSampler
from mcmc_dynamics_amd.sampler import EnsembleSampler, default_gamma0

SEED = 0x9E3779B97F4A7C15


# ---- numbers ------------------------------------------------------------------------------------------------------------
def test_numbers_of_the_library_are_the_header_s(built_library):
    """``mcd_de_numbers`` (the library's host code) and the CPU build of the header give the same numbers."""
    from mcmc_dynamics_amd import _native
    for B, W in ((1, 4), (3, 10), (2, 50)):
        lib = _native.de_numbers(SEED, 3, 6, B, W, 4, 0.7, 1e-5)
        emu = dh.numbers(SEED, 3, 6, B, W, 0.7, 1e-5)
        for a, b in zip(lib, emu):
            assert a.dtype == b.dtype and np.array_equal(a, b)
    flat = _native.de_numbers(SEED, 3, 6, 1, 10, 4, 0.7, 1e-5, squeeze=True)
    assert flat[0].shape == (6, 10) and flat[1].shape == (6, 2, 5)


def test_partners_order_and_thresholds():
    B, W, n = 3, 10, 40
    half = W // 2
    order, pa, pb, gamma, thr = dh.numbers(SEED, 0, n, B, W, 0.5, 1e-5)
    assert pa.min() >= 0 and pa.max() < half and pb.min() >= 0 and pb.max() < half
    assert np.all(pa != pb)
    assert np.array_equal(np.sort(order, axis=2), np.broadcast_to(np.arange(W, dtype=np.int32), (n, B, W)))
    assert len({tuple(o) for o in order.reshape(-1, W)}) > n          # (the splits differ between steps and ensembles)
    # thr == det_log(u) of the replayed word; the partners and the ordering key from the same call
    for (i, h, b, j) in ((0, 0, 0, 0), (7, 1, 2, 3), (39, 0, 1, 4)):
        w = dh.words(SEED, i, h, b, j, 0)
        assert thr[i, h, b, j] == dh.det_log(dh.uniform53(w[2]))
        a = min(int(dh.uniform53(w[0]) * half), half - 1)
        c = min(int(dh.uniform53(w[1]) * (half - 1)), half - 2)
        assert pa[i, h, b, j] == a and pb[i, h, b, j] == c + (c >= a)
    assert np.all(np.isfinite(gamma)) and np.all(np.abs(gamma / 0.5 - 1.0) < 1e-3) and np.unique(gamma).size > n


def test_split_is_the_sort_of_the_keys():
    """order = the walkers sorted by (upper 44 bits of word 3, walker index), walker = h W/2 + j."""
    W = 8
    order = dh.numbers(SEED, 5, 1, 2, W, 0.5, 0.0)[0]
    for b in range(2):
        keys = [((int(dh.words(SEED, 5, w // (W // 2), b, w % (W // 2), 0)[3]) >> 20), w) for w in range(W)]
        assert [w for _, w in sorted(keys)] == list(order[0, b])


def test_raw_words_are_numpy_philox():
    rng = np.random.default_rng(11)
    for _ in range(12):
        seed = int(rng.integers(0, 2 ** 63)) * 2 + int(rng.integers(0, 2))
        step, h, b, j, call = int(rng.integers(0, 2 ** 40)), int(rng.integers(0, 2)), int(rng.integers(0, 60)), \
            int(rng.integers(0, 500)), int(rng.integers(0, 17))
        assert np.array_equal(dh.words(seed, step, h, b, j, call), dh.numpy_words(seed, [step, h + 2 * call, b, j]))


def test_blocks_continue_each_other_through_step0():
    whole = dh.numbers(SEED, 0, 10, 2, 12, 0.4, 1e-5)
    head, tail = dh.numbers(SEED, 0, 4, 2, 12, 0.4, 1e-5), dh.numbers(SEED, 4, 6, 2, 12, 0.4, 1e-5)
    for a, b, c in zip(whole, head, tail):
        assert np.array_equal(a, np.concatenate([b, c]))


def test_stream_differs_from_the_stretch_move_s():
    order, pa, pb, gamma, thr = dh.numbers(SEED, 0, 8, 1, 16, 0.4, 1e-5)
    s_order, s_zz, s_thr, s_pick = dh.stretch_numbers(SEED, 0, 8, 1, 16, 1)      # (P = 1: thr = log u there as well)
    assert not np.array_equal(order, s_order) and not np.array_equal(pa, s_pick)
    assert not np.any(thr == s_thr)
    assert dh.key() != 0x6d63645f636861


def test_normal_and_its_fallback():
    """The polar method's value restated in NumPy on the replayed words, and the documented fallback behind ``max_calls``."""
    n_fallback, values = 0, []
    for j in range(400):
        full, used = dh.normal(SEED, 2, 1, 0, j, 16)
        values.append(full)
        pair = (used - 1) // 2, (used - 1) % 2
        w = dh.words(SEED, 2, 1, 0, j, 1 + pair[0])
        u, v = 2.0 * dh.uniform53(w[2 * pair[1]]) - 1.0, 2.0 * dh.uniform53(w[2 * pair[1] + 1]) - 1.0
        s = u * u + v * v
        assert 0.0 < s < 1.0 and full == u * np.sqrt(-2.0 * dh.det_log(s) / s)
        if used > 2:                                          # both pairs of the first call were rejected
            short, used_short = dh.normal(SEED, 2, 1, 0, j, 1)
            assert short == 0.0 and used_short == 2
            n_fallback += 1
    assert n_fallback > 0                                     # (probability (1 - pi/4)^2 = 4.6 % per draw)
    values = np.array(values)
    assert abs(values.mean()) < 5.0 / np.sqrt(400) and 0.8 < values.std() < 1.2


def test_ordered_pairs_are_uniform():
    """2e5 draws at half = 5: chi^2 of the 20 ordered pairs below the 0.999 quantile of chi^2(19)."""
    _, pa, pb, _, _ = dh.numbers(SEED, 0, 1000, 20, 10, 0.5, 0.0)
    assert pa.size == 200000
    counts = np.bincount((pa.ravel() * 5 + pb.ravel()), minlength=25).reshape(5, 5)
    assert np.all(np.diag(counts) == 0)
    observed = counts[~np.eye(5, dtype=bool)]
    chi2 = float(np.sum((observed - 10000.0) ** 2 / 10000.0))
    print("chi2 of the 20 ordered pairs:", chi2)
    assert chi2 < 43.8


# ---- block bit-identity -----------------------------------------------------------------------------------------------
def _plan(P, case, rng):
    """-> (plan, K-column loglike, start box): identity columns, or the named variation."""
    src, const, fac = np.arange(P, dtype=np.int32), np.zeros(P), np.ones(P)
    lo, hi, prior = np.full(P, -np.inf), np.full(P, np.inf), None
    if case == "fixed":                                       # a fixed column in front, a unit factor on the last one
        src, const, fac = np.concatenate([[-1], src]).astype(np.int32), np.concatenate([[0.3], const]), np.concatenate([[1.0], fac])
        fac[-1] = 60.0
    elif case == "prior":                                     # a normal prior on the first, a log-normal on the last coordinate
        kind = np.zeros(P, dtype=np.int32)
        kind[0], kind[-1] = 1, 2
        prior = (kind, np.where(kind == 2, 0.1, 0.2), np.full(P, 0.8))
        lo[:] = -6.0
        hi[:] = 6.0
    elif case == "tight":                                     # a box so tight that some half steps have no valid proposal
        lo[:] = -0.02
        hi[:] = 0.02
    K = src.size
    centre = rng.uniform(-0.3, 0.3, size=K) if case != "tight" else rng.uniform(-0.01, 0.01, size=K)
    if case == "prior":
        centre[-1] = 1.0
    width = rng.uniform(0.5, 2.0, size=K) * (60.0 if case == "fixed" else 1.0) if case != "tight" else np.full(K, 0.02)
    plan = {"col_source": src, "col_const": const, "col_factor": fac, "lo": lo, "hi": hi, "fixed_ok": True, "prior": prior}
    return plan, dh.table_loglike(centre, width)


def _start(plan, lead, W, P, rng):
    pos = rng.uniform(-0.015, 0.015, size=lead + (W, P)) if np.isfinite(plan["lo"]).all() and plan["hi"][0] < 1.0 else \
        rng.normal(0.0, 0.5, size=lead + (W, P))
    if plan["prior"] is not None:
        pos[..., -1] = np.abs(pos[..., -1]) + 0.2              # inside the log-normal prior's support
    return pos


@pytest.mark.parametrize("case", ["plain", "fixed", "prior", "tight"])
@pytest.mark.parametrize("W,P", [(4, 1), (8, 4), (50, 12), (50, 1), (8, 1)])
def test_block_is_the_numpy_loop(W, P, case, built_library):
    """de_block (CPU build) == the NumPy loop of EnsembleSampler and of BinnedSampler (B = 3), whole and cut into blocks."""
    from mcmc_dynamics_amd import _native
    rng = np.random.default_rng(1000 * W + P)
    plan, loglike = _plan(P, case, rng)
    inner = dh.plan_lnprob(plan, loglike, _native.prior_eval)
    empty = []

    def lnprob(values):                                       # (counts the half steps without a proposal inside the prior)
        out = inner(values)
        if np.shape(values)[-2] == W // 2 and not np.isfinite(out).any():
            empty.append(1)
        return out
    n, g0 = 9, default_gamma0(P)
    for lead in ((), (3,)):
        B = lead[0] if lead else 1
        pos0 = _start(plan, lead, W, P, rng)
        lnp0 = lnprob(pos0)
        assert np.all(np.isfinite(lnp0))
        if lead:
            s = BinnedSampler(B, W, P, lnprob, seed=SEED, rng="device", move="de")
            s.device_block_steps = 4                          # blocks of 4, 4, 1 steps
            out_pos, out_lnp, _ = s.run_mcmc(pos0, n)
        else:
            s = EnsembleSampler(W, P, lnprob, vectorize=True, seed=SEED, rng="device", move="de")
            s.block_steps = 4
            out_pos, out_lnp, _ = s.run_mcmc(pos0, n, log_prob0=lnp0)
        assert s.rng_step == n and s.gamma0 == g0 and s.sigma == 1e-5
        nums = dh.numbers(SEED, 0, n, B, W, g0, 1e-5)
        if not lead:
            nums = tuple(a[:, 0] if a.ndim == 3 else a[:, :, 0] for a in nums)
        whole = dh.block(plan, pos0, lnp0, nums, loglike)
        assert whole["status"] == 0
        assert np.array_equal(whole["chain"], s.get_chain()) and np.array_equal(whole["pos"], out_pos)
        assert np.array_equal(whole["lnprob_chain"], s._lnprob[:n]) and np.array_equal(whole["lnp"], out_lnp)
        assert np.array_equal(whole["accepted"], s._accepted.astype(np.int64))
        # the same run cut into blocks of 2 and 7 steps
        first = dh.block(plan, pos0, lnp0, tuple(a[:2] for a in nums), loglike)
        second = dh.block(plan, first["pos"], first["lnp"], tuple(a[2:] for a in nums), loglike, accepted=first["accepted"])
        assert np.array_equal(np.concatenate([first["chain"], second["chain"]]), whole["chain"])
        assert np.array_equal(second["accepted"], whole["accepted"])
        assert whole["accepted"].sum() > 0 and np.any(np.diff(whole["chain"], axis=0) != 0.0)
        if lead:
            s.close()
    if case == "tight" and (W, P) == (4, 1):
        assert empty                                          # (two proposals per half step, a step of 1.7 differences)


class _LoopCatalogue(object):
    """What numpy_de_block asks of a catalogue: ``loglike`` on ([B,] rows, K) -> ([B,] rows) around a callback on (n, K)."""

    def __init__(self, fn):
        self.fn = fn

    def loglike(self, rows):
        rows = np.asarray(rows)
        return self.fn(rows.reshape(-1, rows.shape[-1])).reshape(rows.shape[:-1])


def _same_block(got, ref):
    assert got["status"] == 0
    return dh.same((got["pos"], got["lnp"], got["chain"], got["lnprob_chain"], got["accepted"]), ref)


def test_host_block_is_the_numpy_loop_over_ensembles():
    """de_block (CPU build) with B = 3 lock-stepped ensembles of 8 walkers against the multi-ensemble NumPy loop, whose donor
    rule is stated without csrc/mcd_de.h.  The box is as wide as the start (+-0.02 under a likelihood of width 0.1: the
    ensembles keep filling it), so that 12 steps hold, on the NumPy side alone: a half step with some rows inside and some
    outside in EVERY ensemble; one in which an ensemble has no valid row and is lent another's; one without any valid row,
    which is not evaluated."""
    B, W, P, n, box = 3, 8, 4, 12, 0.02
    half = W // 2
    rng = np.random.default_rng(2001)
    plan = dh.identity_plan(P, lo=np.full(P, -box), hi=np.full(P, box))
    loglike = dh.table_loglike(rng.uniform(-0.01, 0.01, P), np.full(P, 0.1))
    calls = []

    def counted(table):
        calls.append(len(table))
        return loglike(table)
    cat = _LoopCatalogue(counted)
    pos0 = rng.uniform(-box, box, (B, W, P))
    lnp0 = _LoopCatalogue(loglike).loglike(pos0)
    nums = dh.numbers(SEED, 0, n, B, W, default_gamma0(P), 1e-5)
    ref = dh.numpy_de_block(cat, plan, pos0, lnp0, nums)
    n_ok = ref[5]["n_ok"]
    assert n_ok.shape == (n, 2, B) and ref[5]["half"] == half
    mixed_everywhere = np.all((n_ok > 0) & (n_ok < half), axis=2)
    lent = (n_ok == 0).any(axis=2) & (n_ok > 0).any(axis=2)
    empty = n_ok.sum(axis=2) == 0
    print("half steps: mixed in every ensemble", mixed_everywhere.sum(), "donor of another ensemble", lent.sum(), "empty", empty.sum())
    assert mixed_everywhere.any() and lent.any() and empty.any()
    assert ref[5]["mixed"] == ((n_ok > 0) & (n_ok < half)).sum()
    assert calls == [B * half] * int((~empty).sum())            # one call of all rows per half step, none for an empty one
    assert ref[4].sum() > 0 and np.all(np.abs(ref[2]) <= box)
    # (the NumPy loop leaves an ensemble without a valid row alone; de_block lends it the donor row and masks the value)
    got = dh.block(plan, pos0, lnp0, nums, loglike)
    assert _same_block(got, ref)
    # the one-ensemble form is the special case B = 1 of the same loop
    one = tuple(a[:, 0] if a.ndim == 3 else a[:, :, 0] for a in dh.numbers(SEED, 0, n, 1, W, default_gamma0(P), 1e-5))
    ref1 = dh.numpy_de_block(cat, plan, pos0[0], lnp0[0], one)
    lead = dh.numpy_de_block(cat, plan, pos0[:1], lnp0[:1], tuple(a[:, None] if a.ndim == 2 else a[:, :, None] for a in one))
    assert ref1[0].shape == (W, P) and dh.same(ref1[:5], (lead[0][0], lead[1][0], lead[2][:, 0], lead[3][:, 0], lead[4][0]))
    assert _same_block(dh.block(plan, pos0[0], lnp0[0], one, loglike), ref1)


def test_host_block_with_a_log_normal_coordinate_across_zero(built_library):
    """The same comparison with a log-normal prior on a coordinate whose walkers sit next to zero: proposals with that
    coordinate <= 0 are outside the prior (mcd_prior.h: prior_row_inside), beside proposals inside, in one half step."""
    from mcmc_dynamics_amd import _native
    B, W, P, n = 3, 8, 3, 9
    half = W // 2
    rng = np.random.default_rng(2100)
    kind = np.array([_native.PRIOR_NORMAL, _native.PRIOR_FLAT, _native.PRIOR_LOGNORMAL], dtype=np.int32)
    prior = (kind, np.array([0.2, 0.0, np.log(0.1)]), np.array([0.8, 1.0, 1.5]))
    plan = dh.identity_plan(P, prior=prior)
    loglike = dh.table_loglike(np.array([0.1, -0.2, 0.1]), np.array([1.0, 0.7, 0.3]))
    cat = _LoopCatalogue(loglike)
    pos0 = rng.normal(0.0, 0.5, (B, W, P))
    pos0[..., 2] = np.abs(rng.normal(0.0, 0.15, (B, W))) + 0.01
    lnp0 = dh.plan_lnprob(plan, loglike, _native.prior_eval)(pos0)
    assert np.all(np.isfinite(lnp0))
    nums = dh.numbers(SEED, 0, n, B, W, default_gamma0(P), 1e-5)
    ref = dh.numpy_de_block(cat, plan, pos0, lnp0, nums, _native.prior_eval)
    below, n_ok = ref[5]["nonpositive"], ref[5]["n_ok"]
    print("proposals with the log-normal coordinate <= 0:", below.sum(), "of", n * 2 * B * half)
    assert np.any((below > 0) & (below < half)) and np.array_equal(n_ok, half - below)    # (nothing else rejects here)
    assert np.all(ref[2][..., 2] > 0.0) and ref[4].sum() > 0
    assert _same_block(dh.block(plan, pos0, lnp0, nums, loglike), ref)


def test_four_walkers_leave_one_pair_of_partners():
    """W = 4: half = 2, pick_b is whichever slot pick_a is not; both orders of the pair equally often."""
    _, pa, pb, _, _ = dh.numbers(SEED, 0, 2000, 1, 4, 0.5, 1e-5)
    assert pa.shape == (2000, 2, 1, 2)
    assert np.all(pa != pb) and set(np.unique(pa)) == {0, 1} and set(np.unique(pb)) == {0, 1}
    for pair in ((0, 1), (1, 0)):
        share = float(np.mean((pa == pair[0]) & (pb == pair[1])))
        print("ordered pair", pair, share)
        assert 0.4 <= share <= 0.6


class _Columns(object):
    def __init__(self, k):
        self.k = k


@pytest.mark.parametrize("model,free,k", [(4, False, 9), (5, False, 7), (6, False, 6), (7, True, 11), (8, False, 12), (8, True, 14),
                                          (5, True, 9), (7, False, 9)])
def test_helper_models_give_rows_inside_their_box(model, free, k):
    """de_helper's catalogues, walkers and box of the models the GPU tests add: K columns in the order of include/mcd.h,
    every start row inside the box, the box closed where the model needs it."""
    import double_helper
    rng = np.random.default_rng(50 + model)
    cols, sv = dh.gpu_columns(rng, 33, model)
    want = {4: {"density"}, 5: {"lnlike_bg", "density"}, 6: {"lnlike_bg", "pmember"}, 7: set(), 8: {"density"}}[model]
    assert set(cols) == {"ra", "dec", "v", "verr"} | want and all(len(c) == 33 for c in cols.values())
    assert dh.n_columns(model, free) == k and (model < 7 or double_helper.n_columns(model, free) == k)
    for w in (4, 48, 130):
        pos = dh.gpu_walkers(rng, w, model, sv, free)
        assert pos.shape == (w, k) and pos.flags["C_CONTIGUOUS"] and np.all(np.isfinite(pos))
        lo, hi = dh.gpu_box(_Columns(k), pos, model, sv)
        assert lo.shape == hi.shape == (k,) and np.all((pos >= lo) & (pos <= hi))
        assert lo[1] == 0.0 and lo[2] == 1.0 and lo[5] == 1.0
        if model in (4, 5, 8):
            assert (lo[-1], hi[-1]) == (0.0, 1.0) and np.all((pos[:, -1] > 0) & (pos[:, -1] < 1))
        if model >= 7:
            names = double_helper.column_names(model, free)
            at = names.index("r_peak_ratio")
            assert (lo[at], hi[at]) == (1e-3, 1.0) and np.std(pos[:, names.index("v_maxx_c")]) > 0
        if free:
            at = 9 if model >= 7 else 6
            assert np.all(np.abs(pos[:, at:at + 2] - np.array(dh.CENTRE)) <= 0.005) and np.all(np.isfinite(lo[at:at + 2]))
    assert dh.gpu_box(_Columns(k), pos, model, sv, margin=0.0)[1][0] == pos[:, 0].max()


# ---- stationarity and mixing ------------------------------------------------------------------------------------------
_RUNS = {}


def _gaussian_runs():
    """8 000 steps of both moves on a correlated Gaussian (P = 6, W = 32) through the NumPy loop, computed once."""
    if not _RUNS:
        P, W, n = 6, 32, 8000
        cov, inv = dh.correlated_gaussian(P)

        def lnprob(x):
            return -0.5 * np.einsum("...i,ij,...j->...", x, inv, x)

        start = np.random.default_rng(3).multivariate_normal(np.zeros(P), cov, size=W)
        for move in ("stretch", "de"):
            s = EnsembleSampler(W, P, lnprob, vectorize=True, seed=20240607, rng="device", move=move)
            s.run_mcmc(start, n)
            chain = s.get_chain()[1000:]                      # (steps, W, P)
            tau = np.array([dh.autocorr_time(chain[:, :, c]) for c in range(P)])
            _RUNS[move] = {"chain": chain, "tau": tau, "acc": float(s.acceptance_fraction.mean())}
        _RUNS["cov"] = cov
    return _RUNS


@pytest.mark.parametrize("move", ["stretch", "de"])
def test_moves_sample_the_gaussian(move, built_library):
    runs = _gaussian_runs()
    chain, tau, cov = runs[move]["chain"], runs[move]["tau"], runs["cov"]
    n_eff = chain.shape[0] * chain.shape[1] / tau
    sd = np.sqrt(np.diag(cov))
    mean, var = chain.mean(axis=(0, 1)), chain.var(axis=(0, 1))
    print(move, "acceptance", runs[move]["acc"], "tau", tau, "mean / se", mean / (sd / np.sqrt(n_eff)), "var ratio", var / sd ** 2)
    assert np.all(np.abs(mean) < 5.0 * sd / np.sqrt(n_eff))
    assert np.all(np.abs(var / sd ** 2 - 1.0) < 0.05)


def test_de_mixes_faster_than_the_stretch_move(built_library):
    runs = _gaussian_runs()
    print("acceptance: stretch", runs["stretch"]["acc"], "de", runs["de"]["acc"])
    print("tau: stretch", runs["stretch"]["tau"], "de", runs["de"]["tau"])
    assert 0.15 <= runs["de"]["acc"] <= 0.45
    assert runs["de"]["tau"].max() <= 0.6 * runs["stretch"]["tau"].max()


# ---- argument checks ------------------------------------------------------------------------------------------------
def _flat(x):
    return np.zeros(np.shape(x)[:-1])


def test_argument_checks():
    with pytest.raises(ValueError):
        EnsembleSampler(8, 2, _flat, vectorize=True, rng="host", move="de")
    with pytest.raises(ValueError):
        BinnedSampler(2, 8, 2, _flat, rng="host", move="de")
    with pytest.raises(ValueError):
        EnsembleSampler(8, 2, _flat, vectorize=True, rng="device", move="snooker")
    with pytest.raises(ValueError):
        EnsembleSampler(2, 1, _flat, vectorize=True, rng="device", move="de")
    for bad in (0.0, -1.0, np.inf, np.nan):
        with pytest.raises(ValueError):
            EnsembleSampler(8, 2, _flat, vectorize=True, rng="device", move="de", gamma0=bad)
    with pytest.raises(ValueError):
        EnsembleSampler(8, 2, _flat, vectorize=True, rng="device", move="de", sigma=-1e-5)
    s = EnsembleSampler(8, 2, _flat, vectorize=True, rng="device")
    assert s.move == "stretch" and s.gamma0 is None            # the default stays the stretch move
    assert EnsembleSampler(2, 1, _flat, vectorize=True, rng="device").nwalkers == 2   # (which W = 2 still satisfies)


def test_reset_keeps_rng_step(built_library):
    s = EnsembleSampler(8, 2, lambda x: -0.5 * np.sum(np.asarray(x) ** 2, axis=-1), vectorize=True, seed=5, rng="device", move="de")
    start = np.random.default_rng(1).normal(size=(8, 2))
    whole = EnsembleSampler(8, 2, s.log_prob_fn, vectorize=True, seed=5, rng="device", move="de")
    whole.run_mcmc(start, 9)
    pos, _, _ = s.run_mcmc(start, 4)
    s.reset()
    assert s.iteration == 0 and s.rng_step == 4 and s.get_chain().shape[0] == 0
    s.run_mcmc(pos, 5)
    assert s.rng_step == 9 and np.array_equal(s.get_chain(), whole.get_chain()[4:])

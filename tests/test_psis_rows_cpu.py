"""CPU: the oracle and the crafted rows of tests/psis_rows_helper.py, which tests/test_gpu_psis_rows.py pins psis_row
(csrc/mcd_psis_row.h) to.  The general oracle against psis_helper.psis_star and mmatch_helper.psis_lw; the conditions on the
inputs under which the device comparison means what it says (the rank gap, the oracle's own error, the straddle, the radix
digits, every way out of the select); and the harness's cross-compile for gfx950."""
import math
import os

import numpy as np
import pytest

import mmatch_helper as mm
import psis_helper as psh
import psis_rows_helper as rh

TAILED = [(S, M) for S, M in rh.SHAPES if M >= 5]


@pytest.mark.parametrize("S", [20, 24, 65, 400, 1000])
def test_the_general_oracle_is_psis_star_and_psis_lw(S):
    M = psh.tail_len(S, 1.0)
    for lnl in np.concatenate([psh.near_gaussian(2, S), psh.heavy_tailed(2, S), psh.repeated_rows(2, S)]):
        k, elpd, neff, lppd, logw, _ = rh.row_oracle(-lnl, lnl, M, True)
        assert (elpd, k, lppd, neff) == tuple(float(v) for v in psh.psis_star(lnl))
        lw, k2 = mm.psis_lw(-lnl)
        assert k2 == k and np.array_equal(logw, lw - lw.max())
    # r_eff only sets M; -inf ratios (moment matching's rows outside the prior)
    lnl = psh.near_gaussian(1, S, seed=5)[0]
    r = 0.37
    k, elpd, neff, lppd, _, _ = rh.row_oracle(-lnl, lnl, psh.tail_len(S, r), True)
    e2, k2, l2, n2 = psh.psis_star(lnl, r)
    assert (k, elpd, lppd) == (k2, e2, l2) and abs(neff * r - n2) <= 1e-15 * n2
    ratio = -lnl.copy()
    ratio[::3] = -np.inf
    lw, k2 = mm.psis_lw(ratio)
    k, _, _, lppd, logw, _ = rh.row_oracle(ratio, lnl, M, False)
    assert k == k2 and np.array_equal(logw, lw - lw.max()) and math.isnan(lppd)
    assert np.all(np.isneginf(logw[::3]))


def test_r_eff_for_gives_the_tail_the_shape_names():
    for S, M in rh.SHAPES:
        assert psh.tail_len(S, rh.r_eff_for(S, M)) == M
        assert M < 5 or (M <= math.ceil(0.2 * S) and M <= rh.MAX_TAIL and M + 1 <= S)
    assert (12800, rh.MAX_TAIL) in rh.SHAPES and psh.tail_len(12800, 0.0175) == rh.MAX_TAIL
    assert rh.harness_lds_bytes(rh.MAX_TAIL) == 64000


@pytest.mark.parametrize("S,M", rh.SHAPES)
def test_gaps_and_the_oracles_own_error(S, M):
    """The conditions on the inputs: wherever a tail is smoothed, neighbouring ranks differ by MIN_GAP or more in log
    weight, a thousand times the bound that has to see them swapped; and NumPy and the emulation -- two implementations
    with a serial sort -- agree within every bound of the device test, so the oracle is not what that test measures."""
    for loo in (True, False):
        ratio, lnl, fams, want, nz = rh.shape_case(S, M, loo)
        smoothed = np.isfinite(want["pareto_k"])
        assert np.array_equal(np.isfinite(want["gap"]), smoothed)
        assert np.all(want["gap"][smoothed] >= rh.MIN_GAP), float(want["gap"].min())
        assert not np.any(np.isnan(want["logw"])) and np.all(want["logw"].max(axis=1) == 0.0)
        if M >= 5:
            assert np.isneginf(want["pareto_k"][[at for name, at, _ in fams if name == "constant"]]).all()
    ratio, lnl, fams, want, nz = rh.shape_case(S, M, True)
    r_eff = rh.r_eff_for(S, M)
    em = psh.emul_psis(lnl, r_eff)
    em["n_eff"] = em["n_eff"] / r_eff
    fin = np.isfinite(want["pareto_k"])
    dk = np.abs(em["pareto_k"][fin] - want["pareto_k"][fin])
    de = np.abs(em["elpd_loo"] - want["elpd_loo"]) / np.maximum(1.0, np.abs(want["elpd_loo"]))
    print("S {0} M {1}: smallest gap {2:.1e}, NumPy vs emulation k^ {3:.1e} elpd {4:.1e}, k^ noise {5:.1e}".format(
        S, M, float(want["gap"].min()), float(dk.max()) if dk.size else 0.0, float(de.max()), float(nz.max())))
    psh.assert_matches(em, want, elpd_tol=rh.ELPD_TOL, k_tol=rh.K_TOL, lppd_tol=rh.LPPD_TOL)


@pytest.mark.parametrize("S,M", rh.SHAPES)
def test_the_straddle_group_lies_across_the_cutoff(S, M):
    ratio, fams = rh.shape_rows(S, M)
    g_in, g_out = rh.group_sizes(S, M)
    assert g_out >= 1 and (g_in == 0) == (M < 13) and g_in <= rh.xstar_index(M)
    for step in rh.STEPS:
        at, cnt = next((a, c) for name, a, c in fams if name == "straddle_{0}".format(step))
        for row in ratio[at:at + cnt]:
            group = rh.group_mask(row, step)
            assert group.sum() == g_in + g_out
            order = np.argsort(row, kind="stable")
            assert group[order[S - M - 1]]                                 # rank M + 1 from the top: the cutoff
            assert group[order[S - M - g_out:S - M + g_in]].all()          # g_out at and below it, g_in in the tail
            if step == 0 and M >= 5:
                # an exact tie group: over more than one 64-sample block of the index scan and the gather from S = 129 on
                # (the scan's blocks count from the top index)
                at_s = np.flatnonzero(group)
                assert S < 129 or (len(set(at_s // 64)) > 1 and len(set((S - 1 - at_s) // 64)) > 1)


@pytest.mark.parametrize("S,M", TAILED)
def test_each_power_of_256_puts_the_groups_first_difference_in_its_digit(S, M):
    """step = 256^d ulp(0.25) between neighbours of the group is 256^d / 2^(e+2) key units of lw = ratio - max, |lw| in
    [2^e, 2^(e+1)) with e = -1 ... 3 here: neighbouring keys first differ, from the low end, in digit d - 1, so the select
    cannot be left before the pass of digit d (the group shares all above it but for a carry) and must be left at the pass
    of digit d - 1 at the latest.  step 0 and 1 give equal keys (1: 1/2 ... 1/32 of a key unit, rounded away) and the
    index scan decides (1: unless the cutoff is the odd one out of its group, alone with its key at the last pass)."""
    ratio, fams = rh.shape_rows(S, M)
    for step in rh.STEPS:
        at, cnt = next((a, c) for name, a, c in fams if name == "straddle_{0}".format(step))
        for row in ratio[at:at + cnt]:
            k = np.unique(rh.keys(row - row.max())[rh.group_mask(row, step)])
            gaps = np.diff(k).astype(np.float64)
            left, c = rh.select_break(row, M)
            assert rh.group_mask(row, step)[c]
            if step in (0, 1):
                assert (left == 8 and k.size == 1) if step == 0 else (left >= 7 and k.size < rh.group_mask(row, step).sum())
                continue
            if step == 255:
                assert gaps.min() >= 255 / 32 - 1 and left in (6, 7)
                continue
            d = (step.bit_length() - 1) // 8
            assert 256.0 ** (d - 1) <= gaps.min() and gaps.max() < 256.0 ** d, (step, gaps.min(), gaps.max())
            assert 7 - d <= left <= 8 - d, (step, left)


def test_every_way_out_of_the_select_is_taken():
    """Over the crafted rows the select is left after each of its eight passes, and not at all (8)."""
    seen = {}
    for S, M in TAILED:
        ratio, fams = rh.shape_rows(S, M)
        for name, at, cnt in fams:
            for row in ratio[at:at + cnt]:
                seen.setdefault(rh.select_break(row, M)[0], set()).add(name.split("_")[0])
        assert rh.select_break(ratio[next(a for name, a, _ in fams if name == "early_break")], M)[0] == 0
    for p in sorted(seen):
        print("left after pass", p, sorted(seen[p]))
    assert sorted(seen) == list(range(9))
    for d, step in enumerate(rh.STEPS[3:], start=1):                          # 256^d: the pass of digit d - 1 is reached
        hit = set()
        for S, M in TAILED:
            ratio, fams = rh.shape_rows(S, M)
            at, cnt = next((a, c) for name, a, c in fams if name == "straddle_{0}".format(step))
            hit |= {rh.select_break(row, M)[0] for row in ratio[at:at + cnt]}
        assert 8 - d in hit, (step, hit)


def test_keys_are_the_librarys():
    rng = np.random.default_rng(3)
    v = np.concatenate([[0.0, -0.0, -np.inf, -1.0, -np.nextafter(1.0, 2.0), -5e-324], -rng.exponential(size=200) * 10.0,
                        rh.straddle(1, 129, 26, 2 ** 24)[0] - 4.0])
    got = rh.keys(v)
    want = np.array([psh.lib().emul_psis_key(float(x)) for x in v], dtype=np.uint64)
    assert np.array_equal(got, want)
    assert got[0] == got[1] and np.array_equal(np.argsort(got, kind="stable"), np.argsort(v + 0.0, kind="stable"))


@pytest.mark.parametrize("S,M", TAILED)
def test_rows_with_minus_infinity(S, M):
    """What the oracle defines for -inf ratios, and that its k^ is good enough to compare values with: under one-ulp changes
    of the finite ratios it moves by less than 1e-11 on every such row (where the fit fails it does not move at all)."""
    ratio, lnl, kinds, want, nz = rh.inf_case(S, M)
    n_inf = np.isneginf(ratio).sum(axis=1)
    assert kinds == ("body", "cutoff", "one_in_tail", "tail")
    assert n_inf[0] < S - M - 1 and n_inf[1] == S - M and n_inf[2] == S - M + 1 and n_inf[3] - (S - M) > rh.xstar_index(M)
    assert np.all(nz < rh.INF_VALUES_NOISE), nz
    dead = np.isneginf(want["logw"])
    fits = rh.xstar_index(M) >= 1                         # M = 5: x* is x_1 itself, and one -inf in the tail fails the fit
    assert np.all(np.isfinite(want["pareto_k"][:2])) and want["pareto_k"][3] == np.inf
    assert np.isfinite(want["pareto_k"][2]) == fits
    for i in (0, 1, 3) + (() if fits else (2,)):
        assert np.array_equal(dead[i], np.isneginf(ratio[i]))
    if fits:
        # one -inf sample is in a smoothed tail: the one of the highest index, with the lowest of the tail's weights
        alive = np.flatnonzero(np.isneginf(ratio[2]) & ~dead[2])
        assert alive.tolist() == [int(np.flatnonzero(np.isneginf(ratio[2])).max())]
    for i in range(4):
        cut = rh.select_break(ratio[i], M)[1]
        assert np.isneginf(ratio[i][cut]) == (i > 0)


def test_the_harness_cross_compiles_for_gfx950(tmp_path):
    """Build only (hipcc needs no GPU), into a directory of this run's own."""
    out = rh.build_harness(str(tmp_path / "libpsis_row_harness.so"))
    assert os.path.getsize(out) > 0
    with open(out, "rb") as f:
        blob = f.read()
    assert b"gfx950" in blob and b"psis_row_harness" in blob

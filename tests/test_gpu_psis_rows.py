"""GPU: psis_row (csrc/mcd_psis_row.h) -- the wave's radix select, index scan, ballot gather and rank sort, then the GPD fit
and the sums -- through the device harness of tests/psis_row_harness on the crafted rows of tests/psis_rows_helper.py,
against the NumPy oracle and, for the LOO form, the emulation (tests/emul/psis_emul.cpp), both of which sort serially.

The bounds are psis_helper.assert_matches': elpd within 1e-11 max(1, |elpd|), k^ within 1e-10 (against NumPy
max(1e-10, 10 k_noise), as tests/test_gpu_psis.py has it), lppd within 1e-12, n_eff within 1e-9; and per sample the log
weight within 1e-9 of the oracle's, an exact 0 where the oracle has none.  tests/test_psis_rows_cpu.py holds the conditions
under which the last bound sees two ranks swapped (neighbouring tail log weights differ by 1e-6 or more) and under which
the oracle itself is inside every bound."""
import numpy as np
import pytest

import psis_helper as psh
import psis_rows_helper as rh

pytestmark = pytest.mark.gpu
FORMS = [True, False]
_worst = {}                                             # family -> worst (k^, elpd, log weight) difference from NumPy


def _note(family, worst):
    family = "straddle" if family.startswith("straddle") else family
    _worst[family] = tuple(max(a, b) for a, b in zip(_worst.get(family, (0.0, 0.0, 0.0)), worst))


@pytest.mark.parametrize("loo", FORMS)
@pytest.mark.parametrize("S,M", rh.SHAPES)
def test_crafted_rows_match_the_oracle(S, M, loo):
    """All families of one shape in one launch (so rows are addressed at different offsets), each against NumPy."""
    ratio, lnl, fams, want, nz = rh.shape_case(S, M, loo)
    out = rh.run_rows(ratio, lnl, M, loo)
    got = rh.derived(out, S, loo)
    assert not np.any(np.isnan(out["wout"])) and np.all(out["wout"].max(axis=1) == 1.0)
    k_tol = np.maximum(rh.K_TOL, 10.0 * nz)
    for family, at, cnt in fams:
        rows = slice(at, at + cnt)
        try:
            worst = rh.differences(rh.take(got, rows), rh.take(want, rows), k_tol=k_tol[rows])
        except AssertionError as e:
            raise AssertionError("{0} S={1} M={2} loo={3}: {4}".format(family, S, M, loo, e)) from e
        _note(family, worst)
    if loo:                                              # the emulation on the same rows: 1e-10 outright
        r_eff = rh.r_eff_for(S, M)
        em = psh.emul_psis(lnl, r_eff)
        em["n_eff"] = em["n_eff"] / r_eff
        psh.assert_matches(got, em, elpd_tol=rh.ELPD_TOL, k_tol=rh.K_TOL, lppd_tol=rh.LPPD_TOL)
    # a second launch of the same rows: the same bits
    again = rh.run_rows(ratio, lnl, M, loo)
    for key in out:
        assert np.array_equal(out[key], again[key], equal_nan=True), key


@pytest.mark.parametrize("S,M", [(S, M) for S, M in rh.SHAPES if M >= 5])
def test_rows_with_minus_infinity(S, M):
    """psis_row<false> with -inf ratios, as moment matching passes them for rows outside the prior: exact zeros for the
    samples the oracle gives no weight, the same samples with weight, the same finite / infinite k^; values as well, since
    the oracle's k^ is good to 1e-11 on these rows (tests/test_psis_rows_cpu.py)."""
    ratio, lnl, kinds, want, nz = rh.inf_case(S, M)
    out = rh.run_rows(ratio, lnl, M, False)
    got = rh.derived(out, S, False)
    dead = np.isneginf(want["logw"])
    assert np.all(out["wout"][dead] == 0.0) and np.all(out["wout"][~dead] > 0.0)
    for i, kind in enumerate(kinds):
        rows = slice(i, i + 1)
        rh.differences(rh.take(got, rows), rh.take(want, rows), values=False)
        if nz[i] < rh.INF_VALUES_NOISE:
            _note("minus_infinity", rh.differences(rh.take(got, rows), rh.take(want, rows)))


@pytest.mark.parametrize("loo", FORMS)
@pytest.mark.parametrize("S,M", [(21, 5), (65, 13), (400, 60), (12800, rh.MAX_TAIL)])
def test_a_row_alone_has_the_bits_it_has_among_others(S, M, loo):
    ratio, lnl, fams, want, nz = rh.shape_case(S, M, loo)
    out = rh.run_rows(ratio, lnl, M, loo)
    for family in ("straddle_0", "straddle_256", "heavy_tailed"):
        i = next(at for name, at, _ in fams if name == family) + 1
        alone = rh.run_rows(ratio[i], lnl[i], M, loo)
        for key in out:
            assert np.array_equal(out[key][i], alone[key][0], equal_nan=True), (family, key)


def test_the_harness_refuses_what_the_entry_points_cannot_ask_for():
    """Host-side bounds of the harness itself: no launch with a tail beyond the LDS cap, beyond ceil(0.2 S), or without a
    cutoff."""
    x = np.zeros((1, 12805))
    f, w = np.zeros((1, 8)), np.zeros((1, 12805))
    call = rh.harness().psis_row_harness
    for S, M in ((12805, 2561), (100, 21), (5, 5)):
        assert call(1, S, M, 1, x.ctypes.data, x.ctypes.data, f.ctypes.data, w.ctypes.data) != 0
    assert call(0, 100, 20, 1, x.ctypes.data, x.ctypes.data, f.ctypes.data, w.ctypes.data) != 0
    assert call(1, 100, 20, 1, None, x.ctypes.data, f.ctypes.data, w.ctypes.data) != 0


def test_accuracy_lines():
    """Last in the file: the worst differences from the NumPy oracle that the tests above met, per family (DESIGN.md
    section 3.8 quotes them)."""
    for family in sorted(_worst):
        print("PSIS_ROWS_ACCURACY family={0} k_hat={1:.3e} elpd={2:.3e} log_weight={3:.3e}".format(family, *_worst[family]))
    for worst in _worst.values():
        assert worst[0] <= 1.0 and worst[1] <= rh.ELPD_TOL and worst[2] <= rh.LOGW_TOL

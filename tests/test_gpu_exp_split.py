"""The split exponent offset of the direct chunks (option "exp_split"; csrc/mcd_math.h: BgFixedAcc::add_gs,
csrc/mcd_exp_split.h) on the GPU: against the NumPy oracle and the form without the split, across the kernel's loop
variants, with idle lanes and a single walker tile, next to chunks on the general form, through the denormal re-run, and
what must not change -- with the option off, the bits of a library without it (tests/golden/exp_split_off_20011.npy,
written by the parent commit's build on an MI355X with tools/exp_split_golden.py)."""
import os

import numpy as np
import pytest

from mcmc_dynamics_amd import synthetic
from oracle import lnprob_numpy as oracle

pytestmark = pytest.mark.gpu

NAMES4 = ["v_sys", "sigma_max", "v_maxx", "v_maxy"]
CENTRE = (synthetic.CENTER_RA_DEG, synthetic.CENTER_DEC_DEG)
ROWS = [0, 1, 63, 64, 200, 255]
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
N = 20011                       # not a multiple of 8: tail chunks and the 4-star group both occur


def rel(a, b):
    return float(np.max(np.abs(a - b) / np.abs(b)))


def _c3(n, seed_shift=0):
    cat = synthetic.make_catalog(n, config=3, seed=synthetic.CATALOG_SEED_BASE + 3 + seed_shift, background=True)
    cat["lnlike_bg"] = oracle.gaussian_background(cat["v"], cat["verr"], 20.0, 40.0)
    pos = synthetic.make_walkers(256, NAMES4, cat["truth"], config=3)
    return cat, pos


def _make(native, cat, **options):
    c = native.Catalog(native.default_context(), cat["ra"], cat["dec"], cat["v"], cat["verr"],
                       model=native.MODEL_CONST_BGFIXED, centre=CENTRE, lnlike_bg=cat["lnlike_bg"], pmember=cat["pmember"])
    for k, v in options.items():
        c.set_option(k, v)
    return c


@pytest.fixture(scope="module")
def c3():
    cat, pos = _c3(N)
    want = oracle.batched_constant_lnlike(cat, pos[ROWS], *CENTRE, lnlike_background=cat["lnlike_bg"], pmember=cat["pmember"])
    return cat, pos, want


def test_split_against_oracle_unsplit_form_golden_and_loop_variants(c3):
    from mcmc_dynamics_amd import _native as native
    cat, pos, want = c3
    c = _make(native, cat, verr_sorted=1)
    got = c.loglike(pos)
    info = c.launch_info()
    assert c.fast_level == 2 and c.rerun_count == 0
    assert info["exp_split"] == 1 and c.last_exp_split == 1 and c.last_direct_chunks >= 1
    assert np.array_equal(got, c.loglike(pos))                                      # repeatable bit for bit
    print("split vs oracle {0:.2e} ({1} direct chunks of {2})".format(rel(got[ROWS], want), c.last_direct_chunks, info["chunks"]))
    assert rel(got[ROWS], want) <= 1e-12
    c.set_option("exp_split", 0)
    off = c.loglike(pos)
    assert c.last_exp_split == 0 and c.launch_info()["exp_split"] == 0 and c.last_direct_chunks == info["direct_chunks"]
    print("split vs exp_split=0 {0:.2e}".format(rel(got, off)))
    assert rel(got, off) <= 1e-13
    # with the option off: the bits of a library without it
    assert np.array_equal(off, np.load(os.path.join(GOLDEN, "exp_split_off_20011.npy")))
    # the loop variants decide alike and multiply alike: same bits with and without the prefetch and the bounded loop
    for split, ref in ((1, got), (0, off)):
        c.set_option("exp_split", split)
        for prefetch in (0, 1):
            for bounded in (0, 1):
                c.set_option("prefetch", prefetch)
                c.set_option("narrow_bounded", bounded)
                out = c.loglike(pos)
                assert c.last_prefetch == prefetch and c.last_narrow_bounded == (32 if prefetch and bounded else 0)
                assert c.last_exp_split == split
                assert np.array_equal(out, ref), (split, prefetch, bounded)
    c.close()


@pytest.mark.parametrize("n_walkers", [200, 64])
def test_idle_lanes_and_a_single_walker_tile(c3, n_walkers):
    from mcmc_dynamics_amd import _native as native
    cat, pos, want = c3
    rows = [r for r in ROWS if r < n_walkers]
    c = _make(native, cat, verr_sorted=1)
    got = c.loglike(pos[:n_walkers])
    assert c.fast_level == 2 and c.rerun_count == 0 and c.last_exp_split == 1 and c.last_direct_chunks >= 1
    assert np.array_equal(got, c.loglike(pos[:n_walkers]))
    assert rel(got[rows], want[:len(rows)]) <= 1e-12
    c.set_option("exp_split", 0)
    off = c.loglike(pos[:n_walkers])
    assert c.last_exp_split == 0
    assert rel(got, off) <= 1e-13
    c.close()


def test_planted_certain_members_keep_their_chunks_on_the_general_form(c3):
    from mcmc_dynamics_amd import _native as native
    cat, pos, _ = c3
    base = _make(native, cat, verr_sorted=1)
    base.loglike(pos)
    n_free = base.last_direct_chunks
    assert n_free > 0
    base.close()
    planted = [5, 7000, 13001, 20010]
    cat = dict(cat)
    cat["pmember"] = cat["pmember"].copy()
    cat["pmember"][planted] = 1.0
    c = _make(native, cat, verr_sorted=1)
    got = c.loglike(pos)
    assert c.fast_level == 2 and c.rerun_count == 0 and c.last_exp_split == 1        # no re-run
    flagged = n_free - c.last_direct_chunks
    assert 1 <= flagged <= len(planted), (n_free, c.last_direct_chunks)              # the flagged chunks keep the general form
    want = oracle.batched_constant_lnlike(cat, pos[ROWS], *CENTRE, lnlike_background=cat["lnlike_bg"], pmember=cat["pmember"])
    assert rel(got[ROWS], want) <= 1e-12
    c.set_option("fast_path", 2)                         # the general form throughout
    assert rel(got, c.loglike(pos)) <= 1e-13
    assert c.last_exp_split == 0
    c.close()


def test_denormal_rerun_returns_the_plain_kernels_values(c3):
    """Certain members far from the cluster (the recipe of test_gpu_kernels.py): their chunks take the general form, which
    meets the reference's denormal regime and hands the batch to the plain kernels.  What comes back is the plain
    kernels' result, bit for bit the same with the option on and off: no chunk constant leaks into it."""
    from mcmc_dynamics_amd import _native as native
    cat, pos, _ = c3
    cat = dict(cat)
    cat["pmember"] = cat["pmember"].copy()
    cat["v"] = cat["v"].copy()
    cat["pmember"][:3] = 1.0
    cat["v"][:3] = [900.0, -1500.0, 4000.0]
    cat["lnlike_bg"] = oracle.gaussian_background(cat["v"], cat["verr"], 20.0, 40.0)
    c = _make(native, cat, verr_sorted=1)
    got = c.loglike(pos[:64])
    assert c.rerun_count == 1
    c.set_option("exp_split", 0)
    off = c.loglike(pos[:64])
    assert c.rerun_count == 2
    c.set_option("fast_path", 0)
    plain = c.loglike(pos[:64])
    assert c.rerun_count == 2
    assert np.array_equal(got, off) and np.array_equal(got, plain)
    c.close()

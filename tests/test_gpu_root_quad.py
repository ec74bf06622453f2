"""The quadratic series root on 32-star bands (option "root_quad"; csrc/mcd_math.h: RootQuad, csrc/mcd_exp_split.h:
quad_block_consts) on the GPU: against the NumPy oracle and the cubic it economises, across the kernel's loop variants, with
idle lanes and a single walker tile, a walker whose variance is at the edge of the direct form, next to chunks on the general
form, through the denormal re-run, and what must not change -- with the option off, the bits of a library without it
(tests/golden/root_quad_off_20011.npy, written by the parent commit's build on an MI355X with tools/root_quad_golden.py)."""
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
N_TIGHT = 12000                 # stars with verr in 1 .. 1.0005: chunks that pass all three votes
CHUNK_LEN = 64                  # short chunks: some pass the direct vote and fail the third (none do from 160 stars on)


def rel(a, b):
    return float(np.max(np.abs(a - b) / np.abs(b)))


def _c3(n=N):
    """The C3 catalogue with a tight verr band in front of its own verr distribution, so that chunks in the quadratic
    form, chunks in the cubic direct form only and chunks on the other loops all occur"""
    cat = synthetic.make_catalog(n, config=3, seed=synthetic.CATALOG_SEED_BASE + 3, background=True)
    cat["verr"] = cat["verr"].copy()
    cat["verr"][:N_TIGHT] = 1.0 + 5e-4 * np.random.default_rng(13).random(N_TIGHT)
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
    cat, pos = _c3()
    want = oracle.batched_constant_lnlike(cat, pos[ROWS], *CENTRE, lnlike_background=cat["lnlike_bg"], pmember=cat["pmember"])
    return cat, pos, want


def test_defaults_against_oracle_cubic_form_golden_and_loop_variants(c3):
    from mcmc_dynamics_amd import _native as native
    cat, pos, want = c3
    c = _make(native, cat, verr_sorted=1, chunk_len=CHUNK_LEN)
    got = c.loglike(pos)
    info = c.launch_info()
    assert c.fast_level == 2 and c.rerun_count == 0 and c.last_exp_split == 1
    print("quad {0}, direct {1}, series {2} of {3} chunks".format(c.last_quad_chunks, c.last_direct_chunks,
                                                                  c.last_series_chunks, info["chunks"]))
    assert c.last_root_quad == 1 and info["quad_chunks"] == c.last_quad_chunks
    assert 1 <= c.last_quad_chunks < c.last_direct_chunks < info["chunks"]
    assert np.array_equal(got, c.loglike(pos))                                      # repeatable bit for bit
    print("quad vs oracle {0:.2e}".format(rel(got[ROWS], want)))
    assert rel(got[ROWS], want) <= 1e-12
    c.set_option("root_quad", 0)
    off = c.loglike(pos)
    assert c.last_root_quad == 0 and c.last_quad_chunks == 0 and c.last_direct_chunks == info["direct_chunks"]
    assert c.last_exp_split == 1
    print("quad vs root_quad=0 {0:.2e}".format(rel(got, off)))
    assert rel(got, off) <= 1e-13
    assert not np.array_equal(got, off)             # the device did take the other root somewhere (187 chunks x 256 walkers)
    # with the option off: the bits of a library without it
    assert np.array_equal(off, np.load(os.path.join(GOLDEN, "root_quad_off_20011.npy")))
    # the loop variants decide alike and multiply alike: same bits with and without the prefetch and the bounded loop
    for quad, ref in ((1, got), (0, off)):
        c.set_option("root_quad", quad)
        for prefetch in (0, 1):
            for bounded in (0, 1):
                c.set_option("prefetch", prefetch)
                c.set_option("narrow_bounded", bounded)
                out = c.loglike(pos)
                assert c.last_prefetch == prefetch and c.last_narrow_bounded == (32 if prefetch and bounded else 0)
                assert c.last_root_quad == quad
                assert np.array_equal(out, ref), (quad, prefetch, bounded)
    c.close()


@pytest.mark.parametrize("n_walkers", [200, 64])
def test_idle_lanes_and_a_single_walker_tile(c3, n_walkers):
    from mcmc_dynamics_amd import _native as native
    cat, pos, want = c3
    rows = [r for r in ROWS if r < n_walkers]
    c = _make(native, cat, verr_sorted=1)
    got = c.loglike(pos[:n_walkers])
    assert c.fast_level == 2 and c.rerun_count == 0 and c.last_root_quad == 1 and c.last_quad_chunks >= 1
    assert np.array_equal(got, c.loglike(pos[:n_walkers]))
    assert rel(got[rows], want[:len(rows)]) <= 1e-12
    c.set_option("root_quad", 0)
    off = c.loglike(pos[:n_walkers])
    assert c.last_root_quad == 0
    assert rel(got, off) <= 1e-13
    c.close()


@pytest.mark.parametrize("s2", [7.02, 6.9])
def test_one_walker_at_the_edge_of_the_direct_form(c3, s2):
    """One walker with sigma^2 at 7 verr^2 of the tight band (verr^2 = 1 .. 1.001).  Just above (7.02) the direct vote
    passes on the tight band's chunks and nowhere else, and so does the third (187 quad chunks of 187 direct ones): the
    quadratic runs and one walker's sum comes out with the bits of root_quad = 0.  Just below (6.9) the direct vote fails
    everywhere and the third is never held: no quad chunk, equal bits.  The host's counts at the edge of the direct form are
    what this case pins; the chunks that pass the direct vote and FAIL the third are in
    test_third_vote_fails_everywhere_while_the_direct_vote_passes."""
    from mcmc_dynamics_amd import _native as native
    cat, pos, _ = c3
    one = pos[:1].copy()
    one[0, 1] = np.sqrt(s2)
    c = _make(native, cat, verr_sorted=1, chunk_len=CHUNK_LEN)
    got = c.loglike(one)
    assert c.fast_level == 2 and c.rerun_count == 0
    n_quad, n_direct, n_series = c.last_quad_chunks, c.last_direct_chunks, c.last_series_chunks
    c.set_option("root_quad", 0)
    off = c.loglike(one)
    print("sigma^2 = {0}: quad {1}, direct {2}, series {3} chunks, on/off {4:.2e}".format(s2, n_quad, n_direct, n_series, rel(got, off)))
    assert n_quad <= n_direct <= n_series and n_series >= 1
    assert n_quad == 0 or np.array_equal(got, off)
    if s2 < 7.0:
        assert n_direct == 0 and n_quad == 0 and np.array_equal(got, off)
    else:
        assert n_direct >= 1
    want = oracle.batched_constant_lnlike(cat, one, *CENTRE, lnlike_background=cat["lnlike_bg"], pmember=cat["pmember"])
    assert rel(got, want) <= 1e-12
    c.close()


def _c3_wide():
    """The same catalogue with its front band at verr = 2.8 .. 3.0: with the benchmark's walkers (sigma^2 >= 68.6) its 64-star
    chunks pass the series and the direct vote (7 verr^2 <= 63) and every 32-star block is at least 2.5 times wider than
    2^-17.5 (verr^2 + sigma^2) -- computed on the CPU with NumPy: 236 direct chunks of 313, none for the quadratic"""
    cat, pos = _c3()
    cat["verr"][:N_TIGHT] = 2.8 + 0.2 * np.random.default_rng(13).random(N_TIGHT)
    cat["lnlike_bg"] = oracle.gaussian_background(cat["v"], cat["verr"], 20.0, 40.0)
    return cat, pos


@pytest.mark.parametrize("n_walkers", [256, 1])
def test_third_vote_fails_everywhere_while_the_direct_vote_passes(n_walkers):
    """Chunks that pass the direct vote and fail the third run the split loop: the launch offers the quadratic form, no chunk
    is counted for it, and the result has the bits of root_quad = 0 -- over 256 walkers x 236 direct chunks a vote that let
    one of them through (blocks 2.5 to 30 times too wide, an economisation error from 1.7 u up) changes them: a build whose
    third vote always passes fails this case at the comparison with root_quad = 0 (tried once on an MI355X) -- whatever the
    loop variant.  One walker is the case as first asked for; its sum over 20 011 stars hides such a build, so the 256 walkers
    are what checks the vote."""
    from mcmc_dynamics_amd import _native as native
    cat, pos = _c3_wide()
    pos = pos[:n_walkers]
    c = _make(native, cat, verr_sorted=1, chunk_len=CHUNK_LEN)
    got = c.loglike(pos)
    assert c.fast_level == 2 and c.rerun_count == 0 and c.last_exp_split == 1 and c.last_root_quad == 1
    print("wide band, {0} walkers: quad {1}, direct {2} of {3} chunks".format(n_walkers, c.last_quad_chunks, c.last_direct_chunks,
                                                                            c.launch_info()["chunks"]))
    assert c.last_direct_chunks >= 1 and c.last_quad_chunks == 0
    c.set_option("root_quad", 0)
    off = c.loglike(pos)
    assert c.last_root_quad == 0
    assert np.array_equal(got, off)
    c.set_option("root_quad", 1)
    for prefetch in (0, 1):
        for bounded in (0, 1):
            c.set_option("prefetch", prefetch)
            c.set_option("narrow_bounded", bounded)
            assert np.array_equal(c.loglike(pos), off), (prefetch, bounded)
    want = oracle.batched_constant_lnlike(cat, pos[:1], *CENTRE, lnlike_background=cat["lnlike_bg"], pmember=cat["pmember"])
    assert rel(got[:1], want) <= 1e-12
    c.close()


def test_planted_certain_members_keep_their_chunks_on_the_general_form(c3):
    from mcmc_dynamics_amd import _native as native
    cat, pos, _ = c3
    base = _make(native, cat, verr_sorted=1)
    base.loglike(pos)
    n_free = base.last_quad_chunks
    assert n_free > 0
    base.close()
    planted = [5, 7000, 13001, 20010]
    cat = dict(cat)
    cat["pmember"] = cat["pmember"].copy()
    cat["pmember"][planted] = 1.0
    c = _make(native, cat, verr_sorted=1)
    got = c.loglike(pos)
    assert c.fast_level == 2 and c.rerun_count == 0 and c.last_root_quad == 1       # no re-run
    flagged = n_free - c.last_quad_chunks
    assert 1 <= flagged <= len(planted), (n_free, c.last_quad_chunks)                # the flagged chunks keep the general form
    want = oracle.batched_constant_lnlike(cat, pos[ROWS], *CENTRE, lnlike_background=cat["lnlike_bg"], pmember=cat["pmember"])
    assert rel(got[ROWS], want) <= 1e-12
    c.set_option("fast_path", 2)                         # the general form throughout
    assert rel(got, c.loglike(pos)) <= 1e-13
    assert c.last_root_quad == 0
    c.close()


def test_denormal_rerun_returns_the_plain_kernels_values(c3):
    """Certain members far from the cluster (the recipe of test_gpu_exp_split.py): their chunks take the general form, which
    meets the reference's denormal regime and hands the batch to the plain kernels.  What comes back is the plain
    kernels' result, bit for bit the same with the option on and off."""
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
    c.set_option("root_quad", 0)
    off = c.loglike(pos[:64])
    assert c.rerun_count == 2
    c.set_option("fast_path", 0)
    plain = c.loglike(pos[:64])
    assert c.rerun_count == 2
    assert np.array_equal(got, off) and np.array_equal(got, plain)
    c.close()

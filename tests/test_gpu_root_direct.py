"""The direct form of the series reciprocal root (option "root_direct"; csrc/mcd_math.h: RootDirect) on the GPU: against
the delta form, the NumPy oracle, across the kernel's loop variants, and what must not change -- with the option off, the
bits of a library without it (tests/golden/root_direct_off_*.npy, written by the parent commit's build on an MI355X with
tools/root_direct_golden.py)."""
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


def test_defaults_take_the_direct_form_on_a_large_catalogue():
    """180 000 stars: 8.6 MB of records, above the 8 MiB rule that sorts them by verr -- nothing else is set."""
    from mcmc_dynamics_amd import _native as native
    cat, pos = _c3(180000)
    c = _make(native, cat)
    got = c.loglike(pos)
    info = c.launch_info()
    print("defaults, 180000 stars: direct chunks {0}, series chunks {1} of {2}".format(c.last_direct_chunks, c.last_series_chunks,
                                                                                   info["chunks"]))
    assert c.fast_level == 2 and c.rerun_count == 0
    assert 0 < c.last_direct_chunks <= c.last_series_chunks <= info["chunks"]
    assert info["direct_chunks"] == c.last_direct_chunks and info["series_chunks"] == c.last_series_chunks
    assert np.array_equal(got, c.loglike(pos))                           # repeatable bit for bit
    want = oracle.batched_constant_lnlike(cat, pos[ROWS], *CENTRE, lnlike_background=cat["lnlike_bg"], pmember=cat["pmember"])
    assert rel(got[ROWS], want) <= 1e-12
    series_before = c.last_series_chunks
    c.set_option("root_direct", 0)
    off = c.loglike(pos)
    assert c.last_direct_chunks == 0 and c.last_series_chunks == series_before      # the series' count keeps its meaning
    assert rel(got, off) <= 1e-13
    assert np.array_equal(off, np.load(os.path.join(GOLDEN, "root_direct_off_180000.npy")))
    c.set_option("root_direct", 1)
    c.set_option("root_series", 0)
    c.loglike(pos)
    assert c.last_direct_chunks == 0 and c.last_series_chunks == 0                  # no series, no direct form
    c.close()


@pytest.mark.parametrize("n", [1000000, 20011])
def test_direct_and_delta_agree_with_each_other_and_the_oracle(n):
    from mcmc_dynamics_amd import _native as native
    cat, pos = _c3(n)
    want = oracle.batched_constant_lnlike(cat, pos[ROWS], *CENTRE, lnlike_background=cat["lnlike_bg"], pmember=cat["pmember"])
    c = _make(native, cat, verr_sorted=1)
    out = {}
    for direct in (1, 0):
        c.set_option("root_direct", direct)
        out[direct] = c.loglike(pos)
        assert c.fast_level == 2 and c.rerun_count == 0
        assert c.last_series_chunks > 0 and (c.last_direct_chunks > 0) == bool(direct), c.last_direct_chunks
        assert c.last_direct_chunks <= c.last_series_chunks
        assert np.array_equal(out[direct], c.loglike(pos))               # repeatable bit for bit
        print("n {0} root_direct {1}: direct chunks {2}, series chunks {3} of {4}, rel err vs oracle {5:.2e}".format(
            n, direct, c.last_direct_chunks, c.last_series_chunks, c.launch_info()["chunks"], rel(out[direct][ROWS], want)))
        assert rel(out[direct][ROWS], want) <= 1e-12
    print("direct vs delta {0:.2e}".format(rel(out[1], out[0])))
    assert rel(out[1], out[0]) <= 1e-13
    # with the option off: the bits of a library without it
    assert np.array_equal(out[0], np.load(os.path.join(GOLDEN, "root_direct_off_{0}.npy".format(n))))
    # the loop variants decide alike: same bits with and without the prefetch and the bounded loop, for both forms
    for direct in (1, 0):
        c.set_option("root_direct", direct)
        for prefetch in (0, 1):
            for bounded in (0, 1):
                c.set_option("prefetch", prefetch)
                c.set_option("narrow_bounded", bounded)
                got = c.loglike(pos)
                assert c.last_prefetch == prefetch and c.last_narrow_bounded == (32 if prefetch and bounded else 0)
                assert np.array_equal(got, out[direct]), (direct, prefetch, bounded)
    c.close()


def test_large_verr_takes_the_delta_form_bit_for_bit():
    """verr 30 .. 30.3 against sigma ~ 8 - 12: verr^2 is ~90 % of the variance, far beyond the direct form's 1/8, while a
    ~50-star chunk spans 0.02 in verr^2 against an admitted half-width of 2^-13 1000 = 0.12: every chunk takes the series,
    none the direct form, and the option changes no bit."""
    from mcmc_dynamics_amd import _native as native
    cat, pos = _c3(51200)
    cat["verr"] = np.random.default_rng(3).uniform(30.0, 30.3, 51200)
    cat["lnlike_bg"] = oracle.gaussian_background(cat["v"], cat["verr"], 20.0, 40.0)
    c = _make(native, cat, verr_sorted=1, balance=1)
    out = {}
    for direct in (1, 0):
        c.set_option("root_direct", direct)
        out[direct] = c.loglike(pos[:64])
        assert c.fast_level == 2 and c.last_direct_chunks == 0 and c.last_series_chunks > 0
        assert c.launch_info()["chunks"] == 1024
    assert np.array_equal(out[0], out[1])
    want = oracle.batched_constant_lnlike(cat, pos[:4], *CENTRE, lnlike_background=cat["lnlike_bg"], pmember=cat["pmember"])
    assert rel(out[1][:4], want) <= 1e-12
    c.close()


def test_wide_verr_spread_takes_the_rsq_loops_bit_for_bit():
    """As test_gpu_root_series: verr over two orders of magnitude, no chunk narrow enough for the series -- none for the
    direct form either, and the rsq loops' bits whatever the two options say."""
    from mcmc_dynamics_amd import _native as native
    cat, pos = _c3(51200)
    cat["verr"] = 10.0 ** np.random.default_rng(3).uniform(0.5, 2.5, 51200)
    cat["lnlike_bg"] = oracle.gaussian_background(cat["v"], cat["verr"], 20.0, 40.0)
    c = _make(native, cat, verr_sorted=1, balance=1)
    out = {}
    for series, direct in ((1, 1), (1, 0), (0, 1)):
        c.set_option("root_series", series)
        c.set_option("root_direct", direct)
        out[series, direct] = c.loglike(pos[:64])
        assert c.fast_level == 2 and c.last_series_chunks == 0 and c.last_direct_chunks == 0
    assert np.array_equal(out[1, 1], out[0, 1]) and np.array_equal(out[1, 0], out[0, 1])
    c.close()


def test_planted_certain_members_keep_their_chunks_on_the_general_form():
    from mcmc_dynamics_amd import _native as native
    cat, pos = _c3(20011)
    base = _make(native, cat, verr_sorted=1)
    base.loglike(pos)
    n_free = base.last_direct_chunks
    assert n_free > 0
    base.close()
    planted = [5, 7000, 13001, 20010]
    cat["pmember"] = cat["pmember"].copy()
    cat["pmember"][planted] = 1.0
    c = _make(native, cat, verr_sorted=1)
    got = c.loglike(pos)
    assert c.fast_level == 2 and c.rerun_count == 0
    flagged = n_free - c.last_direct_chunks
    assert 1 <= flagged <= len(planted), (n_free, c.last_direct_chunks)
    want = oracle.batched_constant_lnlike(cat, pos[ROWS], *CENTRE, lnlike_background=cat["lnlike_bg"], pmember=cat["pmember"])
    assert rel(got[ROWS], want) <= 1e-12
    c.set_option("fast_path", 2)                         # the general form throughout
    assert rel(got, c.loglike(pos)) <= 1e-13
    c.close()

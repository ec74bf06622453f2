"""The verr-sorted record array of the main kernel and the series reciprocal root (options "verr_sorted", "root_series")
on the GPU: against each other, the NumPy oracle, across the kernel's loop variants, and what must not change."""
import numpy as np
import pytest

from mcmc_dynamics_amd import synthetic
from oracle import lnprob_numpy as oracle

pytestmark = pytest.mark.gpu

NAMES4 = ["v_sys", "sigma_max", "v_maxx", "v_maxy"]
CENTRE = (synthetic.CENTER_RA_DEG, synthetic.CENTER_DEC_DEG)
ROWS = [0, 1, 63, 64, 200, 255]


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


@pytest.mark.parametrize("n", [1000000, 20011])
def test_series_and_rsq_agree_with_each_other_and_the_oracle(n):
    from mcmc_dynamics_amd import _native as native
    cat, pos = _c3(n)
    want = oracle.batched_constant_lnlike(cat, pos[ROWS], *CENTRE, lnlike_background=cat["lnlike_bg"], pmember=cat["pmember"])
    c = _make(native, cat, verr_sorted=1)
    out = {}
    for series in (1, 0):
        c.set_option("root_series", series)
        out[series] = c.loglike(pos)
        assert c.fast_level == 2 and c.rerun_count == 0
        assert (c.last_series_chunks > 0) == bool(series), c.last_series_chunks
        assert np.array_equal(out[series], c.loglike(pos))               # repeatable bit for bit
        print("n {0} root_series {1}: series chunks {2} of {3}, rel err vs oracle {4:.2e}".format(
            n, series, c.last_series_chunks, c.launch_info()["chunks"], rel(out[series][ROWS], want)))
        assert rel(out[series][ROWS], want) <= 1e-12
    print("series vs rsq {0:.2e}".format(rel(out[1], out[0])))
    assert rel(out[1], out[0]) <= 1e-13
    # the loop variants decide alike: same bits with and without the prefetch and the bounded loop
    c.set_option("root_series", 1)
    for prefetch in (0, 1):
        for bounded in (0, 1):
            c.set_option("prefetch", prefetch)
            c.set_option("narrow_bounded", bounded)
            got = c.loglike(pos)
            assert c.last_prefetch == prefetch and c.last_narrow_bounded == (32 if prefetch and bounded else 0)
            assert np.array_equal(got, out[1]), (prefetch, bounded)
    # catalogue order agrees to rounding (another fixed order of the same sum)
    c.set_option("prefetch", -1)
    c.set_option("verr_sorted", 0)
    plain_order = c.loglike(pos)
    assert c.last_series_chunks == 0
    assert rel(plain_order, out[0]) <= 1e-13
    c.close()


def test_defaults_sort_large_catalogues_only():
    from mcmc_dynamics_amd import _native as native
    cat, pos = _c3(180000)                       # 8.6 MB of records: above the 8 MiB rule
    c = _make(native, cat)
    c.loglike(pos)
    assert c.last_series_chunks > 0
    c.close()
    small = {k: (v[:20011] if isinstance(v, np.ndarray) else v) for k, v in cat.items()}
    c = _make(native, small)
    a = c.loglike(pos)
    assert c.last_series_chunks == 0
    c.set_option("verr_sorted", 0)
    c.set_option("root_series", 0)
    assert np.array_equal(a, c.loglike(pos))     # small catalogues: today's order, today's bits
    c.set_option("prefetch", 1)                  # the prefetch option does not switch the order
    assert np.array_equal(a, c.loglike(pos))
    c.close()


def test_wide_verr_spread_takes_the_rsq_loops_bit_for_bit():
    """verr over two orders of magnitude from sigma / 3 up, ~50 stars per chunk (one-round plan, 1024 chunks x 64 walkers):
    the narrowest chunk spans 0.09 in verr^2 against an admitted half-width of 2^-13 (10 + 70) = 0.01 -- no chunk
    qualifies, and the series build gives the rsq loops' bits."""
    from mcmc_dynamics_amd import _native as native
    cat, pos = _c3(51200)
    cat["verr"] = 10.0 ** np.random.default_rng(3).uniform(0.5, 2.5, 51200)
    cat["lnlike_bg"] = oracle.gaussian_background(cat["v"], cat["verr"], 20.0, 40.0)
    c = _make(native, cat, verr_sorted=1, balance=1)
    out = {}
    for series in (1, 0):
        c.set_option("root_series", series)
        out[series] = c.loglike(pos[:64])
        assert c.fast_level == 2 and c.last_series_chunks == 0
        assert c.launch_info()["chunks"] == 1024
    assert np.array_equal(out[0], out[1])
    want = oracle.batched_constant_lnlike(cat, pos[:4], *CENTRE, lnlike_background=cat["lnlike_bg"], pmember=cat["pmember"])
    assert rel(out[1][:4], want) <= 1e-12
    c.close()


def test_planted_certain_members_keep_their_chunks_on_the_general_form():
    from mcmc_dynamics_amd import _native as native
    cat, pos = _c3(20011)
    base = _make(native, cat, verr_sorted=1)
    base.loglike(pos)
    n_free = base.last_series_chunks
    base.close()
    planted = [5, 7000, 13001, 20010]
    cat["pmember"] = cat["pmember"].copy()
    cat["pmember"][planted] = 1.0
    c = _make(native, cat, verr_sorted=1)
    got = c.loglike(pos)
    assert c.fast_level == 2 and c.rerun_count == 0
    flagged = n_free - c.last_series_chunks
    assert 1 <= flagged <= len(planted), (n_free, c.last_series_chunks)
    want = oracle.batched_constant_lnlike(cat, pos[ROWS], *CENTRE, lnlike_background=cat["lnlike_bg"], pmember=cat["pmember"])
    assert rel(got[ROWS], want) <= 1e-12
    c.set_option("fast_path", 2)                         # the general form throughout
    assert rel(got, c.loglike(pos)) <= 1e-13
    c.close()


def test_per_star_outputs_stay_in_catalogue_order():
    from mcmc_dynamics_amd import _native as native
    cat, pos = _c3(20011)
    a = _make(native, cat, verr_sorted=1)
    b = _make(native, cat, verr_sorted=0)
    a.loglike(pos)
    b.loglike(pos)
    assert a.last_series_chunks > 0 and b.last_series_chunks == 0
    assert np.array_equal(a.membership(pos[3]), b.membership(pos[3]))
    a.close()
    b.close()

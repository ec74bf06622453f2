"""GPU parity of the HIP kernels (through the C-ABI) against golden vectors taken from the reference
and against the NumPy oracle.  Tolerance: float64, relative 1e-12 on each walker's log-likelihood
(north_star asks for a stated float64 tolerance; BASELINE.md proposes <= 1e-11)."""
import numpy as np
import pytest

from conftest import load_golden, rel_err

pytestmark = pytest.mark.gpu

RTOL = 1e-12


@pytest.fixture(scope="module")
def native():
    from mcmc_dynamics_amd import _native
    return _native


@pytest.fixture(scope="module")
def ctx(native):
    return native.default_context()


def _likelihood_part(g):
    """Golden lnprob = lnprior + lnlike; with flat priors lnlike == lnprob where the prior is finite."""
    want = g["lnprob"].copy()
    return want, np.isfinite(g["lnprior"]) if "lnprior" in g else np.isfinite(want)


@pytest.mark.parametrize("fast", [1, 0])
def test_constant_fixed_centre_golden(native, ctx, fast):
    g = load_golden("constant_fixed")
    cat = native.Catalog(ctx, g["ra"], g["dec"], g["v"], g["verr"], model=native.MODEL_CONST,
                         centre=(float(g["ra_center"]), float(g["dec_center"])))
    cat.set_option("fast_path", fast)
    got = cat.loglike(g["values"])
    want, ok = _likelihood_part(g)
    assert rel_err(got[ok], want[ok]) < RTOL


@pytest.mark.parametrize("fast", [1, 0])
def test_constant_free_centre_golden(native, ctx, fast):
    g = load_golden("constant_free")
    cat = native.Catalog(ctx, g["ra"], g["dec"], g["v"], g["verr"], model=native.MODEL_CONST, centre=None)
    cat.set_option("fast_path", fast)
    got = cat.loglike(g["values"])
    want, ok = _likelihood_part(g)
    assert rel_err(got[ok], want[ok]) < RTOL


@pytest.mark.parametrize("which", ["fixed", "free"])
@pytest.mark.parametrize("fast_path,level", [(1, 2), (2, 1), (0, 0)])
def test_fixed_gaussian_background_golden(native, ctx, which, fast_path, level):
    """ConstantFit + background.Gaussian against lnprob of the reference, through all three kernel families: the
    narrow-range variant (what the guard picks for this catalogue: every pmember < 1, lnL_bg > -150), the general fast
    formulation and the plain kernels."""
    g = load_golden("constant_bg_gaussian_" + which)
    centre = (float(g["ra_center"]), float(g["dec_center"])) if which == "fixed" else None
    cat = native.Catalog(ctx, g["ra"], g["dec"], g["v"], g["verr"], model=native.MODEL_CONST_BGFIXED, centre=centre,
                         lnlike_bg=g["lnlike_background"], pmember=g["pmember"])
    cat.set_option("fast_path", fast_path)
    want, ok = _likelihood_part(g)
    ok &= g["values"][:, 1] > 0                       # sigma = 0 rows: the guard sends the whole batch to the plain kernels
    got = cat.loglike(g["values"][ok])
    assert cat.fast_level == level
    assert rel_err(got, want[ok]) < RTOL
    assert rel_err(cat.loglike(g["values"])[_likelihood_part(g)[1]], want[_likelihood_part(g)[1]]) < RTOL


@pytest.mark.parametrize("which", ["fixed", "free"])
def test_walker_gaussian_background_golden(native, ctx, which):
    g = load_golden("constant_gb_" + which)
    centre = (float(g["ra_center"]), float(g["dec_center"])) if which == "fixed" else None
    cat = native.Catalog(ctx, g["ra"], g["dec"], g["v"], g["verr"], model=native.MODEL_CONST_BGGAUSS, centre=centre,
                         density=g["density"])
    got = cat.loglike(g["values"])
    want, ok = _likelihood_part(g)
    assert rel_err(got[ok], want[ok]) < RTOL
    # the three kernel families on the rows every one of them admits (f_back > 0, sigma > 0: narrow-range variant eligible)
    names = [str(x) for x in g["names"]]
    inner = ok & (g["values"][:, names.index("f_back")] > 1e-6) & (g["values"][:, names.index("sigma_max")] > 0)
    assert inner.sum() >= 6
    for fast_path, level in ((1, 2), (2, 1), (0, 0)):
        cat.set_option("fast_path", fast_path)
        res = cat.loglike(g["values"][inner])
        assert cat.fast_level == level
        assert rel_err(res, want[inner]) < RTOL
    cat.set_option("fast_path", 1)
    # membership probabilities, constant.py:366-374
    row = int(g["membership_row"])
    mem = cat.membership(g["values"][row])
    assert np.max(np.abs(mem - g["membership"])) < 1e-11   # probabilities in [0, 1]; exp() of lnL ~ -1e3


def test_example_catalogue_golden(native, ctx):
    g = load_golden("example_catalog")
    cat = native.Catalog(ctx, g["ra"], g["dec"], g["v"], g["verr"], model=native.MODEL_CONST,
                         centre=(float(g["ra_center"]), float(g["dec_center"])))
    got = cat.loglike(g["values"])
    assert rel_err(got, g["lnprob"]) < RTOL


def test_radial_bins_golden(native, ctx):
    """B independent per-bin posteriors in ONE launch (bin/run_tests.py:75-124 runs them serially)."""
    g = load_golden("radial_bins")
    bins = g["bins_n200_d005"]
    order = np.argsort(bins, kind="stable")
    n_bins = int(bins.max()) + 1
    offs = np.concatenate([[0], np.cumsum(np.bincount(bins, minlength=n_bins))])
    cat = native.Catalog(ctx, g["ra"][order], g["dec"][order], g["v"][order], g["verr"][order],
                         model=native.MODEL_CONST, centre=(float(g["ra_center"]), float(g["dec_center"])),
                         bin_offsets=offs)
    params = np.broadcast_to(g["values"], (n_bins,) + g["values"].shape)
    got = cat.loglike(params)
    assert got.shape == g["lnprob_per_bin"].shape
    assert rel_err(got, g["lnprob_per_bin"]) < RTOL
    # sum over bins with identical parameters == un-binned value
    assert rel_err(got.sum(axis=0), g["lnprob_all"]) < RTOL


def test_abi_errors(native, ctx):
    g = load_golden("constant_fixed")
    cat = native.Catalog(ctx, g["ra"], g["dec"], g["v"], g["verr"], model=native.MODEL_CONST,
                         centre=(float(g["ra_center"]), float(g["dec_center"])))
    with pytest.raises(ValueError):
        cat.loglike(np.zeros((4, 6)))
    with pytest.raises(native.NativeError):
        native.Catalog(ctx, g["ra"], g["dec"], g["v"], g["verr"], model=native.MODEL_CONST_BGGAUSS, centre=None)
    empty = native.Catalog(ctx, [], [], [], [], model=native.MODEL_CONST, centre=(0.0, 0.0))
    assert np.array_equal(empty.loglike(g["values"]), np.zeros(len(g["values"])))
    # call-order and option misuse: status codes with a message, never a crash
    fresh = native.Catalog(ctx, g["ra"], g["dec"], g["v"], g["verr"], model=native.MODEL_CONST,
                           centre=(float(g["ra_center"]), float(g["dec_center"])))
    assert fresh.fast_level == -1
    with pytest.raises(native.NativeError, match="staged|evaluated"):
        fresh.enqueue()
    for key, bad in (("fast_path", 3), ("fast_path", -1), ("timing_stride", 0), ("timing_reserve", -5),
                     ("target_waves", 0), ("no_such_option", 1)):
        with pytest.raises(native.NativeError):
            fresh.set_option(key, bad)
    with pytest.raises(native.NativeError):
        fresh.membership(g["values"][0])                 # membership needs a background model
    ok_rows = g["values"][np.isfinite(g["lnprior"])]
    assert np.all(np.isfinite(fresh.loglike(ok_rows)))   # still usable afterwards
    # a failed upload leaves NOTHING staged: enqueue / fetch answer with a status, they must not touch evicted buffers
    # (more than 8 walker counts evict the cache of work buffers; the 10th upload then fails on its column count)
    import ctypes
    for w in range(1, 10):
        fresh.loglike(ok_rows[:w])
    bad = np.zeros((3, 5))
    rc = fresh.lib.mcd_params_upload(fresh.handle, 3, 5, bad.ctypes.data_as(ctypes.POINTER(ctypes.c_double)))
    assert rc == -1 and b"columns" in fresh.lib.mcd_last_error()
    with pytest.raises(native.NativeError, match="staged"):
        fresh.enqueue()
    with pytest.raises(native.NativeError, match="evaluated|staged"):
        fresh.fetch()
    assert np.array_equal(fresh.loglike(ok_rows[:4]), fresh.loglike(ok_rows)[:4])       # and it recovers
    fresh.set_option("chunk_len", 100)                   # tuning option: rounded up to 128, results unchanged to rounding
    assert rel_err(fresh.loglike(ok_rows), native.Catalog(ctx, g["ra"], g["dec"], g["v"], g["verr"], model=native.MODEL_CONST,
                                                          centre=(float(g["ra_center"]), float(g["dec_center"]))).loglike(ok_rows)) < 1e-13
    fresh.close()
    with pytest.raises(native.NativeError):
        fresh.loglike(g["values"])                       # closed catalogue


# ------------------------------------------------------------------------------------------------
# size-independent properties at BASELINE sizes (the oracle would take minutes there)
def _synthetic(n, config, background=False, min_sep_arcmin=1e-2):
    """Synthetic catalogue for property tests.  Stars closer than ``min_sep_arcmin`` to the centre are moved onto
    another star's position: there theta = arctan2(dy, dx) is ill-conditioned in the reference's own formula
    (calc_xy_offset.py:31 subtracts two O(0.4) products), so one ulp in sin/cos between the device libm and NumPy
    shifts lnL by ~1e-16 / r -- a property of the formula, checked separately in test_precision_sweep_c5."""
    from mcmc_dynamics_amd import synthetic
    from oracle import lnprob_numpy as oracle
    c = synthetic.make_catalog(n, config=config, background=background)
    centre = (synthetic.CENTER_RA_DEG, synthetic.CENTER_DEC_DEG)
    if min_sep_arcmin and n > 1:
        dx, dy = oracle.calc_xy_offset(c["ra"], c["dec"], *centre)
        r = np.hypot(dx, dy)
        near = r < min_sep_arcmin
        if near.any():
            donor = int(np.argmax(r))
            c["ra"][near], c["dec"][near] = c["ra"][donor], c["dec"][donor]
    return c, centre


NAMES4 = ["v_sys", "sigma_max", "v_maxx", "v_maxy"]


def test_full_size_c3_properties(native, ctx):
    """1e6 stars x 256 walkers, background mixture: fast == plain path, shard sums == total, bitwise
    reproducible, and a 16-walker x 1e5-star slice agrees with the oracle."""
    from mcmc_dynamics_amd import synthetic
    from oracle import lnprob_numpy as oracle
    c, centre = _synthetic(1000000, 3, background=True)
    pos = synthetic.make_walkers(256, NAMES4, c["truth"], config=3)
    lnbg = oracle.gaussian_background(c["v"], c["verr"], 20.0, 40.0)

    def make(sl, model=None):
        return native.Catalog(ctx, c["ra"][sl], c["dec"][sl], c["v"][sl], c["verr"][sl],
                              model=native.MODEL_CONST_BGFIXED, centre=centre, lnlike_bg=lnbg[sl], pmember=c["pmember"][sl])

    full = make(slice(None))
    a = full.loglike(pos)
    b = full.loglike(pos)
    assert np.array_equal(a, b)                                       # fixed reduction tree: bitwise stable
    full.set_option("fast_path", 0)
    assert rel_err(full.loglike(pos), a) < RTOL                        # both formulations, 2.56e8 terms
    parts = sum(make(slice(lo, hi)).loglike(pos) for lo, hi in ((0, 333333), (333333, 700001), (700001, 1000000)))
    assert rel_err(parts, a) < RTOL                                    # sharded sum == un-sharded
    sl = slice(0, 100000)
    sub = {k: v[sl] for k, v in c.items() if isinstance(v, np.ndarray)}
    want = oracle.batched_constant_lnlike(sub, pos[:16], *centre, lnlike_background=lnbg[sl], pmember=sub["pmember"])
    assert rel_err(make(sl).loglike(pos[:16]), want) < RTOL
    full.upload_params(pos)                                            # device-resident pipeline == blocking call
    full.set_option("fast_path", 1)
    full.upload_params(pos)
    full.enqueue()
    full.enqueue()
    assert np.array_equal(full.fetch(), a)


def test_ragged_shapes(native, ctx):
    """W not a multiple of the 64-lane walker tile, N not a multiple of the 8-star group, tiny N."""
    from mcmc_dynamics_amd import synthetic
    from oracle import lnprob_numpy as oracle
    for n, w in ((1, 1), (7, 3), (63, 65), (1001, 130), (4097, 64), (3000, 300), (2500, 512), (900, 1000)):
        c, centre = _synthetic(n, 2)
        pos = synthetic.make_walkers(w, NAMES4, c["truth"], config=2)
        cat = native.Catalog(ctx, c["ra"], c["dec"], c["v"], c["verr"], model=native.MODEL_CONST, centre=centre)
        want = oracle.batched_constant_lnlike(c, pos, *centre)
        assert rel_err(cat.loglike(pos), want) < RTOL
        cat.set_option("target_waves", 64)                             # long chunks: many 8-groups + tail
        assert rel_err(cat.loglike(pos), want) < RTOL


def test_physical_invariances(native, ctx):
    """(2) pmember == 1 mixture == no-background; (3) rotating every position angle and theta_0 by the same
    angle leaves lnL unchanged; f_back = 0 mixture == no-background."""
    from mcmc_dynamics_amd import synthetic
    c, centre = _synthetic(20000, 3, background=True)
    pos = synthetic.make_walkers(64, NAMES4, c["truth"], config=3)
    plain = native.Catalog(ctx, c["ra"], c["dec"], c["v"], c["verr"], model=native.MODEL_CONST, centre=centre).loglike(pos)
    mix = native.Catalog(ctx, c["ra"], c["dec"], c["v"], c["verr"], model=native.MODEL_CONST_BGFIXED, centre=centre,
                         lnlike_bg=np.full(20000, -7.0), pmember=np.ones(20000)).loglike(pos)
    assert rel_err(mix, plain) < RTOL
    pos7 = np.hstack([pos, np.tile([20.0, 40.0, 0.0], (64, 1))])
    gb = native.Catalog(ctx, c["ra"], c["dec"], c["v"], c["verr"], model=native.MODEL_CONST_BGGAUSS, centre=centre,
                        density=c["density"]).loglike(pos7)
    assert rel_err(gb, plain) < RTOL
    # rotate the sky about the centre by delta: (dx, dy) -> R(delta)(dx, dy), and (v_maxx, v_maxy) likewise
    from oracle import lnprob_numpy as oracle
    delta = 0.7
    dx, dy = oracle.calc_xy_offset(c["ra"], c["dec"], *centre)
    rx, ry = np.cos(delta) * dx - np.sin(delta) * dy, np.sin(delta) * dx + np.cos(delta) * dy
    ra2, dec2 = synthetic.offsets_to_radec(rx, ry, *centre)
    pos_rot = pos.copy()
    pos_rot[:, 2] = np.cos(delta) * pos[:, 2] - np.sin(delta) * pos[:, 3]
    pos_rot[:, 3] = np.sin(delta) * pos[:, 2] + np.cos(delta) * pos[:, 3]
    rot = native.Catalog(ctx, ra2, dec2, c["v"], c["verr"], model=native.MODEL_CONST, centre=centre).loglike(pos_rot)
    assert rel_err(rot, plain) < 1e-10                                   # inverse projection round trip ~1e-13 rad


def test_out_of_range_inputs_take_the_plain_path(native, ctx):
    """sigma = 0 with a zero-error star makes norm = 0: the range guard must route to the plain kernels,
    which reproduce the reference's non-finite result instead of a wrong finite one."""
    from mcmc_dynamics_amd import synthetic
    c, centre = _synthetic(500, 2)
    verr = c["verr"].copy()
    verr[10] = 0.0
    cat = native.Catalog(ctx, c["ra"], c["dec"], c["v"], verr, model=native.MODEL_CONST, centre=centre)
    pos = synthetic.make_walkers(8, NAMES4, c["truth"], config=2)
    assert np.all(np.isfinite(cat.loglike(pos)))
    pos[3, 1] = 0.0
    out = cat.loglike(pos)
    assert not np.isfinite(out[3]) and np.all(np.isfinite(np.delete(out, 3)))
    huge = pos.copy()
    huge[:, 1] = 1e40                                                    # sigma^2 = 1e80 > 2^60: guard -> plain
    from oracle import lnprob_numpy as oracle
    cat2 = native.Catalog(ctx, c["ra"], c["dec"], c["v"], c["verr"], model=native.MODEL_CONST, centre=centre)
    assert rel_err(cat2.loglike(huge), oracle.batched_constant_lnlike(c, huge, *centre)) < RTOL


def test_precision_sweep_c5(native, ctx):
    """float32 vs float64 on a radial-binned catalogue (C5): f32 terms + f64 accumulation <= 1e-6, pure f32
    <= 2e-5 relative (SURVEY appendix measured 9.5e-9 / 1.8e-7 at 1e5 stars)."""
    from mcmc_dynamics_amd import synthetic
    from oracle import lnprob_numpy as oracle
    c, centre = _synthetic(200000, 5, min_sep_arcmin=0)
    dx, dy = oracle.calc_xy_offset(c["ra"], c["dec"], *centre)
    bins = oracle.make_radial_bins(np.hypot(dx, dy), 1000, 0.05).astype(np.int64)
    order = np.argsort(bins, kind="stable")
    offs = np.concatenate([[0], np.cumsum(np.bincount(bins))])
    n_bins = len(offs) - 1
    pos = synthetic.make_walkers(128, NAMES4, c["truth"], config=5)
    params = np.broadcast_to(pos, (n_bins,) + pos.shape)
    out = {}
    for prec in ("f64", "f32acc64", "f32"):
        cat = native.Catalog(ctx, c["ra"][order], c["dec"][order], c["v"][order], c["verr"][order],
                             model=native.MODEL_CONST, centre=centre, bin_offsets=offs, precision=prec)
        out[prec] = cat.loglike(params)
        assert out[prec].shape == (n_bins, 128)
    b0 = slice(offs[0], offs[1])
    sub = {k: c[k][order][b0] for k in ("ra", "dec", "v", "verr")}
    # The innermost bin holds stars within ~1e-3 arcsec of the centre, where theta = arctan2(dy, dx) is
    # ill-conditioned in the reference's own formula (calc_xy_offset.py:31 subtracts two O(0.4) products to
    # get dy ~ 1e-9): one ulp in sin/cos (device libm vs NumPy) moves theta by ~1e-16 / r.  Measured 9e-12.
    assert rel_err(out["f64"][0], oracle.batched_constant_lnlike(sub, pos, *centre)) < 1e-10
    b5 = slice(offs[5], offs[6])
    sub5 = {k: c[k][order][b5] for k in ("ra", "dec", "v", "verr")}
    assert rel_err(out["f64"][5], oracle.batched_constant_lnlike(sub5, pos, *centre)) < RTOL
    assert rel_err(out["f32acc64"], out["f64"]) < 1e-6
    assert rel_err(out["f32"], out["f64"]) < 2e-5


def test_rank_mode_context_single_rank(native):
    """One-process-per-GPU entry point with a world of one: no RCCL, same numbers."""
    from mcmc_dynamics_amd import synthetic
    c, centre = _synthetic(3000, 4)
    pos = synthetic.make_walkers(64, NAMES4, c["truth"], config=4)
    ctx1 = native.Context(rank=0, n_ranks=1, device=0)
    a = native.Catalog(ctx1, c["ra"], c["dec"], c["v"], c["verr"], model=native.MODEL_CONST, centre=centre).loglike(pos)
    b = native.Catalog(native.default_context(), c["ra"], c["dec"], c["v"], c["verr"], model=native.MODEL_CONST,
                       centre=centre).loglike(pos)
    assert np.array_equal(a, b)


@pytest.mark.parametrize("kind", ["rank", "single_process"])
def test_rccl_call_path_on_one_rank(native, kind):
    """MCD_FORCE_RCCL=1, both context kinds: unique id -> ncclCommInitRank(1 rank) (one process per GPU), and
    ncclCommInitAll(1 device) + ncclGroupStart/End (one process, several GPUs) -> ncclAllReduce(sum, f64) on the
    catalogue's stream.  Exercises librccl loading and the collective call site on a single GPU; sums are unchanged."""
    import os
    from mcmc_dynamics_amd import synthetic
    c, centre = _synthetic(5000, 4)
    pos = synthetic.make_walkers(128, NAMES4, c["truth"], config=4)
    ref = native.Catalog(native.default_context(), c["ra"], c["dec"], c["v"], c["verr"], model=native.MODEL_CONST,
                         centre=centre).loglike(pos)
    os.environ["MCD_FORCE_RCCL"] = "1"
    try:
        if kind == "rank":
            uid = native.Context.unique_id()
            assert len(uid) == native.UNIQUE_ID_BYTES and any(uid)
            ctx1 = native.Context(rank=0, n_ranks=1, unique_id=uid, device=0)
        else:
            ctx1 = native.Context(n_devices=1)
    finally:
        del os.environ["MCD_FORCE_RCCL"]
    info = ctx1.comm_info()                                   # what RCCL itself says about the communicator
    assert info["size"] == 1 and info["rank"] == 0 and info["rccl_version"] > 20000, info
    assert native.default_context().comm_info()["size"] == 0  # the plain single-GPU context never loads RCCL
    cat = native.Catalog(ctx1, c["ra"], c["dec"], c["v"], c["verr"], model=native.MODEL_CONST, centre=centre)
    for _ in range(3):
        assert np.array_equal(cat.loglike(pos), ref)
    # Pipelined use: the all-reduce of step i runs on the communication stream while step i + 1 computes, results
    # alternate between two buffers.  Different walker tables per step, so that a stale or half-reduced buffer shows.
    plain = native.Catalog(native.default_context(), c["ra"], c["dec"], c["v"], c["verr"], model=native.MODEL_CONST,
                           centre=centre)
    rng = np.random.default_rng(5)
    for depth in (1, 2, 3, 7):
        tables = [pos * (1.0 + 0.01 * rng.normal(size=pos.shape)) for _ in range(depth)]
        for t in tables[:-1]:                       # results of these steps are overwritten, never fetched
            cat.upload_params(t)
            cat.enqueue()
        cat.upload_params(tables[-1])
        for _ in range(depth):                      # same table enqueued repeatedly: both buffers hold its result
            cat.enqueue()
        assert np.array_equal(cat.fetch(), plain.loglike(tables[-1]))
    # a mixture catalogue in the denormal regime: the re-run flag word travels through the all-reduce in either buffer
    g = load_golden("constant_bg_gaussian_fixed")
    pm = g["pmember"].copy()
    pm[:3] = 1.0
    v = g["v"].copy()
    v[:3] = [900.0, -1500.0, 4000.0]
    gc = (float(g["ra_center"]), float(g["dec_center"]))
    kw = dict(model=native.MODEL_CONST_BGFIXED, centre=gc, lnlike_bg=g["lnlike_background"], pmember=pm)
    rows = g["values"][np.isfinite(g["lnprior"]) & (g["values"][:, 1] > 0)]
    mix = native.Catalog(ctx1, g["ra"], g["dec"], v, g["verr"], **kw)
    want = native.Catalog(native.default_context(), g["ra"], g["dec"], v, g["verr"], **kw).loglike(rows)
    for _ in range(3):
        got = mix.loglike(rows)
        assert np.array_equal(np.isfinite(got), np.isfinite(want)) and np.all(np.isneginf(want))
    assert mix.rerun_count == 3
    mix.close()
    cat.close()
    plain.close()
    ctx1.close()


def test_pipelined_enqueue_never_mixes_steps(native, ctx):
    """mcd_params_upload / mcd_loglike_enqueue / mcd_loglike_fetch with DIFFERENT walker tables per step, different
    pipeline depths and blocking calls in between: every fetched result equals the blocking call's, bit for bit."""
    from mcmc_dynamics_amd import synthetic
    c, centre = _synthetic(60000, 3, background=True)
    names = NAMES4
    lnbg = synthetic_gaussian_background(c)
    cat = native.Catalog(ctx, c["ra"], c["dec"], c["v"], c["verr"], model=native.MODEL_CONST_BGFIXED, centre=centre,
                         lnlike_bg=lnbg, pmember=c["pmember"])
    ref = native.Catalog(ctx, c["ra"], c["dec"], c["v"], c["verr"], model=native.MODEL_CONST_BGFIXED, centre=centre,
                         lnlike_bg=lnbg, pmember=c["pmember"])
    rng = np.random.default_rng(12)
    base = synthetic.make_walkers(192, names, c["truth"], config=3)
    for depth in (1, 2, 3, 4, 9):
        tables = [base * (1.0 + 0.02 * rng.normal(size=base.shape)) for _ in range(depth)]
        want = [ref.loglike(t) for t in tables]
        for t in tables:                                   # only the last result is fetched ...
            cat.upload_params(t)
            cat.enqueue()
        assert np.array_equal(cat.fetch(), want[-1])
        for t, w in zip(tables, want):                     # ... and every one when fetched step by step
            cat.upload_params(t)
            cat.enqueue()
            assert np.array_equal(cat.fetch(), w)
        cat.upload_params(tables[0])
        for _ in range(depth + 1):
            cat.enqueue()
        assert np.array_equal(cat.loglike(tables[-1]), want[-1])      # blocking call right behind pipelined steps
        cat.enqueue()                                                # pipelined step right behind a blocking call
        assert np.array_equal(cat.fetch(), want[-1])
    cat.close()
    ref.close()


def synthetic_gaussian_background(c):
    from mcmc_dynamics_amd.background import Gaussian
    return Gaussian(20.0, 40.0)(c["v"], c["verr"])


def test_c4_size_shards(native, ctx):
    """1e7 stars x 256 walkers (C4): the eight 1.25e6-star shards a node would hold sum to the un-sharded value
    (what the RCCL all-reduce computes), and the sum over radial bins equals it too."""
    from mcmc_dynamics_amd import distributed, synthetic
    c, centre = _synthetic(10000000, 4)
    pos = synthetic.make_walkers(256, NAMES4, c["truth"], config=4)
    full = native.Catalog(ctx, c["ra"], c["dec"], c["v"], c["verr"], model=native.MODEL_CONST, centre=centre)
    want = full.loglike(pos)
    assert np.all(np.isfinite(want)) and np.all(want < -3e7)
    total = np.zeros(256)
    for rank in range(8):
        lo, hi = distributed.shard_bounds(10000000, rank, 8)
        assert hi - lo == 1250000
        total += native.Catalog(ctx, c["ra"][lo:hi], c["dec"][lo:hi], c["v"][lo:hi], c["verr"][lo:hi],
                                model=native.MODEL_CONST, centre=centre).loglike(pos)
    assert rel_err(total, want) < RTOL
    full.close()


def test_single_stars_background(native, ctx):
    """background.SingleStars (KDE over comparison stars) feeding the fixed-background kernel (runner.py:96-106)."""
    from mcmc_dynamics_amd import SingleStars, synthetic
    from oracle import lnprob_numpy as oracle
    c, centre = _synthetic(4000, 3, background=True)
    comp = np.random.default_rng(2).normal(20.0, 40.0, size=300)
    lnbg = SingleStars(comp)(c["v"], c["verr"])
    pos = synthetic.make_walkers(32, NAMES4, c["truth"], config=3)
    cat = native.Catalog(ctx, c["ra"], c["dec"], c["v"], c["verr"], model=native.MODEL_CONST_BGFIXED, centre=centre,
                         lnlike_bg=lnbg, pmember=c["pmember"])
    want = oracle.batched_constant_lnlike(c, pos, *centre, lnlike_background=lnbg, pmember=c["pmember"])
    assert rel_err(cat.loglike(pos), want) < RTOL


def _kde_err(got, want):
    """max |got - want| / max(1, |want|): the KDE log-likelihood crosses zero, so a floor of 1 on the scale."""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and np.isfinite(got).all()
    return float(np.max(np.abs(got - want) / np.maximum(1.0, np.abs(want)))) if got.size else 0.0


def test_kde_background_matches_reference_golden(native, ctx):
    """mcd_kde_background against background.SingleStars of the reference itself (tests/golden/single_stars.npz,
    single_stars.py:42-77): sigma_int = 0 / 2.5 km/s, a > 1e4-sigma outlier whose other kernels all underflow, a test
    star exactly on a comparison star, M = 1; tolerance 1e-13 relative (f64)."""
    g = load_golden("single_stars")
    for tag in ("s0", "s2"):
        got = ctx.kde_background(g["comp"], g["v"], g["verr"], float(g["sigma_int_" + tag]))
        assert _kde_err(got, g["lnlike_" + tag]) < 1e-13
    assert _kde_err(ctx.kde_background([12.5], g["v"][:50], g["verr"][:50]), g["lnlike_m1"]) < 1e-13


@pytest.mark.parametrize("n,m", [(1, 1), (63, 7), (64, 8), (65, 513), (1000, 5000), (200, 70001), (30000, 2000)])
def test_kde_background_shapes_against_oracle(native, ctx, n, m):
    """Ragged tiles (n not a multiple of 64), ragged slices (m not a multiple of 8 / of the slice length), several
    slices per tile (small n, large m) and a single slice (large n): all against the NumPy restatement."""
    from oracle import lnprob_numpy as oracle
    rng = np.random.default_rng(1000 * n + m)
    comp = rng.normal(15.0, 45.0, m)
    v = rng.normal(0.0, 60.0, n)
    verr = 0.05 + rng.lognormal(0.0, 0.7, n)
    for s_int in (0.0, 1.7):
        got = ctx.kde_background(comp, v, verr, s_int)
        want = oracle.single_stars_background(comp, v, verr, s_int)
        assert got.shape == (n,) and _kde_err(got, want) < 1e-13
    again = ctx.kde_background(comp, v, verr, 1.7)
    assert np.array_equal(got, again)                               # fixed combination order: bitwise repeatable


def test_kde_background_edges(native, ctx):
    """Empty test set is a no-op; no comparison stars is an error (the reference raises on the empty maximum); isolated
    test stars 1e6 sigma away stay finite (log-sum-exp about the nearest comparison star)."""
    assert ctx.kde_background([1.0, 2.0], [], []).shape == (0,)
    with pytest.raises(native.NativeError):
        ctx.kde_background([], [1.0], [1.0])
    with pytest.raises(ValueError):
        ctx.kde_background([1.0], [1.0, 2.0], [1.0])
    far = ctx.kde_background([0.0, 5.0], [1.0e4], [0.01])
    want = -0.5 * (1.0e4 - 5.0) ** 2 / 1e-4 - 0.5 * np.log(2 * np.pi * 1e-4) - np.log(2.0)
    assert np.isfinite(far[0]) and abs(far[0] - want) <= 1e-13 * abs(want)


def test_runner_with_single_stars_background_matches_reference(native, ctx):
    """ConstantFit(background=SingleStars(...)): the KDE precompute (device) feeding the fixed-background kernel, against
    lnprob of the reference on the same catalogue (tests/golden/single_stars.npz)."""
    from mcmc_dynamics_amd import DataReader, SingleStars
    from mcmc_dynamics_amd.analysis import ConstantFit
    g = load_golden("single_stars")
    data = DataReader({k: g[k] for k in ("ra", "dec", "v", "verr", "pmember")})
    cf = ConstantFit(data, background=SingleStars(g["comp"]), context=ctx)
    cf.parameters["ra_center"].set(value=float(g["ra_center"]), fixed=True)
    cf.parameters["dec_center"].set(value=float(g["dec_center"]), fixed=True)
    assert _kde_err(cf.lnlike_background, g["lnlike_background"]) < 1e-13
    assert [str(x) for x in g["names"]] == list(cf.fitted_parameters)
    assert rel_err(cf.lnprob_batch(g["values"]), g["lnprob"]) < RTOL
    cf.close()


def test_closed_form_known_answer(native, ctx):
    """SURVEY.md 8(c) known-answer (1): v_max = 0 => lnL = sum -1/2 [log(2 pi (e_i^2 + s^2)) + (v_i - v_sys)^2 / (e_i^2 + s^2)]
    on three hand-computable stars, through every kernel formulation; and (6): sigma = 0 is accepted by the kernels."""
    ra, dec = np.array([10.0, 10.01, 9.99]), np.array([0.0, 0.01, -0.01])
    v, verr = np.array([1.0, -2.0, 0.5]), np.array([1.0, 2.0, 0.5])
    rows = np.array([[0.25, 3.0, 0.0, 0.0], [-1.0, 0.0, 0.0, 0.0], [0.0, 7.5, 0.0, 0.0]])
    want = np.array([np.sum(-0.5 * (np.log(2 * np.pi * (verr ** 2 + s ** 2)) + (v - vs) ** 2 / (verr ** 2 + s ** 2)))
                     for vs, s, _, _ in rows])
    for fast in (1, 0):
        cat = native.Catalog(ctx, ra, dec, v, verr, model=native.MODEL_CONST, centre=(10.0, 0.0))
        cat.set_option("fast_path", fast)
        assert np.max(np.abs(cat.loglike(rows) - want)) < 1e-13
        free = native.Catalog(ctx, ra, dec, v, verr, model=native.MODEL_CONST, centre=None)
        free.set_option("fast_path", fast)
        assert np.max(np.abs(free.loglike(np.hstack([rows, np.tile([10.0, 0.0], (3, 1))])) - want)) < 1e-13
    # ModelFit with v_max = 0 and a -> infinity is the constant-dispersion model
    prof = native.Catalog(ctx, ra, dec, v, verr, model=native.MODEL_PROFILE, centre=(10.0, 0.0))
    prows = np.column_stack([rows[:, 0], rows[:, 1], np.full(3, 1e12), rows[:, 2], rows[:, 3], np.full(3, 60.0)])
    assert np.max(np.abs(prof.loglike(prows) - want)) < 1e-9


@pytest.mark.parametrize("model", [0, 1, 2, 3, 4, 5])
def test_fast_and_plain_kernels_agree_over_wide_ranges(native, ctx, model):
    """Device counterpart of tests/test_guard_random_cpu.py: random catalogues / walkers spanning many orders of
    magnitude (velocity scale 0.1 .. 3000 km/s, errors 1e-3 .. 300 km/s, gross outliers, pmember in {0, 1}, density 0).
    With the fast path enabled (the library's guard decides per call) and disabled, the results must agree, including
    which walkers are -inf.  This exercises v_rsq_f64 / v_rcp_f64 + Newton steps on the hardware."""
    from test_guard_random_cpu import CENTRE, MODELS, random_case
    rng = np.random.default_rng(500 + model)
    reruns = 0
    for trial in range(200):
        cat, params = random_case(rng, model, n=int(rng.integers(1, 900)), w=int(rng.integers(1, 140)))
        kw = {}
        if model == 1:
            kw = dict(lnlike_bg=cat["lnlike_bg"], pmember=cat["pmember"])
        elif model in (2, 4):
            kw = dict(density=cat["density"])
        elif model == 5:
            kw = dict(lnlike_bg=cat["lnlike_bg"], density=cat["density"])
        g = native.Catalog(ctx, cat["ra"], cat["dec"], cat["v"], cat["verr"], model=model, centre=CENTRE, **kw)
        assert g.k == MODELS[model]
        fast = g.loglike(params)
        reruns += g.rerun_count
        g.set_option("fast_path", 0)
        plain = g.loglike(params)
        g.close()
        assert np.array_equal(np.isfinite(fast), np.isfinite(plain)), (trial, fast, plain)
        ok = np.isfinite(plain)
        # every term is O(1 .. 10): a total that cancels below the number of stars is judged on that scale
        assert np.max(np.abs(fast[ok] - plain[ok]) / np.maximum(np.abs(plain[ok]), len(cat["v"])), initial=0.0) < 1e-11, trial
    assert reruns == 0 or model in (1, 2, 4, 5)          # only mixtures can meet the reference's denormal regime


@pytest.mark.parametrize("model", [0, 1, 2, 3, 5])
def test_fast_and_plain_kernels_agree_free_centre(native, ctx, model):
    """Same as above with the centre as a walker parameter (geometry recomputed per term)."""
    from test_guard_random_cpu import CENTRE, random_case
    rng = np.random.default_rng(900 + model)
    head = 6 if model >= 3 else 4
    for trial in range(60):
        cat, params = random_case(rng, model, n=int(rng.integers(1, 700)), w=int(rng.integers(1, 100)))
        centre_cols = np.column_stack([CENTRE[0] + rng.normal(0, 0.01, len(params)), CENTRE[1] + rng.normal(0, 0.01, len(params))])
        params = np.hstack([params[:, :head], centre_cols, params[:, head:]])
        kw = {}
        if model == 1:
            kw = dict(lnlike_bg=cat["lnlike_bg"], pmember=cat["pmember"])
        elif model == 2:
            kw = dict(density=cat["density"])
        elif model == 5:
            kw = dict(lnlike_bg=cat["lnlike_bg"], density=cat["density"])
        g = native.Catalog(ctx, cat["ra"], cat["dec"], cat["v"], cat["verr"], model=model, centre=None, **kw)
        fast = g.loglike(params)
        g.set_option("fast_path", 0)
        plain = g.loglike(params)
        g.close()
        assert np.array_equal(np.isfinite(fast), np.isfinite(plain)), trial
        ok = np.isfinite(plain)
        assert np.max(np.abs(fast[ok] - plain[ok]) / np.maximum(np.abs(plain[ok]), len(cat["v"])), initial=0.0) < 1e-11, trial


@pytest.mark.parametrize("model", [1, 2, 5])
def test_binned_mixture_models(native, ctx, model):
    """Radial bins with the mixture likelihoods: every bin's value equals a stand-alone catalogue of that bin's
    stars (per-bin constants such as the hoisted sum of lnL_bg included), for per-bin walker ensembles."""
    from mcmc_dynamics_amd import synthetic
    from oracle import lnprob_numpy as oracle
    from test_guard_random_cpu import random_case, CENTRE
    rng = np.random.default_rng(40 + model)
    cat, params = random_case(rng, model, n=6000, w=40)
    dx, dy = oracle.calc_xy_offset(cat["ra"], cat["dec"], *CENTRE)
    bins = oracle.make_radial_bins(np.hypot(dx, dy), 700, 0.05).astype(np.int64)
    order = np.argsort(bins, kind="stable")
    offs = np.concatenate([[0], np.cumsum(np.bincount(bins))])
    n_bins = len(offs) - 1
    assert n_bins >= 4
    srt = {k: v[order] for k, v in cat.items()}

    def kw(sl):
        if model == 1:
            return dict(lnlike_bg=srt["lnlike_bg"][sl], pmember=srt["pmember"][sl])
        if model == 2:
            return dict(density=srt["density"][sl])
        return dict(lnlike_bg=srt["lnlike_bg"][sl], density=srt["density"][sl])

    per_bin_params = np.stack([params * (1.0 + 0.002 * b) for b in range(n_bins)])
    if model in (2, 5):
        per_bin_params[..., -1] = np.clip(per_bin_params[..., -1], 0.0, 1.0)
    full = native.Catalog(ctx, srt["ra"], srt["dec"], srt["v"], srt["verr"], model=model, centre=CENTRE,
                          bin_offsets=offs, **kw(slice(None)))
    got = full.loglike(per_bin_params)
    assert got.shape == (n_bins, 40)
    for b in range(n_bins):
        sl = slice(offs[b], offs[b + 1])
        one = native.Catalog(ctx, srt["ra"][sl], srt["dec"][sl], srt["v"][sl], srt["verr"][sl], model=model,
                             centre=CENTRE, **kw(sl))
        want = one.loglike(per_bin_params[b])
        one.close()
        assert rel_err(got[b], want) < RTOL, b


def test_lifetime_order_is_safe(native):
    """Closing a context closes its catalogues first; a closed catalogue refuses work instead of crashing."""
    from mcmc_dynamics_amd import synthetic
    c, centre = _synthetic(500, 2)
    pos = synthetic.make_walkers(8, NAMES4, c["truth"], config=2)
    ctx2 = native.Context(n_devices=1)
    cat = native.Catalog(ctx2, c["ra"], c["dec"], c["v"], c["verr"], model=native.MODEL_CONST, centre=centre)
    assert np.all(np.isfinite(cat.loglike(pos)))
    ctx2.close()
    assert cat.handle is None
    with pytest.raises(native.NativeError):
        cat.loglike(pos)
    cat.close()
    ctx2.close()


def _realistic_case(rng, n=None):
    """Random catalogue in the ranges of real data (what oracle/crosscheck_reference.py feeds the reference itself)."""
    n = int(rng.integers(5, 3000)) if n is None else n
    scale_v = 10.0 ** rng.uniform(0, 2.5)
    sep = np.maximum(np.abs(rng.normal(0, 2.0 / 60.0, n)), 1e-4)
    th = rng.uniform(-np.pi, np.pi, n)
    cat = {"ra": CENTRE_RA + sep * np.cos(th) / np.cos(np.radians(CENTRE_DEC)), "dec": CENTRE_DEC + sep * np.sin(th),
           "v": rng.normal(0, scale_v, n), "verr": 10.0 ** rng.uniform(-2, 1.5) * rng.lognormal(0, 0.7, n)}
    cat["v"][: min(2, n)] *= 20.0
    cat["density"] = np.clip(rng.random(n), 0.02, 1.0)
    cat["pmember"] = np.clip(rng.random(n) * 1.1 - 0.05, 0.0, 1.0)
    return cat, scale_v


CENTRE_RA, CENTRE_DEC = 56.345, -26.675


# mcd_guard.h: fast_level for the 24 trials of the test below, from a CPU run of the host build of the guard
# (tests/emul_helper.py: fast_level_at) on the same seeds: MODEL_CONST has no narrow variant, MODEL_PROFILE has one for a
# fixed centre (even trials) only; the guard bounds the variance of the profile mixtures by verr^2 alone, so the trials of
# models 4 and 5 with small errors beside the gross outliers take the general form or the plain kernels
REALISTIC_LEVELS = {
    0: [1] * 24,
    1: [2] * 24,
    2: [2] * 24,
    3: [2, 1] * 12,
    4: [1, 2, 2, 0, 1, 1, 0, 0, 1, 0, 1, 1, 1, 2, 1, 0, 0, 1, 1, 1, 2, 1, 2, 2],
    5: [0, 2, 2, 0, 0, 1, 1, 2, 0, 2, 0, 0, 2, 1, 0, 2, 2, 1, 2, 0, 0, 1, 1, 0],
}


@pytest.mark.parametrize("model", [0, 1, 2, 3, 4, 5])
def test_random_realistic_catalogues_against_the_oracle(native, ctx, model):
    """Device results (whatever kernel family the guard picks) against the NumPy restatement of the reference on random
    catalogues and parameter rows in the ranges of real data, fixed and free centre, all six models; 1e-12 relative on
    the scale max(|lnL|, N)."""
    from oracle import lnprob_numpy as oracle
    rng = np.random.default_rng(7000 + model)
    families = set()
    expected = REALISTIC_LEVELS[model]
    for trial in range(24):
        cat, sv = _realistic_case(rng)
        n = len(cat["v"])
        w = int(rng.integers(1, 12))
        free = bool(trial % 2)
        cols = [rng.normal(0, sv, w), sv * 10.0 ** rng.uniform(-1.5, 0.7, w)]
        if model >= 3:
            cols.append(10.0 ** rng.uniform(0, 2.5, w))                       # a [arcsec]
        cols += [rng.normal(0, sv, w), rng.normal(0, sv, w)]
        if model >= 3:
            cols.append(10.0 ** rng.uniform(0, 2.5, w))                       # r_peak
        if free:
            cols += [CENTRE_RA + rng.normal(0, 0.005, w), CENTRE_DEC + rng.normal(0, 0.005, w)]
        mean_b, sig_b = rng.normal(0, sv), 3 * sv
        if model in (2, 4):
            cols += [rng.normal(0, sv, w), sv * 10.0 ** rng.uniform(-0.5, 1.0, w), rng.random(w)]
        if model == 5:
            cols.append(rng.random(w))
        params = np.stack(cols, axis=1)
        lnbg = oracle.gaussian_background(cat["v"], cat["verr"], mean_b, sig_b)
        kw = {}
        if model == 1:
            kw = dict(lnlike_bg=lnbg, pmember=cat["pmember"])
        elif model in (2, 4):
            kw = dict(density=cat["density"])
        elif model == 5:
            kw = dict(lnlike_bg=lnbg, density=cat["density"])
        g = native.Catalog(ctx, cat["ra"], cat["dec"], cat["v"], cat["verr"], model=model,
                           centre=None if free else (CENTRE_RA, CENTRE_DEC), **kw)
        got = g.loglike(params)
        # the guard's verdict for this trial; a fast mixture kernel that met the reference's denormal regime hands the
        # batch to the plain kernels (level 0, counted in rerun_count)
        assert g.fast_level == expected[trial] or (g.rerun_count == 1 and g.fast_level == 0), (trial, g.fast_level, expected[trial])
        families.add(g.fast_level)
        g.close()
        want = np.empty(w)
        old_err = np.seterr(divide="ignore")              # the reference's log-sum-exp takes log(0) for pmember == 0 stars
        for i, row in enumerate(params):
            rc, dc = (row[6 if model >= 3 else 4], row[7 if model >= 3 else 5]) if free else (CENTRE_RA, CENTRE_DEC)
            if model == 0:
                want[i] = oracle.faithful_constant_lnlike(cat, row[0], row[1], row[2], row[3], rc, dc)
            elif model == 1:
                want[i] = oracle.faithful_constant_lnlike(cat, row[0], row[1], row[2], row[3], rc, dc, lnbg, cat["pmember"])
            elif model == 2:
                want[i] = oracle.faithful_constant_gb_lnlike(cat, row[0], row[1], row[2], row[3], rc, dc, *row[-3:])
            elif model == 3:
                want[i] = oracle.faithful_model_lnlike(cat, *row[:6], rc, dc)
            elif model == 4:
                want[i] = oracle.faithful_model_gb_lnlike(cat, *row[:6], rc, dc, *row[-3:])
            else:
                want[i] = oracle.faithful_model_cb_lnlike(cat, *row[:6], rc, dc, row[-1], lnbg)
        np.seterr(**old_err)
        assert np.array_equal(np.isfinite(got), np.isfinite(want)), (trial, got, want)
        ok = np.isfinite(want)
        assert np.max(np.abs(got[ok] - want[ok]) / np.maximum(np.abs(want[ok]), n), initial=0.0) < 1e-12, (trial, got, want)
    assert families >= set(expected), (families, set(expected))      # every family the guard chose did run on the device


@pytest.mark.parametrize("model,precision", [(0, "f64"), (1, "f64"), (2, "f64"), (5, "f64"), (0, "f32"), (1, "f32")])
def test_record_prefetch_does_not_change_results(native, ctx, model, precision):
    """Option "prefetch" (mcd_math.h: RecordPrefetch) only touches memory the loop reads one iteration later: the sums
    are bitwise the same with it on and off, on ragged chunk lengths, and the last chunk's look-ahead past the end of
    the record array stays inside the allocation's slack (a fault there would kill this test)."""
    from oracle import lnprob_numpy as oracle
    rng = np.random.default_rng(8100 + model)
    for n in (1, 37, 4099, 70001):
        cat, sv = _realistic_case(rng, n=n)
        w = 9
        cols = [rng.normal(0, sv, w), sv * 10.0 ** rng.uniform(-0.5, 0.5, w), rng.normal(0, sv, w), rng.normal(0, sv, w)]
        if model == 2:
            cols += [rng.normal(0, sv, w), sv * 10.0 ** rng.uniform(-0.3, 0.6, w), rng.random(w)]
        if model == 5:
            cols = cols[:2] + [10.0 ** rng.uniform(0, 2, w)] + cols[2:] + [10.0 ** rng.uniform(0, 2, w), rng.random(w)]
        params = np.stack(cols, axis=1)
        lnbg = oracle.gaussian_background(cat["v"], cat["verr"], 0.0, 3 * sv)
        kw = {}
        if model == 1:
            kw = dict(lnlike_bg=lnbg, pmember=cat["pmember"])
        elif model == 2:
            kw = dict(density=cat["density"])
        elif model == 5:
            kw = dict(lnlike_bg=lnbg, density=cat["density"])
        g = native.Catalog(ctx, cat["ra"], cat["dec"], cat["v"], cat["verr"], model=model, centre=(CENTRE_RA, CENTRE_DEC),
                           precision=precision, **kw)
        g.set_option("f32_domain", 0)          # (bitwise equality of two float32 evaluations: the accuracy domain is not the point)
        g.set_option("prefetch", 0)
        off = g.loglike(params)
        g.set_option("prefetch", 1)
        on = g.loglike(params)
        g.set_option("prefetch", -1)
        auto = g.loglike(params)
        g.close()
        assert np.array_equal(off, on, equal_nan=True) and np.array_equal(off, auto, equal_nan=True), (n, off, on)
    g2 = native.Catalog(ctx, cat["ra"], cat["dec"], cat["v"], cat["verr"], model=0, centre=(CENTRE_RA, CENTRE_DEC))
    with pytest.raises(native.NativeError, match="prefetch"):
        g2.set_option("prefetch", 2)
    g2.close()


@pytest.mark.parametrize("model", [0, 1, 2, 3, 4, 5, 6])
def test_balanced_plans_and_combining_workgroups_against_the_oracle(native, ctx, model):
    """Round 3: one round of equal waves (option "balance") with 4-, 8- and 16-wave workgroups (option "combine") for
    1 .. 4 walker tiles and a ragged walker count, every model, fixed and free centre: each plan against the oracle (1e-12)
    and within rounding of the multi-round schedule; bitwise repeatable; the plain kernels (fast_path 0) on the same plan."""
    from oracle import lnprob_numpy as oracle
    rng = np.random.default_rng(9300 + model)
    for trial, (n, w) in enumerate([(20011, 256), (40000, 128), (30000, 64), (12345, 200), (9000, 320)]):
        cat, sv = _realistic_case(rng, n=n)
        cat["pmember"] = np.clip(cat["pmember"], 0.02, 0.98)          # (certain members / non-members: covered elsewhere)
        free = bool(trial % 2) and model != 6
        cols = [rng.normal(0, sv, w), sv * 10.0 ** rng.uniform(-0.5, 0.5, w)]
        if model >= 3:
            cols.append(10.0 ** rng.uniform(0.5, 2.0, w))
        cols += [rng.normal(0, sv, w), rng.normal(0, sv, w)]
        if model >= 3:
            cols.append(10.0 ** rng.uniform(0.5, 2.0, w))
        if free:
            cols += [CENTRE_RA + rng.normal(0, 0.005, w), CENTRE_DEC + rng.normal(0, 0.005, w)]
        if model in (2, 4):
            cols += [rng.normal(0, sv, w), sv * 10.0 ** rng.uniform(-0.3, 0.6, w), 0.05 + 0.9 * rng.random(w)]
        if model == 5:
            cols.append(0.05 + 0.9 * rng.random(w))
        params = np.stack(cols, axis=1)
        lnbg = oracle.gaussian_background(cat["v"], cat["verr"], 0.0, 3 * sv)
        kw = {}
        if model in (1, 6):
            kw = dict(lnlike_bg=lnbg, pmember=cat["pmember"])
        elif model in (2, 4):
            kw = dict(density=cat["density"])
        elif model == 5:
            kw = dict(lnlike_bg=lnbg, density=cat["density"])
        g = native.Catalog(ctx, cat["ra"], cat["dec"], cat["v"], cat["verr"], model=model,
                           centre=None if free else (CENTRE_RA, CENTRE_DEC), **kw)
        g.set_option("balance", 0)
        ref = g.loglike(params)
        want = np.empty(min(w, 6))
        for i, row in enumerate(params[:len(want)]):
            rc, dc = (row[6 if model >= 3 else 4], row[7 if model >= 3 else 5]) if free else (CENTRE_RA, CENTRE_DEC)
            if model == 0:
                want[i] = oracle.faithful_constant_lnlike(cat, row[0], row[1], row[2], row[3], rc, dc)
            elif model == 1:
                want[i] = oracle.faithful_constant_lnlike(cat, row[0], row[1], row[2], row[3], rc, dc, lnbg, cat["pmember"])
            elif model == 2:
                want[i] = oracle.faithful_constant_gb_lnlike(cat, row[0], row[1], row[2], row[3], rc, dc, *row[-3:])
            elif model == 3:
                want[i] = oracle.faithful_model_lnlike(cat, *row[:6], rc, dc)
            elif model == 4:
                want[i] = oracle.faithful_model_gb_lnlike(cat, *row[:6], rc, dc, *row[-3:])
            elif model == 5:
                want[i] = oracle.faithful_model_cb_lnlike(cat, *row[:6], rc, dc, row[-1], lnbg)
            else:
                want[i] = oracle.faithful_model_lnlike(cat, *row[:6], rc, dc, lnbg, cat["pmember"])
        assert np.max(np.abs(ref[:len(want)] - want) / np.maximum(np.abs(want), n)) < 1e-12
        seen = set()
        for balance in (-1, 1, 2, 3, 4, 8):
            for combine in (0, 1, 8, 16):
                for fast_path in (1, 0):
                    g.set_option("fast_path", fast_path)
                    g.set_option("combine", combine)
                    g.set_option("balance", balance)
                    got = g.loglike(params)
                    again = g.loglike(params)
                    info = g.launch_info()
                    seen.add((info["chunks"], info["workgroups"]))
                    assert np.array_equal(got, again), "not bitwise repeatable"
                    assert np.max(np.abs(got - ref) / np.maximum(np.abs(ref), n)) < 2e-13, (n, w, balance, combine, fast_path)
        assert len(seen) >= (6 if trial == 0 else 1), seen           # the options really changed the launch shape
        with pytest.raises(native.NativeError, match="balance"):
            g.set_option("balance", 9)
        with pytest.raises(native.NativeError, match="combine"):
            g.set_option("combine", 3)
        g.close()

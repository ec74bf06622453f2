"""GPU: the differential-evolution move with the ensembles resident on the device (csrc/mcd_de.hip) against the host-driven
loop of the same library (option "device_chain" = 0, csrc/mcd_de.h), against ``mcd_de_move`` fed the replayed numbers of
``mcd_de_numbers``, and against a NumPy restatement of the sampler's half-step loop around ``mcd_loglike_batch``.  The bar is
bit-identity, also when the device gives a block back and however a run is cut into blocks; then the move end to end
through ``ConstantFit``, ``BinnedConstantFit`` and the lock-stepped refits.

Every device model (0 .. 8) runs the four-way comparison, the widest rows also against the 80-bit oracle at the chain's own
rows; the NumPy loop reports the valid rows of every half step, and the tests assert from it that the masks they mean to
exercise (some rows inside and some outside the prior in one half step, a log-normal coordinate on both sides of zero)
did occur.  Beyond that: more ensembles than the step kernel has threads, W = 4 / 8192 / 8194, a seeded block longer than
one grid of the numbers kernel, and each of the four reasons for which the device gives a block back."""
import numpy as np
import pytest

import de_helper as dh
from conftest import load_golden

pytestmark = pytest.mark.gpu
SEED = 0xC0FFEE1234567


@pytest.fixture(scope="module")
def native():
    from mcmc_dynamics_amd import _native
    return _native


@pytest.fixture(scope="module")
def ctx(native):
    return native.default_context()


def run_seeded(cat, plan, pos, lnp, gamma0, sigma, seed, step0, n_steps, device, outputs=True):
    cat.set_option("device_chain", int(device))          # 0 host-driven, 1 resident
    pos, lnp = pos.copy(), lnp.copy()
    lead = pos.shape[:-1]
    chain, lnpc, acc = np.empty((n_steps,) + pos.shape), np.empty((n_steps,) + lead), np.zeros(lead, dtype=np.int64)
    if outputs:
        cat.de_move_seeded(plan, pos, lnp, gamma0, sigma, seed, step0, n_steps, chain, lnpc, acc)
        return pos, lnp, chain, lnpc, acc
    cat.de_move_seeded(plan, pos, lnp, gamma0, sigma, seed, step0, n_steps)
    return pos, lnp


def run_numbers(cat, plan, pos, lnp, nums, device):
    cat.set_option("device_chain", int(device))
    n_steps = nums[0].shape[0]
    pos, lnp = pos.copy(), lnp.copy()
    lead = pos.shape[:-1]
    chain, lnpc, acc = np.empty((n_steps,) + pos.shape), np.empty((n_steps,) + lead), np.zeros(lead, dtype=np.int64)
    cat.de_move(plan, pos, lnp, *nums, chain, lnpc, acc)
    return pos, lnp, chain, lnpc, acc


def de_numbers(native, seed, step0, n, B, W, P, gamma0, sigma, squeeze):
    return tuple(np.ascontiguousarray(a) for a in native.de_numbers(seed, step0, n, B, W, P, gamma0, sigma, squeeze=squeeze))


MODELS = [(0, False), (0, True), (1, False), (3, False), (2, True)]     # CONST, free centre, CONST_BGFIXED, PROFILE, BGGAUSS free
SHAPES = [(33, 8), (4099, 48), (33, 130), (4099, 600)]
CASES = [(m, f, n, w) for (m, f) in MODELS for (n, w) in SHAPES] + \
    [(1, False, n, w) for (n, w) in [(4099, 8), (33, 48), (4099, 130), (33, 600)]]


@pytest.mark.parametrize("model,free,n_stars,w", CASES)
def test_resident_block_is_the_host_driven_one(native, ctx, model, free, n_stars, w):
    """7 steps, continued by 5 through step0.  600 walkers: the strided loops iterate; 130: a ragged last wave."""
    from mcmc_dynamics_amd.sampler import default_gamma0
    rng = np.random.default_rng(7100 + 100 * model + 10 * free + n_stars + w)
    cat, sv = dh.gpu_catalogue(native, ctx, rng, n_stars, model, free)
    pos = dh.gpu_walkers(rng, w, model, sv, free)
    assert pos.shape[1] == cat.k
    lo, hi = dh.gpu_box(cat, pos, model, sv)
    plan = dh.identity_plan(cat.k, lo, hi)
    lnp = cat.loglike(pos)
    assert np.all(np.isfinite(lnp))
    g0, sigma, seed = default_gamma0(cat.k), 1e-5, SEED + model
    before, s_before = cat.de_info(), cat.stretch_info()
    dev = run_seeded(cat, plan, pos, lnp, g0, sigma, seed, 100, 7, device=1)
    mid = cat.de_info()
    assert mid["device_blocks"] == before["device_blocks"] + 1 and mid["discarded_blocks"] == before["discarded_blocks"], mid
    host = run_seeded(cat, plan, pos, lnp, g0, sigma, seed, 100, 7, device=0)
    after = cat.de_info()
    assert after["host_blocks"] == mid["host_blocks"] + 1 and after["device_blocks"] == mid["device_blocks"]
    assert dh.same(dev, host)
    nums = de_numbers(native, seed, 100, 7, 1, w, cat.k, g0, sigma, True)
    assert dh.same(dev, run_numbers(cat, plan, pos, lnp, nums, device=0))
    assert dh.same(dev, run_numbers(cat, plan, pos, lnp, nums, device=1))
    loop = dh.numpy_de_block(cat, plan, pos, lnp, nums)
    assert dh.same(dev, loop)
    # the box did cut into the proposals of a half step without taking them all (otherwise the donor row, the masked rows
    # of the launch and of the walker constants were not exercised)
    assert loop[5]["mixed"] >= 1, loop[5]["n_ok"]
    assert 0 < dev[4].sum() < 7 * w and np.all(np.isfinite(dev[3]))
    # a second block of 5 steps continues the first through step0: resident == host-driven == one block of 12
    dev2 = run_seeded(cat, plan, dev[0], dev[1], g0, sigma, seed, 107, 5, device=1)
    host2 = run_seeded(cat, plan, host[0], host[1], g0, sigma, seed, 107, 5, device=0)
    whole = run_seeded(cat, plan, pos, lnp, g0, sigma, seed, 100, 12, device=1)
    assert dh.same(dev2, host2)
    assert np.array_equal(np.concatenate([dev[2], dev2[2]]), whole[2]) and np.array_equal(dev[4] + dev2[4], whole[4])
    assert not np.array_equal(run_seeded(cat, plan, pos, lnp, g0, sigma, seed + 1, 100, 7, device=1)[2], dev[2])
    assert cat.de_info()["discarded_blocks"] == before["discarded_blocks"]
    assert cat.stretch_info() == s_before                              # DE blocks are counted apart
    cat.close()


WIDE_MODELS = [(4, False), (5, False), (6, False), (7, True), (8, False), (8, True)]   # ... BGDENS, BGFIXED, the double models
WIDE_CASES = [(m, f, n, w) for (m, f) in WIDE_MODELS for (n, w) in [(33, 48), (4099, 130)]]


def _oracle_errors(model, free, cols, rows, got):
    """(error of the device's log-likelihoods against the 80-bit oracle at the same rows, its allowance), both on the scale
    max(|lnL|, N): models 4 .. 6 by oracle/lnprob_numpy.py in longdouble under the rule of tests/test_gpu_variant_matrix.py
    (2 x the error of the float64 oracle + that model's floor), models 7 and 8 by double_helper under the bound of
    tests/test_gpu_double_live.py for the same sums (1e-12, the RTOL of the variant matrix)."""
    import double_helper
    import variant_helper as vh
    from test_gpu_variant_matrix import FLOOR, RTOL
    n, centre = len(cols["v"]), None if free else dh.CENTRE
    mod = double_helper if model >= 7 else vh
    exact = np.array([mod.exact(model, cols, row, centre) for row in rows], dtype=vh.L)
    err = vh.scaled_err(got, exact, n)
    if model >= 7:
        return err, np.full(len(rows), RTOL)
    f64 = np.array([vh.value(model, cols, row, centre) for row in rows])
    return err, 2.0 * vh.scaled_err(f64, exact, n) + FLOOR[(model, free)]


@pytest.mark.parametrize("model,free,n_stars,w", WIDE_CASES)
def test_wide_rows_resident_host_driven_replayed_and_numpy(native, ctx, model, free, n_stars, w):
    """The models with the widest rows (K up to 14), a fixed per-star background or f_back behind the centre: resident ==
    host-driven == ``mcd_de_move`` fed ``mcd_de_numbers`` == the NumPy loop over 7 steps, continued by 5; the last stored
    lnprob row against the 80-bit oracle at the chain's own rows."""
    import variant_helper as vh
    from mcmc_dynamics_amd.sampler import default_gamma0
    rng = np.random.default_rng(7100 + 100 * model + 10 * free + n_stars + w)
    cols, sv = dh.gpu_columns(rng, n_stars, model)
    cat = native.Catalog(ctx, cols["ra"], cols["dec"], cols["v"], cols["verr"], model=model, centre=None if free else dh.CENTRE,
                         **{k: v for k, v in cols.items() if k not in ("ra", "dec", "v", "verr")})
    pos = dh.gpu_walkers(rng, w, model, sv, free)
    assert pos.shape[1] == cat.k == dh.n_columns(model, free)
    lo, hi = dh.gpu_box(cat, pos, model, sv)
    plan = dh.identity_plan(cat.k, lo, hi)
    lnp = cat.loglike(pos)
    assert np.all(np.isfinite(lnp))
    g0, sigma, seed = default_gamma0(cat.k), 1e-5, SEED + model
    before = cat.de_info()
    dev = run_seeded(cat, plan, pos, lnp, g0, sigma, seed, 100, 7, device=1)
    mid = cat.de_info()
    assert mid["device_blocks"] == before["device_blocks"] + 1 and mid["discarded_blocks"] == before["discarded_blocks"], mid
    host = run_seeded(cat, plan, pos, lnp, g0, sigma, seed, 100, 7, device=0)
    assert cat.de_info()["host_blocks"] == mid["host_blocks"] + 1
    assert dh.same(dev, host)
    nums = de_numbers(native, seed, 100, 7, 1, w, cat.k, g0, sigma, True)
    assert dh.same(dev, run_numbers(cat, plan, pos, lnp, nums, device=0))
    assert dh.same(dev, run_numbers(cat, plan, pos, lnp, nums, device=1))
    loop = dh.numpy_de_block(cat, plan, pos, lnp, nums)
    assert dh.same(dev, loop)
    assert loop[5]["mixed"] >= 1, loop[5]["n_ok"]
    assert 0 < dev[4].sum() < 7 * w and np.all(np.isfinite(dev[3]))
    assert np.all((dev[2] >= lo) & (dev[2] <= hi))
    dev2 = run_seeded(cat, plan, dev[0], dev[1], g0, sigma, seed, 107, 5, device=1)
    whole = run_seeded(cat, plan, pos, lnp, g0, sigma, seed, 100, 12, device=1)
    assert dh.same(dev2, run_seeded(cat, plan, host[0], host[1], g0, sigma, seed, 107, 5, device=0))
    assert np.array_equal(np.concatenate([dev[2], dev2[2]]), whole[2]) and np.array_equal(dev[4] + dev2[4], whole[4])
    assert cat.de_info()["discarded_blocks"] == before["discarded_blocks"]
    cat.close()
    if vh.HAVE_LONGDOUBLE:
        err, allowed = _oracle_errors(model, free, cols, whole[2][-1], whole[3][-1])
        worst = int(np.argmax(err / allowed))
        print("oracle", (model, free, n_stars, w), "worst row", worst, "err %.2e allowed %.2e" % (err[worst], allowed[worst]))
        assert np.all(err <= allowed), (worst, err[worst], allowed[worst])


def _many_bins(native):
    """The catalogue and binning of test_hundreds_of_ensembles (tests/test_gpu_device_chain.py): B > 300 bins of 50 stars."""
    from mcmc_dynamics_amd import DataReader, synthetic
    from mcmc_dynamics_amd.analysis import BinnedConstantFit
    cat = synthetic.make_catalog(40000, config=5)
    reader = DataReader({k: cat[k] for k in ("ra", "dec", "v", "verr")})
    reader.make_radial_bins(synthetic.CENTER_RA_DEG, synthetic.CENTER_DEC_DEG, nstars=50, dlogr=0.002)
    bf = BinnedConstantFit(reader)
    bf.parameters["ra_center"].set(value=synthetic.CENTER_RA_DEG, fixed=True)
    bf.parameters["dec_center"].set(value=synthetic.CENTER_DEC_DEG, fixed=True)
    pos1 = synthetic.make_walkers(16, ["v_sys", "sigma_max", "v_maxx", "v_maxy"], cat["truth"], config=5)
    pos = np.ascontiguousarray(np.broadcast_to(pos1, (bf.n_bins,) + pos1.shape)) * \
        (1.0 + 1e-3 * np.random.default_rng(3).normal(size=(bf.n_bins, 16, 4)))
    pos[..., 1] = np.abs(pos[..., 1])
    return bf, pos


def test_hundreds_of_ensembles(native):
    """More ensembles than the step kernel has threads: workgroup 0 walks the table of all ensembles' ranges in strides.
    Resident == host-driven == the multi-ensemble NumPy loop; an ensemble behind the first stride that has no valid proposal
    (status 8), and one whose proposals alone change the guard's verdict (status 4), both give the block back."""
    bf, pos = _many_bins(native)
    B, W, P = bf.n_bins, 16, 4
    assert B > 300 and pos.shape == (B, W, P), B
    lnp = np.ascontiguousarray(bf.lnprob_batch(pos))
    assert np.all(np.isfinite(lnp))
    cat = bf._catalog
    plan = dict(bf._stretch_plan())
    g0 = 2.38 / np.sqrt(2.0 * P)
    before = cat.de_info()
    dev = run_seeded(cat, plan, pos, lnp, g0, 1e-5, SEED, 0, 5, device=1)
    dev2 = run_seeded(cat, plan, dev[0], dev[1], g0, 1e-5, SEED, 5, 4, device=1)
    info = cat.de_info()
    assert info["device_blocks"] == before["device_blocks"] + 2 and info["discarded_blocks"] == before["discarded_blocks"], info
    host = run_seeded(cat, plan, pos, lnp, g0, 1e-5, SEED, 0, 5, device=0)
    host2 = run_seeded(cat, plan, host[0], host[1], g0, 1e-5, SEED, 5, 4, device=0)
    assert dh.same(dev, host) and dh.same(dev2, host2)
    nums = de_numbers(native, SEED, 0, 9, B, W, P, g0, 1e-5, False)
    loop = dh.numpy_de_block(cat, plan, pos, lnp, nums, native.prior_eval)
    assert np.array_equal(loop[2], np.concatenate([dev[2], dev2[2]])) and np.array_equal(loop[3], np.concatenate([dev[3], dev2[3]]))
    assert np.array_equal(loop[0], dev2[0]) and np.array_equal(loop[1], dev2[1]) and np.array_equal(loop[4], dev[4] + dev2[4])
    assert np.all(dev2[4].sum(axis=1) + dev[4].sum(axis=1) > 0) and np.all(np.isfinite(dev2[3]))
    assert cat.de_info()["discarded_blocks"] == before["discarded_blocks"]
    # an ensemble behind the first 256 entirely outside a tightened box: the block comes back with status 8
    e = B - 2
    assert e >= 256
    tight = dict(plan, lo=plan["lo"].copy(), hi=plan["hi"].copy())
    tight["hi"][0] = pos[..., 0].max() + 1.0
    far, far_lnp = pos.copy(), lnp.copy()
    far[e, :, 0] = tight["hi"][0] + 50.0
    far_lnp[e] = -np.inf
    before = cat.de_info()
    dev3 = run_seeded(cat, tight, far, far_lnp, g0, 1e-5, SEED, 0, 3, device=1)
    info = cat.de_info()
    assert info["discarded_blocks"] == before["discarded_blocks"] + 1 and info["last_discard_status"] & 8, info
    assert dh.same(dev3, run_seeded(cat, tight, far, far_lnp, g0, 1e-5, SEED, 0, 3, device=0)) and np.array_equal(dev3[0][e], far[e])
    loop3 = dh.numpy_de_block(cat, tight, far, far_lnp, tuple(a[:3] for a in nums), native.prior_eval)
    assert dh.same(dev3, loop3) and np.all(loop3[5]["n_ok"][:, :, e] == 0) and dev3[4].sum() > 0
    # the scales of step 1, SECOND half step, of that ensemble alone are 1e20: its valid proposals (sigma_max > 0) have
    # |v_sys| + |v_max| beyond the 2^50 the fast kernels of MODEL_CONST admit (mcd_guard.h: guard_verdict), so the verdict
    # on the table of all ensembles is level 0 where the block was enqueued with level 1 -- seen only by a judge that
    # reaches entry B + e of the ranges (parity 1, an ensemble behind the first stride)
    open_plan = dict(plan, lo=np.array([-np.inf, 0.0, -np.inf, -np.inf]), hi=np.full(P, np.inf))
    wild = [a[:3].copy() for a in nums]
    wild[3][1, 1, e, :] = 1e20
    before = cat.de_info()
    calm = run_numbers(cat, open_plan, pos, lnp, [a[:3] for a in nums], device=1)
    info = cat.de_info()
    print("level of the calm block:", cat.fast_level, info)
    assert info["device_blocks"] == before["device_blocks"] + 1 and info["discarded_blocks"] == before["discarded_blocks"], info
    dev4 = run_numbers(cat, open_plan, pos, lnp, wild, device=1)
    info = cat.de_info()
    loop4 = dh.numpy_de_block(cat, open_plan, pos, lnp, wild, native.prior_eval)
    assert 0 < loop4[5]["n_ok"][1, 1, e] and np.all(loop4[5]["n_ok"] > 0)
    assert info["discarded_blocks"] == before["discarded_blocks"] + 1 and info["last_discard_status"] & 4, info
    assert dh.same(dev4, run_numbers(cat, open_plan, pos, lnp, wild, device=0)) and dh.same(dev4, loop4)
    assert not dh.same(dev4, calm)
    bf.close()


@pytest.mark.parametrize("w", [4, 8192, 8194])
def test_ends_of_the_walker_range(native, ctx, w):
    """W = 4: two slots per half step, pick_b forced, one wave mostly idle.  W = 8192: the numbers kernel's ordering keys
    fill 64 KiB of LDS exactly and its rank loop runs 8192 times.  W = 8194: past that, the host fills the pinned numbers
    (de_numbers_of_step) and the resident step kernel consumes them.  Neither may fall back to the host-driven block."""
    rng = np.random.default_rng(7800 + w)
    cat, sv = dh.gpu_catalogue(native, ctx, rng, 33, 0, False)
    pos = dh.gpu_walkers(rng, w, 0, sv, False)
    lo, hi = dh.gpu_box(cat, pos, 0, sv, margin=0.3 if w == 4 else 0.1)    # (two slots: a window that leaves each half step one)
    plan = dh.identity_plan(4, lo, hi)
    lnp = cat.loglike(pos)
    g0, sigma, n = 2.38 / np.sqrt(8.0), 1e-5, 3
    before = cat.de_info()
    dev = run_seeded(cat, plan, pos, lnp, g0, sigma, SEED, 40, n, device=1)
    info = cat.de_info()
    assert info["device_blocks"] == before["device_blocks"] + 1 and info["host_blocks"] == before["host_blocks"] and \
        info["discarded_blocks"] == before["discarded_blocks"], info
    host = run_seeded(cat, plan, pos, lnp, g0, sigma, SEED, 40, n, device=0)
    assert dh.same(dev, host)
    nums = de_numbers(native, SEED, 40, n, 1, w, 4, g0, sigma, True)
    assert dh.same(dev, run_numbers(cat, plan, pos, lnp, nums, device=1))
    assert dh.same(dev, run_numbers(cat, plan, pos, lnp, nums, device=0))
    info = cat.de_info()
    assert info["device_blocks"] == before["device_blocks"] + 2 and info["discarded_blocks"] == before["discarded_blocks"], info
    if w == 4:
        assert np.all(nums[1] != nums[2]) and set(np.unique(nums[1])) <= {0, 1}
        loop = dh.numpy_de_block(cat, plan, pos, lnp, nums)
        assert dh.same(dev, loop) and loop[5]["mixed"] >= 1 and dev[4].sum() > 0
    else:
        assert np.array_equal(np.sort(nums[0], axis=1), np.broadcast_to(np.arange(w, dtype=np.int32), (n, w)))
        assert 0 < dev[4].sum() < n * w
    assert np.all(np.isfinite(dev[3])) and not np.array_equal(dev[0], pos)
    cat.close()


def test_seeded_block_longer_than_one_grid_of_the_numbers_kernel(native, ctx):
    """65 540 steps of 4 walkers: launch_de_numbers needs a second launch (gridDim.y <= 65535), which starts at step
    65 535 of the arrays.  Resident == host-driven == two resident blocks of 65 535 + 5 steps joined through step0.
    (7.7 s on one MI355X for the four blocks together.)"""
    rng = np.random.default_rng(7900)
    cat, sv = dh.gpu_catalogue(native, ctx, rng, 33, 0, False)
    pos = dh.gpu_walkers(rng, 4, 0, sv, False)
    plan = dh.identity_plan(4)                                          # (no box: no half step of two slots without a proposal)
    lnp = cat.loglike(pos)
    g0, n, cut = 2.38 / np.sqrt(8.0), 65540, 65535
    before = cat.de_info()
    dev = run_seeded(cat, plan, pos, lnp, g0, 1e-5, SEED, 0, n, device=1, outputs=False)
    head = run_seeded(cat, plan, pos, lnp, g0, 1e-5, SEED, 0, cut, device=1, outputs=False)
    tail = run_seeded(cat, plan, head[0], head[1], g0, 1e-5, SEED, cut, n - cut, device=1, outputs=False)
    info = cat.de_info()
    assert info["device_blocks"] == before["device_blocks"] + 3 and info["discarded_blocks"] == before["discarded_blocks"], info
    assert dh.same(dev, tail) and not np.array_equal(head[0], tail[0])
    host = run_seeded(cat, plan, pos, lnp, g0, 1e-5, SEED, 0, n, device=0, outputs=False)
    assert dh.same(dev, host) and np.all(np.isfinite(dev[1]))
    cat.close()


def test_log_normal_coordinate_across_zero(native, ctx):
    """The plan of test_priors_fixed_column_and_unit_factor with the log-normal prior on v_maxx (sampled in other units),
    whose walkers sit next to zero: some proposals of a half step have it <= 0 -- outside the prior, no box involved -- and
    some have not.  The block stays resident and equals the host-driven one and the NumPy loop around
    ``mcd_prior_eval``."""
    rng = np.random.default_rng(7250)
    cat, sv = dh.gpu_catalogue(native, ctx, rng, 4099, 1, False)
    w = 48
    half = w // 2
    full = dh.gpu_walkers(rng, w, 1, sv, False)
    pos = np.ascontiguousarray(full[:, [1, 2, 3]])                     # v_sys fixed
    pos[:, 1] = (np.abs(pos[:, 1]) + 0.05) * 60.0                      # v_maxx > 0, sampled in other units
    kind = np.array([native.PRIOR_NORMAL, native.PRIOR_LOGNORMAL, native.PRIOR_FLAT], dtype=np.int32)
    prior = (kind, np.array([sv, np.log(100.0), 0.0]), np.array([6.0, 1.5, 1.0]))
    plan = {"col_source": np.array([-1, 0, 1, 2], dtype=np.int32), "col_const": np.array([0.3, 0, 0, 0]),
            "col_factor": np.array([1.0, 1.0, 1.0 / 60.0, 1.0]), "lo": np.array([-np.inf, -np.inf, -np.inf]),
            "hi": np.full(3, np.inf), "fixed_ok": True, "prior": prior}
    table = np.column_stack([np.full(w, 0.3), pos[:, 0], pos[:, 1] * (1.0 / 60.0), pos[:, 2]])
    lnp = cat.loglike(table) + native.prior_eval(prior, pos)
    assert np.all(np.isfinite(lnp))
    g0 = 2.38 / np.sqrt(6.0)
    before = cat.de_info()
    dev = run_seeded(cat, plan, pos, lnp, g0, 1e-5, SEED, 0, 7, device=1)
    info = cat.de_info()
    assert info["device_blocks"] == before["device_blocks"] + 1 and info["discarded_blocks"] == before["discarded_blocks"], info
    host = run_seeded(cat, plan, pos, lnp, g0, 1e-5, SEED, 0, 7, device=0)
    assert dh.same(dev, host)
    nums = de_numbers(native, SEED, 0, 7, 1, w, 3, g0, 1e-5, True)
    assert dh.same(dev, run_numbers(cat, plan, pos, lnp, nums, device=1))
    loop = dh.numpy_de_block(cat, plan, pos, lnp, nums, native.prior_eval)
    below, n_ok = loop[5]["nonpositive"][:, :, 0], loop[5]["n_ok"][:, :, 0]
    print("proposals with v_maxx <= 0 per half step:", below.ravel())
    assert np.any((below > 0) & (below < half)) and np.array_equal(n_ok, half - below)
    assert dh.same(dev, loop)
    assert 0 < dev[4].sum() < 7 * w and np.all(dev[2][..., 1] > 0.0)
    assert cat.de_info()["discarded_blocks"] == before["discarded_blocks"]
    cat.close()


def test_blocks_given_back_for_a_rerun_and_for_nan(native, ctx):
    """The two reasons test_blocks_the_device_gives_back leaves out, after parts (2) and (1) of the stretch kernel's test
    of that name (tests/test_gpu_device_chain.py)."""
    # (2) re-run request of the fast mixture kernels: certain members that are gross outliers (denormal regime); the tag
    # arrives behind the sums, where workgroup 0 of the next launch compares it
    g = load_golden("constant_bg_gaussian_fixed")
    pm, v = g["pmember"].copy(), g["v"].copy()
    pm[:3] = 1.0
    v[:3] = [900.0, -1500.0, 4000.0]
    gc = (float(g["ra_center"]), float(g["dec_center"]))
    mix = native.Catalog(ctx, g["ra"], g["dec"], v, g["verr"], model=native.MODEL_CONST_BGFIXED, centre=gc,
                         lnlike_bg=g["lnlike_background"], pmember=pm)
    rows = g["values"][np.isfinite(g["lnprior"]) & (g["values"][:, 1] > 0)]
    pos = np.ascontiguousarray(rows[:16])
    lnp = mix.loglike(pos)
    plan = dh.identity_plan(4, lo=[-np.inf, 0.0, -np.inf, -np.inf])
    reruns = mix.rerun_count
    dev = run_seeded(mix, plan, pos, lnp, 0.8, 1e-5, SEED, 0, 4, device=1)
    info = mix.de_info()
    assert info["discarded_blocks"] == 1 and info["last_discard_status"] & 2 and mix.rerun_count > reruns, info
    assert info["device_blocks"] == 0 and info["host_blocks"] == 1
    assert dh.same(dev, run_seeded(mix, plan, pos, lnp, 0.8, 1e-5, SEED, 0, 4, device=0))
    assert dh.same(dev, dh.numpy_de_block(mix, plan, pos, lnp, de_numbers(native, SEED, 0, 4, 1, 16, 4, 0.8, 1e-5, True)))
    assert mix.stretch_info()["discarded_blocks"] == 0
    mix.close()
    # (1) a NaN log-likelihood: the error of the host loop (emcee: "Probability function returned NaN")
    ra = np.array([dh.CENTRE[0] + 0.01, dh.CENTRE[0] - 0.01, dh.CENTRE[0]])
    dec = np.array([dh.CENTRE[1], dh.CENTRE[1] + 0.01, dh.CENTRE[1] - 0.01])
    nan_cat = native.Catalog(ctx, ra, dec, np.array([1.0, 2.0, 3.0]), np.array([0.0, 1.0, 1.0]), model=0, centre=dh.CENTRE)
    pos = np.zeros((8, 4))
    pos[:, 0] = 1.0                                                    # v_sys = v of the verr = 0 star, sigma = 0: 0 / 0
    lnp = np.zeros(8)
    for device in (1, 0):
        with pytest.raises(native.NativeError, match="NaN"):
            run_seeded(nan_cat, dh.identity_plan(4), pos, lnp, 0.8, 1e-5, SEED, 0, 2, device=device)
    info = nan_cat.de_info()
    assert info["last_discard_status"] & 1 and info["discarded_blocks"] == 1 and info["device_blocks"] == 0, info
    nan_cat.close()


def _bins(native):
    from mcmc_dynamics_amd import DataReader
    from mcmc_dynamics_amd.analysis import BinnedConstantFit
    g = load_golden("radial_bins")
    reader = DataReader({k: g[k] for k in ("ra", "dec", "v", "verr")})
    # (three bins of 600, 905 and 1495 stars)
    reader.make_radial_bins(float(g["ra_center"]), float(g["dec_center"]), nstars=600, dlogr=0.4)
    bf = BinnedConstantFit(reader)
    bf.parameters["ra_center"].set(value=float(g["ra_center"]), fixed=True)
    bf.parameters["dec_center"].set(value=float(g["dec_center"]), fixed=True)
    return bf


def test_binned_ensembles(native):
    """B un-equal bins, W = 16: one workgroup per ensemble, the guard judged on the table of all ensembles by the next
    launch; chain and lnprob_chain both given and both NULL; an ensemble without a valid proposal gives the block back."""
    bf = _bins(native)
    B, W, P = bf.n_bins, 16, 4
    assert B == 3 and len(set(np.diff(bf.bin_offsets))) == 3, bf.bin_offsets
    rng = np.random.default_rng(7500)
    pos = np.array([3.0, 9.0, 1.0, -1.0]) * (1.0 + 0.2 * rng.normal(size=(B, W, P)))
    pos[..., 1] = np.abs(pos[..., 1]) + 0.5
    pos = np.ascontiguousarray(pos)
    lnp = np.ascontiguousarray(bf.lnprob_batch(pos))
    assert np.all(np.isfinite(lnp))
    cat = bf._catalog
    plan = dict(bf._stretch_plan())
    g0 = 2.38 / np.sqrt(2.0 * P)
    before = cat.de_info()
    dev = run_seeded(cat, plan, pos, lnp, g0, 1e-5, SEED, 0, 7, device=1)
    info = cat.de_info()
    assert info["device_blocks"] == before["device_blocks"] + 1 and info["discarded_blocks"] == before["discarded_blocks"], info
    host = run_seeded(cat, plan, pos, lnp, g0, 1e-5, SEED, 0, 7, device=0)
    assert dh.same(dev, host)
    nums = de_numbers(native, SEED, 0, 7, B, W, P, g0, 1e-5, False)
    assert dh.same(dev, run_numbers(cat, plan, pos, lnp, nums, device=1))
    assert dh.same(dev, run_numbers(cat, plan, pos, lnp, nums, device=0))
    assert np.all(dev[4].sum(axis=1) > 0) and np.all(np.isfinite(dev[3]))
    for device in (1, 0):                                              # no chain rows asked for
        p, l = run_seeded(cat, plan, pos, lnp, g0, 1e-5, SEED, 0, 7, device=device, outputs=False)
        assert np.array_equal(p, dev[0]) and np.array_equal(l, dev[1])
    dev2 = run_seeded(cat, plan, dev[0], dev[1], g0, 1e-5, SEED, 7, 5, device=1)
    assert dh.same(dev2, run_seeded(cat, plan, host[0], host[1], g0, 1e-5, SEED, 7, 5, device=0))
    # one ensemble entirely outside the prior: the device gives the block back, the host loop lends the bin another's row
    tight = dict(plan, lo=plan["lo"].copy(), hi=plan["hi"].copy())
    tight["hi"][0] = pos[..., 0].max() + 1.0
    far, far_lnp = pos.copy(), lnp.copy()
    far[1, :, 0] = tight["hi"][0] + 50.0
    far_lnp[1] = -np.inf
    before = cat.de_info()
    dev3 = run_seeded(cat, tight, far, far_lnp, g0, 1e-5, SEED, 0, 3, device=1)
    info = cat.de_info()
    assert info["discarded_blocks"] == before["discarded_blocks"] + 1 and info["last_discard_status"] & 8, info
    assert dh.same(dev3, run_seeded(cat, tight, far, far_lnp, g0, 1e-5, SEED, 0, 3, device=0)) and np.array_equal(dev3[0][1], far[1])
    bf.close()


def test_priors_fixed_column_and_unit_factor(native, ctx):
    """A plan as Runner builds it -- one kernel column fixed, one free column with a non-unit factor -- with a normal and
    a log-normal prior through the ``prior`` argument."""
    rng = np.random.default_rng(7200)
    cat, sv = dh.gpu_catalogue(native, ctx, rng, 4099, 1, False)
    w = 48
    full = dh.gpu_walkers(rng, w, 1, sv, False)
    pos = np.ascontiguousarray(full[:, [1, 2, 3]])                     # v_sys fixed
    pos[:, 1] *= 60.0                                                 # v_maxx sampled in other units
    kind = np.array([native.PRIOR_LOGNORMAL, native.PRIOR_NORMAL, native.PRIOR_FLAT], dtype=np.int32)
    prior = (kind, np.array([np.log(sv), 0.0, 0.0]), np.array([0.5, 200.0, 1.0]))
    plan = {"col_source": np.array([-1, 0, 1, 2], dtype=np.int32), "col_const": np.array([0.3, 0, 0, 0]),
            "col_factor": np.array([1.0, 1.0, 1.0 / 60.0, 1.0]), "lo": np.array([-np.inf, -np.inf, -np.inf]),
            "hi": np.full(3, np.inf), "fixed_ok": True, "prior": prior}
    table = np.column_stack([np.full(w, 0.3), pos[:, 0], pos[:, 1] * (1.0 / 60.0), pos[:, 2]])
    lnp = cat.loglike(table) + native.prior_eval(prior, pos)
    g0 = 2.38 / np.sqrt(6.0)
    dev = run_seeded(cat, plan, pos, lnp, g0, 1e-5, SEED, 0, 7, device=1)
    host = run_seeded(cat, plan, pos, lnp, g0, 1e-5, SEED, 0, 7, device=0)
    info = cat.de_info()
    assert dh.same(dev, host) and info["device_blocks"] == 1 and info["discarded_blocks"] == 0, info
    nums = de_numbers(native, SEED, 0, 7, 1, w, 3, g0, 1e-5, True)
    assert dh.same(dev, run_numbers(cat, plan, pos, lnp, nums, device=1))
    assert dh.same(dev, dh.numpy_de_block(cat, plan, pos, lnp, nums, native.prior_eval))
    assert 0 < dev[4].sum() < 7 * w
    flat = run_seeded(cat, dict(plan, prior=None), pos, lnp, g0, 1e-5, SEED, 0, 7, device=1)
    assert not np.array_equal(flat[2], dev[2])                          # (the priors do act)
    # a fixed parameter outside its own bounds: nothing is ever accepted, the device path stands aside
    bad = run_seeded(cat, dict(plan, fixed_ok=False), pos, lnp, g0, 1e-5, SEED, 0, 3, device=1)
    assert np.array_equal(bad[0], pos) and bad[4].sum() == 0 and cat.de_info()["device_blocks"] == 3
    cat.close()


def test_blocks_the_device_gives_back(native, ctx):
    rng = np.random.default_rng(7300)
    # (8) a half step with every proposal outside the prior
    cat, sv = dh.gpu_catalogue(native, ctx, rng, 4099, 0, False)
    w = 16
    pos = dh.gpu_walkers(rng, w, 0, sv, False)
    lnp = cat.loglike(pos)
    plan = dh.identity_plan(4, lo=[1e6, -np.inf, -np.inf, -np.inf])
    dev = run_seeded(cat, plan, pos, lnp, 0.8, 1e-5, SEED, 0, 3, device=1)
    info = cat.de_info()
    assert info["discarded_blocks"] == 1 and info["last_discard_status"] & 8 and info["host_blocks"] == 1, info
    assert np.array_equal(dev[0], pos) and dev[4].sum() == 0
    assert cat.stretch_info()["discarded_blocks"] == 0
    cat.close()
    # (4) the guard picks another kernel family inside a block.  The start has |v_sys| <= 200 with sigma_max <= 0.2: the
    # narrow-range bound d_max^2 <= 2e6 n_min (mcd_guard.h; n_min ~ verr_min^2 = 0.25, so d_max <~ 700) holds for the start and
    # for the proposals of step 0 -- level 2.  The scales of step 1, half step 0 are 30: its proposals lie thousands of km/s
    # out, the guard's verdict on that table is level 1, and the device gives the block back.
    cat, sv = dh.gpu_catalogue(native, ctx, rng, 4099, 1, False)
    pos = dh.gpu_walkers(rng, w, 1, sv, False)
    pos[:, 1] = rng.uniform(0.05, 0.2, w)
    pos[:, 0] = rng.uniform(100.0, 200.0, w)
    lnp = cat.loglike(pos)
    assert cat.fast_level == 2
    plan = dh.identity_plan(4, lo=[-np.inf, 0.0, -np.inf, -np.inf])
    nums = list(de_numbers(native, SEED, 0, 4, 1, w, 4, 0.8, 1e-5, True))
    calm = run_numbers(cat, plan, pos, lnp, nums, device=1)
    info = cat.de_info()
    assert info["device_blocks"] == 1 and info["discarded_blocks"] == 0, info
    assert dh.same(calm, run_numbers(cat, plan, pos, lnp, nums, device=0))
    nums[3] = nums[3].copy()
    nums[3][1, 0, :] = 30.0
    dev = run_numbers(cat, plan, pos, lnp, nums, device=1)
    info = cat.de_info()
    print("level change:", info, "accepted", dev[4].sum())
    assert info["discarded_blocks"] == 1 and info["last_discard_status"] & 4 and info["device_blocks"] == 1, info
    assert dh.same(dev, run_numbers(cat, plan, pos, lnp, nums, device=0))
    assert dh.same(dev, dh.numpy_de_block(cat, plan, pos, lnp, nums))
    assert cat.stretch_info()["discarded_blocks"] == 0
    cat.close()


def test_invalid_arguments_leave_the_state_alone(native, ctx):
    rng = np.random.default_rng(7400)
    cat, sv = dh.gpu_catalogue(native, ctx, rng, 33, 0, False)
    w = 8
    pos = dh.gpu_walkers(rng, w, 0, sv, False)
    lnp = cat.loglike(pos)
    plan = dh.identity_plan(4)
    for mode in (1, 0):
        cat.set_option("device_chain", mode)
        for g0, sigma in ((0.0, 1e-5), (-0.5, 1e-5), (np.inf, 1e-5), (np.nan, 1e-5), (0.8, -1e-5), (0.8, np.nan)):
            p, l = pos.copy(), lnp.copy()
            with pytest.raises(native.NativeError, match="status -?[0-9]+"):
                cat.de_move_seeded(plan, p, l, g0, sigma, SEED, 0, 3)
            assert np.array_equal(p, pos) and np.array_equal(l, lnp)
        for sub in (2, 7):                                              # W < 4, W odd
            p, l = pos[:sub].copy(), lnp[:sub].copy()
            with pytest.raises(native.NativeError):
                cat.de_move_seeded(plan, p, l, 0.8, 1e-5, SEED, 0, 3)
            assert np.array_equal(p, pos[:sub]) and np.array_equal(l, lnp[:sub])
        p, l = np.stack([pos, pos]), np.stack([lnp, lnp])               # n_bins = 2 on a catalogue without bins
        with pytest.raises(native.NativeError):
            cat.de_move_seeded(plan, p, l, 0.8, 1e-5, SEED, 0, 3)
        assert np.array_equal(p[0], pos) and np.array_equal(l[1], lnp)
        nums = list(de_numbers(native, SEED, 0, 3, 1, w, 4, 0.8, 1e-5, True))
        nums[2] = nums[2].copy()
        nums[2][1, 0, 2] = w // 2                                       # a partner outside the half ensemble
        p, l = pos.copy(), lnp.copy()
        with pytest.raises(native.NativeError):
            cat.de_move(plan, p, l, *nums)
        assert np.array_equal(p, pos) and np.array_equal(l, lnp)
    with pytest.raises(native.NativeError):
        native.de_numbers(SEED, 0, 3, 1, 2, 4, 0.8, 1e-5)
    with pytest.raises(native.NativeError):
        native.de_numbers(SEED, 0, 3, 1, 8, 4, 0.0, 1e-5)
    assert cat.de_info() == {"device_blocks": 0, "host_blocks": 0, "discarded_blocks": 0, "last_discard_status": 0}
    cat.close()


def test_stretch_blocks_around_a_de_block(native, ctx):
    """A stretch block run before and after a DE block on the same catalogue gives the bits it gives alone."""
    def fresh():
        rng = np.random.default_rng(7600)
        cat, sv = dh.gpu_catalogue(native, ctx, rng, 4099, 1, False)
        pos = dh.gpu_walkers(rng, 48, 1, sv, False)
        return cat, pos, cat.loglike(pos), dh.identity_plan(4, lo=[-np.inf, 0.0, -np.inf, -np.inf])

    def stretch(cat, plan, pos, lnp, step0):
        p, l = pos.copy(), lnp.copy()
        chain = np.empty((6,) + pos.shape)
        cat.stretch_move_seeded(plan, p, l, 11, step0, 6, chain)
        return p, l, chain

    cat, pos, lnp, plan = fresh()
    alone1 = stretch(cat, plan, pos, lnp, 0)
    alone2 = stretch(cat, plan, alone1[0], alone1[1], 6)
    alone_info = cat.stretch_info()
    cat.close()
    cat, pos, lnp, plan = fresh()
    first = stretch(cat, plan, pos, lnp, 0)
    de = run_seeded(cat, plan, pos, lnp, 0.8, 1e-5, SEED, 0, 5, device=1)
    second = stretch(cat, plan, first[0], first[1], 6)
    assert dh.same(first, alone1) and dh.same(second, alone2)
    assert cat.stretch_info() == alone_info and cat.de_info()["device_blocks"] == 1
    assert not np.array_equal(de[2][-1], second[2][4])
    cat.close()


# ---- end to end -------------------------------------------------------------------------------------------------------
def _cluster(n, seed=3):
    from mcmc_dynamics_amd import DataReader, synthetic
    from mcmc_dynamics_amd.analysis import ConstantFit
    cat = synthetic.make_catalog(n, config=2, seed=seed)
    reader = DataReader({k: cat[k] for k in ("ra", "dec", "v", "verr")})
    cf = ConstantFit(reader, seed=13)
    cf.parameters["ra_center"].set(value=synthetic.CENTER_RA_DEG, fixed=True)
    cf.parameters["dec_center"].set(value=synthetic.CENTER_DEC_DEG, fixed=True)
    names = list(cf.fitted_parameters)
    start = synthetic.make_walkers(32, names, cat["truth"], config=2)
    return cf, start


def test_constant_fit_with_the_de_move(native):
    """400 stars, 32 walkers, 1 500 steps: the two moves sample one posterior, and DE decorrelates faster."""
    cf, start = _cluster(400)
    cf.SAMPLER = "builtin"
    np.random.seed(12)
    s_de = cf(n_walkers=32, n_steps=1500, pos=start, move="de", prefix=None)
    info = cf._catalog.de_info()
    assert s_de.move == "de" and info["device_blocks"] >= 1 and info["host_blocks"] == info["discarded_blocks"], info
    s_st = cf(n_walkers=32, n_steps=1500, pos=start, prefix=None)
    assert s_st.move == "stretch"
    burn = 300
    stats = {}
    for name, s in (("de", s_de), ("stretch", s_st)):
        chain = s.get_chain()[burn:]                                    # (steps, W, P)
        per_walker = chain.mean(axis=0)                                 # batch means over walkers
        tau = np.array([dh.autocorr_time(chain[:, :, c]) for c in range(chain.shape[2])])
        stats[name] = (per_walker.mean(axis=0), per_walker.std(axis=0, ddof=1) / np.sqrt(per_walker.shape[0]), tau,
                       float(s.acceptance_fraction.mean()))
        print(name, "mean", stats[name][0], "se", stats[name][1], "tau", tau, "acceptance", stats[name][3])
    se = np.sqrt(stats["de"][1] ** 2 + stats["stretch"][1] ** 2)
    assert np.all(np.abs(stats["de"][0] - stats["stretch"][0]) < 5.0 * se)
    assert 0.1 <= stats["de"][3] <= 0.6
    assert stats["de"][2].max() < stats["stretch"][2].max()
    cf.close()


def test_binned_constant_fit_with_the_de_move(native):
    """3 bins x 16 walkers x 50 steps: resident, and equal to the NumPy loop of the same sampler."""
    from mcmc_dynamics_amd.analysis.binned import BinnedSampler
    bf = _bins(native)
    B, W = bf.n_bins, 16
    rng = np.random.default_rng(7700)
    pos = np.array([3.0, 9.0, 1.0, -1.0]) * (1.0 + 0.2 * rng.normal(size=(B, W, 4)))
    pos[..., 1] = np.abs(pos[..., 1]) + 0.5
    pos = np.ascontiguousarray(pos)
    s = bf(n_walkers=W, n_steps=50, pos=pos, seed=5, move="de")
    info = bf._catalog.de_info()
    assert s.move == "de" and info["device_blocks"] >= 1 and info["host_blocks"] == info["discarded_blocks"], info
    loop = BinnedSampler(B, W, 4, bf.lnprob_batch, seed=5, rng="device", move="de")
    loop.run_mcmc(pos, 50)
    assert np.array_equal(s.chain, loop.chain) and np.array_equal(s.lnprobability, loop.lnprobability)
    assert np.all(s.acceptance_fraction > 0) and np.all(np.isfinite(s.lnprobability))
    s.close()
    loop.close()
    bf.close()


def test_lock_stepped_refits_take_the_move(native):
    """simulated_fits, holdout_fit and bagged hand ``move`` to their BinnedSampler: finite chains that differ from the stretch
    chains of the same seed, acceptance in (0, 1)."""
    cf, start = _cluster(60)
    truths = np.repeat(start[:1], 3, axis=0) * np.array([[1.0], [1.02], [0.98]])
    sets = [np.arange(0, 5), np.arange(5, 12), np.arange(12, 16)]
    calls = {
        "simulated_fits": lambda **kw: cf.simulated_fits(truths, n_walkers=8, n_steps=30, n_burn=10, seed=21, **kw),
        "holdout_fit": lambda **kw: cf.holdout_fit(sets, n_walkers=8, n_steps=30, n_burn=10, seed=21,
                                                   pos=np.ascontiguousarray(np.broadcast_to(start[:8], (3, 8, start.shape[1]))) *
                                                   (1.0 + 1e-3 * np.random.default_rng(2).normal(size=(3, 8, start.shape[1]))), **kw),
        "bagged": lambda **kw: cf.bagged(n_bags=3, n_walkers=8, n_steps=30, n_burn=10, seed=21,
                                         pos=np.ascontiguousarray(np.broadcast_to(start[:8], (3, 8, start.shape[1]))) *
                                         (1.0 + 1e-3 * np.random.default_rng(2).normal(size=(3, 8, start.shape[1]))), **kw),
    }
    for name, call in calls.items():
        de, st = call(move="de")["sampler"], call()["sampler"]
        assert de.move == "de" and st.move == "stretch", name
        assert de.chain.shape == st.chain.shape == (3, 8, 30, start.shape[1]), name
        assert np.all(np.isfinite(de.chain)) and np.all(np.isfinite(de.lnprobability)), name
        assert not np.array_equal(de.chain, st.chain), name
        acc = de.acceptance_fraction
        assert np.all(acc > 0.0) and np.all(acc < 1.0), (name, acc)
    cf.close()

"""CPU: the Hamiltonian Monte Carlo algebra of csrc/mcd_hmc.h (host build through tests/emul/hmc_emul.cpp), the sampler
class and the plumbing of Runner.hmc, on analytic targets passed as callables.  No GPU, no library call that needs one."""
import warnings

import numpy as np
import pytest

import emul_helper as eh
import hmc_helper as hh
from mcmc_dynamics_amd import synthetic
from mcmc_dynamics_amd.analysis import ConstantFit
from mcmc_dynamics_amd.sampler import HMCSampler
from mcmc_dynamics_amd.utils.data_reader import DataReader

SEEDS = (1, 0x9E3779B97F4A7C15, 2 ** 64 - 1)


def gaussian(mean, cov):
    """lnL(x) = -1/2 (x - mean)^T cov^-1 (x - mean) and its gradient, for rows of a table."""
    mean, prec = np.asarray(mean, dtype=np.float64), np.linalg.inv(cov)

    def f(x):
        d = x - mean
        return -0.5 * np.einsum("wi,ij,wj->w", d, prec, d), -d @ prec
    return f


COV3 = np.array([[1.0, 0.6, -0.3], [0.6, 2.0, 0.5], [-0.3, 0.5, 0.5]])
MEAN3 = np.array([1.0, -2.0, 0.5])


# ------------------------------------------------------------------------------------------ the numbers of a step
@pytest.mark.parametrize("p", [1, 11])
@pytest.mark.parametrize("w", [1, 65])
@pytest.mark.parametrize("seed", SEEDS)
def test_numbers_against_numpy_philox(seed, w, p):
    step = 7 + (seed % 5)
    z, thr, r = hh.numbers(seed, step, 1, w, p)
    for walker in range(w):
        zz, t, rr = hh.numpy_numbers(seed, step, walker, p, eh.det_log)
        assert z[0, walker].tobytes() == zz.tobytes(), (seed, walker)
        assert thr[0, walker] == t and r[0, walker] == rr
    assert np.all((r >= -1.0) & (r < 1.0)) and np.all(thr <= 0.0)


def test_library_numbers_are_the_harness_numbers(built_library):
    """mcd_hmc_numbers (host code of the library) and the harness compile the same header."""
    from mcmc_dynamics_amd import _native
    for seed in SEEDS:
        got = _native.hmc_numbers(seed, 5, 3, 65, 11)
        want = hh.numbers(seed, 5, 3, 65, 11)
        for a, b in zip(got, want):
            assert a.tobytes() == b.tobytes()


def test_normal_moments():
    n = 200000
    z, thr, r = hh.numbers(12345, 0, n // (100 * 10), 100, 10)
    z = z.ravel()
    assert z.size == n
    # standard errors of the sample mean, variance and 4th moment of a standard normal: 1/sqrt(n), sqrt(2/n), sqrt(96/n)
    assert abs(z.mean()) < 5 / np.sqrt(n)
    assert abs((z ** 2).mean() - 1.0) < 5 * np.sqrt(2.0 / n)
    assert abs((z ** 4).mean() - 3.0) < 5 * np.sqrt(96.0 / n)
    u = np.exp(thr.ravel())
    assert abs(u.mean() - 0.5) < 5 / np.sqrt(12 * u.size) and abs(r.mean()) < 5 * 2 / np.sqrt(12 * r.size)


def test_rejected_pairs_advance_and_the_fallback_is_reached():
    # a counter whose first candidate pair is rejected (probability 1 - pi/4 each): found by search, then pinned
    seed = 99
    found = None
    for walker in range(200):
        zfull, pairs = hh.normal(seed, 0, walker, 0, 16)
        if pairs >= 3:
            found = (walker, zfull, pairs)
            break
    assert found is not None, "no walker with two rejected pairs among 200: probability (1 - 0.046)^200"
    walker, zfull, pairs = found
    # with ONE generator call (two pairs) allowed the draw gives up and returns the documented value 0.0 ...
    z1, used = hh.normal(seed, 0, walker, 0, 1)
    assert z1 == 0.0 and used == 2
    # ... with the full budget it takes the pair the NumPy restatement takes
    want, _, _ = hh.numpy_numbers(seed, 0, walker, 1, eh.det_log)
    assert zfull == want[0] and zfull != 0.0
    z0, used0 = hh.normal(seed, 0, walker, 0, 0)
    assert z0 == 0.0 and used0 == 0


def test_stream_differs_from_the_stretch_moves():
    order, zz, thr, pick = eh.chain_numbers(5, 0, 1, 1, 64, 3)
    z, t, r = hh.numbers(5, 0, 1, 64, 3)
    assert not np.intersect1d(thr.ravel(), t.ravel()).size


# ------------------------------------------------------------------------------------------ momentum, leapfrog
def test_momentum_and_kinetic_energy():
    chol = np.linalg.cholesky(COV3)
    z = np.array([0.3, -1.2, 2.0])
    p = hh.momentum(chol, z)
    assert np.allclose(chol.T @ p, z, rtol=1e-14, atol=0)
    assert np.isclose(hh.kinetic(chol, p), 0.5 * z @ z, rtol=1e-14)
    # p ~ N(0, M) with M^-1 = L L^T: kinetic energy 1/2 p^T M^-1 p
    assert np.isclose(hh.kinetic(chol, p), 0.5 * p @ COV3 @ p, rtol=1e-13)


@pytest.mark.parametrize("dense", [False, True])
def test_leapfrog_is_reversible(dense):
    f = gaussian(MEAN3, COV3)
    chol = np.linalg.cholesky(COV3) if dense else np.diag(np.sqrt(np.diag(COV3)))
    lo, hi = np.full(3, -np.inf), np.full(3, np.inf)
    q0, p0 = np.array([0.2, -1.0, 1.5]), np.array([1.0, -0.5, 2.0])
    for n_leap in (1, 8):
        alive, q1, p1 = hh.leapfrog(chol, lo, hi, 0.3, n_leap, q0, p0, f)
        assert alive == 1 and not np.allclose(q1, q0)
        alive, q2, p2 = hh.leapfrog(chol, lo, hi, 0.3, n_leap, q1, -p1, f)
        assert alive == 1
        assert np.max(np.abs(q2 - q0) / np.abs(q0)) <= 1e-12
        assert np.max(np.abs(-p2 - p0) / np.abs(p0)) <= 1e-12


def test_energy_error_is_second_order_in_the_step_size():
    """Halving eps at a fixed trajectory length (n_leap doubled) divides |dH| by 4 up to O(eps^2): the leapfrog's order."""
    f = gaussian(MEAN3, COV3)
    chol = np.diag([1.0, 1.0, 1.0])
    rng = np.random.default_rng(2)
    pos = MEAN3 + rng.normal(size=(256, 3)) @ np.linalg.cholesky(COV3).T
    plan = hh.identity_plan(3)
    a = hh.block(plan, chol, 0.1, 4, pos, 11, 0, 1, f, jitter=0.0)
    b = hh.block(plan, chol, 0.05, 8, pos, 11, 0, 1, f, jitter=0.0)
    assert a["status"] == hh.HMC_OK and b["status"] == hh.HMC_OK
    ea, eb = np.median(a["energy_error"][0]), np.median(b["energy_error"][0])
    assert np.isfinite(ea) and eb > 0
    assert 3.0 <= ea / eb <= 5.0, (ea, eb)


# ------------------------------------------------------------------------------------------ the box prior
def flat(x):
    return np.zeros(x.shape[0]), np.zeros_like(x)


def test_diagonal_metric_reflects_at_a_bound():
    chol = np.diag([1.0, 2.0])
    lo, hi = np.array([0.0, -5.0]), np.array([1.0, 5.0])
    q, p = np.array([0.9, 0.0]), np.array([1.0, 0.25])
    alive, q1, p1 = hh.leapfrog(chol, lo, hi, 0.3, 1, q, p, flat)
    # free flight: q0 -> 0.9 + 0.3 = 1.2, mirrored at 1 to 0.8, p0 negated; coordinate 1 moves by eps M^-1 p = 0.3 * 4 * 0.25
    assert alive == 1
    assert np.isclose(q1[0], 0.8, rtol=0, atol=1e-15) and p1[0] == -1.0
    assert np.isclose(q1[1], 0.3, rtol=0, atol=1e-15) and p1[1] == 0.25
    # a flight of more than one box width is mirrored at both walls
    alive, q2, p2 = hh.leapfrog(chol, lo, hi, 1.4, 1, q, p, flat)
    assert alive == 1 and np.isclose(q2[0], 0.3, rtol=0, atol=1e-14) and p2[0] == 1.0       # 2.3 -> -0.3 -> 0.3
    # the bounds are inclusive: a walker that lands exactly on one is inside
    alive, q3, p3 = hh.leapfrog(chol, lo, hi, 0.1, 1, q, p, flat)
    assert alive == 1 and q3[0] == 1.0 and p3[0] == 1.0


def test_dense_metric_ends_the_trajectory_at_a_bound():
    chol = np.array([[1.0, 0.0], [0.5, 2.0]])
    lo, hi = np.array([0.0, -5.0]), np.array([1.0, 5.0])
    alive, _, _ = hh.leapfrog(chol, lo, hi, 0.3, 1, np.array([0.9, 0.0]), np.array([1.0, 0.25]), flat)
    assert alive == 0
    alive, _, _ = hh.leapfrog(chol, lo, hi, 0.01, 1, np.array([0.9, 0.0]), np.array([1.0, 0.25]), flat)
    assert alive == 1


@pytest.mark.parametrize("dense", [False, True])
def test_block_at_a_bound(dense):
    """Walkers aimed at a wall: with a diagonal metric every chain row is inside the box and moves are accepted; with a
    dense one the trajectories that leave are rejected (the walker stays), the others move."""
    cov = np.array([[1.0, 0.5], [0.5, 1.0]])
    f = gaussian([0.0, 0.0], cov)
    chol = np.linalg.cholesky(cov) if dense else np.eye(2)
    plan = hh.identity_plan(2, lo=[-0.2, -3.0], hi=[0.2, 3.0])
    pos = np.tile([0.19, 0.0], (64, 1))
    out = hh.block(plan, chol, 0.5, 4, pos, 4, 0, 5, f)
    assert out["status"] == hh.HMC_OK
    c = out["chain"]
    assert np.all(c[..., 0] >= -0.2) and np.all(c[..., 0] <= 0.2) and np.all(np.abs(c[..., 1]) <= 3.0)
    ended = np.isinf(out["energy_error"])
    if dense:
        assert ended.any() and not ended.all()
        stayed = np.all(c[0] == pos, axis=1)
        assert np.all(stayed[ended[0]])
    else:
        assert not ended.any()
        assert out["accepted"].sum() > 0.8 * 64 * 5


def test_fixed_parameter_outside_its_bounds_rejects_everything():
    f = gaussian(MEAN3, COV3)
    pos = MEAN3 + np.random.default_rng(0).normal(size=(8, 3))
    out = hh.block(hh.identity_plan(3, fixed_ok=False), np.eye(3), 0.2, 3, pos, 1, 0, 4, f)
    assert out["status"] == hh.HMC_OK
    assert out["accepted"].sum() == 0 and np.all(out["chain"] == pos[None]) and np.array_equal(out["pos"], pos)
    assert np.all(np.isinf(out["energy_error"]))


def test_nan_gradient_mid_trajectory_rejects_and_nan_at_the_start_is_an_error():
    good = gaussian(MEAN3, COV3)
    calls = {"n": 0}

    def poisoned(x):
        calls["n"] += 1
        v, g = good(x)
        if calls["n"] == 3:                      # start point, leapfrog point 1, then point 2 of the first step
            g[::2, 1] = np.nan
        return v, g
    pos = MEAN3 + np.random.default_rng(0).normal(size=(8, 3))
    out = hh.block(hh.identity_plan(3), np.eye(3), 0.2, 3, pos, 1, 0, 1, poisoned)
    assert out["status"] == hh.HMC_OK and calls["n"] == 4
    assert np.all(out["accepted"][::2] == 0) and np.all(out["chain"][0, ::2] == pos[::2])
    assert np.all(np.isinf(out["energy_error"][0, ::2])) and np.all(np.isfinite(out["energy_error"][0, 1::2]))
    assert out["accepted"][1::2].sum() > 0

    def nan_value(x):
        v, g = good(x)
        v[-1] = np.nan
        return v, g
    bad = hh.block(hh.identity_plan(3), np.eye(3), 0.2, 3, pos, 1, 0, 1, nan_value)
    assert bad["status"] == hh.HMC_NONFINITE and np.array_equal(bad["pos"], pos) and np.all(np.isnan(bad["lnp"]))
    outside = hh.block(hh.identity_plan(3, lo=[-9, -9, 5.0], hi=[9, 9, 9.0]), np.eye(3), 0.2, 3, pos, 1, 0, 1, good)
    assert outside["status"] == hh.HMC_NONFINITE


def test_bad_arguments():
    f = gaussian(MEAN3, COV3)
    pos = np.tile(MEAN3, (2, 1))
    upper = np.eye(3)
    upper[0, 2] = 0.1
    for chol, eps, jit, leap in ((upper, 0.1, 0.1, 1), (np.eye(3), 0.0, 0.1, 1), (np.eye(3), 0.1, 1.0, 1),
                                 (np.eye(3), 0.1, 0.1, 0), (np.diag([1.0, 0.0, 1.0]), 0.1, 0.1, 1)):
        assert hh.block(hh.identity_plan(3), chol, eps, leap, pos, 1, 0, 1, f, jitter=jit)["status"] == hh.HMC_BAD_ARGS


# ------------------------------------------------------------------------------------------ the chain
def test_chain_rule_and_column_map():
    """Five kernel columns: one constant, one free parameter feeding TWO columns (one through a unit factor)."""
    plan = {"col_source": np.array([0, -1, 1, 1, 0], dtype=np.int32), "col_const": np.array([0.0, 7.0, 0.0, 0.0, 0.0]),
            "col_factor": np.array([1.0, 1.0, 2.0, 1.0, 3.0]), "lo": np.full(2, -np.inf), "hi": np.full(2, np.inf),
            "fixed_ok": True}
    seen = []

    def f(t):
        seen.append(t.copy())
        # lnL = -1/2 sum_j c_j t_j^2 over the columns: d/dx0 = -(c0 t0 + 3 c4 t4), d/dx1 = -(2 c2 t2 + c3 t3)
        c = np.array([1.0, 5.0, 0.5, 0.25, 0.1])
        return -0.5 * (c * t * t).sum(axis=1), -c * t
    pos = np.array([[0.5, -0.25], [1.0, 2.0]])
    out = hh.block(plan, np.eye(2), 0.05, 2, pos, 3, 0, 3, f, jitter=0.0)
    assert out["status"] == hh.HMC_OK
    assert np.array_equal(seen[0], np.stack([pos[:, 0], np.full(2, 7.0), 2 * pos[:, 1], pos[:, 1], 3 * pos[:, 0]], axis=1))
    # in free parameters the target is Gaussian with precision diag(1 + 0.9, 2 + 0.25): energy is conserved to O(eps^2)
    assert np.all(out["energy_error"] < 1e-2) and out["accepted"].sum() == 6


def test_stationary_distribution_of_a_correlated_gaussian():
    f = gaussian(MEAN3, COV3)
    rng = np.random.default_rng(8)
    chol_true = np.linalg.cholesky(COV3)
    pos = MEAN3 + rng.normal(size=(64, 3)) @ chol_true.T
    out = hh.block(hh.identity_plan(3), chol_true, 0.9, 4, pos, 2024, 0, 400, f)
    assert out["status"] == hh.HMC_OK
    assert 0.6 < out["accepted"].mean() / 400 <= 1.0
    c = out["chain"]                                              # (steps, W, P); the walkers are independent chains
    d = c - MEAN3
    # batch means over walkers: each walker's time average is one independent estimate
    for stat, truth in ((d, np.zeros(3)), (d[..., :, None] * d[..., None, :], COV3)):
        per_walker = stat.mean(axis=0)
        est, se = per_walker.mean(axis=0), per_walker.std(axis=0, ddof=1) / np.sqrt(64)
        assert np.all(np.abs(est - truth) < 5 * se), (est, truth, se)
    assert np.all(out["lnprob_chain"][-1] == out["lnp"]) and np.array_equal(c[-1], out["pos"])
    assert np.allclose(out["lnp"], f(out["pos"])[0], rtol=1e-13)


def test_blocks_continue_each_other():
    f = gaussian(MEAN3, COV3)
    pos = MEAN3 + np.random.default_rng(1).normal(size=(5, 3))
    chol = np.linalg.cholesky(COV3)
    whole = hh.block(hh.identity_plan(3), chol, 0.7, 3, pos, 77, 10, 6, f)
    first = hh.block(hh.identity_plan(3), chol, 0.7, 3, pos, 77, 10, 3, f)
    second = hh.block(hh.identity_plan(3), chol, 0.7, 3, first["pos"], 77, 13, 3, f)
    for key in ("chain", "lnprob_chain", "energy_error"):
        assert np.concatenate([first[key], second[key]]).tobytes() == whole[key].tobytes(), key
    assert np.array_equal(first["accepted"] + second["accepted"], whole["accepted"])
    assert second["pos"].tobytes() == whole["pos"].tobytes() and second["lnp"].tobytes() == whole["lnp"].tobytes()
    other = hh.block(hh.identity_plan(3), chol, 0.7, 3, pos, 77, 0, 6, f)
    assert other["chain"].tobytes() != whole["chain"].tobytes()


# ------------------------------------------------------------------------------------------ HMCSampler, Runner.hmc
def emul_block_fn(f, plan, record=None):
    """A block_fn for HMCSampler on the host build: what Runner._hmc_block does through the library."""
    def block_fn(pos, lnp, chol, step_size, n_leap, jitter, seed, step0, n_steps, chain, lnprob_chain, accepted, energy):
        if record is not None:
            record.append({"seed": seed, "step0": step0, "n_steps": n_steps, "step_size": step_size})
        out = hh.block(plan, chol, step_size, n_leap, pos, seed, step0, n_steps, f, jitter=jitter)
        assert out["status"] == hh.HMC_OK
        pos[:], lnp[:], chain[:], lnprob_chain[:], energy[:] = out["pos"], out["lnp"], out["chain"], out["lnprob_chain"], \
            out["energy_error"]
        accepted += out["accepted"]
    return block_fn


def test_sampler_attributes_and_reset_keeps_the_generator_moving():
    f = gaussian(MEAN3, COV3)
    calls = []
    s = HMCSampler(6, 3, emul_block_fn(f, hh.identity_plan(3), calls), np.linalg.cholesky(COV3), 0.8, n_leap=3, seed=5)
    s.block_steps = 4
    pos0 = MEAN3 + np.random.default_rng(3).normal(size=(6, 3))
    s.reserve(10)
    pos, lnp, _ = s.run_mcmc(pos0, 10)
    assert [c["step0"] for c in calls] == [0, 4, 8] and [c["n_steps"] for c in calls] == [4, 4, 2]
    assert s.chain.shape == (6, 10, 3) and s.lnprobability.shape == (6, 10) and s.energy_error.shape == (6, 10)
    assert s.acceptance_fraction.shape == (6,) and np.all(s.acceptance_fraction <= 1.0) and s.iteration == 10
    assert np.array_equal(s.chain[:, -1], pos) and np.array_equal(s.lnprobability[:, -1], lnp)
    one = HMCSampler(6, 3, emul_block_fn(f, hh.identity_plan(3)), np.linalg.cholesky(COV3), 0.8, n_leap=3, seed=5)
    one.block_steps = 64
    one.run_mcmc(pos0, 10)
    assert one.chain.tobytes() == s.chain.tobytes()               # the chain does not depend on how it is cut into blocks
    first_steps = s.chain[:, :2].copy()
    s.reset()
    assert s.iteration == 0 and s.chain.shape == (6, 0, 3) and s.rng_step == 10
    del calls[:]
    s.run_mcmc(pos0, 2)
    assert calls[0]["step0"] == 10                                 # NOT rewound: the numbers of step 0 are not replayed
    assert hh.numbers(s.seed64, 10, 1, 6, 3)[0].tobytes() != hh.numbers(s.seed64, 0, 1, 6, 3)[0].tobytes()
    assert s.chain.tobytes() != first_steps.tobytes()
    with pytest.raises(ValueError):
        HMCSampler(6, 3, None, np.triu(np.ones((3, 3))), 0.8)
    with pytest.raises(ValueError):
        s.run_mcmc(pos0[:3], 1)


def small_fit(**kwargs):
    c = synthetic.make_catalog(300, config=2)
    fit = ConstantFit(DataReader({k: c[k] for k in c if k != "truth"}), **kwargs)
    fit.parameters["ra_center"].set(value=c["truth"]["ra_center"], fixed=True)
    fit.parameters["dec_center"].set(value=c["truth"]["dec_center"], fixed=True)
    return fit


@pytest.mark.parametrize("start, direction", [(8.0, -1), (0.01, +1)])
def test_runner_hmc_adapts_the_step_size_then_freezes_it(start, direction):
    """A fake posterior (a 4-D Gaussian in the free parameters) behind Runner.hmc: the warm-up moves eps down from a
    value that rejects nearly everything and up from one that accepts everything, and the production run uses one eps."""
    fit = small_fit()
    n_p = fit.n_fitted_parameters
    assert n_p == 4
    mean, cov = np.array([0.0, 10.0, 3.0, 4.0]), np.diag([0.25, 0.16, 0.5, 0.5])
    f = gaussian(mean, cov)
    calls = []
    fit._hmc_block = emul_block_fn(f, fit._stretch_plan(), calls)
    fit.maximize = fit.laplace = lambda *a, **k: pytest.fail("pos and covariance were given")
    pos = mean + np.random.default_rng(0).normal(size=(32, 4)) @ np.linalg.cholesky(cov).T
    s = fit.hmc(n_walkers=32, n_steps=30, pos=pos, covariance=cov, step_size=start, n_leap=4, n_warmup=40, seed=9)
    path = np.array(s.warmup_step_sizes)
    assert path[0] == start and len(path) == 5                      # four warm-up blocks of 10 steps
    assert direction * (path[1] - path[0]) > 0 and direction * (path[-1] - path[0]) > 0
    warm, prod = calls[:4], calls[4:]
    assert [c["step_size"] for c in warm] == list(path[:4])
    assert prod and all(c["step_size"] == path[-1] for c in prod) and s.step_size == path[-1]
    assert prod[0]["step0"] == 40 and s.rng_step == 70              # the production run continues the generator
    assert s.chain.shape == (32, 30, 4) and s.iteration == 30
    assert [c["seed"] for c in calls] == [9] * len(calls)


def test_runner_hmc_supplies_start_and_metric_and_falls_back_to_a_diagonal_one():
    fit = small_fit()
    mean, cov = np.array([0.0, 10.0, 3.0, 4.0]), np.diag([0.25, 0.16, 0.5, 0.5])
    cov[0, 1] = cov[1, 0] = 0.1
    f = gaussian(mean, cov)
    seen = {}

    def block_fn(pos, lnp, chol, *rest):
        seen["chol"] = chol.copy()
        return emul_block_fn(f, fit._stretch_plan())(pos, lnp, chol, *rest)
    fit._hmc_block = block_fn
    fit.maximize = lambda *a, **k: {"x": mean.copy()}
    fit.laplace = lambda x, **k: {"covariance": cov}
    s = fit.hmc(n_walkers=16, n_steps=4, n_warmup=0, seed=1)
    assert np.allclose(seen["chol"], np.linalg.cholesky(cov)) and s.chain.shape == (16, 4, 4)

    def at_a_bound(x, **k):
        raise ValueError("laplace: x sits on a bound of the prior")
    fit.laplace = at_a_bound
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        fit.hmc(n_walkers=16, n_steps=2, n_warmup=0, seed=1, pos=np.tile(mean, (16, 1)))
    assert any("diagonal metric" in str(w.message) for w in caught)
    assert np.count_nonzero(seen["chol"] - np.diag(np.diag(seen["chol"]))) == 0


def test_runner_hmc_refusals():
    fit = small_fit()
    fit._hmc_block = lambda *a: pytest.fail("must not run")
    fit.parameters["v_maxy"].set(expr="v_maxx")
    with pytest.raises(NotImplementedError):
        fit.hmc(n_walkers=8, n_steps=2)
    fit = small_fit()
    fit.parameters["v_maxy"].set(lnprior="-0.5 * v_maxy ** 2")
    with pytest.raises(NotImplementedError):
        fit.hmc(n_walkers=8, n_steps=2)
    fit32 = small_fit(precision="f32")
    with pytest.raises(NotImplementedError):
        fit32.hmc(n_walkers=8, n_steps=2, pos=np.zeros((8, 4)), covariance=np.eye(4))
    fit = small_fit()
    with pytest.raises(ValueError):                                  # a start outside the box (sigma_max >= 0)
        fit.hmc(n_walkers=8, n_steps=2, pos=np.tile([0.0, -1.0, 1.0, 1.0], (8, 1)), covariance=np.eye(4))

"""CPU: the parallel-tempering algebra of csrc/mcd_temper.h in its host build (tests/temper_helper.py) -- the swap
numbers, a ladder of one rung against the seeded stretch move, the swap phase on hand-set states, every rung's stationary
distribution, the evidence against closed forms, crossing between modes -- and the Python layer on top of it
(sampler.TemperedSampler, analysis.runner.evidence_summary / bayes_factor, Runner.tempered's ladder and refusals)."""
import math
import warnings

import numpy as np
import pytest

import emul_helper as eh
import hmc_helper as hh
import temper_helper as th
from mcmc_dynamics_amd import synthetic
from mcmc_dynamics_amd.analysis import ConstantFit
from mcmc_dynamics_amd.analysis.runner import bayes_factor, evidence_summary
from mcmc_dynamics_amd.sampler import TemperedSampler, default_ladder
from mcmc_dynamics_amd.utils.data_reader import DataReader

SEEDS = (1, 0x9E3779B97F4A7C15, 2 ** 64 - 1)              # the seeds of test_hmc_cpu.py


def gaussian(mean, sd):
    mean, sd = np.asarray(mean, dtype=np.float64), np.asarray(sd, dtype=np.float64)

    def f(table):
        t = (table - mean) / sd
        return -0.5 * np.sum(t * t, axis=1)
    return f


# ------------------------------------------------------------------------------------------ the swap numbers
@pytest.mark.parametrize("seed", SEEDS)
def test_swap_numbers_against_numpy_philox(seed):
    step = 7 + (seed % 5)
    thr = th.numbers(seed, step, 2, 4, 5)
    assert thr.shape == (2, 3, 5)
    for i in range(2):
        for t in range(3):
            for w in range(5):
                assert thr[i, t, w] == th.numpy_swap_thr(seed, step + i, t, w, eh.det_log), (seed, i, t, w)


def test_library_numbers_are_the_harness_numbers(built_library):
    from mcmc_dynamics_amd import _native
    for seed in SEEDS:
        got = _native.temper_numbers(seed, 5, 3, 6, 66)
        assert got.shape == (3, 5, 66) and got.tobytes() == th.numbers(seed, 5, 3, 6, 66).tobytes()
    assert _native.temper_numbers(1, 0, 3, 1, 4).shape == (3, 0, 4)


def test_stream_differs_from_the_stretch_moves_and_hmcs():
    assert th.key() not in (int(hh.lib().emul_hmc_key()), 0x6d63645f636861)
    for seed in SEEDS:
        swap = set(th.numbers(seed, 3, 2, 9, 64).ravel().tolist())
        order, zz, thr, pick = eh.chain_numbers(seed, 3, 2, 9, 64, 4)
        z, hthr, r = hh.numbers(seed, 3, 2, 64, 4)
        assert len(swap) == 2 * 8 * 64
        for other in (zz, thr, hthr, r, z):
            assert not swap & set(np.asarray(other).ravel().tolist())


# ------------------------------------------------------------------------------------------ T = 1 is the stretch move
@pytest.mark.parametrize("p", [1, 4])
@pytest.mark.parametrize("w", [2, 66])
def test_one_rung_is_the_seeded_stretch_move(w, p):
    """betas = [1], no structured prior: thr < 1.0 * (a - b) is thr < a - b exactly, so the new loop reproduces
    stretch_block fed chain_numbers_of_step -- chain, lnprob rows and accept counts, bit for bit."""
    mean, sd = np.linspace(0.5, 2.0, p), np.linspace(1.0, 3.0, p)
    f = gaussian(mean, sd)
    lo, hi = mean - 1.5 * sd, mean + 4.0 * sd                     # some proposals leave the box
    plan = th.identity_plan(p, lo, hi)
    pos = mean + sd * np.random.default_rng(w * 10 + p).uniform(-1.0, 1.0, size=(w, p))
    lnp = f(pos)
    a = th.block(plan, [1.0], pos[None], lnp[None], 77, 3, 40, f)
    b = th.stretch_seeded(plan, pos, lnp, 77, 3, 40, f)
    assert a["status"] == th.TEMPER_OK and b["status"] == 0
    assert a["chain"][:, 0].tobytes() == b["chain"].tobytes()
    assert a["lnlike_chain"][:, 0].tobytes() == b["lnprob_chain"].tobytes()
    assert np.array_equal(a["accepted"][0], b["accepted"]) and b["accepted"].sum() > 0
    assert a["pos"][0].tobytes() == b["pos"].tobytes() and a["lnlike"][0].tobytes() == b["lnp"].tobytes()
    assert np.all(a["lnprior"] == 0.0) and a["swap_proposed"].size == 0
    assert np.all(a["chain"] >= lo) and np.all(a["chain"] <= hi)


# ------------------------------------------------------------------------------------------ the swap phase
def frozen(table):
    """Every proposal has zero likelihood: the stretch move rejects everything and only the swaps move walkers."""
    return np.full(table.shape[0], -np.inf)


def hand_set(T=5, W=6, P=2, seed=4):
    rng = np.random.default_rng(seed)
    pos = rng.normal(size=(T, W, P))
    ll = rng.normal(scale=3.0, size=(T, W))
    return pos, ll


BETAS5 = np.array([1.0, 0.5, 0.2, 0.05, 0.0])


@pytest.mark.parametrize("step0", [0, 1, 6, 7])
def test_swap_decisions_parity_and_counters(step0):
    pos, ll = hand_set()
    T, W, P = pos.shape
    prior = (np.array([1, 0], dtype=np.int32), np.array([0.0, 0.0]), np.array([2.0, 1.0]))
    plan = th.identity_plan(P, prior=prior)
    out = th.block(plan, BETAS5, pos, ll, 11, step0, 1, frozen, n_chain_temps=T)
    assert out["status"] == th.TEMPER_OK and out["accepted"].sum() == 0
    thr = th.numbers(11, step0, 1, T, W)[0]
    lp0 = -0.5 * (pos[:, :, 0] / 2.0) ** 2 - math.log(2.0) - 0.5 * math.log(2.0 * math.pi)
    want_pos, want_ll, want_lp = pos.copy(), ll.copy(), lp0.copy()
    proposed, accepted = np.zeros(T - 1, dtype=np.int64), np.zeros(T - 1, dtype=np.int64)
    for t in range(T - 1):
        if t % 2 != step0 % 2:
            continue
        proposed[t] = W
        for w in range(W):
            if thr[t, w] < (BETAS5[t] - BETAS5[t + 1]) * (ll[t + 1, w] - ll[t, w]):        # the stated inequality
                accepted[t] += 1
                for a in (want_pos, want_ll, want_lp):
                    a[[t, t + 1], w] = a[[t + 1, t], w]
    assert 0 < accepted.sum() < proposed.sum()
    assert np.array_equal(out["swap_proposed"], proposed) and np.array_equal(out["swap_accepted"], accepted)
    assert out["pos"].tobytes() == want_pos.tobytes() and out["lnlike"].tobytes() == want_ll.tobytes()
    assert np.allclose(out["lnprior"], want_lp, rtol=1e-14, atol=0)              # position, ll and lp travel together
    assert out["chain"][0].tobytes() == want_pos.tobytes() and out["lnlike_chain"][0].tobytes() == want_ll.tobytes()
    untouched = [t for t in range(T) if not (t % 2 == step0 % 2 and t + 1 < T) and not (t >= 1 and (t - 1) % 2 == step0 % 2)]
    for t in untouched:
        assert np.array_equal(out["pos"][t], pos[t])


def test_counters_add_up_over_blocks_and_follow_the_absolute_step():
    pos, ll = hand_set()
    whole = th.block(th.identity_plan(2), BETAS5, pos, ll, 5, 3, 5, frozen)
    a = th.block(th.identity_plan(2), BETAS5, pos, ll, 5, 3, 2, frozen)
    b = th.block(th.identity_plan(2), BETAS5, a["pos"], a["lnlike"], 5, 5, 3, frozen)
    assert np.array_equal(whole["swap_proposed"], [12, 18, 12, 18])            # steps 3 .. 7: odd pairs 3 times, even ones twice
    assert np.array_equal(a["swap_proposed"] + b["swap_proposed"], whole["swap_proposed"])
    assert np.array_equal(a["swap_accepted"] + b["swap_accepted"], whole["swap_accepted"])
    assert b["pos"].tobytes() == whole["pos"].tobytes() and b["lnlike"].tobytes() == whole["lnlike"].tobytes()


def test_outside_the_box_and_zero_likelihood_are_rejected_at_beta_zero_too():
    """At beta = 0 the acceptance threshold ignores the likelihood -- but not the prior, and not a point of zero
    likelihood: 0 * (-inf) must not become an accept."""
    rng = np.random.default_rng(2)
    pos = rng.uniform(-1.0, 1.0, size=(2, 32, 1))
    ll = np.zeros((2, 32))
    box = th.identity_plan(1, [-1.0], [1.0])
    out = th.block(box, [1.0, 0.0], pos, ll, 9, 0, 30, lambda t: np.zeros(t.shape[0]), n_chain_temps=2)
    assert out["status"] == th.TEMPER_OK and out["accepted"][1].sum() > 0
    assert np.all(np.abs(out["chain"]) <= 1.0)
    assert out["accepted"][1].sum() < 30 * 32                                    # proposals beyond the box were refused
    out = th.block(th.identity_plan(1), [1.0, 0.0], pos, ll, 9, 0, 10, frozen)
    assert out["status"] == th.TEMPER_OK and out["accepted"].sum() == 0


def test_nan_is_an_error_and_a_fixed_parameter_outside_its_bounds_moves_nothing():
    pos, ll = hand_set()
    plan = th.identity_plan(2)
    out = th.block(plan, BETAS5, pos, ll, 1, 0, 2, lambda t: np.full(t.shape[0], np.nan))
    assert out["status"] == th.TEMPER_NAN
    out = th.block(dict(plan, fixed_ok=False), BETAS5, pos, ll, 1, 0, 4, gaussian([0, 0], [1, 1]), n_chain_temps=5)
    assert out["status"] == th.TEMPER_OK and out["accepted"].sum() == 0 and out["swap_accepted"].sum() == 0
    assert np.all(out["chain"] == pos[None]) and out["swap_proposed"].sum() > 0
    bad = pos.copy()
    bad[3, 2, 0] = 9.0
    assert th.block(th.identity_plan(2, [-8, -8], [8, 8]), BETAS5, bad, ll, 1, 0, 1, frozen)["status"] == th.TEMPER_OUTSIDE


def test_bad_arguments():
    pos, ll = hand_set()
    plan = th.identity_plan(2)
    for betas in ([0.9, 0.5, 0.2, 0.1, 0.0], [1.0, 0.5, 0.5, 0.1, 0.0], [1.0, 0.5, 0.2, 0.1, -0.1], [1.0, 1.5, 0.2, 0.1, 0.0],
                  [1.0, 0.5, np.nan, 0.1, 0.0]):
        assert th.block(plan, betas, pos, ll, 1, 0, 1, frozen)["status"] == th.TEMPER_BAD_ARGS, betas
    assert th.block(plan, BETAS5, pos[:, :5], ll[:, :5], 1, 0, 1, frozen)["status"] == th.TEMPER_BAD_ARGS      # odd W
    assert th.block(plan, BETAS5, pos, ll, 1, 0, 1, frozen, n_chain_temps=6)["status"] == th.TEMPER_BAD_ARGS
    assert th.block(th.identity_plan(13), [1.0], np.zeros((1, 4, 13)), np.zeros((1, 4)), 1, 0, 1, frozen)["status"] == \
        th.TEMPER_BAD_ARGS


# ------------------------------------------------------------------------------------------ stationary distributions
MEAN2, SD2 = np.array([0.0, 1.0]), np.array([1.0, 2.0])
LO2, HI2 = np.array([-0.5, -9.0]), np.array([6.0, 11.0])          # truncates the first coordinate half a sigma below its mean
LADDER = np.array([1.0, 0.5, 0.25, 0.125, 1.0 / 16, 1.0 / 32, 1.0 / 64, 0.0])

_RUNS = {}


def tempered_run(name):
    """One run per target for the whole module (fixed seeds: deterministic)."""
    if name in _RUNS:
        return _RUNS[name]
    if name == "box":
        f, plan, n_dim = gaussian(MEAN2, SD2), th.identity_plan(2, LO2, HI2), 2
        start = np.random.default_rng(1).uniform([0.0, 0.0], [1.0, 2.0], size=(32, 2))
        betas, steps, seed = LADDER, 6000, 21
    else:                                                         # a conjugate pair: N(1.5, 0.5) likelihood, N(0, 2) prior
        f = gaussian([1.5], [0.5])
        prior = (np.array([1], dtype=np.int32), np.array([0.0]), np.array([2.0]))
        plan, n_dim = th.identity_plan(1, [-60.0], [60.0], prior=prior), 1
        start = np.random.default_rng(2).normal(1.0, 0.5, size=(32, 1))
        betas, steps, seed = LADDER, 6000, 22
    s = TemperedSampler(32, n_dim, betas, th.emul_block_fn(f, plan), f, seed=seed, store_temps=len(betas))
    s.run_mcmc(start, steps)
    _RUNS[name] = s
    return s


DISCARD = 500


def test_every_rung_samples_its_own_target():
    s = tempered_run("box")
    assert s.swap_acceptance_fraction.min() > 0.2 and s.acceptance_fraction.min() > 0.1
    worst = 0.0
    for t, beta in enumerate(s.betas):
        x = np.swapaxes(s.get_chain(temp=t, discard=DISCARD), 0, 1)                  # (W, steps, P)
        for c in range(2):
            m, v, _, _ = th.truncated_gaussian(MEAN2[c], SD2[c], LO2[c], HI2[c], beta)
            got_m, se_m = th.walker_means(x[:, :, c])
            got_v, se_v = th.walker_means((x[:, :, c] - m) ** 2)
            worst = max(worst, abs(got_m - m) / se_m, abs(got_v - v) / se_v)
            assert abs(got_m - m) < 5.0 * se_m, (beta, c, got_m, m, se_m)
            assert abs(got_v - v) < 5.0 * se_v, (beta, c, got_v, v, se_v)
    print("largest |z| over rungs, coordinates, mean and variance:", worst)


# ------------------------------------------------------------------------------------------ the evidence
def closed_form(name, betas):
    """(log Z, the trapezoid of the closed-form E_beta[lnL] over the ladder)"""
    if name == "box":
        parts = [th.truncated_gaussian(MEAN2[c], SD2[c], LO2[c], HI2[c], 1.0) for c in range(2)]
        log_z = sum(p[2] for p in parts) - math.log(np.prod(HI2 - LO2))
        mean_ll = [sum(-0.5 * th.truncated_gaussian(MEAN2[c], SD2[c], LO2[c], HI2[c], b)[3] / SD2[c] ** 2 for c in range(2))
                   for b in betas]
    else:
        m, s, t0 = 1.5, 0.5, 2.0
        log_z = 0.5 * math.log(s * s / (s * s + t0 * t0)) - 0.5 * m * m / (s * s + t0 * t0)
        mean_ll = []
        for b in betas:
            prec = b / (s * s) + 1.0 / (t0 * t0)
            mu = (b * m / (s * s)) / prec
            mean_ll.append(-0.5 * (1.0 / prec + (mu - m) ** 2) / (s * s))
    betas, mean_ll = np.asarray(betas), np.asarray(mean_ll)
    return log_z, float(np.sum(0.5 * (betas[:-1] - betas[1:]) * (mean_ll[:-1] + mean_ll[1:])))


@pytest.mark.parametrize("name", ["box", "conjugate"])
def test_evidence_against_closed_forms(name, built_library):
    s = tempered_run(name)
    ev = s.log_evidence(discard=DISCARD)
    log_z, ti = closed_form(name, s.betas)
    z = (ev["log_evidence"] - log_z) / ev["se"]
    z_ti = (ev["log_evidence_ti"] - ti) / ev["se_ti"]
    print(name, "log Z", log_z, "stepping stone", ev["log_evidence"], "+-", ev["se"], "z", z, "| TI", ev["log_evidence_ti"],
          "+-", ev["se_ti"], "against its trapezoid", ti, "z", z_ti, "| pair ESS min", ev["pair_ess"].min())
    assert ev["se"] <= 0.05                                        # a large se must not hide a wrong estimate
    assert abs(z) < 5.0
    assert abs(z_ti) < 5.0
    assert ev["pair_ess"].min() > 100.0 and abs(ev["log_evidence_ti"] - log_z) > 0.0
    assert math.isclose(ev["pair_log_ratio"].sum(), ev["log_evidence"]) and math.isclose(np.hypot.reduce(ev["pair_se"]), ev["se"])


# ------------------------------------------------------------------------------------------ crossing between modes
def two_modes(table):
    return np.logaddexp(-0.5 * (table[:, 0] + 10.0) ** 2, -0.5 * (table[:, 0] - 10.0) ** 2) - 0.5 * table[:, 1] ** 2


def test_tempering_is_what_crosses_between_modes():
    """Two unit Gaussians 20 apart (a barrier of 50 nats), every walker started in the left one."""
    plan = th.identity_plan(2, [-20.0, -10.0], [20.0, 10.0])
    start = np.array([-10.0, 0.0]) + np.random.default_rng(3).normal(size=(32, 2))
    alone = TemperedSampler(32, 2, [1.0], th.emul_block_fn(two_modes, plan), two_modes, seed=31)
    alone.run_mcmc(start, 2000)
    assert np.all(alone.chain[:, :, 0] < 0.0) and alone.acceptance_fraction.mean() > 0.3
    betas = default_ladder(10, 0.5)                                # 1 .. 1/256, 0
    s = TemperedSampler(32, 2, betas, th.emul_block_fn(two_modes, plan), two_modes, seed=32)
    s.run_mcmc(start, 6000)
    right = (s.chain[:, 1000:, 0] > 0.0).astype(np.float64)
    share, se = th.walker_means(right)
    print("share right of the midpoint", share, "+-", se, "swap acceptance", s.swap_acceptance_fraction)
    assert 0.3 <= share <= 0.7 and abs(share - 0.5) < 5.0 * se


# ------------------------------------------------------------------------------------------ plumbing
def test_evidence_summary_refuses_and_warns(built_library):
    rng = np.random.default_rng(0)
    ll = rng.normal(size=(3, 8, 200))
    for betas in ([1.0, 0.5, 0.1], [0.9, 0.5, 0.0], [1.0, 0.0, 0.0], [1.0]):
        with pytest.raises(ValueError):
            evidence_summary(ll[:len(betas)], betas)
    with pytest.raises(ValueError):
        evidence_summary(ll, [1.0, 0.5])
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        fine = evidence_summary(ll, [1.0, 0.5, 0.0])
    assert fine["pair_ess"].min() > 100 and fine["n_samples"] == 1600
    with pytest.warns(UserWarning, match="too coarse"):
        coarse = evidence_summary(40.0 * ll, [1.0, 0.5, 0.0], discard=10)
    assert coarse["pair_ess"].min() < 100 and coarse["n_samples"] == 8 * 190


def test_se_batch_on_independent_input_and_its_short_chain_branch(built_library):
    """Independent draws: the batch-means error and the delta-method error estimate the same thing.  With 20 batches the
    batch estimate has a relative spread of 1 / sqrt(2 * 19) = 0.16: a factor 2 either way is six of those.  Fewer than
    two steps per batch: NaN, and everything else as usual."""
    rng = np.random.default_rng(7)
    ll = rng.normal(size=(3, 16, 400))
    ev = evidence_summary(ll, [1.0, 0.5, 0.0])
    assert np.isfinite(ev["se_batch"]) and 0.5 * ev["se"] < ev["se_batch"] < 2.0 * ev["se"]
    short = evidence_summary(ll[:, :, :39], [1.0, 0.5, 0.0])
    assert math.isnan(short["se_batch"]) and np.isfinite(short["se"]) and np.isfinite(short["log_evidence"])
    assert np.isfinite(evidence_summary(ll[:, :, :40], [1.0, 0.5, 0.0])["se_batch"])


def test_bayes_factor_arithmetic():
    out = bayes_factor({"log_evidence": -10.0, "se": 0.03}, {"log_evidence": -12.5, "se": 0.04})
    assert out["log_bf"] == 2.5 and math.isclose(out["se"], 0.05)


def test_default_ladder():
    assert np.array_equal(default_ladder(5, 0.5), [1.0, 0.5, 0.25, 0.125, 0.0])
    assert np.array_equal(default_ladder(4, 0.5, proper=False), [1.0, 0.5, 0.25, 0.125])
    assert np.array_equal(default_ladder(1), [1.0])
    with pytest.raises(ValueError):
        default_ladder(3, 1.0)


def small_fit(**kwargs):
    c = synthetic.make_catalog(300, config=2)
    fit = ConstantFit(DataReader({k: c[k] for k in c if k != "truth"}), **kwargs)
    fit.parameters["ra_center"].set(value=c["truth"]["ra_center"], fixed=True)
    fit.parameters["dec_center"].set(value=c["truth"]["dec_center"], fixed=True)
    return fit


def fake_posterior(fit, record):
    """A 4-D Gaussian behind Runner.tempered: the CPU harness as the block, NumPy as the start's evaluation."""
    f = gaussian([0.0, 10.0, 3.0, 4.0], [0.5, 0.4, 0.7, 0.7])
    block = th.emul_block_fn(f, fit._stretch_plan())

    def block_fn(betas, *rest):
        record.append(np.array(betas))
        return block(betas, *rest)
    fit._temper_block = block_fn
    fit._temper_lnlike = f
    return np.array([0.0, 10.0, 3.0, 4.0]) + 0.3 * np.random.default_rng(0).normal(size=(8, 4))


def test_runner_tempered_has_a_zero_rung_exactly_when_the_prior_is_proper():
    fit = small_fit()
    seen = []
    pos = fake_posterior(fit, seen)
    s = fit.tempered(n_temps=4, n_walkers=8, n_steps=6, pos=pos, seed=3)          # v_sys, v_maxx, v_maxy are unbounded
    assert np.array_equal(s.betas, [1.0, 0.5, 0.25, 0.125]) and np.array_equal(seen[0], s.betas)
    assert s.chain.shape == (8, 6, 4) and s.lnlikelihood.shape == (4, 8, 6) and s.lnprobability.shape == (8, 6)
    assert s.acceptance_fraction.shape == (4, 8) and s.swap_acceptance_fraction.shape == (3,)
    assert set(s.improper) >= {"v_sys", "v_maxx", "v_maxy"}
    with pytest.raises(ValueError, match="v_sys"):
        s.log_evidence()
    with pytest.raises(ValueError):
        s.get_chain(temp=1)
    fit = small_fit()
    fit.parameters["v_sys"].set(min=-50.0, max=50.0)
    fit.parameters["sigma_max"].set(prior=("lognormal", 2.0, 1.0))                 # (its lower bound is 0, the upper one open)
    fit.parameters["v_maxx"].set(prior=("normal", 0.0, 10.0))
    fit.parameters["v_maxy"].set(min=-30.0, max=30.0)
    pos = fake_posterior(fit, seen)
    s = fit.tempered(n_temps=4, n_walkers=8, n_steps=6, pos=pos, seed=3, store_temps=2)
    assert np.array_equal(s.betas, [1.0, 0.5, 0.25, 0.0]) and s.improper == ()
    assert s.get_chain(temp=1).shape == (6, 8, 4) and s.rng_step == 6
    assert fit.tempered(n_walkers=8, n_steps=2, pos=pos, betas=[1.0, 0.3]).ntemps == 2


def test_runner_tempered_refusals():
    fit = small_fit()
    fit._temper_block = lambda *a: pytest.fail("must not run")
    fit.parameters["v_maxy"].set(expr="v_maxx")
    with pytest.raises(NotImplementedError):
        fit.tempered(n_temps=2, n_walkers=8, n_steps=2)
    fit = small_fit()
    fit.parameters["v_maxy"].set(lnprior="-0.5 * v_maxy ** 2")
    with pytest.raises(NotImplementedError):
        fit.tempered(n_temps=2, n_walkers=8, n_steps=2)
    fit32 = small_fit(precision="f32")
    with pytest.raises(NotImplementedError):
        fit32.tempered(n_temps=2, n_walkers=8, n_steps=2, pos=np.zeros((8, 4)))
    from mcmc_dynamics_amd.analysis import BinnedConstantFit
    c = synthetic.make_catalog(300, config=2)
    reader = DataReader({k: c[k] for k in c if k not in ("truth", "pmember")})
    reader.make_radial_bins(c["truth"]["ra_center"], c["truth"]["dec_center"], nstars=100, dlogr=0.05)
    binned = BinnedConstantFit(reader)
    with pytest.raises(NotImplementedError):
        binned.tempered(n_temps=2, n_walkers=8, n_steps=2)

"""GPU: mcd_temper_block (csrc/mcd_temper.hip, csrc/mcd_api_temper.hip) -- the block resident on the device against the
host-driven loop around mcd_loglike_batch (bit for bit), a ladder of one rung against the seeded stretch move, the stored
log-likelihoods against the kernels, continuation, the box, the refusals, and Runner.tempered end to end: its posterior
against the stretch move's and its log-evidence against a closed form.

Catalogues: mcmc_dynamics_amd/synthetic.py, the three model setups of tests/test_gpu_hmc.py.  Shapes: N in {33, 4099} x
(T, W) in {(1, 2), (2, 66), (5, 258)}: one row per launch, a ragged second 64-row tile, 645 rows with a partial last tile;
and (2, 1030), whose rungs are wider than their workgroup."""
import math

import numpy as np
import pytest

import test_gpu_hmc as hmc_cases
from mcmc_dynamics_amd import synthetic

pytestmark = pytest.mark.gpu

CENTRE = (synthetic.CENTER_RA_DEG, synthetic.CENTER_DEC_DEG)
MODELS = hmc_cases.MODELS
LADDERS = {1: np.array([1.0]), 2: np.array([1.0, 0.5]), 5: np.array([1.0, 0.6, 0.3, 0.1, 0.0])}
SHAPES = [(1, 2), (2, 66), (5, 258)]
# a normal and a log-normal prior on two coordinates of each setup's free parameters (sigma_max takes the log-normal one)
PRIORS = {"const": (1, 2), "bgfixed": (2, 1), "profile_gb_free": (1, 2)}


@pytest.fixture(scope="module")
def native():
    from mcmc_dynamics_amd import _native
    return _native


@pytest.fixture(scope="module")
def ctx(native):
    return native.default_context()


def with_prior(kind, plan, x, scale):
    """The plan with a normal / log-normal prior on its first two free parameters, a few posterior widths wide."""
    k = np.zeros(x.size, dtype=np.int32)
    p0, p1 = np.zeros(x.size), np.ones(x.size)
    for c in (0, 1):
        k[c] = PRIORS[kind][c]
        if k[c] == 1:
            p0[c], p1[c] = x[c] + scale[c], 3.0 * scale[c]
        else:
            p0[c], p1[c] = math.log(x[c]), 0.2
    return dict(plan, prior=(k, p0, p1))


def table_of(plan, pos):
    """(n, P) free parameters -> the (n, K) kernel table of the plan's column map."""
    n = pos.shape[0]
    return np.ascontiguousarray(np.stack(
        [pos[:, s] * plan["col_factor"][j] if s >= 0 else np.full(n, plan["col_const"][j])
         for j, s in enumerate(plan["col_source"])], axis=1))


def plain_loglike(cat, plan, pos, batch):
    """Log-likelihood of (n, P) positions through the library's plain kernels, in launches of ``batch`` rows -- the launch
    shape of a tempered half step (the chunk plan, and with it the order of the sums, belongs to the row count)."""
    assert pos.shape[0] % batch == 0
    found = cat.get_option("fast_path", 1)
    cat.set_option("fast_path", 0)
    try:
        table = table_of(plan, pos)
        return np.concatenate([cat.loglike(table[i:i + batch]) for i in range(0, pos.shape[0], batch)])
    finally:
        cat.set_option("fast_path", found)


def start_state(cat, plan, x, scale, t, w, seed=5):
    """Start positions in a ball of half a posterior width around the truth.  Two walkers get a ball of a twentieth of a
    width: their proposals lie on the line through both, so across the ball the log-likelihood (and log-prior) differs by
    ~1e-2, and a proposal is accepted whenever its stretch factor z exceeds 1 (thr = log u - (P - 1) log z < 0 then), i.e.
    with probability 1 - (sqrt 2 - 1) = 0.59 or more whatever P is -- ten proposals of a 5-step block all fail with
    probability 1.5e-4, so the single-row launch shape shows its accept path too."""
    ball = 0.1 if w == 2 else 1.0
    pos = hmc_cases.start(x, ball * scale, plan, t * w, seed=seed).reshape(t, w, x.size)
    ll = plain_loglike(cat, plan, pos.reshape(t * w, -1), t * (w // 2)).reshape(t, w)
    return np.ascontiguousarray(pos), np.ascontiguousarray(ll)


def run(cat, plan, betas, pos, ll, seed, step0, n_steps, resident, store=None):
    cat.set_option("device_chain", 1 if resident else 0)
    t, w, p = pos.shape
    store = t if store is None else store
    out = {"pos": pos.copy(), "lnlike": ll.copy(), "lnprior": np.full((t, w), np.nan),
           "chain": np.full((n_steps, store, w, p), np.nan), "lnlike_chain": np.full((n_steps, t, w), np.nan),
           "accepted": np.zeros((t, w), dtype=np.int64), "swap_proposed": np.zeros(t - 1, dtype=np.int64),
           "swap_accepted": np.zeros(t - 1, dtype=np.int64)}
    before = cat.temper_info()
    try:
        cat.temper_block(plan, betas, out["pos"], out["lnlike"], out["lnprior"], seed, step0, n_steps, out["chain"],
                         out["lnlike_chain"], out["accepted"], out["swap_proposed"], out["swap_accepted"])
    finally:
        cat.set_option("device_chain", 1)
    after = cat.temper_info()
    out["device_blocks"] = after["device_blocks"] - before["device_blocks"]
    out["host_blocks"] = after["host_blocks"] - before["host_blocks"]
    return out


KEYS = ("pos", "lnlike", "lnprior", "chain", "lnlike_chain", "accepted", "swap_proposed", "swap_accepted")


# ------------------------------------------------------------------------------------------ resident == host-driven
@pytest.mark.parametrize("prior", [False, True])
@pytest.mark.parametrize("t, w", SHAPES)
@pytest.mark.parametrize("n", [33, 4099])
@pytest.mark.parametrize("kind", MODELS)
def test_resident_block_is_the_host_driven_block(native, ctx, kind, n, t, w, prior):
    cat, plan, x, scale, _ = hmc_cases.case(native, ctx, kind, n)
    if prior:
        plan = with_prior(kind, plan, x, scale)
    pos, ll = start_state(cat, plan, x, scale, t, w)
    dev = run(cat, plan, LADDERS[t], pos, ll, 31, 3, 5, resident=True)
    host = run(cat, plan, LADDERS[t], pos, ll, 31, 3, 5, resident=False)
    assert (dev["device_blocks"], dev["host_blocks"]) == (1, 0)
    assert (host["device_blocks"], host["host_blocks"]) == (0, 1)
    for key in KEYS:
        assert dev[key].tobytes() == host[key].tobytes(), (key, kind, n, t, w, prior)
    # not a trivial agreement: the chains moved
    assert np.all(np.isfinite(dev["chain"])) and np.all(np.isfinite(dev["lnlike_chain"])) and np.all(np.isfinite(dev["lnprior"]))
    assert dev["accepted"].sum() > 0 and not np.array_equal(dev["pos"], pos)
    if t > 1:
        assert dev["swap_accepted"].sum() > 0
        assert np.array_equal(dev["swap_proposed"], [w * sum(1 for s in range(3, 8) if s % 2 == k % 2) for k in range(t - 1)])
    assert np.array_equal(dev["chain"][-1], dev["pos"]) and np.array_equal(dev["lnlike_chain"][-1], dev["lnlike"])
    assert np.all(dev["lnprior"] == 0.0) == (not prior)


def test_a_rung_wider_than_its_workgroup(native, ctx):
    """W/2 = 515 slots per rung: every thread of the rung's 256-thread workgroup strides over two or three of them."""
    cat, plan, x, scale, _ = hmc_cases.case(native, ctx, "const", 4099)
    pos, ll = start_state(cat, plan, x, scale, 2, 1030)
    dev = run(cat, plan, LADDERS[2], pos, ll, 31, 3, 4, resident=True)
    host = run(cat, plan, LADDERS[2], pos, ll, 31, 3, 4, resident=False)
    assert (dev["device_blocks"], host["host_blocks"]) == (1, 1)
    for key in KEYS:
        assert dev[key].tobytes() == host[key].tobytes(), key
    assert np.all(dev["accepted"].sum(axis=1) > 515) and dev["swap_accepted"].sum() > 0


# ------------------------------------------------------------------------------------------ T = 1 is the seeded stretch move
@pytest.mark.parametrize("w", [2, 66])
@pytest.mark.parametrize("kind", MODELS)
def test_one_rung_is_the_seeded_stretch_move(native, ctx, kind, w):
    cat, plan, x, scale, _ = hmc_cases.case(native, ctx, kind, 4099)
    pos, ll = start_state(cat, plan, x, scale, 1, w)
    found = cat.get_option("fast_path", 1)
    cat.set_option("fast_path", 0)
    try:
        for resident in (True, False):
            cat.set_option("device_chain", 1 if resident else 0)
            p, lnp = pos[0].copy(), ll[0].copy()
            chain, lnpc = np.full((6, w, x.size), np.nan), np.full((6, w), np.nan)
            acc = np.zeros(w, dtype=np.int64)
            cat.stretch_move_seeded(plan, p, lnp, 19, 7, 6, chain, lnpc, acc)
            got = run(cat, plan, LADDERS[1], pos, ll, 19, 7, 6, resident=resident)
            assert got["chain"][:, 0].tobytes() == chain.tobytes(), (kind, w, resident)
            assert got["lnlike_chain"][:, 0].tobytes() == lnpc.tobytes()
            assert np.array_equal(got["accepted"][0], acc) and acc.sum() > 0
            assert got["pos"][0].tobytes() == p.tobytes() and got["lnlike"][0].tobytes() == lnp.tobytes()
    finally:
        cat.set_option("fast_path", found)
        cat.set_option("device_chain", 1)


# ------------------------------------------------------------------------------------------ the fast_path option
@pytest.mark.parametrize("resident", [False, True])
@pytest.mark.parametrize("option", [0, 1, 2])
def test_a_block_leaves_the_fast_path_option_as_it_found_it(native, ctx, option, resident):
    """The block evaluates with the plain kernels whatever option "fast_path" says and puts nothing else in its place: an
    evaluation of the same table takes the same kernel family (Catalog.fast_level) before and after a block, host-driven
    and resident -- the plain one when the option was 0 beforehand -- and returns the same bytes."""
    cat, plan, x, scale, _ = hmc_cases.case(native, ctx, "bgfixed", 4099)
    pos, ll = start_state(cat, plan, x, scale, 2, 66)
    table = table_of(plan, pos.reshape(-1, x.size))
    found = cat.get_option("fast_path", 1)
    cat.set_option("fast_path", option)
    try:
        before = cat.loglike(table)
        level = cat.fast_level
        out = run(cat, plan, LADDERS[2], pos, ll, 3, 0, 4, resident=resident)
        assert out["accepted"].sum() > 0 and (out["device_blocks"], out["host_blocks"]) == ((1, 0) if resident else (0, 1))
        after = cat.loglike(table)
        print("fast_path", option, "resident" if resident else "host-driven", "kernel family before / after:", level,
              cat.fast_level)
        assert cat.fast_level == level and after.tobytes() == before.tobytes()
        if option == 0:
            assert level == 0
    finally:
        cat.set_option("fast_path", found)


# ------------------------------------------------------------------------------------------ the stored values
@pytest.mark.parametrize("kind", MODELS)
def test_stored_loglikelihoods_are_the_kernels_values(native, ctx, kind):
    """Every row of lnlike_chain equals the plain kernels' log-likelihood of that rung's chain positions, byte for byte:
    values travel with their walkers through accepts and swaps, and the block ran at guard level 0 although the
    catalogue's fast_path option is at its default."""
    cat, plan, x, scale, _ = hmc_cases.case(native, ctx, kind, 4099)
    t, w = 5, 66
    pos, ll = start_state(cat, plan, x, scale, t, w)
    for resident in (True, False):
        out = run(cat, plan, LADDERS[t], pos, ll, 5, 0, 4, resident=resident)
        want = plain_loglike(cat, plan, out["chain"].reshape(-1, x.size), t * (w // 2)).reshape(4, t, w)
        assert out["lnlike_chain"].tobytes() == want.tobytes(), (kind, resident)
        assert out["swap_accepted"].sum() > 0 and out["accepted"].sum() > 0


# ------------------------------------------------------------------------------------------ continuation, the box
@pytest.mark.parametrize("kind", ["const", "profile_gb_free"])
def test_blocks_continue_each_other_on_the_device(native, ctx, kind):
    cat, plan, x, scale, _ = hmc_cases.case(native, ctx, kind, 4099)
    plan = with_prior(kind, plan, x, scale)
    pos, ll = start_state(cat, plan, x, scale, 5, 66)
    whole = run(cat, plan, LADDERS[5], pos, ll, 8, 5, 6, resident=True)
    first = run(cat, plan, LADDERS[5], pos, ll, 8, 5, 3, resident=True)
    second = run(cat, plan, LADDERS[5], first["pos"], first["lnlike"], 8, 8, 3, resident=True)
    assert whole["device_blocks"] == first["device_blocks"] == second["device_blocks"] == 1
    for key in ("chain", "lnlike_chain"):
        assert np.concatenate([first[key], second[key]]).tobytes() == whole[key].tobytes(), key
    for key in ("accepted", "swap_proposed", "swap_accepted"):
        assert np.array_equal(first[key] + second[key], whole[key]), key
    assert not np.array_equal(first["swap_proposed"], second["swap_proposed"])          # steps 5, 6, 7 and 8, 9, 10: the parity
    for key in ("pos", "lnlike", "lnprior"):
        assert second[key].tobytes() == whole[key].tobytes(), key


def test_every_chain_row_of_every_rung_is_inside_a_tight_box(native, ctx):
    cat, plan, x, scale, _ = hmc_cases.case(native, ctx, "const", 4099)
    tight = dict(plan, lo=x - 0.7 * scale, hi=x + 0.7 * scale)
    t, w = 5, 66
    pos = np.ascontiguousarray(np.clip(hmc_cases.start(x, scale, plan, t * w), tight["lo"], tight["hi"]).reshape(t, w, 4))
    ll = plain_loglike(cat, tight, pos.reshape(t * w, 4), t * (w // 2)).reshape(t, w)
    out = run(cat, tight, LADDERS[t], pos, ll, 4, 0, 6, resident=True)
    c = out["chain"]
    assert c.shape == (6, t, w, 4) and np.all(c >= tight["lo"]) and np.all(c <= tight["hi"])
    rate = out["accepted"].sum(axis=1) / (6.0 * w)
    print("acceptance per rung in the tight box:", rate)
    assert np.all(rate > 0.0) and np.all(rate < 1.0)                    # some proposals left the box, at beta = 0 too
    host = run(cat, tight, LADDERS[t], pos, ll, 4, 0, 6, resident=False)
    assert host["chain"].tobytes() == c.tobytes()


# ------------------------------------------------------------------------------------------ refusals
def test_refusals_leave_everything_untouched(native, ctx):
    kw, plan, x, scale, _ = hmc_cases.setup("const", 33)
    cols = [kw.pop(k) for k in ("ra", "dec", "v", "verr")]
    pos = hmc_cases.start(x, scale, plan, 16).reshape(2, 8, 4)

    def refused(cat, plan, betas, pos, store=1, status="status -1"):
        for resident in (1, 0):
            cat.set_option("device_chain", resident)
            t, w, p = pos.shape
            arrays = [pos.copy(), np.full((t, w), -1.5), np.full((t, w), np.nan), np.full((2, store, w, p), np.nan),
                      np.full((2, t, w), np.nan)]
            counts = [np.zeros((t, w), dtype=np.int64), np.zeros(t - 1, dtype=np.int64), np.zeros(t - 1, dtype=np.int64)]
            keep = [a.copy() for a in arrays]
            with pytest.raises(native.NativeError, match=status):
                cat.temper_block(plan, betas, arrays[0], arrays[1], arrays[2], 1, 0, 2, arrays[3], arrays[4], *counts)
            for a, b in zip(arrays, keep):
                assert a.tobytes() == b.tobytes()
            assert all(c.sum() == 0 for c in counts)
        cat.set_option("device_chain", 1)
        assert cat.temper_info() == {"device_blocks": 0, "host_blocks": 0}

    for more in ({"bin_offsets": np.array([0, 10, 33], dtype=np.int64)}, {"precision": "f32"}):
        cat = native.Catalog(ctx, *cols, **dict(kw, **more))
        refused(cat, plan, [1.0, 0.5], pos)
        cat.close()
    cat = native.Catalog(ctx, *cols, **kw)
    refused(cat, plan, [1.0, 0.5], np.ascontiguousarray(pos[:, :7]))                  # odd W
    refused(cat, plan, [1.0, 1.0], pos)                                               # not strictly decreasing
    refused(cat, plan, [1.0, 0.2, 0.4], np.ascontiguousarray(np.concatenate([pos, pos[:1]])))
    refused(cat, plan, [1.0, -0.5], pos)                                              # outside [0, 1]
    refused(cat, plan, [0.9, 0.5], pos)                                               # betas[0] != 1
    refused(cat, plan, [1.0, 0.5], pos, store=3)                                      # n_chain_temps outside 1 .. T
    wide = {key: (np.append(val, val[-1:]) if key.startswith("col_") else val) for key, val in plan.items()}
    cat.k += 1                                                                        # the binding's own check looks at this
    try:
        refused(cat, wide, [1.0, 0.5], pos)                                           # map.k is not the catalogue's
    finally:
        cat.k -= 1
    # a start outside the box: MCD_ERR_NONFINITE in both forms
    bad = pos.copy()
    bad[1, 3, 1] = -1.0                                                               # sigma_max below its bound
    refused(cat, plan, [1.0, 0.5], bad, status="status -5")
    cat.close()


# ------------------------------------------------------------------------------------------ end to end
def test_runner_tempered_against_the_stretch_move():
    """ConstantFit on 2 000 synthetic stars: the rung-0 posterior means of Runner.tempered (4 rungs of 64 walkers) and of the
    sampler Runner.__call__ drives by default agree within 5 combined Monte-Carlo standard errors; so do two runs of that
    sampler with different seeds (the criterion is met by existing code alone).  z-scores observed: DESIGN 3.14."""
    from mcmc_dynamics_amd import DataReader
    from mcmc_dynamics_amd.analysis import ConstantFit
    cat = synthetic.make_catalog(2000, config=2)
    fit = ConstantFit(DataReader({k: cat[k] for k in ("ra", "dec", "v", "verr")}), seed=13)
    fit.parameters["ra_center"].set(value=CENTRE[0], fixed=True)
    fit.parameters["dec_center"].set(value=CENTRE[1], fixed=True)
    x_map = fit.maximize()["x"]
    cov = fit.laplace(x_map)["covariance"]
    np.random.seed(101)
    pos = fit.get_initials_laplace(64, x_map, cov)
    pt = fit.tempered(n_temps=4, n_walkers=64, n_steps=1200, pos=pos, seed=2024)
    assert np.array_equal(pt.betas, [1.0, 0.5, 0.25, 0.125]) and pt.chain.shape == (64, 1200, 4)      # improper prior: no zero rung
    assert fit._catalog.temper_info()["device_blocks"] > 0 and fit._catalog.temper_info()["host_blocks"] == 0
    assert fit._catalog.get_option("fast_path") == 1                    # the start's plain evaluation put the option back
    print("acceptance per rung", pt.acceptance_fraction.mean(axis=1), "swaps", pt.swap_acceptance_fraction)
    assert pt.swap_acceptance_fraction.min() > 0.05 and pt.acceptance_fraction.mean() > 0.2
    m_pt, se_pt = hmc_cases.walker_means(pt.chain[:, 400:])
    stretch = []
    for seed in (7, 8):
        np.random.seed(seed)
        pos = fit.get_initials_laplace(64, x_map, cov)
        s = fit(n_walkers=64, n_steps=1200, pos=pos, prefix=None)
        stretch.append(hmc_cases.walker_means(np.asarray(s.chain)[:, 400:]))
    (m_a, se_a), (m_b, se_b) = stretch
    z_self = (m_a - m_b) / np.hypot(se_a, se_b)
    z_pt = (m_pt - m_a) / np.hypot(se_pt, se_a)
    print("z stretch vs stretch", z_self, " z tempered vs stretch", z_pt)
    assert np.all(np.abs(z_self) < 5.0)
    assert np.all(np.abs(z_pt) < 5.0)


def test_log_evidence_against_the_closed_form():
    """2 000 stars without background, only v_sys free in a finite box (sigma_max, a zero rotation and the centre fixed):
    the likelihood is exactly Gaussian in v_sys, exp(c0) exp(-A (v_sys - m)^2 / 2), and
    log Z = c0 + 1/2 log(2 pi / A) + log(Phi((hi - m) sqrt A) - Phi((lo - m) sqrt A)) - log(hi - lo)
    from the catalogue's columns, in numpy.longdouble.  Ladder and steps were sized on the CPU harness with a NumPy
    likelihood of this catalogue (12 rungs of ratio 1/2 down to 1/1024 and 0, 64 walkers, 1 000 steps, 200 discarded):
    se = 0.0074 there, half the cap and less."""
    from mcmc_dynamics_amd import DataReader
    from mcmc_dynamics_amd.analysis import ConstantFit
    cat = synthetic.make_catalog(2000, config=2, background=False)
    L = np.longdouble
    v, e = cat["v"].astype(L), cat["verr"].astype(L)
    n = L(10.0) ** 2 + e * e
    A = (1 / n).sum()
    m = (v / n).sum() / A
    c0 = (-0.5 * np.log(2 * L(np.pi) * n)).sum() - 0.5 * (v * v / n).sum() + 0.5 * A * m * m
    lo, hi = round(float(m) - 4.0, 1), round(float(m) + 6.0, 1)
    root = math.sqrt(float(A) / 2.0)
    mass = 0.5 * (math.erfc(-(hi - float(m)) * root) - math.erfc(-(lo - float(m)) * root))
    log_z = float(c0 + 0.5 * np.log(2 * L(np.pi) / A) + np.log(L(mass)) - np.log(L(hi) - L(lo)))

    fit = ConstantFit(DataReader({k: cat[k] for k in ("ra", "dec", "v", "verr")}), seed=13)
    fit.parameters["ra_center"].set(value=CENTRE[0], fixed=True)
    fit.parameters["dec_center"].set(value=CENTRE[1], fixed=True)
    fit.parameters["sigma_max"].set(value=10.0, fixed=True)
    fit.parameters["v_maxx"].set(value=0.0, fixed=True)
    fit.parameters["v_maxy"].set(value=0.0, fixed=True)
    fit.parameters["v_sys"].set(min=lo, max=hi)
    pos = float(m) + 0.2 * np.random.default_rng(1).normal(size=(64, 1))
    pt = fit.tempered(n_temps=12, n_walkers=64, n_steps=1000, pos=pos, seed=5)
    assert pt.betas[-1] == 0.0 and pt.betas[-2] == 2.0 ** -10
    ev = pt.log_evidence(discard=200)
    z = (ev["log_evidence"] - log_z) / ev["se"]
    print("log Z", log_z, "stepping stone", ev["log_evidence"], "+-", ev["se"], "z", z, "TI", ev["log_evidence_ti"], "+-",
          ev["se_ti"], "pair ESS min", ev["pair_ess"].min())
    assert ev["se"] <= 0.1
    assert abs(z) < 5.0

"""GPU: structured priors (csrc/mcd_prior.h) inside the library's blocks -- mcd_stretch_move_prior / _seeded_prior resident
on the device (csrc/mcd_stretch.hip) against the host-driven loop and a NumPy restatement, mcd_hmc_block_prior resident
against host-driven and against the 80-bit gradient restatement, Runner.lnprob_grad_batch, and two end-to-end posteriors
whose answer is known without the library: a conjugate Gaussian one and a log-normal one by quadrature.

Shapes: N in {33, 4099} (one chunk, several) x W in {2, 66, 258} (+ 514 un-binned: the general step kernel); every such
launch has <= 256 partial sums per walker and runs the step kernel that adds them up itself (kFused), one case with 257
chunks runs the other."""
import numpy as np
import pytest

import grad_helper as gh
import prior_helper as ph
import variant_helper as vh
from mcmc_dynamics_amd import synthetic

pytestmark = pytest.mark.gpu

CENTRE = (synthetic.CENTER_RA_DEG, synthetic.CENTER_DEC_DEG)
L = vh.L
STEPS = 6


@pytest.fixture(scope="module")
def native():
    from mcmc_dynamics_amd import _native
    return _native


@pytest.fixture(scope="module")
def ctx(native):
    return native.default_context()


# ------------------------------------------------------------------------------------------ the stretch chain
def setup(kind, n):
    """(catalogue keyword arguments, plan with its prior, centre of the start ensemble, its relative spread per column)"""
    c = synthetic.make_catalog(n, config=2, background=kind == "profile")
    t = c["truth"]
    base = dict(ra=c["ra"], dec=c["dec"], v=c["v"], verr=c["verr"])
    inf = np.inf
    if kind in ("const", "binned"):
        # v_sys, sigma_max, v_maxx, v_maxy: normal on v_sys, log-normal on sigma_max, whose box reaches below zero
        plan = {"col_source": np.arange(4, dtype=np.int32), "col_const": np.zeros(4), "col_factor": np.ones(4),
                "lo": np.array([-inf, -5.0, -inf, -inf]), "hi": np.full(4, inf), "fixed_ok": True,
                "prior": (np.array([1, 2, 0, 0], dtype=np.int32), np.array([0.5, np.log(8.0), 0.0, 0.0]), np.array([2.0, 0.3, 1.0, 1.0]))}
        x = np.array([0.3, 9.0, t["v_maxx"], t["v_maxy"]])
        kw = dict(base, model=0, centre=CENTRE)
        if kind == "binned":
            kw["bin_offsets"] = np.array([0, n // 3, n // 2, n], dtype=np.int64)
        return kw, plan, x, np.array([1.0, 1.5, 1.0, 1.0])
    # PROFILE_BGGAUSS, free centre, K = 11: v_sys, sigma_max, a, v_maxx, v_maxy, r_peak, ra, dec, v_back, sigma_back, f_back;
    # normal priors on both centre columns, log-normal on a, and `a` sampled in arcmin (a unit factor of 60 on its column)
    kind_, p0, p1 = np.zeros(11, dtype=np.int32), np.zeros(11), np.ones(11)
    kind_[[6, 7]], p0[[6, 7]], p1[[6, 7]] = 1, [CENTRE[0] + 0.001, CENTRE[1] - 0.001], 0.004
    kind_[2], p0[2], p1[2] = 2, np.log(1.5), 0.4
    fac = np.ones(11)
    fac[2] = 60.0
    plan = {"col_source": np.arange(11, dtype=np.int32), "col_const": np.zeros(11), "col_factor": fac,
            "lo": np.array([-inf, 0.0, 1.0 / 60.0, -inf, -inf, 1.0, CENTRE[0] - 0.05, CENTRE[1] - 0.05, -inf, 0.0, 0.0]),
            "hi": np.array([inf, inf, 10.0, inf, inf, 600.0, CENTRE[0] + 0.05, CENTRE[1] + 0.05, inf, inf, 1.0]),
            "fixed_ok": True, "prior": (kind_, p0, p1)}
    x = np.array([t["v_sys"], t["sigma_max"], 2.0, t["v_maxx"], t["v_maxy"], 60.0, CENTRE[0], CENTRE[1], t["v_back"],
                  t["sigma_back"], t["f_back"]])
    spread = np.array([1.0, 0.1, 0.1, 1.0, 1.0, 0.1, 0.003, 0.003, 3.0, 0.1, 0.1])
    return dict(base, model=4, centre=None, density=c["density"]), plan, x, spread


_CASES = {}


def case(native, ctx, kind, n):
    if (kind, n) not in _CASES:
        kw, plan, x, spread = setup(kind, n)
        cat = native.Catalog(ctx, kw.pop("ra"), kw.pop("dec"), kw.pop("v"), kw.pop("verr"), **kw)
        _CASES[(kind, n)] = (cat, plan, x, spread)
    return _CASES[(kind, n)]


def ensemble(plan, x, spread, lead, w, seed=5):
    """Start positions: a ball around x (narrow for W = 2, where ONE proposal outside the prior leaves a half step without
    a valid proposal and the device hands the block back), and the plan with a box that cuts into the larger ensembles."""
    rng = np.random.default_rng(seed)
    width = 0.02 if w == 2 else 1.0
    multiplicative = np.isin(np.arange(x.size), [1, 2, 5, 9, 10]) & (x.size == 11) | ((np.arange(x.size) == 1) & (x.size == 4))
    g = rng.normal(size=lead + (w, x.size))
    pos = np.where(multiplicative, x * np.exp(0.3 * width * spread * g), x + width * spread * g)
    if x.size == 4 and w > 2:
        pos[..., ::5, 1] = 0.5 + rng.random(pos[..., ::5, 1].shape)      # proposals that cross sigma_max = 0
    pos = np.ascontiguousarray(np.clip(pos, np.maximum(plan["lo"], np.where(plan["prior"][0] == 2, 1e-3, -np.inf)), plan["hi"]))
    plan = dict(plan, lo=plan["lo"].copy(), hi=plan["hi"].copy())
    if w > 2:
        col = 0
        plan["hi"][col] = np.sort(pos[..., col].ravel())[-max(2, w // 16)]      # a tight box: some proposals are rejected by it
        pos[..., col] = np.minimum(pos[..., col], plan["hi"][col])
    return pos, plan


def table_of(plan, p):
    src, fac, const = plan["col_source"], plan["col_factor"], plan["col_const"]
    cols = p[..., np.maximum(src, 0)]
    return np.ascontiguousarray(np.where(src >= 0, np.where(fac == 1.0, cols, cols * fac), const))


def lnprob(native, cat, plan, pos):
    """Log-likelihood plus log-prior of positions inside the prior: what a chain's lnp holds."""
    lp = native.prior_eval(plan["prior"], pos.reshape(-1, pos.shape[-1])).reshape(pos.shape[:-1])
    return np.ascontiguousarray(cat.loglike(table_of(plan, pos)) + lp)


def numpy_block(native, cat, plan, pos, lnp, order, zz, thr, pick):
    """sampler.py's half-step loop for [B] ensembles with ``cat.loglike`` + ``mcd_prior_eval`` as the posterior."""
    pos, lnp = pos.copy(), lnp.copy()
    lead = pos.shape[:-2]
    B, (w, p) = int(np.prod(lead, dtype=int)), pos.shape[-2:]
    half, n_steps = w // 2, order.shape[0]
    P, LP = pos.reshape(B, w, p), lnp.reshape(B, w)
    O, Z, T, K = order.reshape(n_steps, B, w), zz.reshape(n_steps, 2, B, half), thr.reshape(n_steps, 2, B, half), \
        pick.reshape(n_steps, 2, B, half)
    chain, lnpc, acc = np.empty((n_steps, B, w, p)), np.empty((n_steps, B, w)), np.zeros((B, w), dtype=np.int64)
    rejected_by_prior = 0
    for i in range(n_steps):
        for h in (0, 1):
            first = O[i, :, :half] if h == 0 else O[i, :, half:]
            second = O[i, :, half:] if h == 0 else O[i, :, :half]
            b_idx = np.arange(B)[:, None]
            s, partners = P[b_idx, first], P[b_idx, np.take_along_axis(second, K[i, h], axis=1)]
            proposal = partners - (partners - s) * Z[i, h][..., None]
            flat = proposal.reshape(-1, p)
            box = np.all((flat >= plan["lo"]) & (flat <= plan["hi"]), axis=1)
            lp = native.prior_eval(plan["prior"], flat)
            ok = box & (lp > -np.inf)
            rejected_by_prior += int(np.count_nonzero(~ok))
            new = np.full(B * half, -np.inf)
            if ok.any():
                rows = flat.copy()
                rows[~ok] = rows[np.argmax(ok)]
                t = table_of(plan, rows)
                ll = cat.loglike(t.reshape(B, half, -1) if lead else t).reshape(-1)
                new[ok] = (ll + lp)[ok]
            new = new.reshape(B, half)
            accept = T[i, h] < new - LP[b_idx, first]
            for b in range(B):
                idx = first[b][accept[b]]
                P[b, idx], LP[b, idx] = proposal[b][accept[b]], new[b][accept[b]]
                acc[b, idx] += 1
        chain[i], lnpc[i] = P, LP
    return (P.reshape(pos.shape), LP.reshape(lnp.shape), chain.reshape((n_steps,) + pos.shape), lnpc.reshape((n_steps,) + lnp.shape),
            acc.reshape(lnp.shape)), rejected_by_prior


def run_block(cat, plan, pos, lnp, mode, numbers=None, seed=None, step0=0, n_steps=STEPS):
    cat.set_option("device_chain", mode)                 # 0 host-driven, 1 resident
    pos, lnp = pos.copy(), lnp.copy()
    chain, lnpc, acc = np.empty((n_steps,) + pos.shape), np.empty((n_steps,) + lnp.shape), np.zeros(lnp.shape, dtype=np.int64)
    if numbers is not None:
        cat.stretch_move(plan, pos, lnp, *numbers, chain, lnpc, acc)
    else:
        cat.stretch_move_seeded(plan, pos, lnp, seed, step0, n_steps, chain, lnpc, acc)
    cat.set_option("device_chain", 1)
    return pos, lnp, chain, lnpc, acc


def same(a, b):
    return all(x.tobytes() == y.tobytes() for x, y in zip(a, b))


SHAPES = [("const", n, w) for n in (33, 4099) for w in (2, 66, 258, 514)] + \
         [("profile", n, w) for n in (33, 4099) for w in (2, 66, 258, 514)] + \
         [("binned", n, w) for n in (33, 4099) for w in (2, 66, 258)]


@pytest.mark.parametrize("kind,n,w", SHAPES)
def test_chain_with_priors_resident_host_driven_and_numpy(native, ctx, kind, n, w):
    cat, plan0, x, spread = case(native, ctx, kind, n)
    lead = (3,) if kind == "binned" else ()
    pos, plan = ensemble(plan0, x, spread, lead, w)
    lnp = lnprob(native, cat, plan, pos)
    assert np.all(np.isfinite(lnp))
    assert cat.launch_info()["chunks"] <= 256            # with option "fused_reduce" (default): the kFused step kernel
    seed = 20261018 + w
    numbers = native.chain_numbers(seed, 0, STEPS, len(lead) and 3, w, x.size, squeeze=not lead)
    before = cat.stretch_info()
    dev = run_block(cat, plan, pos, lnp, 1, numbers=numbers)
    mid = cat.stretch_info()
    host = run_block(cat, plan, pos, lnp, 0, numbers=numbers)
    after = cat.stretch_info()
    assert mid["device_blocks"] == before["device_blocks"] + 1 and mid["discarded_blocks"] == before["discarded_blocks"], mid
    assert after["host_blocks"] == mid["host_blocks"] + 1 and after["device_blocks"] == mid["device_blocks"]
    assert same(dev, host)
    ref, rejected = numpy_block(native, cat, plan, pos, lnp, *numbers)
    assert same(dev, ref)
    if w > 2:
        assert rejected > 0 and 0 < dev[4].sum() < STEPS * w * max(1, len(lead) * 3)
    # the seeded form: the same numbers generated inside the library, resident and host-driven, and 3 + 3 steps == 6
    sdev = run_block(cat, plan, pos, lnp, 1, seed=seed)
    assert same(sdev, dev) and same(run_block(cat, plan, pos, lnp, 0, seed=seed), dev)
    a = run_block(cat, plan, pos, lnp, 1, seed=seed, n_steps=3)
    b = run_block(cat, plan, a[0], a[1], 1, seed=seed, step0=3, n_steps=3)
    assert np.concatenate([a[2], b[2]]).tobytes() == dev[2].tobytes() and b[0].tobytes() == dev[0].tobytes()
    assert b[1].tobytes() == dev[1].tobytes() and np.array_equal(a[4] + b[4], dev[4])
    info = cat.stretch_info()
    assert info["discarded_blocks"] == before["discarded_blocks"] and info["device_blocks"] == after["device_blocks"] + 3
    # the prior is in the numbers: the chain's values are likelihood + prior of its positions, and differ without it
    # (evaluated W / 2 rows at a time, as the chain does: the chunk table, hence the order of summation, depends on the row
    # count -- and, beyond one walker tile, on the row's place in the table, which a walker changes from step to step)
    half = w // 2
    for part in (slice(0, half), slice(half, w)):
        again = lnprob(native, cat, plan, np.ascontiguousarray(dev[0][..., part, :]))
        assert np.array_equal(dev[1][..., part], again) if half <= 64 else np.allclose(dev[1][..., part], again, rtol=1e-12, atol=0)
    if w > 2:
        flat = dict(plan, prior=None)
        assert run_block(cat, flat, pos, lnp, 1, numbers=numbers)[2].tobytes() != dev[2].tobytes()


def test_chain_with_priors_without_the_fused_reduction(native, ctx):
    """257 chunks of 64 stars: more partial sums per walker than the step kernel adds up itself -- the reduction kernel runs
    and the step kernel is the instantiation that reads its sums."""
    n, w = 64 * 257 - 13, 66
    kw, plan0, x, spread = setup("const", n)
    cat = native.Catalog(ctx, kw.pop("ra"), kw.pop("dec"), kw.pop("v"), kw.pop("verr"), **kw)
    for key, value in (("balance", 0), ("combine", 0), ("tail_split", 0), ("chunk_len", 64)):
        cat.set_option(key, value)
    pos, plan = ensemble(plan0, x, spread, (), w)
    cat.loglike(table_of(plan, pos[: w // 2]))
    assert cat.launch_info()["chunks"] == 257
    lnp = lnprob(native, cat, plan, pos)
    numbers = native.chain_numbers(77, 0, STEPS, 0, w, 4, squeeze=True)
    dev = run_block(cat, plan, pos, lnp, 1, numbers=numbers)
    info = cat.stretch_info()
    assert info["device_blocks"] == 1 and info["discarded_blocks"] == 0
    assert same(dev, run_block(cat, plan, pos, lnp, 0, numbers=numbers))
    assert same(dev, numpy_block(native, cat, plan, pos, lnp, *numbers)[0])
    cat.close()


# ------------------------------------------------------------------------------------------ no prior == today's entry points
def hmc_run(cat, plan, chol, eps, n_leap, pos, seed, step0, n_steps, resident, jitter=0.1):
    cat.set_option("device_chain", 1 if resident else 0)
    pos = pos.copy()
    w, p = pos.shape
    out = {"pos": pos, "lnp": np.full(w, np.nan), "chain": np.full((n_steps, w, p), np.nan),
           "lnprob_chain": np.full((n_steps, w), np.nan), "accepted": np.zeros(w, dtype=np.int64),
           "energy_error": np.full((n_steps, w), np.nan)}
    before = cat.hmc_info()
    cat.hmc_block(plan, chol, eps, n_leap, pos, out["lnp"], seed, step0, n_steps, out["chain"], out["lnprob_chain"],
                  out["accepted"], out["energy_error"], jitter=jitter)
    after = cat.hmc_info()
    out["where"] = (after["device_blocks"] - before["device_blocks"], after["host_blocks"] - before["host_blocks"])
    cat.set_option("device_chain", 1)
    return out


HMC_KEYS = ("chain", "lnprob_chain", "accepted", "energy_error", "pos", "lnp")


def test_null_and_all_flat_priors_are_the_entry_points_without_priors(native, ctx):
    cat, plan0, x, spread = case(native, ctx, "const", 4099)
    pos, plan = ensemble(plan0, x, spread, (), 66)
    plan["lo"][1] = 0.0
    pos[:, 1] = np.maximum(pos[:, 1], 0.5)
    todays = {k: v for k, v in plan.items() if k != "prior"}          # no "prior" entry: mcd_stretch_move, mcd_hmc_block
    null = dict(todays, prior=None)                                    # the *_prior entry points with NULL
    flat = dict(todays, prior=(np.zeros(4, dtype=np.int32), np.full(4, np.nan), np.full(4, -1.0)))
    lnp = np.ascontiguousarray(cat.loglike(table_of(plan, pos)))
    numbers = native.chain_numbers(5, 0, STEPS, 0, 66, 4, squeeze=True)
    chol = np.diag([0.3, 0.2, 0.4, 0.4])
    for mode in (1, 0):
        ref = run_block(cat, todays, pos, lnp, mode, numbers=numbers)
        sref = run_block(cat, todays, pos, lnp, mode, seed=5)
        href = hmc_run(cat, todays, chol, 0.6, 3, pos, 31, 2, 4, resident=bool(mode))
        for other in (null, flat):
            assert same(ref, run_block(cat, other, pos, lnp, mode, numbers=numbers))
            assert same(sref, run_block(cat, other, pos, lnp, mode, seed=5))
            h = hmc_run(cat, other, chol, 0.6, 3, pos, 31, 2, 4, resident=bool(mode))
            assert h["where"] == href["where"] == ((1, 0) if mode else (0, 1))
            for key in HMC_KEYS:
                assert h[key].tobytes() == href[key].tobytes(), key


# ------------------------------------------------------------------------------------------ HMC
def hmc_setup(native, ctx, n, dense):
    cat, plan0, x, spread = case(native, ctx, "const", n)
    plan = dict(plan0, lo=plan0["lo"].copy())
    plan["lo"][1] = 0.0
    s = 10.0 / np.sqrt(n)
    scale = np.array([s, 0.7 * s, 1.4 * s, 1.4 * s])
    # priors about as wide as the data's constraint, so that they shape the trajectories
    plan["prior"] = (np.array([1, 2, 0, 1], dtype=np.int32), np.array([0.5 * s, np.log(10.0 - s), 0.0, 1.0]),
                     np.array([1.5 * s, 0.1 * s, 1.0, 2.0 * s]))
    chol = np.diag(scale)
    if dense:
        chol = chol @ (np.eye(4) + 0.2 * np.tril(np.ones((4, 4)), -1) / 4)
    t = synthetic.make_catalog(n, config=2)["truth"]
    mode = np.array([t["v_sys"], t["sigma_max"], t["v_maxx"], t["v_maxy"]])
    return cat, plan, mode, scale, chol


@pytest.mark.parametrize("dense", [False, True])
@pytest.mark.parametrize("n_leap", [1, 3])
@pytest.mark.parametrize("w", [1, 65, 257])
@pytest.mark.parametrize("n", [33, 4099])
def test_hmc_with_priors_resident_is_host_driven(native, ctx, n, w, n_leap, dense):
    cat, plan, mode, scale, chol = hmc_setup(native, ctx, n, dense)
    pos = np.ascontiguousarray(np.clip(mode + 0.5 * scale * np.random.default_rng(5).normal(size=(w, 4)), plan["lo"] + 1e-3, plan["hi"]))
    dev = hmc_run(cat, plan, chol, 0.6, n_leap, pos, 31, 2, 4, resident=True)
    host = hmc_run(cat, plan, chol, 0.6, n_leap, pos, 31, 2, 4, resident=False)
    assert dev["where"] == (1, 0) and host["where"] == (0, 1)
    for key in HMC_KEYS:
        assert dev[key].tobytes() == host[key].tobytes(), (key, n, w, n_leap, dense)
    assert np.all(np.isfinite(dev["chain"])) and np.all(np.isfinite(dev["lnprob_chain"]))
    if w > 1:
        assert dev["accepted"].sum() > 0 and not np.array_equal(dev["pos"], pos)
    # lnp is likelihood plus prior of the final positions, in the library's own bits
    value, _ = cat.loglike_grad(table_of(plan, dev["pos"]))
    lp, _ = native.prior_eval(plan["prior"], dev["pos"], want_grad=True)
    assert (value + lp).tobytes() == dev["lnp"].tobytes()
    flat = hmc_run(cat, dict(plan, prior=None), chol, 0.6, n_leap, pos, 31, 2, 4, resident=True)
    assert flat["chain"].tobytes() != dev["chain"].tobytes() or w == 1


def prior_exact(prior, q):
    """(value, gradient) of the structured priors at one row q, in longdouble."""
    kind, p0, p1 = prior
    value, grad = L(0), np.zeros(q.size, dtype=L)
    for c, k in enumerate(kind):
        if k == 0:
            continue
        u = np.log(q[c]) if k == 2 else q[c]
        t = (u - L(p0[c])) / L(p1[c])
        value += -np.log(L(p1[c])) - ph.HALF_LOG_2PI - (u if k == 2 else 0) - t * t / 2
        grad[c] = -t / L(p1[c]) if k == 1 else -(1 + t / L(p1[c])) / q[c]
    return value, grad


def test_energy_error_with_priors_is_the_numpy_restatements(native, ctx):
    """tests/test_gpu_hmc.py's energy test with the prior in the potential: CONST, N = 4099, W = 65, one step of two
    leapfrog points from ~10 posterior widths off the mode, H = -(lnlike + lnprior) + kinetic on the 80-bit gradient
    restatement plus the longdouble prior.  Bound: that test's own, 1e-9 relative to |dH|."""
    eps, n_leap, jitter, seed = 1.2, 2, 0.1, 17
    cat, plan, mode, scale, chol = hmc_setup(native, ctx, 4099, False)
    c = synthetic.make_catalog(4099, config=2)
    cols = {k: c[k] for k in ("ra", "dec", "v", "verr")}
    rng = np.random.default_rng(3)
    pos = np.ascontiguousarray(mode + 10.0 * scale * rng.choice([-1.0, 1.0], size=(65, 4)) * rng.uniform(0.8, 1.2, size=(65, 4)))
    z, thr, r = native.hmc_numbers(seed, 0, 1, 65, 4)
    diag = np.diag(chol).copy()
    cl = chol.astype(L)
    minv = cl @ cl.T
    want = np.empty(65, dtype=L)

    def potential(q):
        value, grad = prior_exact(plan["prior"], q)
        return -(vh.exact(0, cols, q, CENTRE) + value), gh.grad(0, cols, q, CENTRE, L)[0] + grad
    for w in range(65):
        q = pos[w].astype(L)
        p = (z[0, w] / diag).astype(L)
        e = L(eps) * (L(1) + L(jitter) * L(r[0, w]))
        y = cl.T @ p
        u0, g = potential(q)
        h0 = u0 + L(0.5) * (y @ y)
        p = p + L(0.5) * e * g
        for leap in range(1, n_leap + 1):
            q = q + e * (minv @ p)
            assert np.all(q >= plan["lo"]) and np.all(q <= plan["hi"]) and q[1] > 0
            u1, g = potential(q)
            p = p + (e if leap < n_leap else L(0.5) * e) * g
        y = cl.T @ p
        want[w] = (u1 + L(0.5) * (y @ y)) - h0
    got = hmc_run(cat, plan, chol, eps, n_leap, pos, seed, 0, 1, resident=True, jitter=jitter)
    want_abs = np.abs(want).astype(np.float64)
    err = np.abs(got["energy_error"][0] - want_abs) / want_abs
    print("min / median |dH| (NumPy):", want_abs.min(), np.median(want_abs), " largest relative difference:", err.max())
    assert want_abs.min() > 0.1, "the configuration is meant to keep every |dH| away from 0"
    assert np.all(err <= 1e-9), (err.max(), int(np.argmax(err)))
    no_prior = hmc_run(cat, dict(plan, prior=None), chol, eps, n_leap, pos, seed, 0, 1, resident=True, jitter=jitter)
    assert np.max(np.abs(no_prior["energy_error"][0] - want_abs) / want_abs) > 1e-3       # the prior is in the energy


def test_errors(native, ctx):
    cat, plan, mode, scale, chol = hmc_setup(native, ctx, 33, False)
    pos = np.ascontiguousarray(mode + 0.1 * scale * np.random.default_rng(1).normal(size=(8, 4)))
    lnp = lnprob(native, cat, plan, pos)
    bad = dict(plan, prior=(plan["prior"][0], plan["prior"][1], np.array([1.0, 0.0, 1.0, 1.0])))       # scale = 0
    numbers = native.chain_numbers(1, 0, 2, 0, 8, 4, squeeze=True)
    p, l = pos.copy(), lnp.copy()
    for call in (lambda: cat.stretch_move(bad, p, l, *numbers), lambda: cat.stretch_move_seeded(bad, p, l, 1, 0, 2),
                 lambda: cat.hmc_block(bad, chol, 0.5, 2, p, l, 1, 0, 2)):
        with pytest.raises(native.NativeError, match="status -1"):
            call()
        assert np.array_equal(p, pos) and np.array_equal(l, lnp)
    short = dict(plan, prior=tuple(a[:3] for a in plan["prior"]))                                         # n_dim differs
    with pytest.raises(native.NativeError, match="status -1"):
        cat.stretch_move_seeded(short, p, l, 1, 0, 2)
    # a walker that starts on a log-normal coordinate <= 0 (the box allows it): MCD_ERR_NONFINITE from the HMC block
    wide = dict(plan, lo=np.array([-np.inf, -5.0, -np.inf, -np.inf]))
    p[3, 1] = 0.0
    for resident in (True, False):
        cat.set_option("device_chain", int(resident))
        with pytest.raises(native.NativeError, match="status -5"):
            cat.hmc_block(wide, chol, 0.5, 2, p, l, 1, 0, 2)
    cat.set_option("device_chain", 1)


# ------------------------------------------------------------------------------------------ Runner: gradient
def _constant_fit(n, seed=13, free=("v_sys", "v_maxx", "v_maxy"), sigma=10.0):
    from mcmc_dynamics_amd import DataReader
    from mcmc_dynamics_amd.analysis import ConstantFit
    cat = synthetic.make_catalog(n, config=2)
    cols = {k: cat[k] for k in ("ra", "dec", "v", "verr")}
    fit = ConstantFit(DataReader(cols), seed=seed)
    fit.parameters["ra_center"].set(value=CENTRE[0], fixed=True)
    fit.parameters["dec_center"].set(value=CENTRE[1], fixed=True)
    for name in ("v_sys", "sigma_max", "v_maxx", "v_maxy"):
        if name not in free:
            fit.parameters[name].set(value=sigma if name == "sigma_max" else cat["truth"][name], fixed=True)
    return fit, cols, cat["truth"]


def test_gradient_with_priors_is_the_gradient_plus_the_prior(native):
    """lnprob_grad_batch with priors minus the same call without: the prior alone.  The sum value + prior is ONE float64
    addition, so the two calls differ by the library's prior (mcd_prior_eval) bit for bit; that prior meets the CPU bound
    against the longdouble form; and the difference itself carries, on top of it, the one rounding of the sum (2^-53 of
    the sum: the subtraction that isolates the prior cannot give back what the addition rounded away)."""
    fit, cols, truth = _constant_fit(2000, free=("v_sys", "sigma_max", "v_maxx", "v_maxy"))
    rng = np.random.default_rng(2)
    x = np.array([truth["v_sys"], truth["sigma_max"], truth["v_maxx"], truth["v_maxy"]]) + rng.normal(size=(65, 4)) * [0.5, 0.4, 0.7, 0.7]
    v0, g0 = fit.lnprob_grad_batch(x)
    fit.parameters["v_sys"].set(prior=("normal", 0.4, 0.6))
    fit.parameters["sigma_max"].set(prior=("lognormal", np.log(9.0), 0.2))
    fit.parameters["v_maxy"].set(prior=("normal", -1.0, 3.0))
    prior = fit._plan().prior
    assert prior is not None and list(prior[0]) == [1, 2, 0, 1]
    v1, g1 = fit.lnprob_grad_batch(x)
    lp, glp = native.prior_eval(prior, x, want_grad=True)
    assert v1.tobytes() == (v0 + lp).tobytes() and g1.tobytes() == (g0 + glp).tobytes()
    assert np.array_equal(fit.lnprob_batch(x), fit.lnlike_batch(x) + lp)
    xl = x.astype(L)
    bound_v, bound_g = np.zeros(65, dtype=L), np.zeros((65, 4), dtype=L)
    exact_v, exact_g = np.zeros(65, dtype=L), np.zeros((65, 4), dtype=L)
    for c, k in enumerate(prior[0]):
        if k == 0:
            continue
        s, u = L(prior[2][c]), (np.log(xl[:, c]) if k == 2 else xl[:, c])
        t, l = (u - L(prior[1][c])) / s, (u if k == 2 else 0 * u)
        c0 = -np.log(s) - ph.HALF_LOG_2PI
        exact_v += c0 - l - t * t / 2
        exact_g[:, c] = -t / s if k == 1 else -(1 + t / s) / xl[:, c]
        bound_v += 2.0 ** -52 * (np.abs(c0) + np.abs(l) + t * t / 2) + 3 * 2.0 ** -53 * np.abs(l) * (1 + np.abs(t) / s)
        size = np.abs(t) / s if k == 1 else (1 + np.abs(t) / s) / xl[:, c]
        bound_g[:, c] = 8 * 2.0 ** -53 * size + (3 * 2.0 ** -53 * np.abs(l) / (s * s * xl[:, c]) if k == 2 else 0)
    bound_v += 2 * 2.0 ** -53 * np.abs(exact_v)                         # (the sum over three coordinates: two more additions)
    assert np.all(np.abs(lp - exact_v) <= bound_v) and np.all(np.abs(glp - exact_g) <= bound_g)
    assert np.all(np.abs((v1 - v0) - exact_v) <= bound_v + 2.0 ** -53 * np.abs(v1))
    assert np.all(np.abs((g1 - g0) - exact_g) <= bound_g + 2.0 ** -53 * np.abs(g1))
    # outside the support of the log-normal prior: (-inf, zero row), the other rows untouched
    y = x.copy()
    y[7, 1] = 0.0
    v2, g2 = fit.lnprob_grad_batch(y)
    assert np.isneginf(v2[7]) and np.all(g2[7] == 0.0) and np.array_equal(np.delete(v2, 7), np.delete(v1, 7))
    fit.close()


# ------------------------------------------------------------------------------------------ end to end: conjugate
def _deviations(chain, mean, var):
    """chain (W, steps, P) -> |estimate - truth| / SE of the P means and P variances; SE from batch means over walkers."""
    d = chain - mean
    out = []
    for stat, truth in ((d, np.zeros_like(mean)), (d * d, var)):
        per_walker = stat.mean(axis=1)
        est, se = per_walker.mean(axis=0), per_walker.std(axis=0, ddof=1) / np.sqrt(per_walker.shape[0])
        out.append(np.abs(est - truth) / se)
    return np.concatenate(out)


def _within_cap(dev):
    return np.count_nonzero(dev > 4.0) <= 1 and not np.any(dev > 5.0)


CONJUGATE_SEED = 13


def test_conjugate_posterior(native):
    """ConstantFit, centre and sigma_max fixed, N = 200: the likelihood is Gaussian in (v_sys, v_maxx, v_maxy), and with
    normal priors so is the posterior -- precision A = sum a_i a_i^T / n_i + diag(1 / s^2), a_i = (1, sin theta_i,
    -cos theta_i), n_i = sigma^2 + verr_i^2, mean A^-1 (sum a_i v_i / n_i + loc / s^2).  Every prior is as wide as the
    data's own constraint and sits 5 of those widths off the data's estimate."""
    from oracle import lnprob_numpy as oracle
    sigma = 10.0
    fit, cols, truth = _constant_fit(200, seed=CONJUGATE_SEED, sigma=sigma)
    sin_t, cos_t = oracle.star_geometry_fixed(cols["ra"], cols["dec"], *CENTRE)
    a = np.stack([np.ones(200), sin_t, -cos_t], axis=1).astype(L)
    n_i = (L(sigma) ** 2 + cols["verr"].astype(L) ** 2)
    a_data = (a / n_i[:, None]).T @ a
    b_data = (a / n_i[:, None]).T @ cols["v"].astype(L)
    cov_data = np.linalg.inv(a_data.astype(np.float64))
    mean_data, width = cov_data @ b_data.astype(np.float64), np.sqrt(np.diag(cov_data))
    loc, s = mean_data + 5.0 * width, width
    for j, name in enumerate(("v_sys", "v_maxx", "v_maxy")):
        fit.parameters[name].set(min=mean_data[j] - 40 * width[j], max=mean_data[j] + 40 * width[j],
                                 prior=("normal", float(loc[j]), float(s[j])))
    prec = a_data.astype(np.float64) + np.diag(1.0 / s ** 2)
    cov = np.linalg.inv(prec)
    mean = cov @ (b_data.astype(np.float64) + loc / s ** 2)
    sd = np.sqrt(np.diag(cov))
    assert np.all(np.abs(mean - mean_data) > 3 * sd)                   # a build that ignores the prior fails everything below
    res = fit.maximize()
    print("MAP - mean in posterior widths:", (res["x"] - mean) / sd)
    assert res["converged"] and np.all(np.abs(res["x"] - mean) <= 1e-6 * sd)
    lap = fit.laplace(res["x"], rel_step=1e-4)
    rel = np.abs(lap["covariance"] - cov) / np.sqrt(np.outer(np.diag(cov), np.diag(cov)))
    print("Laplace covariance, largest relative difference:", rel.max())
    assert rel.max() <= 1e-5
    # the seed's own draw of the same size meets the cap
    rng = np.random.default_rng(CONJUGATE_SEED)
    draw = mean + rng.normal(size=(64, 800, 3)) @ np.linalg.cholesky(cov).T
    assert _within_cap(_deviations(draw, mean, np.diag(cov)))
    fit.SAMPLER = "resident"
    start = mean + rng.normal(size=(64, 3)) @ np.linalg.cholesky(cov).T
    sampler = fit(n_walkers=64, n_steps=1200, pos=start, prefix=None)
    info = fit._catalog.stretch_info()
    assert info["device_blocks"] > 0 and info["discarded_blocks"] == 0 and info["host_blocks"] == 0, info
    dev = _deviations(np.asarray(sampler.chain)[:, 400:], mean, np.diag(cov))
    print("resident stretch move: deviations / SE", dev)
    assert _within_cap(dev), dev
    hmc = fit.hmc(64, 300, seed=CONJUGATE_SEED)
    assert fit._catalog.hmc_info()["device_blocks"] > 0 and fit._catalog.hmc_info()["host_blocks"] == 0
    dev = _deviations(np.asarray(hmc.chain), mean, np.diag(cov))
    print("hmc: deviations / SE", dev, "acceptance", hmc.acceptance_fraction.mean())
    assert _within_cap(dev), dev
    fit.close()


# ------------------------------------------------------------------------------------------ end to end: log-normal
def test_lognormal_posterior_against_quadrature(native):
    """Free (v_sys, sigma_max), a log-normal prior on sigma_max that pulls it below the data's value: the posterior mean
    of sigma_max from the resident chain against 2-D quadrature of the NumPy oracle plus scipy's lognorm.logpdf."""
    from scipy import stats
    from oracle import lnprob_numpy as oracle
    fit, cols, truth = _constant_fit(200, seed=21, free=("v_sys", "sigma_max"))
    mu, s = np.log(7.0), 0.05
    fit.parameters["sigma_max"].set(min=0.0, max=30.0, prior=("lognormal", mu, s))
    fit.parameters["v_sys"].set(min=-20.0, max=20.0)
    fixed = [truth["v_maxx"], truth["v_maxy"]]

    def moments(n_grid):
        v = np.linspace(-6.0, 6.0, n_grid)
        sg = np.linspace(4.0, 12.0, n_grid)
        vv, ss = np.meshgrid(v, sg, indexing="ij")
        rows = np.stack([vv.ravel(), ss.ravel(), np.full(vv.size, fixed[0]), np.full(vv.size, fixed[1])], axis=1)
        lnp = oracle.batched_constant_lnlike(cols, rows, *CENTRE) + stats.lognorm.logpdf(rows[:, 1], s, scale=np.exp(mu))
        wgt = np.exp(lnp - lnp.max()).reshape(n_grid, n_grid)
        edge = max(wgt[0].max(), wgt[-1].max(), wgt[:, 0].max(), wgt[:, -1].max())
        return float((wgt * ss).sum() / wgt.sum()), edge
    want, edge = moments(161)
    coarse, _ = moments(81)
    assert edge < 1e-12                                                # the grid holds the posterior
    fit.SAMPLER = "resident"
    rng = np.random.default_rng(21)
    start = np.stack([rng.normal(0.0, 0.5, 64), want * np.exp(0.03 * rng.normal(size=64))], axis=1)
    sampler = fit(n_walkers=64, n_steps=1200, pos=start, prefix=None)
    info = fit._catalog.stretch_info()
    assert info["device_blocks"] > 0 and info["host_blocks"] == 0, info
    per_walker = np.asarray(sampler.chain)[:, 400:, 1].mean(axis=1)
    est, se = per_walker.mean(), per_walker.std(ddof=1) / np.sqrt(64)
    print("sigma_max: chain", est, "+-", se, " quadrature", want, " (half the grid:", coarse, ")")
    assert abs(coarse - want) < 0.05 * se                              # the grid has converged far below the chain's error
    assert abs(est - want) <= 5 * se
    # the prior matters: the data alone put sigma_max near its true value of 10, many standard errors away
    assert abs(truth["sigma_max"] - want) > 20 * se
    fit.close()

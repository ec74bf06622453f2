"""GPU: mcd_hmc_block (csrc/mcd_hmc.hip, csrc/mcd_api_chain.hip) -- the block resident on the device against the
host-driven loop around mcd_loglike_grad_batch (bit for bit), the device gradient's trajectory against a NumPy restatement
(tests/grad_helper.py), continuation, the box, the refusals, and Runner.hmc end to end against the stretch move.

Catalogues: mcmc_dynamics_amd/synthetic.py.  Shapes: N in {33, 4099} x W in {1, 65, 257} (a lone lane, a ragged second
tile, a partial fifth tile) x n_leap in {1, 3}."""
import numpy as np
import pytest

import grad_helper as gh
import variant_helper as vh
from mcmc_dynamics_amd import synthetic

pytestmark = pytest.mark.gpu

CENTRE = (synthetic.CENTER_RA_DEG, synthetic.CENTER_DEC_DEG)
T = synthetic.TRUTH
MODELS = ("const", "bgfixed", "profile_gb_free")


@pytest.fixture(scope="module")
def native():
    from mcmc_dynamics_amd import _native
    return _native


@pytest.fixture(scope="module")
def ctx(native):
    return native.default_context()


def gaussian_lnl(v, verr, mean, sigma):
    n = sigma * sigma + verr * verr
    return -0.5 * np.log(2.0 * np.pi * n) - 0.5 * (v - mean) ** 2 / n


def columns(n, background=True):
    return synthetic.make_catalog(n, config=2, background=background)


def setup(kind, n):
    """(catalogue keyword arguments, plan, truth row in free parameters, posterior scale per free parameter, dense?)
    The catalogue of the model without a background has no background stars: its truth is then close to the mode."""
    c = columns(n, background=kind != "const")
    t = c["truth"]
    base = dict(ra=c["ra"], dec=c["dec"], v=c["v"], verr=c["verr"])
    s = 10.0 / np.sqrt(n)                                      # the scale of v_sys: sigma / sqrt(N)
    inf = np.inf
    if kind == "const":
        # every column free: v_sys, sigma_max, v_maxx, v_maxy
        plan = {"col_source": np.arange(4, dtype=np.int32), "col_const": np.zeros(4), "col_factor": np.ones(4),
                "lo": np.array([-inf, 0.0, -inf, -inf]), "hi": np.full(4, inf), "fixed_ok": True}
        x = np.array([t["v_sys"], t["sigma_max"], t["v_maxx"], t["v_maxy"]])
        return dict(base, model=0, centre=CENTRE), plan, x, np.array([s, 0.7 * s, 1.4 * s, 1.4 * s]), False
    if kind == "bgfixed":
        # v_sys fixed (a constant column), v_maxx sampled in units of 2 km/s (a unit factor)
        plan = {"col_source": np.array([-1, 0, 1, 2], dtype=np.int32), "col_const": np.array([0.5, 0.0, 0.0, 0.0]),
                "col_factor": np.array([1.0, 1.0, 2.0, 1.0]), "lo": np.array([0.0, -inf, -inf]), "hi": np.full(3, inf),
                "fixed_ok": True}
        kw = dict(base, model=1, centre=CENTRE, lnlike_bg=gaussian_lnl(c["v"], c["verr"], 20.0, 40.0), pmember=c["pmember"])
        x = np.array([t["sigma_max"], 0.5 * t["v_maxx"], t["v_maxy"]])
        return kw, plan, x, np.array([0.8 * s, 0.8 * s, 1.6 * s]), False
    # PROFILE_BGGAUSS with a free centre, K = 11: v_sys, sigma_max, a, v_maxx, v_maxy, r_peak, ra, dec, v_back, sigma_back, f_back
    plan = {"col_source": np.arange(11, dtype=np.int32), "col_const": np.zeros(11), "col_factor": np.ones(11),
            "lo": np.array([-inf, 0.0, 1.0, -inf, -inf, 1.0, CENTRE[0] - 0.05, CENTRE[1] - 0.05, -inf, 0.0, 0.0]),
            "hi": np.array([inf, inf, 600.0, inf, inf, 600.0, CENTRE[0] + 0.05, CENTRE[1] + 0.05, inf, inf, 1.0]),
            "fixed_ok": True}
    x = np.array([t["v_sys"], t["sigma_max"], 120.0, t["v_maxx"], t["v_maxy"], 60.0, CENTRE[0], CENTRE[1], t["v_back"],
                  t["sigma_back"], t["f_back"]])
    scale = np.array([s, s, 100.0 * s, 2 * s, 2 * s, 60.0 * s, 0.02 * s, 0.02 * s, 10 * s, 8 * s, 0.05 * s])
    return dict(base, model=4, centre=None, density=c["density"]), plan, x, scale, True


_CASES = {}


def case(native, ctx, kind, n):
    """One catalogue per (model, N) for the whole module."""
    if (kind, n) not in _CASES:
        kw, plan, x, scale, dense = setup(kind, n)
        cat = native.Catalog(ctx, kw.pop("ra"), kw.pop("dec"), kw.pop("v"), kw.pop("verr"), **kw)
        p = x.size
        chol = np.diag(scale)
        if dense:                                              # a dense metric: leaving the box ends the trajectory
            chol = chol @ (np.eye(p) + 0.2 * np.tril(np.ones((p, p)), -1) / p)
        _CASES[(kind, n)] = (cat, plan, x, scale, chol)
    return _CASES[(kind, n)]


def start(x, scale, plan, w, seed=5):
    pos = x + 0.5 * scale * np.random.default_rng(seed).normal(size=(w, x.size))
    return np.ascontiguousarray(np.clip(pos, plan["lo"], plan["hi"]))


def run(cat, plan, chol, eps, n_leap, pos, seed, step0, n_steps, resident, jitter=0.1):
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
    out["device_blocks"] = after["device_blocks"] - before["device_blocks"]
    out["host_blocks"] = after["host_blocks"] - before["host_blocks"]
    cat.set_option("device_chain", 1)
    return out


KEYS = ("chain", "lnprob_chain", "accepted", "energy_error", "pos", "lnp")


# ------------------------------------------------------------------------------------------ resident == host-driven
@pytest.mark.parametrize("n_leap", [1, 3])
@pytest.mark.parametrize("w", [1, 65, 257])
@pytest.mark.parametrize("n", [33, 4099])
@pytest.mark.parametrize("kind", MODELS)
def test_resident_block_is_the_host_driven_block(native, ctx, kind, n, w, n_leap):
    cat, plan, x, scale, chol = case(native, ctx, kind, n)
    pos = start(x, scale, plan, w)
    dev = run(cat, plan, chol, 0.6, n_leap, pos, 31, 2, 4, resident=True)
    host = run(cat, plan, chol, 0.6, n_leap, pos, 31, 2, 4, resident=False)
    assert (dev["device_blocks"], dev["host_blocks"]) == (1, 0)
    assert (host["device_blocks"], host["host_blocks"]) == (0, 1)
    for key in KEYS:
        assert dev[key].tobytes() == host[key].tobytes(), (key, kind, n, w, n_leap)
    # not a trivial agreement: the chains moved, the values are the positions' log-likelihoods
    assert np.all(np.isfinite(dev["chain"])) and np.all(np.isfinite(dev["lnprob_chain"]))
    if w > 1:
        assert dev["accepted"].sum() > 0 and not np.array_equal(dev["pos"], pos)
    assert np.array_equal(dev["chain"][-1], dev["pos"]) and np.array_equal(dev["lnprob_chain"][-1], dev["lnp"])
    table = np.stack([dev["pos"][:, s] * plan["col_factor"][j] if s >= 0 else np.full(w, plan["col_const"][j])
                      for j, s in enumerate(plan["col_source"])], axis=1)
    value, _ = cat.loglike_grad(np.ascontiguousarray(table))
    assert value.tobytes() == dev["lnp"].tobytes()


# ------------------------------------------------------------------------------------------ the gradient drives the chain
def numpy_step(cat_cols, plan, chol, eps, n_leap, pos, z, r, jitter):
    """One HMC step of every walker of a CONST catalogue, restated in NumPy (80-bit where the platform has it) on the
    test-side value and gradient: returns the signed H1 - H0 per walker.  Identity column map, no bound met."""
    L = vh.L
    diag = np.diag(chol).copy()
    assert np.count_nonzero(chol - np.diag(diag)) == 0
    chol = chol.astype(L)
    minv = chol @ chol.T
    out = np.empty(pos.shape[0], dtype=L)
    for w in range(pos.shape[0]):
        q = pos[w].astype(L)
        p = (z[w] / diag).astype(L)                              # L^-T z of a diagonal L, the library's own division
        e = L(eps) * (L(1) + L(jitter) * L(r[w]))
        y = chol.T @ p
        h0 = -vh.exact(0, cat_cols, q, CENTRE) + L(0.5) * (y @ y)
        g, _ = gh.grad(0, cat_cols, q, CENTRE, L)
        p = p + L(0.5) * e * g
        for leap in range(1, n_leap + 1):
            q = q + e * (minv @ p)
            assert np.all(q >= plan["lo"]) and np.all(q <= plan["hi"])
            g, _ = gh.grad(0, cat_cols, q, CENTRE, L)
            p = p + (e if leap < n_leap else L(0.5) * e) * g
        y = chol.T @ p
        out[w] = (-vh.exact(0, cat_cols, q, CENTRE) + L(0.5) * (y @ y)) - h0
    return out


DRIVE = {"eps": 1.2, "n_leap": 2, "spread": 10.0, "seed": 17, "jitter": 0.1}


def drive_inputs():
    c = columns(4099, background=False)
    cols = {k: c[k] for k in ("ra", "dec", "v", "verr")}
    _, plan, x, scale, _ = setup("const", 4099)
    rng = np.random.default_rng(3)
    pos = np.ascontiguousarray(x + DRIVE["spread"] * scale * rng.choice([-1.0, 1.0], size=(65, 4)) *
                               rng.uniform(0.8, 1.2, size=(65, 4)))
    return cols, plan, scale, pos


def test_energy_error_is_the_numpy_gradients_energy_error(native, ctx):
    """CONST, N = 4099, W = 65, one step.  The walkers start ~10 posterior widths from the mode and take two leapfrog
    points of 1.2 widths, so that every |dH| is of order 1 or more (the NumPy side gives 2.7 .. 78, median 38): dH is a
    difference of two H ~ 1.5e4 whose float64 sums carry ~1e-11 absolute, and the bound is 1e-9 RELATIVE to dH itself."""
    cat, plan, x, scale, chol = case(native, ctx, "const", 4099)
    cols, plan, scale, pos = drive_inputs()
    chol = np.diag(scale)
    z, thr, r = native.hmc_numbers(DRIVE["seed"], 0, 1, 65, 4)
    want = numpy_step(cols, plan, chol, DRIVE["eps"], DRIVE["n_leap"], pos, z[0], r[0], DRIVE["jitter"])
    got = run(cat, plan, chol, DRIVE["eps"], DRIVE["n_leap"], pos, DRIVE["seed"], 0, 1, resident=True, jitter=DRIVE["jitter"])
    want_abs = np.abs(want).astype(np.float64)
    err = np.abs(got["energy_error"][0] - want_abs) / want_abs
    print("min / median |dH| (NumPy):", want_abs.min(), np.median(want_abs), " largest relative difference:", err.max())
    assert want_abs.min() > 0.1, "the configuration is meant to keep every |dH| away from 0"
    assert np.all(err <= 1e-9), (err.max(), int(np.argmax(err)))
    # the accept decisions follow from those numbers
    accept = thr[0] < -want.astype(np.float64)
    sure = np.abs(thr[0] + want.astype(np.float64)) > 1e-6
    assert np.array_equal(got["accepted"][sure] == 1, accept[sure])


def test_energy_error_falls_fourfold_when_the_step_is_halved(native, ctx):
    """The same trajectory length with twice the points of half the size: the leapfrog's second order, on the device
    gradient of a (nearly Gaussian) 4099-star posterior."""
    cat, plan, x, scale, chol = case(native, ctx, "const", 4099)
    chol = np.diag(scale)
    pos = start(x, scale, plan, 65, seed=9)
    a = run(cat, plan, chol, 0.4, 2, pos, 23, 0, 1, resident=True, jitter=0.0)
    b = run(cat, plan, chol, 0.2, 4, pos, 23, 0, 1, resident=True, jitter=0.0)
    ea, eb = np.median(a["energy_error"][0]), np.median(b["energy_error"][0])
    print("median |dH|:", ea, eb, "ratio", ea / eb)
    assert np.isfinite(ea) and eb > 0 and 3.0 <= ea / eb <= 5.0


# ------------------------------------------------------------------------------------------ continuation, bounds, refusals
@pytest.mark.parametrize("kind", ["const", "profile_gb_free"])
def test_blocks_continue_each_other_on_the_device(native, ctx, kind):
    cat, plan, x, scale, chol = case(native, ctx, kind, 4099)
    pos = start(x, scale, plan, 65)
    whole = run(cat, plan, chol, 0.6, 3, pos, 8, 5, 6, resident=True)
    first = run(cat, plan, chol, 0.6, 3, pos, 8, 5, 3, resident=True)
    second = run(cat, plan, chol, 0.6, 3, first["pos"], 8, 8, 3, resident=True)
    assert whole["device_blocks"] == first["device_blocks"] == second["device_blocks"] == 1
    for key in ("chain", "lnprob_chain", "energy_error"):
        assert np.concatenate([first[key], second[key]]).tobytes() == whole[key].tobytes(), key
    assert np.array_equal(first["accepted"] + second["accepted"], whole["accepted"])
    assert second["pos"].tobytes() == whole["pos"].tobytes() and second["lnp"].tobytes() == whole["lnp"].tobytes()


@pytest.mark.parametrize("dense", [False, True])
def test_every_chain_row_is_inside_a_tight_box(native, ctx, dense):
    """Diagonal metric: a box of +-0.7 widths and trajectories of 2.4 widths, every one of which meets a wall and is
    reflected.  Dense metric: a box of +-1.5 widths and trajectories of one width, about half of which leave the box and
    are rejected (the same geometry on a unit Gaussian, host build: 46 % end early, 205 of 390 proposals accepted)."""
    cat, plan, x, scale, _ = case(native, ctx, "const", 4099)
    half, eps, n_leap = (1.5, 0.5, 2) if dense else (0.7, 0.8, 3)
    tight = dict(plan, lo=x - half * scale, hi=x + half * scale)
    chol = np.diag(scale)
    if dense:
        chol = chol @ (np.eye(4) + 0.1 * np.tril(np.ones((4, 4)), -1))
    pos = np.ascontiguousarray(np.clip(start(x, scale, plan, 65), tight["lo"], tight["hi"]))
    out = run(cat, tight, chol, eps, n_leap, pos, 4, 0, 6, resident=True)
    c = out["chain"]
    assert np.all(c >= tight["lo"]) and np.all(c <= tight["hi"])
    ended = np.isinf(out["energy_error"])
    print("dense" if dense else "diagonal", "ended early:", float(ended.mean()), "accepted:", int(out["accepted"].sum()))
    if dense:
        assert ended.any() and out["accepted"].sum() > 0                # left the box: rejected; the others move
        assert np.all(c[0][ended[0]] == pos[ended[0]])
    else:
        assert not ended.any() and out["accepted"].mean() / 6 > 0.5      # reflected: nothing is lost at the walls
    host = run(cat, tight, chol, eps, n_leap, pos, 4, 0, 6, resident=False)
    assert host["chain"].tobytes() == c.tobytes()


def test_fixed_parameter_outside_its_bounds_and_a_start_outside_the_box(native, ctx):
    cat, plan, x, scale, chol = case(native, ctx, "const", 33)
    pos = start(x, scale, plan, 65)
    out = run(cat, dict(plan, fixed_ok=False), chol, 0.6, 2, pos, 1, 0, 3, resident=True)
    assert out["accepted"].sum() == 0 and np.all(out["chain"] == pos[None]) and out["device_blocks"] == 1
    bad = pos.copy()
    bad[7, 1] = -1.0                                                    # sigma_max below its bound
    for resident in (True, False):
        with pytest.raises(native.NativeError, match="status -5"):
            run(cat, plan, chol, 0.6, 2, bad, 1, 0, 3, resident=resident)


def test_binned_and_float32_catalogues_are_refused(native, ctx):
    kw, plan, x, scale, _ = setup("const", 33)
    cols = [kw.pop(k) for k in ("ra", "dec", "v", "verr")]
    pos = start(x, scale, plan, 8)
    for more in ({"bin_offsets": np.array([0, 10, 33], dtype=np.int64)}, {"precision": "f32"}):
        cat = native.Catalog(ctx, *cols, **dict(kw, **more))
        for resident in (1, 0):
            cat.set_option("device_chain", resident)
            p, lnp = pos.copy(), np.full(8, np.nan)
            with pytest.raises(native.NativeError, match="status -1"):
                cat.hmc_block(plan, np.diag(scale), 0.5, 2, p, lnp, 1, 0, 2)
            assert np.array_equal(p, pos) and np.all(np.isnan(lnp))
        assert cat.hmc_info() == {"device_blocks": 0, "host_blocks": 0}
        cat.close()


# ------------------------------------------------------------------------------------------ end to end
def walker_means(chain):
    """chain (W, steps, P) -> (mean, standard error) per parameter from the walkers' time averages (batch means)."""
    per_walker = chain.mean(axis=1)
    return per_walker.mean(axis=0), per_walker.std(axis=0, ddof=1) / np.sqrt(chain.shape[0])


def test_runner_hmc_against_the_stretch_move():
    """ConstantFit on 2 000 synthetic stars: the posterior means of Runner.hmc (64 chains, 200 steps) and of the sampler
    Runner.__call__ drives by default agree within 5 combined Monte-Carlo standard errors; so do two runs of that sampler
    with different seeds (the criterion is met by existing code alone).  z-scores observed: DESIGN 3.10."""
    from mcmc_dynamics_amd import DataReader
    from mcmc_dynamics_amd.analysis import ConstantFit
    cat = synthetic.make_catalog(2000, config=2)
    fit = ConstantFit(DataReader({k: cat[k] for k in ("ra", "dec", "v", "verr")}), seed=13)
    fit.parameters["ra_center"].set(value=CENTRE[0], fixed=True)
    fit.parameters["dec_center"].set(value=CENTRE[1], fixed=True)
    np.random.seed(101)
    hmc = fit.hmc(n_walkers=64, n_steps=200, seed=2024)
    acc = float(hmc.acceptance_fraction.mean())
    print("HMC acceptance", acc, "step size", hmc.step_size, "median |dH|", float(np.median(hmc.energy_error)))
    assert hmc.chain.shape == (64, 200, 4) and 0.5 <= acc <= 0.99
    m_hmc, se_hmc = walker_means(hmc.chain)
    stretch = []
    for seed in (7, 8):
        np.random.seed(seed)
        pos = fit.get_initials_laplace(64, m_hmc, np.cov(hmc.flatchain.T))
        s = fit(n_walkers=64, n_steps=1200, pos=pos, prefix=None)
        stretch.append(walker_means(np.asarray(s.chain)[:, 400:]))
    (m_a, se_a), (m_b, se_b) = stretch
    z_self = (m_a - m_b) / np.hypot(se_a, se_b)
    z_hmc = (m_hmc - m_a) / np.hypot(se_hmc, se_a)
    print("z stretch vs stretch", z_self, " z HMC vs stretch", z_hmc)
    assert np.all(np.abs(z_self) < 5.0)
    assert np.all(np.abs(z_hmc) < 5.0)

"""GPU: mcd_pointwise_posterior -- per-star summaries over posterior samples (lppd and the variance of lnL for WAIC, the
posterior mean and spread of the membership probability) -- against NumPy reductions of the per-row outputs the library
already had (Catalog.loglike_per_star / Catalog.membership, the oracle's per-star lnL for the models without a background),
against the reference-pinned lnlike for one sample, and through the Runner methods (pointwise_posterior, waic,
posterior_membership_probabilities)."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import emul_helper as emul
import posterior_helper as ph
from conftest import ROOT, load_golden
from test_posterior_cpu import BG_MODELS, rel, var_ok

pytestmark = pytest.mark.gpu
MODELS = [0, 1, 2, 3, 4, 5, 6]


def _catalog(ctx, cat, model, centre, precision="f64"):
    from mcmc_dynamics_amd import _native
    extra = {}
    bg = emul.BG_OF[model]
    if bg == 1:
        extra = {"lnlike_bg": cat["lnlike_bg"], "pmember": cat["pmember"]}
    elif bg == 2:
        extra = {"density": cat["density"]}
    elif bg == 3:
        extra = {"lnlike_bg": cat["lnlike_bg"], "density": cat["density"]}
    return _native.Catalog(ctx, cat["ra"], cat["dec"], cat["v"], cat["verr"], model=model, centre=centre,
                           precision=precision, **extra)


def _host_loop(gpu, cat, table, model, centre):
    """The per-sample route that existed before: one call per sample, reduced on the host.  The models without a
    background have no per-star entry of their own: their lnL_is comes from the fixed-background twin of the model
    (CONST -> CONST_BGFIXED, PROFILE -> PROFILE_BGFIXED) with pmember = 1 and a background of -1e5, whose mixture is then
    exactly the cluster term, on records prepared by the same device code."""
    if model in BG_MODELS:
        x = np.array([gpu.loglike_per_star(row) for row in table])
        p = np.array([gpu.membership(row) for row in table])
    else:
        twin = dict(cat, pmember=np.ones(len(cat["v"])), lnlike_bg=np.full(len(cat["v"]), -1e5))
        tw = _catalog(gpu.ctx, twin, 1 if model == 0 else 6, centre)
        x = np.array([tw.loglike_per_star(row) for row in table])
        tw.close()
        p = None
    S = x.shape[0]
    mx = x.max(axis=0)
    out = {"lppd": mx + np.log(np.exp(x - mx).sum(axis=0)) - np.log(S), "lnl_var": x.var(axis=0, ddof=1)}
    if p is not None:
        out["pmem_mean"], out["pmem_std"] = p.mean(axis=0), p.std(axis=0, ddof=1)
    return out


@pytest.fixture(scope="module")
def ctx():
    from mcmc_dynamics_amd import _native
    return _native.default_context()


@pytest.fixture(scope="module")
def cat5k():
    return ph.model_catalog(5000, 0)


@pytest.mark.parametrize("model", MODELS)
@pytest.mark.parametrize("free", [False, True])
def test_device_summaries_match_the_per_row_outputs(ctx, cat5k, model, free):
    centre = None if free else ph.CENTRE
    table = ph.samples(cat5k, model, free, 300)
    gpu = _catalog(ctx, cat5k, model, centre)
    mem = model in BG_MODELS
    got = gpu.pointwise_posterior(table, membership=mem)
    want = _host_loop(gpu, cat5k, table, model, centre)
    assert rel(got["lppd"], want["lppd"]) < 1e-12
    assert var_ok(got["lnl_var"], want["lnl_var"], want["lppd"], rtol=1e-10)
    if mem:
        assert np.max(np.abs(got["pmem_mean"] - want["pmem_mean"])) < 1e-12
        assert np.max(np.abs(got["pmem_std"] - want["pmem_std"])) < 1e-10
    # the oracle's per-star functions and the host build of csrc/mcd_posterior.h, on records whose geometry NumPy
    # computed: the fixed-centre offsets of calc_xy_offset.py:31 subtract two O(0.4) products, so one ulp of the device's
    # sin / cos against NumPy's moves a star's lnL by up to ~3e-12 of itself
    tol = 1e-11 if not free else 1e-12
    assert rel(got["lppd"], ph.numpy_posterior(cat5k, table, model, centre)["lppd"]) < tol
    assert rel(got["lppd"], ph.posterior(cat5k, table, model, centre, mem)["lppd"]) < tol
    gpu.close()


@pytest.mark.parametrize("model,precision", [(0, "f32acc64"), (2, "f32acc64"), (4, "f32"), (5, "f32")])
def test_float32_catalogues(ctx, cat5k, model, precision):
    """float32 terms, float64 accumulation: within the per-term float32 tolerance of DESIGN.md section 5 (2e-5)."""
    table = ph.samples(cat5k, model, False, 200)
    mem = model in BG_MODELS
    g32 = _catalog(ctx, cat5k, model, ph.CENTRE, precision)
    g64 = _catalog(ctx, cat5k, model, ph.CENTRE)
    a, b = g32.pointwise_posterior(table, membership=mem), g64.pointwise_posterior(table, membership=mem)
    assert np.max(np.abs(a["lppd"] - b["lppd"]) / np.maximum(np.abs(b["lppd"]), 1.0)) < 2e-5
    if mem:
        assert np.max(np.abs(a["pmem_mean"] - b["pmem_mean"])) < 2e-5
    g32.close()
    g64.close()


@pytest.mark.parametrize("name,model,free", [
    ("constant_fixed", 0, False), ("constant_free", 0, True), ("constant_bg_gaussian_fixed", 1, False),
    ("constant_gb_fixed", 2, False), ("constant_gb_free", 2, True), ("model_fit_fixed", 3, False),
    ("model_fit_free", 3, True), ("model_fit_gb_fixed", 4, False), ("model_fit_cb_free", 5, True),
    ("model_fit_bg_gaussian_fixed", 6, False)])
def test_one_sample_sums_to_the_reference_lnlike(ctx, name, model, free):
    """S = 1: sum_i lppd_i is lnlike(row), the value pinned to the reference by the golden vectors."""
    g = load_golden(name)
    cat = {k: g[k] for k in ("ra", "dec", "v", "verr")}
    if model in (1, 6):
        cat["lnlike_bg"], cat["pmember"] = g["lnlike_background"], g["pmember"]
    if model in (2, 4, 5):
        cat["density"] = g["density"]
    if model == 5:
        cat["lnlike_bg"] = g["lnlike_background"]
    centre = None if free else (float(g["ra_center"]), float(g["dec_center"]))
    gpu = _catalog(ctx, cat, model, centre)
    values = emul.abi_columns(g["names"], g["values"], model, free)
    ok = np.flatnonzero(np.isfinite(g["lnprob"]))
    for r in ok[:4]:
        got = gpu.pointwise_posterior(values[r])
        assert np.all(got["lnl_var"] == 0.0)
        total = float(np.sum(got["lppd"]))
        assert abs(total - gpu.loglike(values[r:r + 1])[0]) < 1e-12 * abs(total)
        if "lnprior" not in g or g["lnprior"][r] == 0.0:
            assert abs(total - g["lnprob"][r]) < 1e-12 * abs(total)
    gpu.close()


def _gb_fit(cat):
    from mcmc_dynamics_amd import DataReader
    from mcmc_dynamics_amd.analysis import ConstantFitGB
    fit = ConstantFitGB(DataReader({k: cat[k] for k in ("ra", "dec", "v", "verr", "density")}))
    fit.parameters["ra_center"].set(value=ph.CENTRE[0], fixed=True)
    fit.parameters["dec_center"].set(value=ph.CENTRE[1], fixed=True)
    return fit


def test_a_chain_of_one_repeated_vector(cat5k):
    """Every sample the same: the posterior average is the point value, with zero spread and zero p_waic."""
    fit = _gb_fit(cat5k)
    vec = ph.samples(cat5k, 2, False, 1)[0]
    chain = np.tile(vec, (16, 12, 1))
    mean, std = fit.posterior_membership_probabilities(chain, n_burn=2)
    point = fit.membership_probabilities(vec)
    assert np.max(np.abs(mean - point)) < 1e-15 and np.all(std == 0.0)
    w = fit.waic(chain, n_burn=2)
    assert w["p_waic"] == 0.0 and w["n_samples"] == 160 and w["n_stars"] == 5000
    assert abs(w["lppd"] - fit.lnlike(vec)) < 1e-12 * abs(w["lppd"])
    assert w["waic"] == -2.0 * w["elpd_waic"] and w["elpd_waic"] == w["lppd"]
    fit.close()


def test_runner_methods_resolve_the_chain_like_lnprob_batch(cat5k):
    """Fixed parameters and thinning: the rows the Runner hands the kernel are those of convert_to_parameters."""
    fit = _gb_fit(cat5k)
    fit.parameters["sigma_back"].set(value=40.0, fixed=True)
    free = ph.samples(cat5k, 2, False, 8 * 20)
    names = ph.abi_names(2, False)
    keep = [names.index(n) for n in fit.fitted_parameters]
    chain = free[:, keep].reshape(8, 20, len(keep))
    pp = fit.pointwise_posterior(chain, n_burn=5, thin=3)
    flat = chain[:, 5::3, :].reshape(-1, len(keep))
    table = free.reshape(8, 20, -1)[:, 5::3, :].reshape(-1, len(names)).copy()
    table[:, names.index("sigma_back")] = 40.0
    want = fit._catalog.pointwise_posterior(table, membership=True)
    assert pp["n_samples"] == flat.shape[0] == 40
    for k in ("lppd", "lnl_var", "pmem_mean", "pmem_std"):
        assert np.array_equal(pp[k], want[k]), k
    fit.close()


@pytest.mark.parametrize("which", ["fixed", "free"])
def test_model_fit_gb_posterior_membership_on_the_reference_chain(which):
    """ModelFitGB on the reference's own chain and catalogue (model_fit_gb_membership_*): mean and sd over the post-burn-in
    samples of oracle.model_membership."""
    from mcmc_dynamics_amd import DataReader
    from mcmc_dynamics_amd.analysis import ModelFitGB
    g = load_golden("model_fit_gb_membership_" + which)
    cat = {k: g[k] for k in ("ra", "dec", "v", "verr", "density")}
    mg = ModelFitGB(DataReader(dict(cat)))
    centre = None
    if which == "fixed":
        centre = (float(g["ra_center"]), float(g["dec_center"]))
        mg.parameters["ra_center"].set(value=centre[0], fixed=True)
        mg.parameters["dec_center"].set(value=centre[1], fixed=True)
    n_burn = int(g["n_burn"])
    mean, std = mg.posterior_membership_probabilities(g["chain"], n_burn)
    flat = g["chain"][:, n_burn:, :].reshape(-1, g["chain"].shape[2])
    rows = emul.abi_columns(g["names"], flat, 4, which == "free")
    p = np.array([ph.star_terms(cat, row, 4, centre)[1] for row in rows])
    assert np.max(np.abs(mean - p.mean(axis=0))) < 1e-12
    assert np.max(np.abs(std - p.std(axis=0, ddof=1))) < 1e-12
    mg.close()


def test_bits_repeat_and_the_sliced_plan_matches_the_host_loop(ctx):
    """1e4 stars x 16 384 samples: the plan with many sample slices (small catalogue), two calls bit for bit, host-side
    passes (option posterior_pass) within the merge tolerance, and the per-sample host loop."""
    cat = ph.model_catalog(10000, 0, seed=9)
    table = ph.samples(cat, 2, False, 16384, seed=21)
    gpu = _catalog(ctx, cat, 2, ph.CENTRE)
    n_slices, _ = ph.plan(10000, 16384)
    assert n_slices > 8
    a = gpu.pointwise_posterior(table, membership=True)
    b = gpu.pointwise_posterior(table, membership=True)
    for k in a:
        assert np.array_equal(a[k], b[k]), k
    gpu.set_option("posterior_pass", 5000)
    c = gpu.pointwise_posterior(table, membership=True)
    gpu.set_option("posterior_pass", 65536)
    for k in a:
        scale = np.maximum(np.abs(a[k]), 1.0)
        assert np.max(np.abs(c[k] - a[k]) / scale) < 1e-13, k
    want = _host_loop(gpu, cat, table, 2, ph.CENTRE)
    assert rel(a["lppd"], want["lppd"]) < 1e-12
    assert var_ok(a["lnl_var"], want["lnl_var"], want["lppd"], rtol=1e-10)
    assert np.max(np.abs(a["pmem_mean"] - want["pmem_mean"])) < 1e-12
    gpu.close()


def test_refusals(ctx, cat5k):
    from mcmc_dynamics_amd import _native
    small = {k: (v[:200] if isinstance(v, np.ndarray) else v) for k, v in cat5k.items()}
    const = _catalog(ctx, small, 0, ph.CENTRE)
    gb = _catalog(ctx, small, 2, ph.CENTRE)
    lib = const.lib
    out = [np.empty(200) for _ in range(4)]
    ptr = [o.ctypes.data_as(ctypes.POINTER(ctypes.c_double)) for o in out]
    row = np.ascontiguousarray(ph.samples(small, 0, False, 3))
    rowp = row.ctypes.data_as(ctypes.POINTER(ctypes.c_double))
    assert lib.mcd_pointwise_posterior(const.handle, 0, 4, rowp, ptr[0], ptr[1], None, None) == -1          # S = 0
    assert b"n_samples" in lib.mcd_last_error()
    assert lib.mcd_pointwise_posterior(const.handle, 3, 5, rowp, ptr[0], ptr[1], None, None) == -1          # wrong k
    assert lib.mcd_pointwise_posterior(const.handle, 3, 4, rowp, ptr[0], ptr[1], ptr[2], None) == -1        # pmem, CONST
    assert b"background" in lib.mcd_last_error()
    assert lib.mcd_pointwise_posterior(const.handle, 3, 4, None, ptr[0], ptr[1], None, None) == -1          # null params
    assert lib.mcd_pointwise_posterior(None, 3, 4, rowp, ptr[0], ptr[1], None, None) == -1                  # null catalogue
    assert lib.mcd_pointwise_posterior(const.handle, 3, 4, rowp, ptr[0], ptr[1], None, None) == 0
    with pytest.raises(_native.NativeError, match="background"):
        const.pointwise_posterior(row, membership=True)
    binned = _native.Catalog(ctx, small["ra"], small["dec"], small["v"], small["verr"], centre=ph.CENTRE,
                             bin_offsets=[0, 80, 200])
    assert lib.mcd_pointwise_posterior(binned.handle, 3, 4, rowp, ptr[0], ptr[1], None, None) == -1
    assert b"un-binned" in lib.mcd_last_error()
    empty = _native.Catalog(ctx, np.empty(0), np.empty(0), np.empty(0), np.empty(0), centre=ph.CENTRE)
    assert lib.mcd_pointwise_posterior(empty.handle, 3, 4, rowp, None, None, None, None) == 0
    assert empty.pointwise_posterior(row)["lppd"].size == 0
    # the public methods
    from mcmc_dynamics_amd import DataReader
    from mcmc_dynamics_amd.analysis import ConstantFit
    from mcmc_dynamics_amd.analysis.binned import BinnedConstantFit
    cf = ConstantFit(DataReader({k: small[k] for k in ("ra", "dec", "v", "verr")}))
    chain = np.tile(ph.samples(small, 0, True, 1)[0], (4, 3, 1))
    with pytest.raises(ValueError, match="no background"):
        cf.posterior_membership_probabilities(chain, 1)
    assert np.isfinite(cf.waic(chain, 1)["waic"])
    reader = DataReader({k: small[k] for k in ("ra", "dec", "v", "verr")})
    reader.make_radial_bins(ph.CENTRE[0], ph.CENTRE[1], nstars=50)
    bf = BinnedConstantFit(reader)
    with pytest.raises(NotImplementedError):
        bf.waic(chain, 1)
    with pytest.raises(NotImplementedError):
        bf.pointwise_posterior(chain, 1)
    for c in (const, gb, binned, empty, cf, bf):
        c.close()


def test_waic_of_two_ranks_on_one_device():
    """Two ranks (one process each, one device, tests/fake_rccl for the collective): waic()'s scalars equal the
    single-rank result."""
    subprocess.run(["make", "-C", os.path.join(ROOT, "tests", "fake_rccl")], check=True, capture_output=True)
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", OMP_NUM_THREADS="1")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr",
           "127.0.0.1", "--master-port", "29587", os.path.join(ROOT, "tests", "posterior_rank_worker.py")]
    res = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-3000:]
    assert "POSTERIOR_RANKS_OK world=2" in res.stdout

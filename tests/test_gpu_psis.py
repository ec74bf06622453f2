"""GPU: mcd_psis_loo -- PSIS-LOO per star on the device -- against the NumPy oracle of tests/psis_helper.py run on the lnL
matrix of the per-row entries the library already had (Catalog.loglike_per_star; for the models without a background
the fixed-background twin of test_gpu_posterior._host_loop), against mcd_pointwise_posterior's lppd, and through
Runner.loo."""
import os
import subprocess
import sys

import numpy as np
import pytest

import posterior_helper as ph
import psis_helper as psh
from conftest import ROOT
from test_gpu_posterior import _catalog
from test_posterior_cpu import BG_MODELS

pytestmark = pytest.mark.gpu
MODELS = [0, 1, 2, 3, 4, 5, 6]


def _lnl_matrix(gpu, cat, table, model, centre):
    """(n, S) lnL_is from one per-star call per sample."""
    if model in BG_MODELS:
        x = np.array([gpu.loglike_per_star(row) for row in table])
    else:
        twin = dict(cat, pmember=np.ones(len(cat["v"])), lnlike_bg=np.full(len(cat["v"]), -1e5))
        tw = _catalog(gpu.ctx, twin, 1 if model == 0 else 6, centre)
        x = np.array([tw.loglike_per_star(row) for row in table])
        tw.close()
    return np.ascontiguousarray(x.T)


def _k_tol(lnl):
    """1e-10, or ten times what one ulp of the terms moves the oracle's k^ by (psis_helper.k_noise)."""
    return np.maximum(1e-10, 10.0 * psh.k_noise(lnl))


@pytest.fixture(scope="module")
def ctx():
    from mcmc_dynamics_amd import _native
    return _native.default_context()


@pytest.fixture(scope="module")
def cat2k():
    return ph.model_catalog(2000, 0, seed=17)


@pytest.mark.parametrize("model", MODELS)
@pytest.mark.parametrize("free", [False, True])
def test_device_psis_matches_the_oracle(ctx, cat2k, model, free):
    centre = None if free else ph.CENTRE
    table = ph.samples(cat2k, model, free, 256)
    gpu = _catalog(ctx, cat2k, model, centre)
    got = gpu.psis_loo(table)
    lnl = _lnl_matrix(gpu, cat2k, table, model, centre)
    psh.assert_matches(got, psh.numpy_psis(lnl), k_tol=_k_tol(lnl))
    pp = gpu.pointwise_posterior(table)
    assert np.all(np.abs(got["lppd"] - pp["lppd"]) <= 1e-13 * np.maximum(np.abs(pp["lppd"]), 1.0))
    gpu.close()


def test_bits_repeat_and_do_not_depend_on_tiles(ctx, cat2k):
    table = ph.samples(cat2k, 2, False, 512, seed=4)
    gpu = _catalog(ctx, cat2k, 2, ph.CENTRE)
    a = gpu.psis_loo(table, r_eff=0.7)
    b = gpu.psis_loo(table, r_eff=0.7)
    gpu.set_option("loo_scratch_mb", 1)                  # 1 MiB: tiles of 192 stars, 11 tiles
    c = gpu.psis_loo(table, r_eff=0.7)
    for k in a:
        assert np.array_equal(a[k], b[k]) and np.array_equal(a[k], c[k]), k
    gpu.set_option("timing", 1)
    gpu.psis_loo(table, r_eff=0.7)
    assert gpu.last_kernel_ms > 0.0
    gpu.close()


def test_heavy_tails_and_ties(ctx, cat2k):
    """A chain of repeated rows (rejected moves) and stars far out in velocity: ties at the cutoff and k^ > 0.7."""
    cat = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in cat2k.items()}
    cat["v"][:40] += 60.0
    table = ph.samples(cat, 0, False, 400, seed=8)
    reps = np.repeat(np.arange(400), np.random.default_rng(2).integers(1, 6, size=400))[:400]
    table = np.ascontiguousarray(table[reps])
    gpu = _catalog(ctx, cat, 0, ph.CENTRE)
    got = gpu.psis_loo(table)
    lnl = _lnl_matrix(gpu, cat, table, 0, ph.CENTRE)
    psh.assert_matches(got, psh.numpy_psis(lnl), k_tol=_k_tol(lnl))
    assert np.count_nonzero(got["pareto_k"] > 0.7) >= 5
    gpu.close()


def test_seventy_thousand_samples(ctx):
    cat = ph.model_catalog(300, 0, seed=5)
    table = ph.samples(cat, 1, False, 70000, seed=6)
    gpu = _catalog(ctx, cat, 1, ph.CENTRE)
    got = gpu.psis_loo(table)
    sub = table[:: 1]
    lnl = np.ascontiguousarray(np.array([gpu.loglike_per_star(row) for row in sub]).T)
    psh.assert_matches(got, psh.numpy_psis(lnl), k_tol=_k_tol(lnl))
    gpu.close()


@pytest.mark.parametrize("model,precision", [(0, "f32acc64"), (2, "f32")])
def test_float32_catalogue(ctx, cat2k, model, precision):
    table = ph.samples(cat2k, model, False, 256)
    g32 = _catalog(ctx, cat2k, model, ph.CENTRE, precision)
    g64 = _catalog(ctx, cat2k, model, ph.CENTRE)
    a, b = g32.psis_loo(table), g64.psis_loo(table)
    assert np.max(np.abs(a["elpd_loo"] - b["elpd_loo"]) / np.maximum(np.abs(b["elpd_loo"]), 1.0)) < 2e-5
    fin = np.isfinite(b["pareto_k"])
    assert np.median(np.abs(a["pareto_k"][fin] - b["pareto_k"][fin])) < 0.05
    g32.close()
    g64.close()


# ---- short chains, ragged groups and the largest tail (the selection itself: tests/test_gpu_psis_rows.py) -----------------
SHORT_S = [1, 20, 21, 24, 63, 65]          # M = 1, 4 (no tail), 5, 5, 13, 13; all but 20 and 24 leave a ragged 16-sample block
STAR_COUNTS = [1, 63, 65, 130]             # a ragged last 64-star group of psis_term_kernel, alone and after full ones
CAP_S, CAP_R_EFF = 12800, 0.0175           # M = min(2 560, ceil(3 sqrt(S / r_eff)) = 2 566): kPsisMaxTail, 64 000 B of LDS
_cap = {}


def _head(cat, n):
    return {k: (v[:n].copy() if isinstance(v, np.ndarray) else v) for k, v in cat.items()}


def cap_case(ctx, cat2k):
    """70 stars of model 2 with CAP_S samples: (catalogue, table, lnL (70, CAP_S)); computed once, read-only (shared with
    tests/test_gpu_loo_expect.py)."""
    if not _cap:
        cat = _head(cat2k, 70)
        table = ph.samples(cat2k, 2, False, CAP_S, seed=23)
        gpu = _catalog(ctx, cat, 2, ph.CENTRE)
        lnl = _lnl_matrix(gpu, cat, table, 2, ph.CENTRE)
        gpu.close()
        table.setflags(write=False)
        lnl.setflags(write=False)
        _cap["case"] = (cat, table, lnl)
    return _cap["case"]


@pytest.fixture(scope="module")
def short_table(cat2k):
    return ph.samples(cat2k, 2, False, max(SHORT_S), seed=21)


@pytest.mark.parametrize("n", STAR_COUNTS)
@pytest.mark.parametrize("S", SHORT_S)
def test_short_chains_and_ragged_groups(ctx, cat2k, short_table, S, n):
    cat = _head(cat2k, n)
    table = np.ascontiguousarray(short_table[:S])
    gpu = _catalog(ctx, cat, 2, ph.CENTRE)
    got = gpu.psis_loo(table)
    lnl = _lnl_matrix(gpu, cat, table, 2, ph.CENTRE)
    assert lnl.shape == (n, S)
    psh.assert_matches(got, psh.numpy_psis(lnl), k_tol=_k_tol(lnl))
    pp = gpu.pointwise_posterior(table)
    assert np.all(np.abs(got["lppd"] - pp["lppd"]) <= 1e-13 * np.maximum(np.abs(pp["lppd"]), 1.0))
    if psh.tail_len(S) < 5:
        assert np.all(got["pareto_k"] == np.inf)
    else:
        assert np.all(got["pareto_k"] < np.inf)
    if S == 1:
        assert np.all(got["n_eff"] == 1.0) and np.array_equal(got["elpd_loo"], got["lppd"])
    gpu.close()


def test_the_largest_tail_is_accepted_and_the_next_refused(ctx, cat2k):
    import ctypes
    cat, table, lnl = cap_case(ctx, cat2k)
    assert psh.tail_len(CAP_S, CAP_R_EFF) == 2560
    gpu = _catalog(ctx, cat, 2, ph.CENTRE)
    got = gpu.psis_loo(table, r_eff=CAP_R_EFF)
    want = psh.numpy_psis(lnl, CAP_R_EFF)
    psh.assert_matches(got, want, k_tol=np.maximum(1e-10, 10.0 * psh.k_noise(lnl, CAP_R_EFF)))
    # S = 12 805: ceil(0.2 S) = 2 561
    more = np.ascontiguousarray(ph.samples(cat2k, 2, False, 12805, seed=23))
    assert psh.tail_len(12805, CAP_R_EFF) > 2560
    dp = ctypes.POINTER(ctypes.c_double)
    outs = [np.full(70, -7.0) for _ in range(4)]
    rc = gpu.lib.mcd_psis_loo(gpu.handle, 12805, more.shape[1], more.ctypes.data_as(dp), CAP_R_EFF,
                              *[o.ctypes.data_as(dp) for o in outs])
    assert rc == -1 and b"S / r_eff too large" in gpu.lib.mcd_last_error()
    for o in outs:
        assert np.all(o == -7.0)
    gpu.close()


def test_refusals(ctx, cat2k):
    import ctypes
    from mcmc_dynamics_amd import _native
    small = {k: (v[:200] if isinstance(v, np.ndarray) else v) for k, v in cat2k.items()}
    const = _catalog(ctx, small, 0, ph.CENTRE)
    lib = const.lib
    row = np.ascontiguousarray(ph.samples(small, 0, False, 30))
    rowp = row.ctypes.data_as(ctypes.POINTER(ctypes.c_double))
    out = np.empty(200)
    op = out.ctypes.data_as(ctypes.POINTER(ctypes.c_double))
    assert lib.mcd_psis_loo(const.handle, 30, 4, rowp, 0.0, op, None, None, None) == -1
    assert b"r_eff" in lib.mcd_last_error()
    assert lib.mcd_psis_loo(const.handle, 0, 4, rowp, 1.0, op, None, None, None) == -1
    assert lib.mcd_psis_loo(const.handle, 30, 5, rowp, 1.0, op, None, None, None) == -1
    assert lib.mcd_psis_loo(const.handle, 30, 4, rowp, 1.0, None, None, None, None) == 0
    assert lib.mcd_psis_loo(const.handle, 30, 4, rowp, 1.0, op, None, None, None) == 0
    assert np.all(np.isfinite(out))
    binned = _native.Catalog(ctx, small["ra"], small["dec"], small["v"], small["verr"], centre=ph.CENTRE,
                             bin_offsets=[0, 80, 200])
    assert lib.mcd_psis_loo(binned.handle, 30, 4, rowp, 1.0, op, None, None, None) == -1
    assert b"un-binned" in lib.mcd_last_error()
    const.close()
    binned.close()


def test_runner_loo_on_constant_fit_gb(cat2k):
    from mcmc_dynamics_amd import DataReader
    from mcmc_dynamics_amd.analysis import ConstantFitGB
    from mcmc_dynamics_amd.analysis.binned import BinnedConstantFit
    from mcmc_dynamics_amd.analysis.runner import elpd_compare
    fit = ConstantFitGB(DataReader({k: cat2k[k] for k in ("ra", "dec", "v", "verr", "density")}))
    fit.parameters["ra_center"].set(value=ph.CENTRE[0], fixed=True)
    fit.parameters["dec_center"].set(value=ph.CENTRE[1], fixed=True)
    free = ph.samples(cat2k, 2, False, 16 * 40, seed=12)
    names = ph.abi_names(2, False)
    keep = [names.index(n) for n in fit.fitted_parameters]
    chain = free[:, keep].reshape(16, 40, len(keep))
    res = fit.loo(chain, n_burn=8, thin=2)
    table = free.reshape(16, 40, -1)[:, 8::2, :].reshape(-1, len(names))
    want = fit._catalog.psis_loo(table)
    assert res["n_samples"] == 16 * 16 and res["n_stars"] == 2000
    assert np.array_equal(res["pointwise"], want["elpd_loo"]) and np.array_equal(res["pareto_k"], want["pareto_k"])
    assert np.array_equal(res["n_eff"], want["n_eff"])
    assert res["elpd_loo"] == pytest.approx(want["elpd_loo"].sum(), rel=1e-13)
    assert res["p_loo"] == pytest.approx((want["lppd"] - want["elpd_loo"]).sum(), rel=1e-10)
    assert res["looic"] == -2.0 * res["elpd_loo"]
    assert res["k_threshold"] == pytest.approx(psh.k_threshold(256))
    assert res["n_bad_k"] == int(np.count_nonzero(want["pareto_k"] > res["k_threshold"]))
    w = fit.waic(chain, n_burn=8, thin=2)
    assert abs(w["lppd"] - res["lppd"]) <= 1e-12 * abs(w["lppd"])
    assert abs(res["elpd_loo"] - w["elpd_waic"]) <= 1e-2 * abs(w["elpd_waic"])
    c = elpd_compare(res, w)
    assert c["n_stars"] == 2000 and np.isfinite(c["se_diff"])
    fit.close()
    reader = DataReader({k: cat2k[k] for k in ("ra", "dec", "v", "verr")})
    reader.make_radial_bins(ph.CENTRE[0], ph.CENTRE[1], nstars=500)
    bf = BinnedConstantFit(reader)
    with pytest.raises(NotImplementedError):
        bf.loo(chain, 1)
    bf.close()


def test_loo_of_two_ranks_on_one_device():
    """Two ranks (one process each, one device, tests/fake_rccl for the collective): loo()'s scalars equal the
    single-rank result."""
    subprocess.run(["make", "-C", os.path.join(ROOT, "tests", "fake_rccl")], check=True, capture_output=True)
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", OMP_NUM_THREADS="1")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr",
           "127.0.0.1", "--master-port", "29591", os.path.join(ROOT, "tests", "psis_rank_worker.py")]
    res = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-3000:]
    assert "PSIS_RANKS_OK world=2" in res.stdout

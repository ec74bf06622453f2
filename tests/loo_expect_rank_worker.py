"""Worker of tests/test_gpu_loo_expect.py::test_loo_pit_of_two_ranks_on_one_device (GPU): one process per rank (RANK /
WORLD_SIZE from the launcher), every rank on device 0, tests/fake_rccl standing in for librccl.so.  Each rank holds its
shard of the stars: the per-star arrays of Runner.loo_pit / Runner.loo_influence must be the rank's slice of the
single-rank arrays, bit for bit (a star's expectations depend on its own rows only), and the summaries, summed over the
host group, must be the single-rank values on every rank."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
os.environ["MCD_RCCL_LIBRARY"] = os.path.join(ROOT, "tests", "fake_rccl", "libfake_rccl.so")
os.environ["MCD_ALLOW_SHARED_DEVICE"] = "1"

from mcmc_dynamics_amd import DataReader, _native as native, distributed   # noqa: E402
from mcmc_dynamics_amd.analysis import ConstantFitGB                      # noqa: E402
import posterior_helper as ph                                             # noqa: E402

N = 6000


def fit_on(cols, ctx):
    fit = ConstantFitGB(DataReader(cols), context=ctx)
    fit.parameters["ra_center"].set(value=ph.CENTRE[0], fixed=True)
    fit.parameters["dec_center"].set(value=ph.CENTRE[1], fixed=True)
    return fit


def main():
    ctx = distributed.rank_context(device=0)
    rank, world, group = ctx.rank, ctx.n_ranks, ctx.host_group
    cat = ph.model_catalog(N, 0, seed=13)
    cols = {k: cat[k] for k in ("ra", "dec", "v", "verr", "density")}
    chain = ph.samples(cat, 2, False, 16 * 20, seed=5).reshape(16, 20, -1)      # the same on every rank
    mine = fit_on(distributed.shard_columns(cols, rank, world), ctx)
    p, f = mine.loo_pit(chain, n_burn=4), mine.loo_influence(chain, n_burn=4)
    one = native.Context(n_devices=1)
    full = fit_on(cols, one)
    p1, f1 = full.loo_pit(chain, n_burn=4), full.loo_influence(chain, n_burn=4)
    lo, hi = distributed.shard_bounds(N, rank, world)
    for k in ("loo_pit", "pit", "z", "vlos", "sigma", "pareto_k", "n_eff", "weight"):
        assert np.array_equal(p[k], p1[k][lo:hi]), k
    for k in ("shift", "loo_mean", "pareto_k"):
        assert np.array_equal(f[k], f1[k][lo:hi]), k
    assert np.array_equal(p["hist"], p1["hist"]) and p["n"] == p1["n"] == float(N) and p["n_stars"] == p1["n_stars"] == N
    assert abs(p["chi2"] - p1["chi2"]) <= 1e-12 * p1["chi2"] and p["tail_fraction"] == p1["tail_fraction"]
    assert p["n_bad_k"] == p1["n_bad_k"] == f["n_bad_k"] == f1["n_bad_k"] and p["n_samples"] == 256
    assert group.same_everywhere(np.concatenate([p["hist"], [p["chi2"], p["tail_fraction"], float(p["n_bad_k"])]]))
    assert np.array_equal(f["mean"], f1["mean"]) and np.array_equal(f["std"], f1["std"])
    assert np.array_equal(f["ranking"], np.argsort(-np.max(np.abs(f["shift"]), axis=1), kind="stable"))
    other = chain + (1e-9 if rank == 1 else 0.0)
    try:
        mine.loo_pit(other, n_burn=4)
        raise AssertionError("different chains were not refused")
    except RuntimeError as e:
        assert "different chains" in str(e)
    mine.close()
    full.close()
    group.barrier()
    if rank == 0:
        print("LOO_EXPECT_RANKS_OK world={0}".format(world))
    ctx.close()
    one.close()
    group.close()


if __name__ == "__main__":
    main()

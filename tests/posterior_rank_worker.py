"""Worker of tests/test_gpu_posterior.py::test_waic_of_two_ranks_on_one_device (GPU): one process per rank (RANK /
WORLD_SIZE from the launcher), every rank on device 0, tests/fake_rccl standing in for librccl.so.  Each rank holds its
shard of the stars; Runner.waic sums the totals over the host group, so every rank must return the single-rank scalars,
and each rank's per-star arrays must be its slice of the single-rank arrays."""
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


def fit_on(cols, ctx):
    fit = ConstantFitGB(DataReader(cols), context=ctx)
    fit.parameters["ra_center"].set(value=ph.CENTRE[0], fixed=True)
    fit.parameters["dec_center"].set(value=ph.CENTRE[1], fixed=True)
    return fit


def main():
    ctx = distributed.rank_context(device=0)
    rank, world, group = ctx.rank, ctx.n_ranks, ctx.host_group
    cat = ph.model_catalog(20000, 0, seed=13)
    cols = {k: cat[k] for k in ("ra", "dec", "v", "verr", "density")}
    chain = ph.samples(cat, 2, False, 24 * 30, seed=5).reshape(24, 30, -1)      # the same on every rank
    mine = fit_on(distributed.shard_columns(cols, rank, world), ctx)
    w = mine.waic(chain, n_burn=10)
    mean, std = mine.posterior_membership_probabilities(chain, n_burn=10)
    one = native.Context(n_devices=1)
    full = fit_on(cols, one)
    w1 = full.waic(chain, n_burn=10)
    mean1, std1 = full.posterior_membership_probabilities(chain, n_burn=10)
    lo, hi = distributed.shard_bounds(20000, rank, world)
    for k in ("elpd_waic", "p_waic", "waic", "se", "lppd"):
        assert abs(w[k] - w1[k]) <= 1e-12 * abs(w1[k]), (k, w[k], w1[k])
    assert w["n_stars"] == w1["n_stars"] == 20000 and w["n_samples"] == w1["n_samples"] == 480
    assert w["n_high_variance"] == w1["n_high_variance"]
    assert group.same_everywhere(np.array([w[k] for k in ("elpd_waic", "p_waic", "waic", "se", "lppd")]))
    assert np.max(np.abs(w["pointwise"] - w1["pointwise"][lo:hi]) / np.maximum(np.abs(w1["pointwise"][lo:hi]), 1.0)) < 1e-13
    assert np.max(np.abs(mean - mean1[lo:hi])) < 1e-13 and np.max(np.abs(std - std1[lo:hi])) < 1e-12
    # a rank that passes a different chain is refused
    other = chain + (1e-9 if rank == 1 else 0.0)
    try:
        mine.waic(other, n_burn=10)
        raise AssertionError("different chains were not refused")
    except RuntimeError as e:
        assert "different chains" in str(e)
    mine.close()
    full.close()
    group.barrier()
    if rank == 0:
        print("POSTERIOR_RANKS_OK world={0}".format(world))
    ctx.close()
    one.close()
    group.close()


if __name__ == "__main__":
    main()

"""Worker of tests/test_gpu_psis.py::test_loo_of_two_ranks_on_one_device (GPU): one process per rank (RANK / WORLD_SIZE
from the launcher), every rank on device 0, tests/fake_rccl standing in for librccl.so.  Each rank holds its shard of the
stars; Runner.loo sums the totals over the host group, so every rank must return the single-rank scalars, and each
rank's per-star arrays must be its slice of the single-rank arrays, bit for bit (a star's PSIS depends on its own terms
only)."""
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
from mcmc_dynamics_amd.analysis.runner import elpd_compare                # noqa: E402
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
    r = mine.loo(chain, n_burn=10)
    w = mine.waic(chain, n_burn=10)
    one = native.Context(n_devices=1)
    full = fit_on(cols, one)
    r1 = full.loo(chain, n_burn=10)
    w1 = full.waic(chain, n_burn=10)
    lo, hi = distributed.shard_bounds(20000, rank, world)
    for k in ("elpd_loo", "p_loo", "looic", "se", "lppd"):
        assert abs(r[k] - r1[k]) <= 1e-12 * abs(r1[k]), (k, r[k], r1[k])
    assert r["n_stars"] == r1["n_stars"] == 20000 and r["n_samples"] == r1["n_samples"] == 480
    assert r["n_bad_k"] == r1["n_bad_k"]
    assert group.same_everywhere(np.array([r[k] for k in ("elpd_loo", "p_loo", "looic", "se", "lppd")]))
    for k in ("pointwise", "pareto_k", "n_eff"):
        assert np.array_equal(r[k], r1[k][lo:hi]), k
    c, c1 = elpd_compare(r, w, group=group), elpd_compare(r1, w1)
    assert abs(c["elpd_diff"] - c1["elpd_diff"]) <= 1e-9 * max(abs(c1["elpd_diff"]), 1.0)
    assert abs(c["se_diff"] - c1["se_diff"]) <= 1e-9 * max(c1["se_diff"], 1e-6)
    other = chain + (1e-9 if rank == 1 else 0.0)
    try:
        mine.loo(other, n_burn=10)
        raise AssertionError("different chains were not refused")
    except RuntimeError as e:
        assert "different chains" in str(e)
    mine.close()
    full.close()
    group.barrier()
    if rank == 0:
        print("PSIS_RANKS_OK world={0}".format(world))
    ctx.close()
    one.close()
    group.close()


if __name__ == "__main__":
    main()

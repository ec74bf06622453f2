"""Worker of tests/test_gpu_predictive.py (GPU): mcd_posterior_predictive on a 3-shard context on ONE device, with
tests/fake_rccl standing in for librccl.so (as tests/grad_sharded_worker.py does): real shards, real kernels.  The call has
no collective of its own -- every shard writes its stars at star_begin -- so what is checked is the placement.

One case: PROFILE_BGGAUSS with a free centre, N = 4099, S = 257.  Every output must equal the one-device result to 1e-13
of its scale: a star's result depends on its own terms only, but the shards' star counts change the slice plan and with
it the order of the merges."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
os.environ["MCD_RCCL_LIBRARY"] = os.path.join(ROOT, "tests", "fake_rccl", "libfake_rccl.so")
os.environ["MCD_ALLOW_SHARED_DEVICE"] = "1"

from mcmc_dynamics_amd import _native as native     # noqa: E402
import emul_helper as emul                            # noqa: E402
import predictive_helper as pr                        # noqa: E402
from test_predictive_cpu import _merge_scale          # noqa: E402


def main():
    model = 4
    cat, table, centre, _ = pr.matrix_case(model, True)
    n = len(cat["v"])
    one = native.Context(n_devices=1)
    many = native.Context(device_ids=[0, 0, 0])
    assert many.n_devices == 3
    ref = pr.device_catalog(one, cat, model, centre)
    gpu = pr.device_catalog(many, cat, model, centre)
    a = ref.posterior_predictive(table, mixture=True)
    b = gpu.posterior_predictive(table, mixture=True)
    b2 = gpu.posterior_predictive(table, mixture=True)
    vmax = float(np.max(np.abs(cat["v"])))
    worst = 0.0
    for k in a:
        assert b[k].tobytes() == b2[k].tobytes(), k
        err = np.abs(b[k] - a[k]) / _merge_scale(a, k, vmax)
        worst = max(worst, float(err.max()))
        assert np.all(err <= 1e-13), (k, int(np.argmax(err)), float(err.max()))
    # placement: the first star of the second and of the third shard carries its own values, not a neighbour's
    for i in (1, 2):
        begin, _ = emul.shard_range(n, i, 3)
        assert 0 < begin < n
        for k in ("vlos_mean", "z_mean", "pit_mix"):
            assert abs(b[k][begin] - a[k][begin]) <= 1e-13 * max(1.0, abs(a[k][begin]), vmax if k == "vlos_mean" else 0.0)
        assert a["z_mean"][begin] != a["z_mean"][begin - 1]
    gpu.close()
    ref.close()
    print("PREDICTIVE_SHARDED_OK worst {0:.2e}".format(worst))


if __name__ == "__main__":
    main()

"""Worker of tests/test_gpu_grad_sharded.py (GPU): mcd_loglike_grad_batch on a 3-shard context on ONE device, with
tests/fake_rccl standing in for librccl.so (as tests/fake_rccl_worker.py does for the value path): real shards, real
kernels, the real all-reduce call sites with count (1 + K) x outputs; only the collective itself is host-staged.

One case: CONST_BGGAUSS, N = 4099, W = 65.  Gradient and value must equal the one-device result to 1e-13 S_k: the same
per-star terms are regrouped into three sums, which perturbs each sum by a few ulps of S_k (S_k = sum of |terms|)."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
os.environ["MCD_RCCL_LIBRARY"] = os.path.join(ROOT, "tests", "fake_rccl", "libfake_rccl.so")
os.environ["MCD_ALLOW_SHARED_DEVICE"] = "1"

from mcmc_dynamics_amd import _native as native     # noqa: E402
import grad_helper as gh                              # noqa: E402
import variant_helper as vh                           # noqa: E402


def main():
    case = vh.make_case(2, False, 4099)
    params = np.ascontiguousarray(case["params"][:65])
    one = native.Context(n_devices=1)
    many = native.Context(device_ids=[0, 0, 0])
    assert many.n_devices == 3
    ref = vh.catalog(native, one, case)
    cat = vh.catalog(native, many, case)
    v1, g1 = ref.loglike_grad(params)
    v3, g3 = cat.loglike_grad(params)
    v3b, g3b = cat.loglike_grad(params)
    assert v3.tobytes() == v3b.tobytes() and g3.tobytes() == g3b.tobytes()
    worst = 0.0
    for r in vh.sample_rows(65):
        s = gh.grad(2, case["cat"], params[r], case["centre"], np.float64)[1]
        err = np.abs(g3[r] - g1[r]) / s
        worst = max(worst, float(err.max()))
        assert np.all(err <= 1e-13), (r, err.tolist())
    assert np.all(vh.scaled_err(v3, v1, 4099) <= 1e-13)
    cat.close()
    ref.close()
    print("GRAD_SHARDED_OK worst {0:.2e}".format(worst))


if __name__ == "__main__":
    main()

"""Regenerates the table FREE_FLOOR of tests/escale_helper.py (not a test; a minute of CPU):
`python tests/escale_floor_sweep.py`: for every free-centre cell of the error-scale models (10, 11) x N in {1, 33, 4099} and
ALL 257 walker rows of escale_helper.make_case, the largest err - 2 err_np64 of

  * the host build of csrc/mcd_grad.h for the BASE model (0, 3) on the catalogue whose error column is multiplied by the
    row's err_scale -- the code grad_bounds.FREE_FLOOR was measured with, on the catalogue the error-scale row is equivalent
    to: what the free-centre record format costs at that cell, measured without a line of the error-scale code;
  * the host build for the error-scale model itself on the same rows, for comparison,

for the geometry columns and for the other columns (err_scale is one of the others), the way tests/grad_floor_sweep.py
measures grad_bounds' own table."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import escale_helper as es                     # noqa: E402
import grad_bounds as gb                       # noqa: E402
import grad_helper as gh                       # noqa: E402
import variant_helper as vh                    # noqa: E402


def main():
    rows = list(range(257))
    for n in (1, 33, 4099):
        for model in es.MODELS:
            base = es.BASE[model]
            case = es.make_case(model, True, n)
            base_rows, s = es.split_rows(model, case["params"])
            geometry = gb.is_geometry(base, True)
            k = es.ES_COLUMN[model]
            _, own = es.emul_grad(model, case["cat"], case["params"][rows], None)
            worst_base, worst_own = [0.0, 0.0], [0.0, 0.0]
            for j, r in enumerate(rows):
                cat64 = {key: np.asarray(v, dtype=np.float64) for key, v in es.scaled_cat(case["cat"], s[r], np.float64).items()}
                _, grad = es.emul_grad(base, cat64, base_rows[r], None)
                args = (base, cat64, base_rows[r], None)
                g80, s80 = gh.grad(*args, vh.L)
                g64, _ = gh.grad(*args, np.float64)
                excess = gh.col_err(grad[0], g80, s80) - 2 * gh.col_err(g64, g80, s80)
                worst_base = [max(worst_base[0], float(excess[geometry].max())), max(worst_base[1], float(excess[~geometry].max()))]
                ref = es.reference(case, r)
                excess = gh.col_err(own[j], ref["g"], ref["s"]) - 2 * ref["err64"]
                geo = np.insert(geometry, k, False)
                worst_own = [max(worst_own[0], float(excess[geo].max())), max(worst_own[1], float(excess[~geo].max()))]
            print("model {0} N = {1}: base model on the scaled catalogues: geometry {2:.3e}, other {3:.3e};  "
                  "error-scale model: geometry {4:.3e}, other {5:.3e}".format(model, n, *(worst_base + worst_own)), flush=True)


if __name__ == "__main__":
    with np.errstate(all="ignore"):
        main()

"""Regenerates the tables of tests/grad_bounds.py (not a test; `python tests/grad_floor_sweep.py`, a few minutes of CPU):
the host build of csrc/mcd_grad.h against the 80-bit gradient over ALL 257 walker rows of every free-centre cell, as the
largest err - 2 err_np64 per (model, N), for the geometry columns and for the other columns."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import grad_bounds as gb                       # noqa: E402
import grad_helper as gh                       # noqa: E402
import variant_helper as vh                    # noqa: E402
from test_grad_emul_cpu import emul_grad       # noqa: E402


def main():
    rows = list(range(257))
    for n in (1, 33, 4099):
        for model in range(7):
            cases = [vh.make_case(model, True, n)]
            if n == 4099 and model in vh.MIXTURE_MODELS:
                cases.append(vh.make_case(model, True, n, plant=True))
            geometry = gb.is_geometry(model, True)
            worst = [0.0, 0.0]
            for case in cases:
                _, grad = emul_grad(case, rows)
                for j, r in enumerate(rows):
                    args = (model, case["cat"], case["params"][r], None)
                    g80, s80 = gh.grad(*args, vh.L)
                    g64, _ = gh.grad(*args, np.float64)
                    excess = gh.col_err(grad[j], g80, s80) - 2 * gh.col_err(g64, g80, s80)
                    worst = [max(worst[0], float(excess[geometry].max())), max(worst[1], float(excess[~geometry].max()))]
            print("model {0} N = {1}: geometry columns {2:.3e}, other columns {3:.3e}".format(model, n, *worst), flush=True)


if __name__ == "__main__":
    with np.errstate(all="ignore"):
        main()

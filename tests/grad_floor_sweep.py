"""Regenerates the tables of tests/grad_bounds.py (not a test; a few minutes of CPU each):
`python tests/grad_floor_sweep.py`: the host build of csrc/mcd_grad.h against the 80-bit gradient over ALL 257 walker rows
of every free-centre cell, as the largest err - 2 err_np64 per (model, N), for the geometry columns and for the other columns.
`python tests/grad_floor_sweep.py plans [first cell [one past the last]]`: the same figure, host build in chunks of 64
stars, for the catalogues of test_gpu_grad_plans.py (grad_bounds.plan_cells) at every prefix length and over every walker
row that module can reach -- the table LARGE_FLOOR."""
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


def plans(first=0, last=None):
    for name, make, lengths, rows in list(gb.plan_cells())[first:last]:
        case = make()
        model, free = case["model"], case["free"]
        rows = list(rows)
        geometry = gb.is_geometry(model, free)
        worst = {n: [0.0, 0.0] for n in lengths}
        grads = {n: emul_grad(gb.sub_case(case, slice(0, n)), rows, gb.PLAN_CHUNK)[1] for n in lengths}
        for j, r in enumerate(rows):
            for n, ref in gb.prefix_reference(case, r, lengths).items():
                excess = gh.col_err(grads[n][j], ref["g"], ref["s"]) - 2 * ref["err64"]
                worst[n] = [max(worst[n][0], float(excess[geometry].max(initial=0.0))),
                            max(worst[n][1], float(excess[~geometry].max()))]
            gb._cache.clear()                              # (one row's figures are used once)
        for n in lengths:
            print("{0} N = {1} ({2} rows): geometry columns {3:.3e}, other columns {4:.3e}".format(name, n, len(rows), *worst[n]),
                  flush=True)
        print("{0}: largest N = {1}, over all prefixes: geometry columns {2:.3e}, other columns {3:.3e}".format(
            name, max(lengths), max(w[0] for w in worst.values()), max(w[1] for w in worst.values())), flush=True)


if __name__ == "__main__":
    with np.errstate(all="ignore"):
        if sys.argv[1:2] == ["plans"]:
            plans(*(int(a) for a in sys.argv[2:4]))
        else:
            main()

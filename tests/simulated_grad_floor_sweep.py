"""Prints the table behind simulated_grad_helper.SIM_FLOOR: per (model, centre, N) cell of the matrix the largest
err - 2 err_np64 of the host build of csrc/mcd_simulated_grad.h over every row the GPU matrix can reach
(`python tests/simulated_grad_floor_sweep.py`; about a minute).  Test infrastructure only."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import simulated_grad_helper as sg             # noqa: E402

if __name__ == "__main__":
    sg.sweep()

#!/usr/bin/env python3
"""Writes the reference output of tests/test_gpu_exp_split.py: the log-likelihoods of its 20 011-star catalogue from a
library WITHOUT the option "exp_split" (the commit before it, selected with MCD_LIB_PATH), i.e. every direct chunk with
the exponent offset taken from the record as it is.

    MCD_LIB_PATH=/path/to/libmcd_hip.so python tools/exp_split_golden.py OUTDIR     # then copy OUTDIR/*.npy to tests/golden/

A library that knows the option is asked to switch it off, so the file can be re-checked with the current build."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main(out):
    import test_gpu_exp_split as t
    from mcmc_dynamics_amd import _native as native
    os.makedirs(out, exist_ok=True)
    cat, pos = t._c3(20011)
    c = t._make(native, cat, verr_sorted=1)
    try:
        c.set_option("exp_split", 0)
    except native.NativeError:
        pass                                        # a library from before the option
    got = c.loglike(pos)
    assert c.fast_level == 2 and c.last_direct_chunks > 0
    np.save(os.path.join(out, "exp_split_off_20011.npy"), got)
    print(20011, "direct chunks", c.last_direct_chunks, "sum", repr(float(got.sum())))
    c.close()


if __name__ == "__main__":
    main(sys.argv[1])

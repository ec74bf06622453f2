#!/usr/bin/env python3
"""Writes the reference outputs of tests/test_gpu_root_direct.py: the log-likelihoods of its catalogues from a library
WITHOUT the option "root_direct" (the commit before it, selected with MCD_LIB_PATH), i.e. every series chunk in the delta
form.

    MCD_LIB_PATH=/path/to/libmcd_hip.so python tools/root_direct_golden.py OUTDIR     # then copy OUTDIR/*.npy to tests/golden/

A library that knows the option is asked to switch it off, so the files can be re-checked with the current build."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main(out):
    import test_gpu_root_direct as t
    from mcmc_dynamics_amd import _native as native
    os.makedirs(out, exist_ok=True)
    for n, options in ((180000, {}), (1000000, {"verr_sorted": 1}), (20011, {"verr_sorted": 1})):
        cat, pos = t._c3(n)
        c = t._make(native, cat, **options)
        try:
            c.set_option("root_direct", 0)
        except native.NativeError:
            pass                                        # a library from before the option
        got = c.loglike(pos)
        assert c.fast_level == 2 and c.last_series_chunks > 0
        np.save(os.path.join(out, "root_direct_off_{0}.npy".format(n)), got)
        print(n, "series chunks", c.last_series_chunks, "sum", repr(float(got.sum())))
        c.close()


if __name__ == "__main__":
    main(sys.argv[1])

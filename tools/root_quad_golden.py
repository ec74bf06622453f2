#!/usr/bin/env python3
"""Writes the reference output of tests/test_gpu_root_quad.py: the log-likelihoods of its 20 011-star catalogue (sorted by
verr, 64-star chunks) from a library WITHOUT the option "root_quad" (the commit before it, selected with MCD_LIB_PATH), i.e.
every direct chunk with the cubic of RootDirect.

    MCD_LIB_PATH=/path/to/libmcd_hip.so python tools/root_quad_golden.py OUTDIR     # then copy OUTDIR/*.npy to tests/golden/

A library that knows the option is asked to switch it off, so the file can be re-checked with the current build."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main(out):
    import test_gpu_root_quad as t
    from mcmc_dynamics_amd import _native as native
    os.makedirs(out, exist_ok=True)
    cat, pos = t._c3()
    c = t._make(native, cat, verr_sorted=1, chunk_len=t.CHUNK_LEN)
    try:
        c.set_option("root_quad", 0)
    except native.NativeError:
        pass                                        # a library from before the option
    got = c.loglike(pos)
    assert c.fast_level == 2 and c.last_direct_chunks > 0 and c.last_exp_split == 1
    np.save(os.path.join(out, "root_quad_off_20011.npy"), got)
    print(t.N, "direct chunks", c.last_direct_chunks, "sum", repr(float(got.sum())))
    c.close()


if __name__ == "__main__":
    main(sys.argv[1])

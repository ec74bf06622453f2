"""Record tests/golden/sampler_streams.npz: the pinned runs of tests/test_stretch_block_cpu.py (``sampler_stream_cases``),
the chains both samplers produce in every driving mode.  Run from the repository root after building the library
(``make -C mcmc_dynamics_amd/csrc``); the fixture is only re-recorded when a change of the random streams is intended."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import test_stretch_block_cpu as t                                     # noqa: E402


def main():
    flat = {"{0}/{1}".format(case, name): np.asarray(value)
            for case, rec in t.sampler_stream_cases().items() if case not in t.STREAM_ALIASES
            for name, value in rec.items()}
    np.savez_compressed(t.STREAMS, **flat)
    print("{0}: {1} arrays, {2} bytes".format(t.STREAMS, len(flat), os.path.getsize(t.STREAMS)))


if __name__ == "__main__":
    main()

"""The block step of the bounded quadratic loop (option "block_step"; csrc/mcd_math.h: chunk_bgfixed_fast<.., BOUNDED, BLOCK>) on
the CPU build of the kernels' arithmetic (tests/emul): the fold, the rescale and the prefetch of a 32-star band in one block
per multiple of 32 of the absolute record index.  Moving the rescale points multiplies by powers of two only, so the loop
must return the doubles of the bounded loop it replaces -- for every place a chunk can start at on the 32-grid, for chunks
shorter than a band and longer than two, in the array's last block with its remainder, and where the quadratic form is
refused.  And the host guard that admits it (csrc/mcd_guard.h: block_step_admitted)."""
import numpy as np
import pytest

import block_step_helper as bs
import emul_helper as emul
import root_series_helper as rs


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    return bs.build(tmp_path_factory.mktemp("block_step"))


@pytest.fixture(scope="module")
def tight():
    """the tight verr band of the shared catalogue, packed and sorted by verr, and 70 walkers"""
    cat = bs.catalogue()
    rec = emul.pack_records(cat, 1, bs.CENTRE)
    rec = rec[rs.verr_order(rec)]
    first = int(np.searchsorted(rec[:, 1], 1.0))
    band = rec[first:first + 3000]
    assert band[-1, 1] <= 1.001
    return band, bs.walkers(70)


@pytest.mark.parametrize("start", [0, 8, 16, 24])
@pytest.mark.parametrize("count", [8, 24, 32, 40, 56, 72, 100])
def test_block_step_returns_the_bounded_loops_doubles(lib, tight, start, count):
    """One chunk that starts `start` records past a multiple of 32 (the third band of a 256-record array): no boundary, one
    or several inside it, with a 4-star group (100) behind the 8-star iterations.  R = 32 and R = 16 in the loop compared
    against: its rescales count from the chunk's start, the block step's from the grid."""
    band, pos = tight
    for iters in (4, 2):
        out, took = bs.chunk(lib, band[:256], 64 + start, count, pos, rescale_iters=iters)
        assert took.all() and np.isfinite(out).all()
        assert np.array_equal(out[:, 0], out[:, 1]), (start, count, iters)


@pytest.mark.parametrize("begin,count", [(0, 100), (32, 68), (64, 36), (72, 28), (88, 12), (96, 4), (40, 57)])
def test_last_block_with_a_remainder(lib, tight, begin, count):
    """An array of 100 records: three blocks, the last one of 36 records.  The boundary at record 96 starts no block -- the
    block step rescales there and folds nothing -- and a chunk that begins behind it keeps the last block's constants."""
    band, pos = tight
    out, took = bs.chunk(lib, band[:100], begin, count, pos)
    assert took.all() and np.isfinite(out).all()
    assert np.array_equal(out[:, 0], out[:, 1]), (begin, count)


def test_array_shorter_than_a_block_is_refused_the_quadratic_form(lib, tight):
    band, pos = tight
    for begin, count in ((0, 24), (8, 16)):
        out, took = bs.chunk(lib, band[:24], begin, count, pos)
        assert not took.any() and np.isfinite(out).all()
        assert np.array_equal(out[:, 0], out[:, 1])


def test_guard_admits_where_56_factors_fit(lib):
    """block_step_admitted: the bounded verdict at R = 32 and, for 56 factors, both of its conditions with the split loop's
    kappa.  The shared catalogue's tables (tests/test_gpu_block_step.py runs them on the device): admitted with the
    benchmark's walkers, refused -- with the bounded loop still at R = 32 -- once a walker lowers the smallest variance."""
    cat = bs.catalogue()
    for n in (1, 64, 65, 256):
        pos = bs.walkers(n)
        assert bs.verdict(lib, cat, pos) == (32, True)
        assert bs.verdict(lib, cat, bs.refused_table(pos)) == (32, False)
    # a confident member: 1 + R log2(1 / (1 - pmember)) <= 1000 holds for 32 factors and fails for 56
    sure = dict(cat)
    sure["pmember"] = cat["pmember"].copy()
    sure["pmember"][7] = 1.0 - 2.0 ** -20
    assert bs.verdict(lib, sure, bs.walkers(64)) == (32, False)
    # where the bounded loop runs at R = 16 or not at all, the block step is never admitted
    sure["pmember"][7] = 1.0 - 2.0 ** -40
    assert bs.verdict(lib, sure, bs.walkers(64)) == (16, False)
    sure["pmember"][7] = 1.0
    assert bs.verdict(lib, sure, bs.walkers(64)) == (0, False)

"""The block step of the bounded quadratic loop (option "block_step"; csrc/mcd_kernels.hip: loglike_block_kernel,
csrc/mcd_math.h: chunk_bgfixed_fast<.., BOUNDED, BLOCK>) on the GPU: one catalogue of 4 000 stars in 160-star chunks, whose
quarter-length tail chunks of 40 stars start off the 32-grid, at 1, 64, 65 and 256 walkers.  With the option on the launch
runs the block-step kernel and returns the bits of the bounded kernel it replaces; a parameter table for which 56 raw factors
do not fit between two rescales is refused the form (the bounded loop still runs at R = 32) and returns the same bits too."""
import numpy as np
import pytest

import block_step_helper as bs

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def device_catalogue():
    from mcmc_dynamics_amd import _native as native
    cat = bs.catalogue()
    c = native.Catalog(native.default_context(), cat["ra"], cat["dec"], cat["v"], cat["verr"], model=native.MODEL_CONST_BGFIXED,
                       centre=bs.CENTRE, lnlike_bg=cat["lnlike_bg"], pmember=cat["pmember"])
    for key, value in (("verr_sorted", 1), ("prefetch", 1), ("chunk_len", 160)):
        c.set_option(key, value)
    return c


def _both(c, pos):
    """(results with block_step = 1, its launch_info and bounded R, results with block_step = 0 and theirs)"""
    out = []
    for on in (1, 0):
        c.set_option("block_step", on)
        got = c.loglike(pos)
        assert c.fast_level == 2 and c.rerun_count == 0
        out += [got, c.launch_info(), c.last_narrow_bounded]
    c.set_option("block_step", 1)
    return out


@pytest.mark.parametrize("n_walkers", [1, 64, 65, 256])
def test_block_step_on_and_off_agree_in_every_bit(device_catalogue, n_walkers):
    c = device_catalogue
    on, info_on, r_on, off, info_off, r_off = _both(c, bs.walkers(n_walkers))
    print("{0} walkers: {1} quad of {2} chunks".format(n_walkers, info_on["quad_chunks"], info_on["chunks"]))
    assert r_on == 32 and r_off == 32
    assert info_on["block_step"] == 1 and info_on["root_quad"] == 1 and info_on["quad_chunks"] >= 8
    assert info_off["block_step"] == 0 and info_off["quad_chunks"] == info_on["quad_chunks"]
    assert np.isfinite(on).all()
    assert np.array_equal(on, off)


def test_table_that_does_not_fit_56_factors_is_refused_the_form(device_catalogue):
    c = device_catalogue
    pos = bs.refused_table(bs.walkers(256))
    on, info_on, r_on, off, info_off, r_off = _both(c, pos)
    assert r_on == 32 and r_off == 32                                    # the bounded loop itself is admitted
    assert info_on["root_quad"] == 1 and info_on["block_step"] == 0 and info_off["block_step"] == 0
    assert np.isfinite(on).all() and np.array_equal(on, off)
    # ... and the next table that fits takes the form again
    c.loglike(bs.walkers(256))
    assert c.last_block_step == 1

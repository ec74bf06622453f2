"""The narrow-range MODEL_BGFIXED loop (csrc/mcd_math.h: chunk_bgfixed_fast, 8-star iterations with one rescale each, then an
optional 4-star group and single stars): chunk lengths that exercise every part of it agree with the plain formulation
on the CPU build, and C3's exact shape (1e6 stars x 256 walkers) agrees with the plain kernel and the NumPy oracle on
the device."""
import numpy as np
import pytest

from conftest import rel_err

import emul_helper as E


def _case(rng, n):
    from oracle import lnprob_numpy as oracle
    from mcmc_dynamics_amd import synthetic
    cat = synthetic.make_catalog(n, config=3, background=True, seed=int(rng.integers(1 << 30)))
    cat["lnlike_bg"] = oracle.gaussian_background(cat["v"], cat["verr"], 20.0, 40.0)
    return cat, (synthetic.CENTER_RA_DEG, synthetic.CENTER_DEC_DEG)


@pytest.mark.parametrize("n", [1, 3, 4, 7, 8, 12, 15, 16, 20, 23, 248, 252, 255, 4099])
def test_narrow_loop_chunk_lengths_cpu(n):
    """Every split of a chunk into 8-star iterations, a trailing 4-star group and single stars: the narrow-range form
    (fast = 2) matches the plain one to 1e-12 and the general fast form to 1e-13."""
    rng = np.random.default_rng(5300 + n)
    cat, centre = _case(rng, n)
    params = np.stack([rng.normal(0, 2, 8), 10.0 ** rng.uniform(0.3, 1.0, 8), rng.normal(0, 2, 8), rng.normal(0, 2, 8)],
                      axis=1)
    assert E.fast_level(cat, params, 1, centre) == 2
    narrow = E.loglike(cat, params, 1, centre, 2, chunk_len=n)
    plain = E.loglike(cat, params, 1, centre, 0, chunk_len=n)
    general = E.loglike(cat, params, 1, centre, 1, chunk_len=n)
    assert rel_err(narrow, plain) < 1e-12
    assert rel_err(narrow, general) < 1e-13


@pytest.mark.gpu
def test_c3_shape_narrow_matches_plain_and_oracle():
    """C3: 1e6 stars x 256 walkers through the narrow-range kernel: bitwise repeatable, equal to the plain kernel to
    1e-11 and, on a 1e5-star x 16-walker slice, to the NumPy oracle to 1e-12."""
    from mcmc_dynamics_amd import _native as native
    from mcmc_dynamics_amd import synthetic
    from oracle import lnprob_numpy as oracle
    ctx = native.default_context()
    cat = synthetic.make_catalog(1000000, config=3, seed=synthetic.CATALOG_SEED_BASE + 3, background=True)
    pos = synthetic.make_walkers(256, ["v_sys", "sigma_max", "v_maxx", "v_maxy"], cat["truth"], config=3)
    centre = (synthetic.CENTER_RA_DEG, synthetic.CENTER_DEC_DEG)
    lnbg = oracle.gaussian_background(cat["v"], cat["verr"], 20.0, 40.0)

    def make(sl):
        return native.Catalog(ctx, cat["ra"][sl], cat["dec"][sl], cat["v"][sl], cat["verr"][sl],
                              model=native.MODEL_CONST_BGFIXED, centre=centre, lnlike_bg=lnbg[sl],
                              pmember=cat["pmember"][sl])

    full = make(slice(None))
    a = full.loglike(pos)
    assert full.fast_level == 2
    assert np.array_equal(a, full.loglike(pos))
    full.set_option("fast_path", 0)
    assert rel_err(full.loglike(pos), a) < 1e-11
    full.close()
    sl = slice(0, 100000)
    sub = {k: v[sl] for k, v in cat.items() if isinstance(v, np.ndarray)}
    part = make(sl)
    got = part.loglike(pos[:16])
    assert part.fast_level == 2
    part.close()
    want = oracle.batched_constant_lnlike(sub, pos[:16], *centre, lnlike_background=lnbg[sl], pmember=sub["pmember"])
    assert rel_err(got, want) < 1e-12


@pytest.fixture(scope="module")
def biased_lib(tmp_path_factory):
    import ctypes
    import subprocess
    out = str(tmp_path_factory.mktemp("bgfixed_emul") / "libbgfixed_emul.so")
    subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-I", E.INC,
                    E.os.path.join(E.ROOT, "tests", "emul", "bgfixed_narrow_emul.cpp"), "-o", out], check=True)
    lib = ctypes.CDLL(out)
    lib.emul_bgfixed_biased.argtypes = [ctypes.c_int64, ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p, ctypes.c_void_p]
    lib.emul_exp_scaled.argtypes = [ctypes.c_int64, ctypes.c_void_p, ctypes.c_void_p]
    return lib


def test_exponent_insertion_matches_ldexp_cpu(biased_lib):
    """exp_tab_scaled (exponent added into the high word of a biased table entry) equals ldexp(exp_tab(u), e) bit for
    bit wherever the exponent is not clamped (e >= -1021), and stays below 2^-1019 where it is."""
    rng = np.random.default_rng(77)
    u = np.concatenate([rng.uniform(-1.1e6, 60.0, 20000), rng.uniform(-760.0, -690.0, 20000), rng.uniform(-5, 5, 2000),
                        np.arange(-720.0, 60.0, 0.37)])
    out = np.empty(2 * len(u))
    assert biased_lib.emul_exp_scaled(len(u), u.ctypes.data, out.ctypes.data) == 0
    ref, got = out[0::2], out[1::2]
    normal = ref >= np.ldexp(1.0, -1019)            # then e >= -1020: no clamp
    assert normal.sum() > 5000 and (~normal).sum() > 20000
    assert np.array_equal(ref[normal], got[normal])
    assert np.all(got[~normal] < np.ldexp(1.0, -1019)) and np.all(got[~normal] >= 0.0)


@pytest.mark.parametrize("n", [1, 4, 8, 12, 23, 255, 4099])
def test_biased_table_chunks_are_bitwise_equal_cpu(biased_lib, n):
    """The narrow and the general form on the exponent-biased table give the same bits as on the plain table, also with
    far outliers (exponent arguments down to -1e6, where the clamp acts)."""
    rng = np.random.default_rng(9100 + n)
    cat, centre = _case(rng, n)
    cat["v"][::5] += rng.choice([-1.0, 1.0], size=len(cat["v"][::5])) * 10.0 ** rng.uniform(1.5, 3.0, len(cat["v"][::5]))
    params = np.stack([rng.normal(0, 2, 8), 10.0 ** rng.uniform(0.0, 1.0, 8), rng.normal(0, 2, 8), rng.normal(0, 2, 8)],
                      axis=1)
    rec = E.pack_records(cat, 1, centre)
    wp = E.pack_walkers(params, 1, False)
    out = np.empty(4 * len(params))
    assert biased_lib.emul_bgfixed_biased(n, rec.ctypes.data, len(params), wp.ctypes.data, out.ctypes.data) == 0
    out = out.reshape(-1, 4)
    assert np.array_equal(out[:, 0], out[:, 1])
    assert np.array_equal(out[:, 2], out[:, 3])
    assert rel_err(out[:, 0], out[:, 2]) < 1e-13          # (chunk sums without the walker-independent sum of lnL_bg)

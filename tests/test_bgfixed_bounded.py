"""The bounded sub-variant of the narrow-range MODEL_BGFIXED loop (csrc/mcd_math.h: chunk_bgfixed_fast<.., BOUNDED>; host guard
csrc/mcd_guard.h: bounded_rescale): no exponent clamp and a rescale every R = 16 or 32 factors.  Wherever the guard admits
it, every term stays inside the domain it was derived for and the loop gives the level-2 loop's bits; C3's exact shape
runs it on the device with the same bits as the forced level-2 loop."""
import ctypes
import subprocess

import numpy as np
import pytest

from conftest import rel_err

import emul_helper as E

K_EXP_TAB_KMIN = -1021 * 1024


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("bgfixed_bounded") / "libbgfixed_bounded.so")
    subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-I", E.INC,
                    E.os.path.join(E.ROOT, "tests", "emul", "bgfixed_bounded_emul.cpp"), "-o", out], check=True)
    L = ctypes.CDLL(out)
    L.emul_bounded_verdict.argtypes = [ctypes.c_int64] + [ctypes.c_void_p] * 5 + [ctypes.c_int64, ctypes.c_void_p]
    L.emul_bounded_terms.argtypes = [ctypes.c_int64, ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p, ctypes.c_void_p,
                                     ctypes.c_void_p]
    L.emul_bounded_chunk.argtypes = [ctypes.c_int64, ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p, ctypes.c_int,
                                     ctypes.c_void_p]
    return L


def _catalog(rng, n, config=3, seed=None):
    from oracle import lnprob_numpy as oracle
    from mcmc_dynamics_amd import synthetic
    cat = synthetic.make_catalog(n, config=config, background=True,
                                 seed=int(rng.integers(1 << 30)) if seed is None else seed)
    cat["lnlike_bg"] = oracle.gaussian_background(cat["v"], cat["verr"], 20.0, 40.0)
    return cat, (synthetic.CENTER_RA_DEG, synthetic.CENTER_DEC_DEG)


def _verdict(L, cat, params):
    cols = [np.ascontiguousarray(cat[k], dtype=np.float64) for k in ("v", "verr", "lnlike_bg", "pmember")]
    params = np.ascontiguousarray(params, dtype=np.float64)
    info = np.zeros(6)
    R = L.emul_bounded_verdict(len(cols[0]), *[c.ctypes.data for c in cols], params.ctypes.data, len(params),
                               info.ctypes.data)
    return R, dict(zip(("nbp_min", "nbp_max", "pm_max", "n_min", "d_max", "level"), info))


def _terms(L, cat, centre, params):
    rec = E.pack_records(cat, 1, centre)
    wp = E.pack_walkers(params, 1, False)
    k = np.zeros(1, np.int32)
    y = np.zeros(2)
    assert L.emul_bounded_terms(len(rec), rec.ctypes.data, len(wp), wp.ctypes.data, k.ctypes.data, y.ctypes.data) == 0
    return int(k[0]), y


def _params(rng, m, scale=1.0, log_sigma=(0.7, 1.1)):
    return np.stack([rng.normal(0, 3 * scale, m), 10.0 ** rng.uniform(*log_sigma, m), rng.normal(0, 3 * scale, m),
                     rng.normal(0, 3 * scale, m)], axis=1)


def test_guard_holds_term_by_term_cpu(lib):
    """Random catalogues and parameter tables: wherever the bounded verdict holds, every (star, walker) term has k at or
    above kExpTabKMin and its mixture value inside [y_lo, y_hi], with R log2(y_hi) and 1 + R (-log2 y_lo) within 1000."""
    rng = np.random.default_rng(20261016)
    admitted = {16: 0, 32: 0}
    refused = 0
    for trial in range(60):
        n = int(rng.integers(50, 600))
        cat, centre = _catalog(rng, n, config=int(rng.choice([2, 3])))
        # stretch the catalogue towards the edges of the domain: tiny errors, outliers, confident members
        cat["verr"] = cat["verr"] * 10.0 ** rng.uniform(-0.7, 0.3)
        if rng.random() < 0.5:
            cat["v"] = cat["v"] + rng.normal(0, 1, n) * 10.0 ** rng.uniform(0.0, 1.7)
        cat["pmember"] = np.minimum(cat["pmember"] ** rng.uniform(0.2, 1.5), 1.0 - 2.0 ** -rng.uniform(2, 30))
        cat["lnlike_bg"] = cat["lnlike_bg"] + rng.uniform(-25.0, 3.0)
        params = _params(rng, int(rng.integers(4, 40)), scale=10.0 ** rng.uniform(0, 0.7),
                         log_sigma=(float(rng.choice([0.4, 0.75, 0.75])), 1.3))
        R, info = _verdict(lib, cat, params)
        if R == 0:
            refused += 1
            continue
        assert R in (16, 32) and info["level"] == 2
        admitted[R] += 1
        kmin, (ylo, yhi) = _terms(lib, cat, centre, params)
        y_lo = 1.0 - info["pm_max"]
        y_hi = 1.0 + np.exp(info["nbp_max"]) / np.sqrt(info["n_min"])
        assert kmin >= K_EXP_TAB_KMIN
        assert y_lo <= ylo and yhi <= y_hi * (1 + 1e-12), (ylo, yhi, y_lo, y_hi)
        assert R * np.log2(y_hi) <= 1000 and 1 + R * -np.log2(y_lo) <= 1000
    assert admitted[32] > 5 and admitted[16] > 0 and refused > 5, (admitted, refused)


def test_c3_statistics_select_r32_cpu(lib):
    """The bench's own C3 catalogue (1e6 stars) and walkers select R = 32; one pmember == 0 star, one 60-sigma outlier or
    a tiny sigma_min each turn the variant off while level 2 stays."""
    from mcmc_dynamics_amd import synthetic
    cat, centre = _catalog(None, 1000000, seed=synthetic.CATALOG_SEED_BASE + 3)
    pos = synthetic.make_walkers(256, ["v_sys", "sigma_max", "v_maxx", "v_maxy"], cat["truth"], config=3)
    R, info = _verdict(lib, cat, pos)
    assert R == 32 and info["level"] == 2, info
    assert 1.0 < info["nbp_min"] < info["nbp_max"] < 14.0
    sub = {k: v[:20000].copy() for k, v in cat.items() if isinstance(v, np.ndarray)}
    assert _verdict(lib, sub, pos)[0] == 32
    zero = {k: v.copy() for k, v in sub.items()}
    zero["pmember"][123] = 0.0
    R, info = _verdict(lib, zero, pos)
    assert R == 0 and info["level"] == 2 and info["nbp_min"] == -2000.0
    outlier = {k: v.copy() for k, v in sub.items()}
    i = int(np.argmin(outlier["verr"]))
    sig = np.sqrt(outlier["verr"][i] ** 2 + pos[:, 1].min() ** 2)
    outlier["v"][i] += 60.0 * sig + np.abs(outlier["v"]).max()
    R, info = _verdict(lib, outlier, pos)
    assert R == 0 and info["level"] == 2
    tiny = pos.copy()
    tiny[0, 1] = 1.0                              # sigma_min of 1 km/s: d_max^2 / (2 n_min) far beyond 700
    R, info = _verdict(lib, sub, tiny)
    assert R == 0 and info["level"] == 2 and info["n_min"] < 2.0


@pytest.mark.parametrize("n", [1, 7, 8, 12, 15, 16, 20, 24, 31, 32, 36, 40, 63, 64, 100, 248, 255, 256, 264, 4099])
@pytest.mark.parametrize("iters", [2, 4])
def test_bounded_loop_is_bitwise_level2_cpu(lib, n, iters):
    """Inside the domain the bounded loop (rescale every 8 `iters` factors) gives the level-2 loop's bits, for chunk lengths
    that are and are not multiples of 8, 16 and 32."""
    rng = np.random.default_rng(4400 + 10 * n + iters)
    cat, centre = _catalog(rng, n)
    params = _params(rng, 16)
    assert _verdict(lib, cat, params)[0] >= 8 * iters
    rec = E.pack_records(cat, 1, centre)
    wp = E.pack_walkers(params, 1, False)
    out = np.empty(2 * len(wp))
    assert lib.emul_bounded_chunk(n, rec.ctypes.data, len(wp), wp.ctypes.data, iters, out.ctypes.data) == 0
    out = out.reshape(-1, 2)
    assert np.array_equal(out[:, 0], out[:, 1])
    assert np.all(np.isfinite(out))


@pytest.mark.gpu
def test_c3_shape_bounded_matches_level2_and_oracle():
    """C3: 1e6 stars x 256 walkers run the bounded loop (R = 32), with the same bits as the forced level-2 loop; both match
    the NumPy oracle on a 1e5-star x 16-walker slice.  One extreme outlier sends the catalogue back to the clamped loop."""
    from mcmc_dynamics_amd import _native as native
    from mcmc_dynamics_amd import synthetic
    from oracle import lnprob_numpy as oracle
    ctx = native.default_context()
    cat = synthetic.make_catalog(1000000, config=3, seed=synthetic.CATALOG_SEED_BASE + 3, background=True)
    pos = synthetic.make_walkers(256, ["v_sys", "sigma_max", "v_maxx", "v_maxy"], cat["truth"], config=3)
    centre = (synthetic.CENTER_RA_DEG, synthetic.CENTER_DEC_DEG)
    lnbg = oracle.gaussian_background(cat["v"], cat["verr"], 20.0, 40.0)

    def make(c, lb):
        return native.Catalog(ctx, c["ra"], c["dec"], c["v"], c["verr"], model=native.MODEL_CONST_BGFIXED, centre=centre,
                              lnlike_bg=lb, pmember=c["pmember"])

    full = make(cat, lnbg)
    a = full.loglike(pos)
    assert full.fast_level == 2 and full.last_prefetch == 1 and full.last_narrow_bounded == 32
    full.set_option("narrow_bounded", 0)
    b = full.loglike(pos)
    assert full.fast_level == 2 and full.last_narrow_bounded == 0
    assert np.array_equal(a, b)
    full.close()

    sl = slice(0, 100000)
    sub = {k: v[sl] for k, v in cat.items() if isinstance(v, np.ndarray)}
    want = oracle.batched_constant_lnlike(sub, pos[:16], *centre, lnlike_background=lnbg[sl], pmember=sub["pmember"])
    for bounded in (1, 0):
        part = make(sub, lnbg[sl])
        part.set_option("prefetch", 1)
        part.set_option("narrow_bounded", bounded)
        got = part.loglike(pos[:16])
        assert part.fast_level == 2 and part.last_narrow_bounded == (32 if bounded else 0)
        part.close()
        assert rel_err(got, want) < 1e-12

    far = {k: v.copy() for k, v in cat.items() if isinstance(v, np.ndarray)}
    far["v"][4321] = 600.0                       # ~90 sigma from every walker's systemic velocity
    lnbg_far = oracle.gaussian_background(far["v"], far["verr"], 20.0, 40.0)
    c = make(far, lnbg_far)
    got = c.loglike(pos)
    assert c.fast_level == 2 and c.last_prefetch == 1 and c.last_narrow_bounded == 0
    c.set_option("fast_path", 0)
    plain = c.loglike(pos)
    c.close()
    assert rel_err(got, plain) < 1e-11

"""The quadratic series root on 32-star bands of the level-2 BGFIXED fixed-centre loops (option "root_quad"; csrc/mcd_math.h:
RootQuad, csrc/mcd_exp_split.h: quad_block .. quad_chunk_width, csrc/mcd_chunks.h: quad_thresholds) on the CPU build of the
kernels' arithmetic (tests/emul): the economisation and the whole root against numpy.longdouble, the third vote, the block
constants and chunk widths of a sorted column, and the three loop shapes against each other and against the split loop."""
import numpy as np
import pytest

import emul_helper as emul
import root_direct_helper as rd
import root_quad_helper as rq
import root_series_helper as rs
from mcmc_dynamics_amd import synthetic
from oracle import lnprob_numpy as oracle
from test_root_direct_cpu import _samples

L = np.longdouble
HAVE_LONGDOUBLE = np.finfo(L).eps < 1e-18
U = 2.0 ** -53
NAMES4 = ["v_sys", "sigma_max", "v_maxx", "v_maxy"]
CENTRE = (synthetic.CENTER_RA_DEG, synthetic.CENTER_DEC_DEG)


def test_threshold_and_the_derived_bound_are_inside_what_the_issue_allows():
    assert rq.max_t() == float.fromhex("0x1.6a09e667f3bcdp-18") == 2.0 ** -17.5
    assert rd.error_bound() < rq.error_bound() <= 5.9e-16


@pytest.mark.skipif(not HAVE_LONGDOUBLE, reason="needs an 80-bit long double")
def test_economisation_alone_against_longdouble():
    """|quadratic - cubic| / g in 80-bit arithmetic, with the cubic's own c3 = -5/16 G q^3 and the block's a2, a1, a0 from m
    and h: at most |c3| h^3 / 4 = (5/64) (h q)^3 G = 0.111 u of g for h q <= 2^-17.5; the issue's ceiling is 0.12 u.
    Blocks inside a chunk band |t| <= 2^-13, rho <= 1/8, the points of a block including the four where |T3| = 1."""
    rng = np.random.default_rng(31)
    n = 4000
    s2 = L(rng.uniform(0.5, 200.0, n))
    rho = L(np.where(rng.random(n) < 0.25, 0.125, rng.uniform(0.0, 0.125, n)))
    eb = rho / (1 - rho) * s2
    hq = L(rq.max_t()) * L(np.where(rng.random(n) < 0.5, 1.0, rng.random(n)))
    t = (L(2.0) ** -13 - hq) * L(rng.uniform(-1.0, 1.0, n))
    m, h = eb + t * (eb + s2), hq * (eb + s2)
    worst = 0.0
    for x in (L(-1.0), L(-0.5), L(0.5), L(1.0), L(rng.uniform(-1.0, 1.0, n))):
        e = m + h * x
        G, q = 2 / np.sqrt(8 * (eb + s2)), 1 / (eb + s2)
        c3 = -G * q ** 3 * 5 / 16
        a2, a1, a0 = 3 * m, L(0.75) * h * h - 3 * m * m, m ** 3 - L(0.75) * h * h * m
        g = 1 / np.sqrt(2 * (e + s2))
        worst = max(worst, float(np.max(np.abs(c3 * ((a2 * e + a1) * e + a0 - e ** 3)) / g)))
    print("economisation: largest |quadratic - cubic| / g = {0:.4f} u".format(worst / U))
    assert worst <= 0.12 * U


@pytest.mark.skipif(not HAVE_LONGDOUBLE, reason="needs an 80-bit long double")
def test_quad_root_against_longdouble():
    """Relative error of g_quad (scaled by c, as the split loop uses it) against c (2 (e + s2))^(-1/2) in long double on the
    inputs of test_root_direct_cpu._samples, each e inside a block of half-width up to 2^-17.5 (eb + s2) (on the threshold for
    a quarter of the sample, e anywhere in the block, its ends included): no greater than the bound derived in the comment
    of RootQuad.

    Measured over this sample (printed below; quoted in DESIGN 3.2): max 2.87e-16, against 2.85e-16 for the scaled cubic of
    RootDirectSplit and 2.87e-16 for the unscaled RootDirect on the same inputs."""
    eb, s2, e = _samples(21, 400000)
    rng = np.random.default_rng(23)
    n = eb.size
    h = rq.max_t() * (eb + s2) * np.where(rng.random(n) < 0.25, 1.0, rng.random(n))
    x = np.where(rng.random(n) < 0.25, rng.choice([-1.0, 1.0], n), rng.uniform(-1.0, 1.0, n))
    e_lo, e_hi = e - h * (1.0 + x), e + h * (1.0 - x)                         # e = m + h x
    keep = e_lo > 0.0
    eb, s2, e, e_lo, e_hi = eb[keep], s2[keep], e[keep], e_lo[keep], e_hi[keep]
    assert eb.size > 300000
    quad, cubic = rq.quad_root(eb, s2, e_lo, e_hi, e)
    want = L(rq.scale()) / np.sqrt(2.0 * (L(e) + L(s2)))
    err_quad = np.abs((L(quad) - want) / want).astype(np.float64)
    err_cubic = np.abs((L(cubic) - want) / want).astype(np.float64)
    direct = rd.direct_root(eb, s2, e)[0]
    err_direct = np.abs((L(direct) * L(rq.scale()) - want) / want).astype(np.float64)
    print("max rel err: quadratic {0:.3e} (median {1:.3e}), scaled cubic {2:.3e}, RootDirect {3:.3e}; derived bound {4:.2e}"
          .format(err_quad.max(), np.median(err_quad), err_cubic.max(), err_direct.max(), rq.error_bound()))
    assert err_quad.max() <= rq.error_bound()


def test_third_vote():
    rng = np.random.default_rng(7)
    for _ in range(2000):
        eb = 2.0 ** rng.uniform(-20, 20)
        s2 = eb * 2.0 ** rng.uniform(3, 12)
        H = rq.max_t() * (eb + s2)
        assert rq.quad_ok(H * (1.0 - 1e-9), eb, s2) and not rq.quad_ok(H * (1.0 + 1e-9), eb, s2)
        assert rq.quad_ok(0.0, eb, s2)                                         # a block of equal verr
    assert not rq.quad_ok(np.nan, 1.0, 100.0) and not rq.quad_ok(1e-9, np.nan, 100.0) and not rq.quad_ok(1e-9, 1.0, np.nan)
    assert not rq.quad_ok(np.inf, 1.0, 100.0)                                  # a chunk that cannot take the form


def _block_ends(n):
    nb = n // 32
    return [(32 * b, n - 1 if b == nb - 1 else 32 * b + 31) for b in range(nb)]


@pytest.mark.parametrize("n", [31, 32, 33, 63, 64, 20011])
def test_block_constants_and_their_slots(n):
    """Blocks in absolute positions, the last one taking the remainder (32 .. 63 stars); a2, a1, a0 rounded once from long
    double; a2 and a1 in slots 6 and 7 of the block's first split record, a0 in slot 6 of its second, zeros elsewhere."""
    rng = np.random.default_rng(n)
    e2 = np.sort(rng.uniform(0.5, 1.5, n) ** 2)
    if n >= 64:
        e2[32:64] = e2[32]                                                    # duplicates: a block of equal verr
        e2 = np.sort(e2)
    got = rq.blocks(e2)
    ends = _block_ends(n)
    assert got.shape[0] == len(ends) == n // 32
    slots = rq.slots(e2)
    want_slots = np.zeros((n, 2))
    for b, (i0, i1) in enumerate(ends):
        assert i1 - i0 + 1 >= 32 and (b < len(ends) - 1 or i1 == n - 1)
        m, h = (L(e2[i0]) + L(e2[i1])) / 2, (L(e2[i1]) - L(e2[i0])) / 2
        want = [3 * m, L(0.75) * h * h - 3 * m * m, m ** 3 - L(0.75) * h * h * m, h]
        if HAVE_LONGDOUBLE:
            assert [float(w) for w in want] == list(got[b])
        else:
            assert np.allclose([float(w) for w in want], got[b], rtol=1e-15)
        want_slots[i0], want_slots[i0 + 1, 0] = got[b, :2], got[b, 2]
    assert np.array_equal(slots, want_slots)
    if n >= 64:
        assert got[1, 3] == 0.0 and got[1, 1] == pytest.approx(-3.0 * e2[32] ** 2, rel=1e-15)       # h = 0: a1 = -3 m^2


def test_chunk_widths_and_thresholds():
    """H of a chunk: the largest h of the blocks it touches, whatever its start inside a block (0, 8 and 24 past a boundary),
    the tail chunk in the last block's remainder; +inf where no block exists or the start is no multiple of 8.  The
    smallest sigma^2 for the quadratic form is no smaller than the direct form's, chunk by chunk."""
    n = 20011
    e2 = np.sort(np.random.default_rng(5).uniform(0.2, 2.5, n) ** 2)
    h = np.array([0.5 * (e2[i1] - e2[i0]) for i0, i1 in _block_ends(n)])
    nb = n // 32
    cuts = np.array([0, 40, 88, 160, 416, 420, 1000, 19968, 20000, n])     # 40 = 32 + 8, 88 = 64 + 24, 420: no multiple of 8
    p = rq.plan(e2, cuts)
    for c in range(cuts.size - 1):
        first, last = min(cuts[c] // 32, nb - 1), min((cuts[c + 1] - 1) // 32, nb - 1)
        want = np.inf if cuts[c] % 8 else h[first:last + 1].max()
        assert p["H"][c] == want, (c, p["H"][c], want)
    assert p["H"][5] == np.inf and p["need_quad"][5] == np.inf
    assert p["H"][7] == h[nb - 1] == p["H"][8]                                 # both inside the last block (32 .. 63 stars)
    assert (p["need_quad"] >= p["need_direct"]).all()
    assert np.array_equal(p["sorted_quad"], np.sort(p["need_quad"])) and np.array_equal(p["sorted_direct"], np.sort(p["need_direct"]))
    assert (p["sorted_quad"] >= p["sorted_direct"]).all()
    for c in (0, 1, 2, 3):                                                     # the threshold is where the vote turns
        eb = 0.5 * e2[cuts[c]] + 0.5 * e2[cuts[c + 1] - 1]
        need = p["H"][c] / rq.max_t() - eb
        assert rq.quad_ok(p["H"][c], eb, need * (1.0 + 1e-9)) and not rq.quad_ok(p["H"][c], eb, need * (1.0 - 1e-9))
        assert p["need_quad"][c] == pytest.approx(max(need, p["need_direct"][c]), rel=1e-12)
    short = rq.plan(e2[:31], np.array([0, 16, 31]))
    assert (short["H"] == np.inf).all()


@pytest.fixture(scope="module")
def tight():
    """the catalogue of tests/test_gpu_root_quad.py, packed and sorted by verr"""
    n = 20011
    cat = synthetic.make_catalog(n, config=3, seed=synthetic.CATALOG_SEED_BASE + 3, background=True)
    cat["verr"][:12000] = 1.0 + 5e-4 * np.random.default_rng(13).random(12000)
    cat["lnlike_bg"] = oracle.gaussian_background(cat["v"], cat["verr"], 20.0, 40.0)
    pos = synthetic.make_walkers(130, NAMES4, cat["truth"], config=3)
    rec = emul.pack_records(cat, 1, CENTRE)
    return rec[rs.verr_order(rec)], pos


@pytest.mark.parametrize("offset,count", [(8, 72), (8, 76), (8, 77), (0, 64), (24, 40), (16, 13)])
def test_loop_shapes_agree_bit_for_bit_and_with_the_split_loop(tight, offset, count):
    """One chunk in the tight verr band, beginning `offset` past a block boundary: 72 stars (nine 8-star iterations over
    three blocks), 76 (a 4-star group at the end), 77 (a single-star tail) and shorter ones whose 4-star group or tail starts
    ON a boundary.  The 4-star, the 8-star and the bounded loop return the same bits; the chunk sum agrees with the split
    loop's to 1e-14 relative."""
    rec, pos = tight
    first = int(np.searchsorted(rec[:, 1], 1.0))
    begin = (first // 32 + 3) * 32 + offset
    assert rec[begin + count - 1, 1] <= 1.001
    for iters in (1, 4):
        out, took = rq.chunk(rec, begin, count, pos, rescale_iters=iters)
        assert took.all() and np.isfinite(out).all()
        assert np.array_equal(out[:, 0], out[:, 1]) and np.array_equal(out[:, 1], out[:, 2])
        err = np.max(np.abs(out[:, 0] - out[:, 3]) / np.abs(out[:, 3]))
        assert err <= 1e-14, err
        assert not np.array_equal(out[:, 0], out[:, 3]) or count < 16          # (another rounding somewhere in 72 x 130 terms)


def test_last_block_remainder_and_refused_chunks(tight):
    """A chunk in the remainder behind the last block's first 32 records keeps that block's constants; a chunk whose start is
    no multiple of 8, or one that fails a vote, takes the split loop (or another), bit for bit as without the option."""
    rec, pos = tight
    first = int(np.searchsorted(rec[:, 1], 1.0))
    n_cut = (first // 32 + 40) * 32 + 24                                       # an array that ends 24 records into a remainder
    sub = rec[:n_cut]
    out, took = rq.chunk(sub, n_cut - 24 - 32 - 8, 8 + 32 + 24, pos)           # crosses into the last block and its remainder
    assert took.all() and np.array_equal(out[:, 0], out[:, 1]) and np.array_equal(out[:, 1], out[:, 2])
    assert np.max(np.abs(out[:, 0] - out[:, 3]) / np.abs(out[:, 3])) <= 1e-14
    out, took = rq.chunk(sub, n_cut - 16, 16, pos)                             # wholly inside the remainder
    assert took.all() and np.array_equal(out[:, 0], out[:, 2])
    assert np.max(np.abs(out[:, 0] - out[:, 3]) / np.abs(out[:, 3])) <= 1e-14
    begin = (first // 32 + 3) * 32
    out, took = rq.chunk(rec, begin + 4, 72, pos)                              # start no multiple of 8: never
    assert not took.any() and np.array_equal(out[:, 1], out[:, 3]) and np.array_equal(out[:, 0], out[:, 2])
    low = pos.copy()
    low[:, 1] = np.sqrt(7.0 * rec[begin + 36, 1] * (1.0 - 1e-6))               # the direct vote fails
    out, took = rq.chunk(rec, begin, 72, low)
    assert not took.any() and np.array_equal(out[:, 0], out[:, 1]) and np.array_equal(out[:, 1], out[:, 2])


def test_chunk_that_passes_the_direct_vote_and_fails_the_third_takes_the_split_loop():
    """The third vote itself, through chunk_loglike: the catalogue of tests/test_gpu_root_quad.py with its front band at
    verr = 2.8 .. 3.0 instead of 1 .. 1.0005 (the wide catalogue of that file) and the benchmark's walkers (sigma^2 from 68.6, here up to 81).
    Its 64-star chunks in the band are narrow enough for the series (half-width <= 2^-13 (eb + s2)) and pass the direct vote
    (7 eb <= 63), while their 32-star blocks are at least 2.5 times wider than 2^-17.5 (eb + s2): every such chunk runs the
    split loop, bit for bit, in all three shapes, and never reads a block constant (`took` is observed from the call)."""
    n = 20011
    cat = synthetic.make_catalog(n, config=3, seed=synthetic.CATALOG_SEED_BASE + 3, background=True)
    cat["verr"][:12000] = 2.8 + 0.2 * np.random.default_rng(13).random(12000)
    cat["lnlike_bg"] = oracle.gaussian_background(cat["v"], cat["verr"], 20.0, 40.0)
    pos = synthetic.make_walkers(130, NAMES4, cat["truth"], config=3)
    pos[:, 1] = np.minimum(pos[:, 1], 9.0)          # (the emulation's lanes vote each for itself: the third must fail in every one)
    s2 = float((pos[:, 1] ** 2).min())
    rec = emul.pack_records(cat, 1, CENTRE)
    rec = rec[rs.verr_order(rec)]
    e2 = rec[:, 1]
    first = int(np.searchsorted(e2, 2.8 ** 2))
    found = 0
    for begin in range((first // 64 + 1) * 64, n - 64, 64 * 40):
        c = e2[begin:begin + 64]
        if c[-1] > 9.0:
            break
        eb, half = 0.5 * c[0] + 0.5 * c[-1], 0.5 * (c[-1] - c[0])
        assert half <= 2.0 ** -13 * (eb + s2) * (1.0 - 1e-9) and 7.0 * eb <= s2 * (1.0 - 1e-9)      # series and direct pass
        h = max(0.5 * (c[31] - c[0]), 0.5 * (c[63] - c[32]))
        assert h > 2.0 * rq.max_t() * (eb + 81.0)                                                   # the third fails in every lane
        for offset, count in ((0, 64), (8, 77)):
            out, took = rq.chunk(rec, begin + offset, count, pos)
            assert not took.any() and np.isfinite(out).all()
            for col in range(3):
                assert np.array_equal(out[:, col], out[:, 3]), (begin, offset, col)
        found += 1
    assert found >= 3

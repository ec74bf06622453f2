"""The split exponent offset of the direct BGFIXED loops (option "exp_split"; csrc/mcd_math.h: BgFixedAcc::add_gs,
csrc/mcd_exp_split.h, csrc/mcd_guard.h: exp_split_admitted) on the CPU build of the kernels' arithmetic (tests/emul): the
record split, the reduced argument on ties, the per-term error against long double, the chunk constants, whole chunks
against the parent's direct form, and the guard."""
import numpy as np
import pytest

import emul_helper as emul
import exp_split_helper as xs
import root_series_helper as rs
from mcmc_dynamics_amd import synthetic
from oracle import lnprob_numpy as oracle

L = np.longdouble
HAVE_LONGDOUBLE = np.finfo(L).eps < 1e-18
NAMES4 = ["v_sys", "sigma_max", "v_maxx", "v_maxy"]
CENTRE = (synthetic.CENTER_RA_DEG, synthetic.CENTER_DEC_DEG)
K = xs.constants()
N = K["N"]
INV_STEP = N / np.log(2.0)


def _c3(n):
    cat = synthetic.make_catalog(n, config=3, seed=synthetic.CATALOG_SEED_BASE + 3, background=True)
    cat["lnlike_bg"] = oracle.gaussian_background(cat["v"], cat["verr"], 20.0, 40.0)
    return cat


def _nbp_samples():
    """nbp over [-2000, 60]: the floor, the ends, a uniform sample, and values whose nbp N / ln 2 lies within 1e-9 of a
    half-integer (both sides, both parities of the integer below)"""
    rng = np.random.default_rng(11)
    halves = (np.round(rng.uniform(-2000.0, 60.0, 4000) * INV_STEP) + 0.5 + rng.uniform(-1e-9, 1e-9, 4000)) / INV_STEP
    return np.concatenate([[-2000.0, 60.0, 0.0, -0.0, 1e-300], rng.uniform(-2000.0, 60.0, 20000), np.clip(halves, -2000.0, 60.0)])


def test_record_split():
    nbp = _nbp_samples()
    M, ompk, nbf, back = xs.record(nbp, 0.75)
    steps = M - xs.MAGIC
    assert (steps == np.round(steps)).all() and (np.abs(steps) < 2.0 ** 31).all()          # M - 1.5 2^52 is an integer
    assert (np.abs(nbf) <= 0.5).all()
    near = np.abs(np.abs(nbf) - 0.5) < 2e-9
    assert near.sum() >= 3000, near.sum()                                                   # the half-integer cases are met
    assert (back <= 1e-18 * np.maximum(1.0, np.abs(nbp))).all(), (back / np.maximum(1.0, np.abs(nbp))).max()
    # omp' = kappa omp with kappa = (c / 32) e^{-nbf ln2/N}, inside (c / 32) (1 +- 3.4e-4) = 1.2011 (1 +- 3.4e-4)
    kappa = ompk / 0.75
    assert (np.abs(kappa / (K["c"] / 32.0) - 1.0) <= 3.4e-4).all()
    assert np.allclose(kappa, K["c"] / 32.0 * np.exp(-nbf * np.log(2.0) / N), rtol=4e-16, atol=0.0)
    assert np.log2(kappa.max()) <= K["log2_kappa_max"]


def test_ties_of_the_rounding_constant():
    """dgs^2 on a half-integer, where shifted = M - dgs^2 would tie.  The square of a double is never exactly a
    half-integer (its denominator is an even power of two), and the FMA rounds M - dgs^2 from the exact square: so the
    closest the loop can come to a tie is dgs = the double next to sqrt(m + 1/2), dgs^2 within 2^-52 (m + 1/2) of it, on
    either side.  Checked against exact rational arithmetic: the low word of shifted is nbi - 5 N + rint(-dgs^2) taken on
    the exact sum, |rv| <= 1/2, and rv is -dgs^2 - w rounded once."""
    from fractions import Fraction
    rng = np.random.default_rng(5)
    q = rng.integers(0, 1 << 20, 6000).astype(np.float64) + 0.5
    dgs = np.sqrt(q)
    dgs = np.where(rng.random(q.size) < 0.5, dgs, np.nextafter(dgs, np.where(dgs * dgs > q, 0.0, np.inf)))
    generic = np.sqrt(rng.uniform(0.0, 3.0e4, 4000))
    dgs = np.concatenate([dgs, generic])
    nbp = rng.uniform(-700.0, 60.0, dgs.size)
    M, _, _, _ = xs.record(nbp, 0.5)
    k, rv = xs.reduce(dgs, M)
    assert (np.abs(rv) <= 0.5).all()
    sides = set()
    for i in range(dgs.size):
        sq = Fraction(float(dgs[i])) ** 2
        total = Fraction(float(M[i] - xs.MAGIC)) - sq               # nbi - 5 N - dgs^2, exact
        assert total.denominator != 2                                # (never an exact tie)
        assert int(k[i]) == round(total), i
        w = int(k[i]) - int(M[i] - xs.MAGIC)
        exact_rv = -sq - w
        assert abs(exact_rv) <= Fraction(1, 2)
        assert abs(Fraction(float(rv[i])) - exact_rv) <= Fraction(1, 1 << 54), i
        if i < q.size:
            assert abs(sq - Fraction(float(q[i]))) <= Fraction(float(q[i])) / (1 << 50)
            sides.add(sq > Fraction(float(q[i])))
    assert sides == {True, False}


def _c3_terms(n_stars=20011, n_walkers=32, chunk_len=96):
    """(eb, s2, e, d, nbp, omp) of the (star, walker) terms of a C3 catalogue as the kernel meets them: records sorted by
    verr, chunks of ``chunk_len`` with their midpoint centre, the benchmark's walker ball; d = v - v_sys (the rotation
    term, a few km/s, left out), restricted to the terms whose chunk passes both of the lane's votes."""
    cat = _c3(n_stars)
    pos = synthetic.make_walkers(256, NAMES4, cat["truth"], config=3)[:n_walkers]
    rec = emul.pack_records(cat, 1, CENTRE)
    rec = rec[rs.verr_order(rec)]
    e = rec[:, 1]
    first = (np.arange(n_stars) // chunk_len) * chunk_len
    last = np.minimum(first + chunk_len - 1, n_stars - 1)
    eb = 0.5 * e[first] + 0.5 * e[last]
    half = 0.5 * (e[last] - e[first])
    s2 = pos[:, 1] ** 2
    EB, S2 = np.meshgrid(eb, s2, indexing="ij")
    HALF = np.meshgrid(half, s2, indexing="ij")[0]
    E = np.meshgrid(e, s2, indexing="ij")[0]
    D = rec[:, 0][:, None] - pos[:, 0][None, :]
    NBP = np.meshgrid(rec[:, 7], s2, indexing="ij")[0]
    OMP = np.meshgrid(rec[:, 6], s2, indexing="ij")[0]
    ok = (8.0 * HALF <= 2.0 ** -13 * 8.0 * (EB + S2)) & (7.0 * EB <= S2)
    return [x[ok] for x in (EB, S2, E, D, NBP, OMP)]


@pytest.mark.skipif(not HAVE_LONGDOUBLE, reason="needs an 80-bit long double")
def test_per_term_error_against_long_double():
    """Largest relative error of one mixture value y = (1 - p) + g e^u over >= 4e5 terms of a C3 catalogue, the parent's
    direct form and the split form (kappa divided out in long double), both through the kernels' own code with the
    exponent-biased table: the split form may exceed the parent's by one ulp (1.11e-16) at most -- the scaled c0 is its
    one extra rounding.  Figures printed below and quoted in DESIGN 3.2."""
    eb, s2, e, d, nbp, omp = _c3_terms()
    assert eb.size >= 400000, eb.size
    ep, es = xs.term_error(eb, s2, e, d, nbp, omp)
    print("terms {0}: nbp {1:.2f} .. {2:.2f}, omp {3:.3f} .. {4:.3f}, d^2 g^2 up to {5:.1f}".format(
        eb.size, nbp.min(), nbp.max(), omp.min(), omp.max(), (d * d / (2 * (e + s2))).max()))
    print("max rel err per term: parent direct {0:.3e} (median {1:.3e}), split {2:.3e} (median {3:.3e})".format(
        ep.max(), np.median(ep), es.max(), np.median(es)))
    assert es.max() <= ep.max() + 1.11e-16


@pytest.mark.skipif(not HAVE_LONGDOUBLE, reason="needs an 80-bit long double")
def test_chunk_constants_sum_to_the_extended_precision_total():
    rng = np.random.default_rng(8)
    nbp = rng.uniform(1.0, 13.5, 1000)
    cuts = np.array([0, 1, 14, 97, 98, 331, 500, 777, 993, 1000])
    consts, nbf = xs.chunk_consts(nbp, cuts)
    total = (L(nbf).sum() * (np.log(L(2.0)) / N)) - L(1000) * np.log(L(K["c"]) / L(32.0))
    assert abs(float((L(consts).sum() - total) / total)) <= 1e-15
    one, _ = xs.chunk_consts(nbp, np.array([0, 1000]))
    assert abs(float((L(one[0]) - total) / total)) <= 1e-15


@pytest.mark.parametrize("count", [416, 13])
def test_chunk_emulation_matches_the_parent_direct_form(count):
    """One chunk, every lane in the direct form: 416 stars, and 13 stars (one 8-star iteration, one 4-star group, one
    single star).  Sum of log y: split against the parent's direct form within 1e-13 relative; the level-2 prefetch loop
    and the bounded loop bit for bit equal to each other in either form."""
    cat = _c3(80000)                     # (dense enough in verr^2 for a 416-star chunk to pass the series' vote)
    pos = synthetic.make_walkers(64, NAMES4, cat["truth"], config=3)
    rec = emul.pack_records(cat, 1, CENTRE)
    rec = rec[rs.verr_order(rec)][12000:12000 + count]
    s2 = pos[:, 1] ** 2
    eb = 0.5 * rec[0, 1] + 0.5 * rec[-1, 1]
    assert (7.0 * eb <= s2).all() and (rec[-1, 1] - rec[0, 1]) * 4.0 <= 2.0 ** -13 * 8.0 * (eb + s2.min())
    out = xs.chunk(rec, pos)
    assert np.isfinite(out).all()
    assert np.array_equal(out[:, 0], out[:, 2]) and np.array_equal(out[:, 1], out[:, 3])
    err = np.max(np.abs(out[:, 1] - out[:, 0]) / np.abs(out[:, 0]))
    print("count {0}: split vs parent direct form {1:.2e}".format(count, err))
    assert err <= 1e-13


def test_guard():
    cat = _c3(20011)
    pos = synthetic.make_walkers(256, NAMES4, cat["truth"], config=3)
    R, bounded, clamp = xs.guard(cat, pos)
    assert R == 32 and bounded and clamp                                   # C3's own statistics: well inside
    width = 32.0 * K["log2_kappa_max"]
    assert 8.4 < width < 8.5
    # 32 hi2 within 32 log2 kappa_max below 1000: bounded_rescale still returns 32, the split form is refused there
    for r in (1000.0 - 0.01 * width, 1000.0 - 0.5 * width, 1000.0 - 0.99 * width):
        R, bounded, clamp = xs.guard(cat, pos, r_hi2=r)
        assert R == 32 and not bounded and clamp, r
    R, bounded, clamp = xs.guard(cat, pos, r_hi2=1000.0 - 1.01 * width)
    assert R == 32 and bounded and clamp
    R, bounded, clamp = xs.guard(cat, pos, r_hi2=700.0)
    assert R == 32 and bounded and clamp
    # the clamp: k at u = -700 with the 5 N shift stays above the table's floor
    # (the guard's note on the clamp puts k at u = -700 at -1034127, three steps below rint(-700 N / ln 2): kept as it is)
    assert K["k_min_bounded"] == -1034127 - 5 * N == -1039247 and K["k_min_bounded"] <= int(np.rint(-700.0 * INV_STEP)) - 5 * N
    assert K["k_min_bounded"] > K["k_min_table"] == -1021 * N

"""Test helper: the device harness around psis_row (tests/psis_row_harness: csrc/mcd_psis_row.h on rows given by the
caller), the NumPy oracle in the same general form (ratio, lnl, M, loo) -- psis_helper.psis_star and mmatch_helper.psis_lw
with the tail length passed in -- and the crafted rows the wave-level selection is pinned on.  Test infrastructure only.

The selection of psis_row: an 8-digit radix select of the (M+1)-th largest key (psis_key of lw = ratio - max ratio), left
early when the cutoff is the only candidate; an index scan among equal keys; a ballot gather of the tail in 64-sample
blocks; a rank sort by (key, index).  A tail sample's weight is psis_smoothed(rank), so the per-sample weights show who
received which rank, which no sum over the row can: swapping two keys one ulp apart moves elpd by 1e-16."""
import ctypes
import functools
import math
import os
import subprocess

import numpy as np

import psis_helper as psh

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HARNESS_DIR = os.path.join(ROOT, "tests", "psis_row_harness")
HARNESS = os.path.join(HARNESS_DIR, "libpsis_row_harness.so")
MAX_TAIL = 2560                                        # csrc/mcd_psis.h: kPsisMaxTail
ROW_FIELDS = ("khat", "mw", "m2", "a1", "a2", "a3", "a4", "lmax")      # csrc/mcd_psis_row.h: PsisRow
# the bounds (psis_helper.assert_matches' and the new one on the weights)
ELPD_TOL, K_TOL, LPPD_TOL, NEFF_TOL = 1e-11, 1e-10, 1e-12, 1e-9
# per-sample log weights: the k^ tolerance times the sensitivity of psis_smoothed to k^, |log(1 - p)| <= log(2 M) < 10
LOGW_TOL = 1e-9
# what the oracle's neighbouring tail log weights must differ by for LOGW_TOL to see two ranks swapped
MIN_GAP = 1e-6
# rows with -inf ratios: values are compared when the oracle's k^ moves by less than this under one-ulp changes of its input
INF_VALUES_NOISE = 1e-11
_harness = None


def build_harness(out=None):
    """make -C tests/psis_row_harness (hipcc cross-compiles for gfx950 without a GPU); returns the library's path."""
    cmd = ["make", "-C", HARNESS_DIR] + (["OUT=" + out] if out else [])
    res = subprocess.run(cmd, capture_output=True, text=True)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-3000:]
    return out or HARNESS


def harness():
    global _harness
    if _harness is None:
        lb = ctypes.CDLL(build_harness())
        lb.psis_row_harness.argtypes = [ctypes.c_int64, ctypes.c_int64, ctypes.c_int64, ctypes.c_int] + [ctypes.c_void_p] * 4
        lb.psis_row_harness.restype = ctypes.c_int
        _harness = lb
    return _harness


def harness_lds_bytes(M):
    """csrc/mcd_psis_row.h: psis_tail_lds_bytes -- hist[256] u32, key / skey [M] u64, idx / sidx [M] i32, two GPD grids
    of kPsisMaxGrid = 96 doubles."""
    return 256 * 4 + M * (8 + 8 + 4 + 4) + 2 * 96 * 8


def xstar_index(M):
    """csrc/mcd_psis.h: gpd_xstar_index -- the 0-based rank in the tail of the quartile entry x* of the GPD fit."""
    return int(math.floor(M / 4.0 + 0.5)) - 1


def run_rows(ratio, lnl, M, loo):
    """psis_row<loo> on the device, one wave per row: dict of the eight PsisRow fields (n,) and "wout" (n, S)."""
    ratio = np.ascontiguousarray(np.atleast_2d(ratio), dtype=np.float64)
    lnl = np.ascontiguousarray(np.atleast_2d(lnl), dtype=np.float64)
    assert ratio.shape == lnl.shape
    n, S = ratio.shape
    fields, wout = np.full((n, 8), np.nan), np.full((n, S), np.nan)
    rc = harness().psis_row_harness(n, S, int(M), int(bool(loo)), ratio.ctypes.data, lnl.ctypes.data, fields.ctypes.data,
                                    wout.ctypes.data)
    assert rc == 0, "psis_row_harness: HIP error {0}".format(rc)
    out = {k: fields[:, i].copy() for i, k in enumerate(ROW_FIELDS)}
    out["wout"] = wout
    return out


def derived(out, S, loo):
    """What the entry points make of a PsisRow, and the log weights shifted so that the row's largest is 0."""
    with np.errstate(divide="ignore", invalid="ignore"):
        lw = np.log(out["wout"])
        d = {"pareto_k": out["khat"], "elpd_loo": (out["m2"] + np.log(out["a3"])) - (out["mw"] + np.log(out["a1"])),
             "n_eff": out["a1"] * out["a1"] / out["a2"],
             "lppd": out["lmax"] + (np.log(out["a4"]) - math.log(S)) if loo else np.full(out["khat"].shape, np.nan),
             "logw": lw - lw.max(axis=1, keepdims=True)}
    return d


# ---- NumPy oracle ------------------------------------------------------------------------------------------------
def row_oracle(ratio, lnl, M, loo):
    """One row in the general form: (k^, elpd, n_eff / r_eff, lppd (nan unless loo), log weights (S,) smoothed, truncated
    and shifted so that the largest is 0, tail log weights (M,) smoothed but not truncated, in rank order (None when
    nothing is smoothed)).  The steps of psis_helper.psis_star / mmatch_helper.psis_lw; the stable argsort is the
    (value, index) rule."""
    ratio, lnl = np.asarray(ratio, dtype=np.float64), np.asarray(lnl, dtype=np.float64)
    S = ratio.size
    with np.errstate(invalid="ignore"):
        lw = ratio - np.max(ratio)
    k_hat, raw = np.inf, None
    if M >= 5:
        order = np.argsort(lw, kind="stable")
        tail = order[S - M:]
        cutoff = lw[order[S - M - 1]]
        vals = lw[tail]
        with np.errstate(all="ignore"):
            if vals.max() - vals.min() < np.finfo(np.float64).eps / 100.0:
                k_hat = -np.inf
            else:
                k_hat, sigma = psh.gpdfit(np.exp(vals) - np.exp(cutoff))
                if np.isfinite(k_hat):
                    p = (np.arange(1, M + 1) - 0.5) / M
                    q = -sigma * np.log1p(-p) if k_hat == 0.0 else sigma * np.expm1(-k_hat * np.log1p(-p)) / k_hat
                    raw = np.log(q + np.exp(cutoff))
                    lw = lw.copy()
                    lw[tail] = raw
    lw = np.minimum(lw, 0.0)
    with np.errstate(divide="ignore"):
        elpd = psh._lse(lw + lnl) - psh._lse(lw)
        w = np.exp(lw - psh._lse(lw))
    lppd = psh._lse(lnl) - np.log(S) if loo else np.nan
    return float(k_hat), float(elpd), float(1.0 / np.sum(w * w)), float(lppd), lw - lw.max(), raw


def rows_oracle(ratio, lnl, M, loo):
    """row_oracle over (n, S): dict pareto_k, elpd_loo, n_eff, lppd (n,), logw (n, S), gap (n,): the smallest difference
    of neighbouring untruncated tail log weights (inf when nothing is smoothed)."""
    ratio, lnl = np.atleast_2d(ratio), np.atleast_2d(lnl)
    rows = [row_oracle(r, l, M, loo) for r, l in zip(ratio, lnl)]
    out = {k: np.array([r[i] for r in rows]) for i, k in enumerate(("pareto_k", "elpd_loo", "n_eff", "lppd"))}
    out["logw"] = np.array([r[4] for r in rows])
    out["gap"] = np.array([np.inf if r[5] is None else float(np.min(np.diff(r[5]))) for r in rows])
    return out


def moved(a, seed=0):
    """Every finite value moved by one ulp, up or down (psis_helper.k_noise's construction)."""
    a = np.asarray(a, dtype=np.float64)
    sign = np.where(np.random.default_rng(seed).uniform(size=a.shape) < 0.5, -1.0, 1.0)
    fin = np.isfinite(a)
    return np.where(fin, a + sign * np.spacing(np.where(fin, a, 1.0)), a)


def k_noise(ratio, lnl, M, loo, want=None):
    """psis_helper.k_noise in the general form: how far the oracle's own k^ moves under one-ulp changes of the ratios (for
    the LOO form lnl = -ratio moves with them)."""
    want = rows_oracle(ratio, lnl, M, loo) if want is None else want
    r2 = moved(ratio)
    other = rows_oracle(r2, -r2 if loo else lnl, M, loo)
    with np.errstate(invalid="ignore"):
        d = np.abs(other["pareto_k"] - want["pareto_k"])
    return np.where(np.isfinite(d), d, 0.0)


def r_eff_for(S, M):
    """An r_eff for which the entry points' tail rule gives M at S samples (1 when it does so already)."""
    if psh.tail_len(S, 1.0) == M:
        return 1.0
    assert M <= math.ceil(0.2 * S)
    r = 0.9 * 9.0 * S / float(M + 2) ** 2                 # 3 sqrt(S / r) ~ 1.05 (M + 2)
    assert psh.tail_len(S, r) == M, (S, M, r, psh.tail_len(S, r))
    return r


# ---- the select, restated: which pass it leaves after ------------------------------------------------------------------
def keys(lw):
    """psis_key (csrc/mcd_psis.h) of an array: order-preserving uint64, -0 with +0."""
    u = (np.asarray(lw, dtype=np.float64) + 0.0).view(np.uint64)
    return np.where(u >> np.uint64(63) != 0, ~u, u | np.uint64(1 << 63))


def select_break(ratio, M):
    """The digit pass (0: the top byte ... 7: the lowest) after which the radix select of the (M+1)-th largest key is left
    because the cutoff is the only candidate, or 8 when all eight passes leave more than one (equal keys: the index scan
    decides).  Also the cutoff's sample index."""
    with np.errstate(invalid="ignore"):
        k = keys(ratio - np.max(ratio))
    order = np.argsort(k, kind="stable")
    c = order[k.size - M - 1]
    for p in range(8):
        sh = np.uint64(56 - 8 * p)
        if np.count_nonzero((k >> sh) == (k[c] >> sh)) == 1:
            return p, int(c)
    return 8, int(c)


# ---- crafted rows --------------------------------------------------------------------------------------------------
STEPS = (0, 1, 255, 256, 2 ** 16, 2 ** 24, 2 ** 32, 2 ** 40)
GROUP_BASE = 0.25


def group_sizes(S, M):
    """(g_in, g_out) of the straddle group.  g_in = 0 for M < 13 and M // 8 above: a group that covers the quartile entry
    x* of the GPD fit makes k^ ill-conditioned (NumPy and the emulation then differ by 1e-5)."""
    return (0 if M < 13 else max(1, M // 8)), min(S - M - 1, 70)


def straddle(n, S, M, step, seed=11):
    """Ratios (n, S): M - g_in well-separated top values 0.5 + Exp(1), a group of g_in + g_out values
    0.25 + j step ulp(0.25) laid across the cutoff, a body at -1 - Exp(1); shuffled."""
    rng = np.random.default_rng([seed, S, M, step % 65521, step.bit_length()])
    g_in, g_out = group_sizes(S, M)
    g = g_in + g_out
    rows = np.empty((n, S))
    for i in range(n):
        top = 0.5 + np.sort(rng.exponential(size=M - g_in))
        group = GROUP_BASE + np.arange(g) * float(step) * np.spacing(GROUP_BASE)
        body = -1.0 - rng.exponential(size=S - M - g_out)
        rows[i] = rng.permutation(np.concatenate([top, group, body]))
    return rows


def group_mask(ratio, step):
    """The straddle group's samples of one row."""
    top = GROUP_BASE + 400.0 * max(step, 1) * np.spacing(GROUP_BASE)
    return (ratio >= GROUP_BASE) & (ratio <= top)


def constant(n, S, seed=12):
    """All S values equal: k^ = -inf, all eight passes with every sample a candidate, the cutoff by index alone."""
    return np.repeat(np.random.default_rng([seed, S]).normal(size=(n, 1)), S, axis=1)


def several_maxima(n, S, M, seed=13, copies=3):
    """The largest ratio `copies` times (lw = +0 more than once, at the top of the tail), separated values below."""
    rng = np.random.default_rng([seed, S, M])
    rows = np.empty((n, S))
    c = min(copies, M - 2)
    for i in range(n):
        top = 0.5 + rng.exponential(size=M - c)
        rows[i] = rng.permutation(np.concatenate([top, np.full(c, top.max() + 0.75), -1.0 - rng.exponential(size=S - M)]))
    return rows


def early_break(S, M):
    """One row whose cutoff is alone in its key's top byte (sign and seven exponent bits): tail in (-1, 0], cutoff -3 below
    the largest, the body 2^17 and more below (the top byte spans sixteen binades, so nothing nearer will do; the body's
    weights underflow to 0 in any float64 arithmetic).  The select is left after its first pass."""
    rng = np.random.default_rng([14, S, M])
    v = np.concatenate([-rng.uniform(0.0, 0.9, size=M - 1), [0.0, -3.0], -2.0 ** 17 * (1.0 + rng.exponential(size=S - M - 1))])
    return rng.permutation(v)[None, :] + 2.0


def neg_inf(S, M, n_inf, seed=15):
    """psis_row<false> only: near-Gaussian ratios of which n_inf are -inf (moment matching's rows outside the prior)."""
    rng = np.random.default_rng([seed, S, M, n_inf])
    v = rng.normal(scale=0.6, size=S)
    v[rng.permutation(S)[:n_inf]] = -np.inf
    return v[None, :]


SHAPES = tuple((S, psh.tail_len(S, 1.0)) for S in (20, 21, 24, 40, 63, 64, 65, 129, 320, 400, 1000, 4096)) + \
    ((12800, MAX_TAIL), (315, 63), (320, 64), (325, 65))


@functools.lru_cache(maxsize=None)
def shape_rows(S, M):
    """The crafted rows of one shape: (ratio (n, S), list of (family, first row, rows)).  Read-only."""
    assert M < 5 or (M <= math.ceil(0.2 * S) and M <= MAX_TAIL)
    parts = [("near_gaussian", -psh.near_gaussian(2, S, seed=S + 1)), ("heavy_tailed", -psh.heavy_tailed(2, S, seed=S + 2)),
             ("repeated_rows", -psh.repeated_rows(2, S, seed=S + 3))]
    parts += [("straddle_{0}".format(step), straddle(2, S, M, step)) for step in STEPS]
    parts += [("constant", constant(1, S)), ("several_maxima", several_maxima(2, S, M))]
    if M >= 5:
        parts.append(("early_break", early_break(S, M)))
    fams, at = [], 0
    for name, r in parts:
        fams.append((name, at, r.shape[0]))
        at += r.shape[0]
    ratio = np.ascontiguousarray(np.concatenate([r for _, r in parts]))
    ratio.setflags(write=False)
    return ratio, tuple(fams)


@functools.lru_cache(maxsize=None)
def inf_rows(S, M):
    """The -inf rows of one shape with a tail (psis_row<false>): (ratio (4, S), kinds).  "body": fewer than S - M - 1 of
    them, all in the body; "cutoff": S - M, the cutoff is the last of them by index and the tail is finite; "one_in_tail":
    S - M + 1, x_1 = 0 and the fit still stands, so the -inf sample of the highest index receives the lowest smoothed
    weight; "tail": so many that the quartile entry x* of the fit is 0 as well, the fit fails, k^ = +inf and nothing is
    smoothed."""
    n_body = max(1, (S - M - 1) // 2)
    ratio = np.concatenate([neg_inf(S, M, n_body), neg_inf(S, M, S - M), neg_inf(S, M, S - M + 1),
                            neg_inf(S, M, S - M + (M + 1) // 2)])
    ratio.setflags(write=False)
    return ratio, ("body", "cutoff", "one_in_tail", "tail")


def other_lnl(shape, seed=16):
    """The values whose weighted mean psis_row<false> forms: independent of the ratios."""
    return -3.0 + np.random.default_rng([seed, shape[1]]).normal(scale=0.5, size=shape)


@functools.lru_cache(maxsize=None)
def shape_case(S, M, loo):
    """(ratio, lnl, families, oracle, k_noise) of one shape and form; computed once, read-only."""
    ratio, fams = shape_rows(S, M)
    lnl = -ratio if loo else other_lnl(ratio.shape)
    want = rows_oracle(ratio, lnl, M, loo)
    return ratio, lnl, fams, want, k_noise(ratio, lnl, M, loo, want)


@functools.lru_cache(maxsize=None)
def inf_case(S, M):
    ratio, kinds = inf_rows(S, M)
    lnl = other_lnl(ratio.shape, seed=17)
    want = rows_oracle(ratio, lnl, M, False)
    return ratio, lnl, kinds, want, k_noise(ratio, lnl, M, False, want)


# ---- the comparison ------------------------------------------------------------------------------------------------
def differences(got, want, k_tol=K_TOL, values=True):
    """`got` (derived()) against the oracle's dict: asserts the bounds and returns the worst (k^, elpd, log weight)
    differences.  values=False: only what holds without a trusted k^ -- the finite / infinite pattern of k^, exact zeros
    where the oracle has -inf, and which samples carry weight."""
    k, wk = got["pareto_k"], want["pareto_k"]
    fin = np.isfinite(wk)
    assert np.array_equal(np.isfinite(k), fin) and np.array_equal(k[~fin], wk[~fin]), (k, wk)
    lw, wl = got["logw"], want["logw"]
    assert not np.any(np.isnan(lw)), "a sample without a weight"
    dead = np.exp(wl) == 0.0                             # -inf, or below float64's smallest weight (early_break's body)
    assert np.array_equal(np.isneginf(lw), dead), "which samples carry weight"
    if not values:
        return 0.0, 0.0, 0.0
    kt = np.broadcast_to(np.asarray(k_tol, dtype=np.float64), wk.shape)
    dk = np.abs(k[fin] - wk[fin])
    de = np.abs(got["elpd_loo"] - want["elpd_loo"]) / np.maximum(1.0, np.abs(want["elpd_loo"]))
    dw = np.abs(np.where(dead, 0.0, lw) - np.where(dead, 0.0, wl))
    worst = (float(dk.max()) if dk.size else 0.0, float(de.max()), float(dw.max()))
    assert np.all(dk <= kt[fin]), (worst, float(np.max(dk - kt[fin])))
    assert np.all(de <= ELPD_TOL), worst
    assert np.all(np.abs(got["n_eff"] - want["n_eff"]) <= NEFF_TOL * np.abs(want["n_eff"]))
    if np.all(np.isfinite(want["lppd"])):
        assert np.all(np.abs(got["lppd"] - want["lppd"]) <= LPPD_TOL * np.maximum(1.0, np.abs(want["lppd"])))
    assert np.all(dw <= LOGW_TOL), worst
    return worst


def take(d, rows):
    return {k: v[rows] for k, v in d.items()}

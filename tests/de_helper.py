"""Test helper: CPU build of the differential-evolution move (tests/emul/de_emul.cpp + csrc/mcd_de.h) -- its numbers, its
host-driven block around a Python log-likelihood -- and the closed-form posteriors the DE tests sample.

Test infrastructure only."""
import ctypes
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "emul", "de_emul.cpp")
INC = os.path.join(ROOT, "mcmc_dynamics_amd", "csrc")
OUT = os.path.join(ROOT, "tests", "emul", "libde_emul.so")

EVAL_FN = ctypes.CFUNCTYPE(ctypes.c_int, ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p)
MASK64 = 0xFFFFFFFFFFFFFFFF
_lib = None


def lib():
    global _lib
    if _lib is None:
        deps = [SRC] + [os.path.join(INC, h) for h in ("mcd_de.h", "mcd_stretch.h", "mcd_prior.h", "mcd_rng.h", "mcd_math.h")]
        if not os.path.exists(OUT) or any(os.path.getmtime(d) > os.path.getmtime(OUT) for d in deps):
            subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-I", INC, SRC, "-o", OUT],
                           check=True)
        L = ctypes.CDLL(OUT)
        L.emul_de_key.restype = ctypes.c_uint64
        L.emul_de_det_log.restype = ctypes.c_double
        L.emul_de_det_log.argtypes = [ctypes.c_double]
        L.emul_de_words.argtypes = [ctypes.c_uint64, ctypes.c_int64, ctypes.c_int, ctypes.c_int64, ctypes.c_int64, ctypes.c_int,
                                    ctypes.c_void_p]
        L.emul_de_words.restype = None
        L.emul_de_normal.argtypes = [ctypes.c_uint64, ctypes.c_int64, ctypes.c_int, ctypes.c_int64, ctypes.c_int64, ctypes.c_int,
                                     ctypes.POINTER(ctypes.c_int)]
        L.emul_de_normal.restype = ctypes.c_double
        L.emul_de_numbers.argtypes = [ctypes.c_uint64, ctypes.c_int64, ctypes.c_int64, ctypes.c_int64, ctypes.c_int64,
                                      ctypes.c_double, ctypes.c_double] + [ctypes.c_void_p] * 5
        L.emul_de_numbers.restype = None
        L.emul_de_stretch_numbers.argtypes = [ctypes.c_uint64, ctypes.c_int64, ctypes.c_int64, ctypes.c_int64, ctypes.c_int64,
                                              ctypes.c_int] + [ctypes.c_void_p] * 4
        L.emul_de_stretch_numbers.restype = None
        L.emul_de_block.argtypes = [ctypes.c_int64, ctypes.c_int64, ctypes.c_int, ctypes.c_int] + [ctypes.c_void_p] * 5 + \
            [ctypes.c_int] + [ctypes.c_void_p] * 3 + [ctypes.c_int64] + [ctypes.c_void_p] * 10 + [EVAL_FN]
        _lib = L
    return _lib


def key():
    return int(lib().emul_de_key())


def det_log(x):
    return float(lib().emul_de_det_log(float(x)))


def words(seed, step, h, b, j, call):
    out = np.empty(4, dtype=np.uint64)
    lib().emul_de_words(seed & MASK64, step, h, b, j, call, out.ctypes.data)
    return out


def normal(seed, step, h, b, j, max_calls):
    """-> (value, pairs drawn)"""
    used = ctypes.c_int(0)
    return float(lib().emul_de_normal(seed & MASK64, step, h, b, j, max_calls, ctypes.byref(used))), used.value


def numbers(seed, step0, n_steps, n_bins, n_walkers, gamma0, sigma):
    """order (n, B, W), pick_a, pick_b, gamma, thr (n, 2, B, W/2) from the host build of csrc/mcd_de.h."""
    b, w = max(int(n_bins), 1), int(n_walkers)
    order = np.empty((n_steps, b, w), dtype=np.int32)
    pa = np.empty((n_steps, 2, b, w // 2), dtype=np.int32)
    pb = np.empty_like(pa)
    gamma = np.empty((n_steps, 2, b, w // 2))
    thr = np.empty_like(gamma)
    lib().emul_de_numbers(seed & MASK64, step0, n_steps, b, w, gamma0, sigma, order.ctypes.data, pa.ctypes.data, pb.ctypes.data,
                          gamma.ctypes.data, thr.ctypes.data)
    return order, pa, pb, gamma, thr


def stretch_numbers(seed, step0, n_steps, n_bins, n_walkers, n_dim):
    b, w = max(int(n_bins), 1), int(n_walkers)
    order = np.empty((n_steps, b, w), dtype=np.int32)
    zz = np.empty((n_steps, 2, b, w // 2))
    thr = np.empty_like(zz)
    pick = np.empty((n_steps, 2, b, w // 2), dtype=np.int32)
    lib().emul_de_stretch_numbers(seed & MASK64, step0, n_steps, b, w, n_dim, order.ctypes.data, zz.ctypes.data, thr.ctypes.data,
                                  pick.ctypes.data)
    return order, zz, thr, pick


def numpy_words(seed, counter):
    """The four words of Philox4x64-10 at ``counter`` (four 64-bit words, low first) under key (seed, key()), from
    ``numpy.random.Philox`` (NumPy increments the counter before it generates a block)."""
    value = sum(int(x) << (64 * i) for i, x in enumerate(counter))
    before = (value - 1) % (1 << 256)
    c = [(before >> (64 * i)) & MASK64 for i in range(4)]
    bg = np.random.Philox(counter=np.array(c, dtype=np.uint64), key=np.array([int(seed) & MASK64, key()], dtype=np.uint64))
    return bg.random_raw(4)


def uniform53(word):
    return float(int(word) >> 11) * (1.0 / 9007199254740992.0)


def wrap_eval(fn, k):
    """``fn(table (n, K)) -> values (n,)`` as the C callback (n = B * rows per ensemble); an exception becomes status 1."""
    def call(table, n, out):
        try:
            rows = call.rows_factor * n
            t = np.ctypeslib.as_array(ctypes.cast(table, ctypes.POINTER(ctypes.c_double)), shape=(rows, k))
            np.ctypeslib.as_array(ctypes.cast(out, ctypes.POINTER(ctypes.c_double)), shape=(rows,))[:] = fn(t)
            return 0
        except Exception:                                    # noqa: BLE001 -- reported through the status
            return 1
    call.rows_factor = 1
    return call


def block(plan, pos, lnp, nums, fn, accepted=None):
    """The host-driven block (csrc/mcd_de.h: de_block) on ``fn``; ``pos`` ([B,] W, P), ``nums`` as ``numbers`` returns them
    (with or without the ensemble axis).  -> dict(status, pos, lnp, chain, lnprob_chain, accepted)"""
    pos, lnp = np.array(pos, dtype=np.float64), np.array(lnp, dtype=np.float64)
    lead, (W, P) = pos.shape[:-2], pos.shape[-2:]
    B = lead[0] if lead else 1
    order, pa, pb, gamma, thr = [np.ascontiguousarray(a) for a in nums]
    n = order.shape[0]
    src = np.ascontiguousarray(plan["col_source"], dtype=np.int32)
    cols = [np.ascontiguousarray(plan[k], dtype=np.float64) for k in ("col_const", "col_factor", "lo", "hi")]
    K = src.size
    chain, lnpc = np.full((n,) + lead + (W, P), np.nan), np.full((n,) + lead + (W,), np.nan)
    acc = np.zeros(lead + (W,), dtype=np.int64) if accepted is None else accepted
    prior = plan.get("prior")
    keep = [None, None, None]
    if prior is not None:
        keep = [np.ascontiguousarray(prior[0], dtype=np.int32), np.ascontiguousarray(prior[1], dtype=np.float64),
                np.ascontiguousarray(prior[2], dtype=np.float64)]
    call = wrap_eval(fn, K)
    call.rows_factor = B
    cb = EVAL_FN(call)
    rc = lib().emul_de_block(B, W, P, K, src.ctypes.data, *[c.ctypes.data for c in cols], 1 if plan.get("fixed_ok", True) else 0,
                             *[a.ctypes.data if a is not None else None for a in keep], n, pos.ctypes.data, lnp.ctypes.data,
                             order.ctypes.data, pa.ctypes.data, pb.ctypes.data, gamma.ctypes.data, thr.ctypes.data,
                             chain.ctypes.data, lnpc.ctypes.data, acc.ctypes.data, cb)
    return {"status": rc, "pos": pos, "lnp": lnp, "chain": chain, "lnprob_chain": lnpc, "accepted": acc}


# ---- closed-form posteriors ----------------------------------------------------------------------------------------
def table_loglike(centre, width):
    """A separable Gaussian log-likelihood of the kernel table's columns, summed column by column in a fixed order:
    (n, K) -> (n,) with the same bits for a row whatever the batch it is part of."""
    centre, width = np.asarray(centre, dtype=np.float64), np.asarray(width, dtype=np.float64)

    def fn(table):
        table = np.asarray(table, dtype=np.float64)
        acc = np.zeros(table.shape[0])
        for c in range(table.shape[1]):
            r = (table[:, c] - centre[c]) / width[c]
            acc = acc - 0.5 * (r * r)
        return acc
    return fn


def plan_lnprob(plan, loglike, prior_eval=None):
    """The log-posterior of ``plan`` as the samplers' NumPy loop needs it: (..., P) -> (...); -inf outside the box (or where a
    log-normal coordinate is <= 0, or fixed_ok is off), else ``loglike(table)`` [+ ``prior_eval(prior, x)``: the library's
    host code, bit for bit what the blocks add]."""
    src, const, fac = np.asarray(plan["col_source"]), np.asarray(plan["col_const"], float), np.asarray(plan["col_factor"], float)
    lo, hi = np.asarray(plan["lo"], float), np.asarray(plan["hi"], float)
    prior = plan.get("prior")

    def fn(values):
        v = np.asarray(values, dtype=np.float64)
        lead, x = v.shape[:-1], v.reshape(-1, v.shape[-1])
        ok = np.all((x >= lo) & (x <= hi), axis=1) & bool(plan.get("fixed_ok", True))
        lp = np.zeros(x.shape[0])
        if prior is not None:
            lp = np.asarray(prior_eval(prior, x), dtype=np.float64)
            ok &= np.isfinite(lp)
        out = np.full(x.shape[0], -np.inf)
        if ok.any():
            table = np.empty((x.shape[0], src.size))
            for c in range(src.size):
                table[:, c] = const[c] if src[c] < 0 else (x[:, src[c]] if fac[c] == 1.0 else x[:, src[c]] * fac[c])
            ll = loglike(table)
            out[ok] = ll[ok] + lp[ok] if prior is not None else ll[ok]
        return out.reshape(lead)
    return fn


def correlated_gaussian(P, rho=0.9, seed=5):
    """A correlated Gaussian target: (covariance, its inverse).  Unequal scales, pairwise correlation ``rho`` mixed by a
    random rotation -- a posterior on which the stretch move mixes slowly."""
    rng = np.random.default_rng(seed)
    scales = np.exp(rng.uniform(-1.0, 1.0, size=P))
    corr = np.full((P, P), rho) + (1.0 - rho) * np.eye(P)
    cov = corr * np.outer(scales, scales)
    return cov, np.linalg.inv(cov)


def autocorr_time(x, c=5.0):
    """emcee's integrated autocorrelation time of a series x (steps, W): the walkers' mean autocorrelation function, Sokal's
    automatic window."""
    x = np.asarray(x, dtype=np.float64)
    n = x.shape[0]
    size = 1 << (2 * n - 1).bit_length()
    f = np.zeros(n)
    for w in range(x.shape[1]):
        y = x[:, w] - x[:, w].mean()
        ft = np.fft.rfft(y, n=size)
        acf = np.fft.irfft(ft * np.conjugate(ft))[:n]
        f += acf / acf[0]
    f /= x.shape[1]
    taus = 2.0 * np.cumsum(f) - 1.0
    m = np.arange(n) < c * taus
    window = int(np.argmin(m)) if not m.all() else n - 1
    return float(taus[window])


# ---- GPU tests: catalogues, walkers and the NumPy loop around the library's evaluation -------------------------------
CENTRE = (56.345, -26.675)
DOUBLE_BASE = {7: 3, 8: 4}                      # double_helper.BASE: the single-component model a double model reduces to


def n_columns(model, free):
    """Kernel columns of ``model`` (include/mcd.h): v_sys, sigma_max [, a], v_maxx, v_maxy [, r_peak] [, v_maxx_c, v_maxy_c,
    r_peak_ratio] [, ra_center, dec_center] [, v_back, sigma_back, f_back | f_back]."""
    return (4 if model < 3 else 6) + (3 if model >= 7 else 0) + (2 if free else 0) + {2: 3, 4: 3, 8: 3, 5: 1}.get(model, 0)


def gpu_walkers(rng, w, model, sv, free, near_centre=False):
    """(w, K) start rows of ``model`` (include/mcd.h) around a cluster of dispersion ``sv``.  Models 7 and 8: the row of
    the single-component counterpart with the second component's three columns of double_helper.make_case behind r_peak,
    its amplitudes in units of ``sv``; from model 4 on a free centre stays within 0.005 deg (variant_helper.make_case)."""
    if model >= 7:
        import double_helper
        base = gpu_walkers(rng, w, DOUBLE_BASE[model], sv, free, near_centre=True)
        case = double_helper.make_case(model, free, 1, seed=int(rng.integers(1 << 31)))
        extra = case["params"][:w, 6:9].copy()
        assert extra.shape == (w, 3)
        extra[:, :2] *= sv / case["scale"]
        return np.ascontiguousarray(np.concatenate([base[:, :6], extra, base[:, 6:]], axis=1))
    cols = [rng.normal(0, 0.2 * sv, w), sv * 10.0 ** rng.uniform(-0.3, 0.3, w)]
    if model >= 3:
        cols.append(10.0 ** rng.uniform(1.0, 2.0, w))
    cols += [rng.normal(0, 0.2 * sv, w), rng.normal(0, 0.2 * sv, w)]
    if model >= 3:
        cols.append(10.0 ** rng.uniform(1.0, 2.0, w))
    if free and (model >= 4 or near_centre):
        cols += [CENTRE[0] + rng.uniform(-0.005, 0.005, w), CENTRE[1] + rng.uniform(-0.005, 0.005, w)]
    elif free:
        cols += [CENTRE[0] + rng.normal(0, 0.002, w), CENTRE[1] + rng.normal(0, 0.002, w)]
    if model in (2, 4):
        cols += [rng.normal(0, 0.3 * sv, w), 3 * sv * 10.0 ** rng.uniform(-0.1, 0.1, w), rng.uniform(0.2, 0.8, w)]
    if model == 5:
        cols.append(rng.uniform(0.2, 0.8, w))                          # f_back
    return np.ascontiguousarray(np.stack(cols, axis=1))


def gpu_columns(rng, n, model):
    """The columns of a small cluster with a background population: (dict of ra, dec, v, verr [, lnlike_bg, pmember |
    density]), dispersion).  From model 4 on the stars keep 0.01 deg from the centre, as the catalogues of
    variant_helper.make_case do (the position angle next to the centre is ill-conditioned in the reference's own formula:
    the accuracy floors of tests/test_gpu_variant_matrix.py are stated for such catalogues)."""
    from oracle import lnprob_numpy as oracle
    sv = 12.0
    sep = np.maximum(np.abs(rng.normal(0, 2.0 / 60.0, n)), 1e-4 if model < 4 else 0.01)
    th = rng.uniform(-np.pi, np.pi, n)
    ra, dec = CENTRE[0] + sep * np.cos(th) / np.cos(np.radians(CENTRE[1])), CENTRE[1] + sep * np.sin(th)
    v, verr = rng.normal(0, sv, n), rng.uniform(0.5, 4.0, n)
    v[::7] = rng.normal(0, 3 * sv, len(v[::7]))                     # a background population
    cols = dict(ra=ra, dec=dec, v=v, verr=verr)
    if model in (1, 6):
        cols.update(lnlike_bg=oracle.gaussian_background(v, verr, 0.0, 3 * sv), pmember=np.clip(rng.random(n), 0.02, 0.98))
    elif model in (2, 4, 8):
        cols.update(density=np.clip(rng.random(n), 0.05, 1.0))
    elif model == 5:
        cols.update(lnlike_bg=oracle.gaussian_background(v, verr, 0.0, 3 * sv), density=np.clip(rng.random(n), 0.05, 1.0))
    return cols, sv


def gpu_catalogue(native, ctx, rng, n, model, free):
    cols, sv = gpu_columns(rng, n, model)
    kw = {k: cols[k] for k in cols if k not in ("ra", "dec", "v", "verr")}
    return native.Catalog(ctx, cols["ra"], cols["dec"], cols["v"], cols["verr"], model=model,
                          centre=None if free else CENTRE, **kw), sv


def gpu_box(cat, pos, model, sv, margin=0.1):
    """An inclusive box that rejects a few proposals: sigma_max > 0, a window around the ensemble's v_sys (``margin``
    dispersions beyond its extremes), f_back in [0, 1]; the double models' r_peak_ratio in [1e-3, 1]
    (analysis/double_model.py) and, from model 4 on, a free centre within 0.005 deg."""
    lo, hi = np.full(cat.k, -np.inf), np.full(cat.k, np.inf)
    lo[1] = 0.0
    lo[0], hi[0] = pos[:, 0].min() - margin * sv, pos[:, 0].max() + margin * sv
    if model in (2, 4, 5, 8):
        lo[-1], hi[-1] = 0.0, 1.0
    if model >= 3:
        lo[2] = lo[5] = 1.0                                            # a, r_peak [arcsec] stay positive
    if model >= 7:
        lo[8], hi[8] = 1e-3, 1.0
    if model >= 4 and cat.k == n_columns(model, True):
        at = 9 if model >= 7 else 6
        lo[at:at + 2], hi[at:at + 2] = np.array(CENTRE) - 0.005, np.array(CENTRE) + 0.005
    return lo, hi


def identity_plan(k, lo=None, hi=None, prior=None):
    plan = {"col_source": np.arange(k, dtype=np.int32), "col_const": np.zeros(k), "col_factor": np.ones(k),
            "lo": np.full(k, -np.inf) if lo is None else np.asarray(lo, dtype=float),
            "hi": np.full(k, np.inf) if hi is None else np.asarray(hi, dtype=float), "fixed_ok": True}
    if prior is not None:
        plan["prior"] = prior
    return plan


def numpy_de_block(cat, plan, pos, lnp, nums, prior_eval=None):
    """The samplers' DE half-step loop with ``cat.loglike`` as the likelihood: box and structured priors from the plan.

    One ensemble -- ``pos`` (W, P), ``order`` (n, W), the other numbers (n, 2, W/2), ``cat.loglike`` on (W/2, K) rows -- or B
    lock-stepped ones: ``pos`` (B, W, P), ``order`` (n, B, W), the others (n, 2, B, W/2), ONE call ``cat.loglike`` on
    (B, W/2, K) rows per half step.  The launch always has all its rows: a row outside the prior is replaced by the first
    valid row of the whole launch, counted ensemble by ensemble and slot by slot, and its value is never looked at (the
    proposal is rejected); a half step without any valid row is not evaluated; an ensemble without a valid row keeps its
    state through that half step.

    -> (pos, lnp, chain, lnprob_chain, accepted, seen): ``seen["n_ok"]`` (n, 2, B) the valid rows of every ensemble in
    every half step, ``seen["nonpositive"]`` (n, 2, B) its proposals with a log-normal coordinate <= 0, ``seen["mixed"]`` the
    number of (half step, ensemble) pairs with 0 < n_ok < W/2, ``seen["half"]`` = W/2."""
    single = np.ndim(pos) == 2
    order, pa, pb, gamma, thr = nums
    if single:
        order, (pa, pb, gamma, thr) = order[:, None], [a[:, :, None] for a in (pa, pb, gamma, thr)]
        pos, lnp = pos[None], lnp[None]
    pos, lnp = pos.copy(), lnp.copy()
    n_steps, n_ens, w = order.shape
    half = w // 2
    chain, lnpc, acc = np.empty((n_steps,) + pos.shape), np.empty((n_steps, n_ens, w)), np.zeros((n_ens, w), dtype=np.int64)
    src, const, fac = plan["col_source"], plan["col_const"], plan["col_factor"]
    prior = plan.get("prior")
    lognormal = np.zeros(pos.shape[-1], dtype=bool) if prior is None else np.asarray(prior[0]) == 2
    n_ok = np.zeros((n_steps, 2, n_ens), dtype=np.int64)
    nonpositive = np.zeros_like(n_ok)
    ens = np.arange(n_ens)[:, None]
    for i in range(n_steps):
        halves = (order[i, :, :half], order[i, :, half:])
        for h in (0, 1):
            first, second = halves[h], halves[1 - h]                   # (B, W/2) walker indices
            xa, xb = np.take_along_axis(second, pa[i, h], axis=1), np.take_along_axis(second, pb[i, h], axis=1)
            proposal = pos[ens, first] + (pos[ens, xa] - pos[ens, xb]) * gamma[i, h][..., None]
            ok = np.all((proposal >= plan["lo"]) & (proposal <= plan["hi"]), axis=2)
            lp = np.zeros((n_ens, half))
            if prior is not None:
                lp = np.asarray(prior_eval(prior, proposal.reshape(n_ens * half, -1))).reshape(n_ens, half)
                ok &= np.isfinite(lp)
                nonpositive[i, h] = np.any(proposal[..., lognormal] <= 0.0, axis=2).sum(axis=1)
            n_ok[i, h] = ok.sum(axis=1)
            new = np.full((n_ens, half), -np.inf)
            if ok.any():
                rows = np.empty((n_ens, half, src.size))
                for c in range(src.size):
                    rows[..., c] = const[c] if src[c] < 0 else (proposal[..., src[c]] if fac[c] == 1.0 else
                                                                proposal[..., src[c]] * fac[c])
                donor = int(np.argmax(ok.reshape(-1)))                 # first valid row in (ensemble, slot) order
                rows[~ok] = rows.reshape(n_ens * half, -1)[donor]
                ll = cat.loglike(np.ascontiguousarray(rows[0] if single else rows)).reshape(n_ens, half)
                new[ok] = ll[ok] + lp[ok] if prior is not None else ll[ok]
            accept = thr[i, h] < new - lnp[ens, first]
            e, j = np.nonzero(accept)
            idx = first[e, j]
            pos[e, idx], lnp[e, idx] = proposal[e, j], new[e, j]
            acc[e, idx] += 1                                           # (the walkers of a half step are distinct)
        chain[i], lnpc[i] = pos, lnp
    seen = {"n_ok": n_ok, "nonpositive": nonpositive, "mixed": int(((n_ok > 0) & (n_ok < half)).sum()), "half": half}
    if single:
        return pos[0], lnp[0], chain[:, 0], lnpc[:, 0], acc[0], seen
    return pos, lnp, chain, lnpc, acc, seen


def same(a, b):
    return all(np.array_equal(x, y, equal_nan=True) for x, y in zip(a, b))

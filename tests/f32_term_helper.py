"""Test helper: the stated per-term tolerance of the float32 per-star terms and per-star summaries (tests/
test_f32_terms_cpu.py on the host, tests/test_gpu_f32_terms.py on the device).  Test infrastructure only.

On a float32 catalogue per_star_kernel, posterior_slice_kernel, predictive_slice_kernel, psis_term_kernel and
loox_term_kernel evaluate star_components<MODEL, FREE, float> -> gauss_lnl<float> / mixture_lnl<float>: the literal
float32 log-sum-exp on records and walker constants rounded to float.  Neither mcd_loglike_per_star / mcd_membership nor
the summary launchers consult the float32 domain, and the stated tolerances of the sums (scale max(|lnL|, N, 32)) say
nothing about one term.  This module states what one term may be off by: a first-order rounding model.

Notation: u = 2^-24; d the residual v - v_los and n the total variance of the cluster term; rot = |v_maxx| + |v_maxy|;
D = |v| + |v_sys| + rot.  Everything is evaluated in numpy.longdouble from the record fields and walker constants of
emul_helper.pack_records / pack_walkers (the layout the device rounds to float).

    A_c = (|d|/n)(D + G) + d^2/n + 1 + |lc|   (+ profile models, free centre: (1 + d^2/n)/(2n) G_n)
        G   = 0                                           fixed centre
        G   = rot / r                                     CONST family, free centre; r the tangent-plane separation [rad]
                                                          from THIS row's centre: the offsets x, y are differences of O(1)
                                                          products, off by ~u absolute, and v_los = (v_maxx y - v_maxy x) / r
        G   = k rot ARCSEC (1 + 2 r^2/(r_peak^2 + r^2))   profile family, free centre; k = 2 r_peak/(r_peak^2 + r^2), r [arcsec]
        G_n = sigma_los^2 r ARCSEC / (a^2 + r^2)          profile family, free centre; sigma_los^2 = sigma_max^2 a/sqrt(a^2 + r^2)
    A_b = |lb|                                            fixed backgrounds (a record field: one rounding)
    A_b = (|d_b|/n_b)(|v| + |v_back|) + d_b^2/n_b + 1 + |lb|        Gaussian background
    A_l = p A_c + (1 - p) A_b + 1 + |l| + (1 - p)/(1 - m)           the mixture value l (A_l = A_c without a background)
    A_p = p (1 - p) (A_c + A_b + 1/(m (1 - m))) + p                 the membership p

p is the exact membership, m the prior (pmember, or rho / (rho + f_back)).  Where the terms come from: d = v - v_sys - rotation
carries the roundings of its inputs and of its own operations, each <= u times the magnitude it rounds, together <= u D (+ u G
with a free centre), and moves lc by |d|/n times that; d^2/n carries a few relative roundings (the square, the variance, the
quotient); log n and the constant and the final sum round at the size of lc; l = max + log(sum) rounds at 1 and |l|; 1 - m is
formed in float (u absolute) and enters log-sum-exp with weight (1 - p)/(1 - m); p = ec / (ec + eb) responds to lc - lb with
p (1 - p), to m with p (1 - p)/(m (1 - m)), and rounds itself a few times (p u).

The bound of a term is C u A, for the membership C u A_p + 2^-126 (exp underflows in float32: p = 1e-113 comes back 0).

C (below) is NOT fitted to any kernel.  The yardstick is term() in numpy.float32 -- correctly rounded float32 operations in
the kernel's order, on the rounded records -- against the same function in longdouble on the unrounded records: C is twice
its worst |np32 - exact| / (u A) over the test matrix, rounded up to an integer.  The factor 2 is for what the device does
differently from correctly rounded float32: v_rcp_f32, v_rsq_f32, v_exp_f32, v_log_f32 at 1 ulp and fma contraction."""
import numpy as np

import emul_helper as emul
import f32_helper as fh
import variant_helper as vh

L = vh.L
U = L(2.0) ** -24
FLOOR = 2.0 ** -126                        # membership: float32 exp underflows
# Measured (tests/test_f32_terms_cpu.py, the F32_TERM_NP32 lines; the matrix of both test files, 14 cells): the worst
# |np32 - exact| / (u A) is 1.65 for the value (model 0, free centre), 1.44 for the membership (model 5, free centre) and 1.86
# for a predictive quantity (sigma_los of model 4, free centre): 2 x 1.86 = 3.7 -> 4.
C = 4
ARCSEC = L(206264.80624709635516)          # csrc/mcd_math.h: kArcsecPerRad
LN2PI = np.log(2 * L(np.pi))

PROFILE = emul.PROFILE_MODELS
BG = emul.BG_OF
PER_STAR_MODELS = (1, 2, 4, 5, 6)          # mcd_loglike_per_star / mcd_membership refuse the models without a background
CELLS = [(m, f) for m in range(7) for f in (False, True)]
IDS = ["{0}-{1}".format(m, "free" if f else "fixed") for m, f in CELLS]

# The shapes of the device file.  per_star_kernel: one thread per star, 256 per block; posterior_slice_kernel: lane = star,
# 64 per wave; S = 65 gives two slices of 33 + 32 samples, S = 257 five of 52 with a short last one of 49.
PER_STAR_N = (1, 2, 63, 64, 65, 255, 256, 257, 4099)
PER_STAR_ROWS = (0, 1, 2)
POST_N = (1, 63, 65, 130)
POST_S = (1, 2, 64, 65, 257)
POST_PASS = 100                            # option posterior_pass at S = 257: three passes of 100, 100 and 57 rows (the sliced
                                           # summaries write every pass at row 0 of one pass buffer; psis_loo fills the whole
                                           # [S][KD] table, so its passes land at the float32 row offsets 100 and 200)
PRED_N = (1, 65, 4099)                     # predictive_helper.MATRIX_N x MATRIX_S
PRED_S = (1, 65, 257)

DEFECTS = ("ln2pi", "one_minus_m", "vmaxy_sign", "star_shift", "sample_shift")


def stars(ns, free):
    """A free centre with one star has no float32 domain (f32_helper.stars): N = 1 is a fixed-centre shape."""
    return tuple(n for n in ns if not (free and n == 1))


def records(case, rows):
    """(rec (n, ND), wp (S, KD)) in float64: what prepare_records_kernel / prepare_walkers_kernel evaluate before rounding."""
    model, centre = case["model"], case["centre"]
    return (emul.pack_records(case["cat"], model, centre),
            emul.pack_walkers(np.atleast_2d(case["params"][list(rows)]), model, centre is None))


def rounded(x):
    """The float32 catalogue's copy of float64 records / walker constants (exactly representable in every wider type)."""
    return np.asarray(x, dtype=np.float64).astype(np.float32)


def term(rec, wp, model, free, dtype, defect=None, slice_len=None, geometry_only=False):
    """star_components + mixture_lnl + both modes of per_star_kernel (csrc/mcd_math.h, csrc/mcd_kernels.hip) restated in
    NumPy, every operation in `dtype`, in the kernel's order (no fused multiply-add), for every (row of wp, star of rec):
    dict of (S, n) arrays -- l (the star's term: the mixture value, or the Gaussian term without a background), p (the
    membership; 1 without a background) and the intermediates the amplifications need.

    dtype numpy.float32 on rounded(rec), rounded(wp): correctly rounded float32, the yardstick of C.
    dtype longdouble on rounded(...): exact at rounded inputs (what is left is input rounding).
    dtype longdouble on the float64 rec, wp: the oracle of the amplifications.

    defect: one of DEFECTS, planted to show that the bound bites (tests/test_f32_terms_cpu.py).
    geometry_only: stop after d, n, sigma_los^2 (and d_b, n_b, m of a Gaussian background): what the predictive fields use."""
    T = dtype
    prof, bg = model in PROFILE, BG[model]
    xb = 6 if (free or prof) else 4
    rec, wp = np.asarray(rec), np.asarray(wp)
    if defect == "star_shift":                                  # the record of star i - 1 read for star i
        rec = np.concatenate([rec[:1], rec[:-1]])
    if defect == "sample_shift":                                # the walker row of sample s - 1 read for sample s beyond the first slice
        src = np.arange(wp.shape[0])
        src[slice_len:] -= 1
        wp = wp[src]
    r = [rec[:, k].astype(T)[None, :] for k in range(rec.shape[1])]
    w = [wp[:, k].astype(T)[:, None] for k in range(wp.shape[1])]
    vsys, s2, vx, vy, sac, cac, sdc, cdc, vb, sb2, fb, a2, s2a, rp2, rp_2 = w[:15]
    if defect == "vmaxy_sign":
        vy = -vy
    ln2pi = T(1.8379) if defect == "ln2pi" else T(LN2PI)
    one, half = T(1), T(0.5)
    out = {}
    if free:
        x = r[3] * sac - r[2] * cac
        t = r[3] * cac + r[2] * sac
        y = r[4] * cdc - sdc * t
    if not prof:
        if free:
            r2 = x * x + y * y
            cross = vx * y - vy * x
            d = -cross * (one / np.sqrt(r2)) + (r[0] - vsys)
            out["r"] = np.sqrt(r2)                               # [rad]
        else:
            d = -vx * r[2] + (vy * r[3] + (r[0] - vsys))
        n = r[1] + s2
        sig2 = s2 + np.zeros_like(n)
    else:
        if free:
            dx, dy = T(ARCSEC) * x, T(ARCSEC) * y
            r2 = dx * dx + dy * dy
        else:
            dx, dy, r2 = r[2], r[3], r[4]
        t = one / np.sqrt(a2 + r2)
        inv = one / (rp2 + r2)
        cross = vx * dy - vy * dx
        d = -(rp_2 * inv) * cross + (r[0] - vsys)
        sig2 = s2a * t
        n = sig2 + r[1]
        out["r"] = np.sqrt(r2) + np.zeros_like(n)                # [arcsec]
        out["a2r2"] = a2 + r2 + np.zeros_like(n)
    out.update(d=d, n=n, sig2=sig2)
    if geometry_only:
        if bg == 2:
            out.update(db=r[0] - vb + np.zeros_like(n), nb=r[1] + sb2 + np.zeros_like(n), m=r[xb] / (r[xb] + fb) + np.zeros_like(n))
        return out
    gauss = lambda dd, nn: -half * (np.log(nn) + ln2pi + dd * dd / nn)
    lc = gauss(d, n)
    out["lc"] = lc
    if bg == 0:
        out.update(l=lc, p=np.ones_like(lc), lb=None, m=None)
        return out
    if bg == 1:
        lb, m = r[xb] + np.zeros_like(lc), r[xb + 1] + np.zeros_like(lc)
    else:
        rho = r[xb + 2] if bg == 3 else r[xb]
        m = rho / (rho + fb)
        if bg == 3:
            lb = r[xb] + np.zeros_like(lc)
        else:
            db, nb = r[0] - vb, r[1] + sb2
            lb = gauss(db, nb)
            out.update(db=db + np.zeros_like(lc), nb=nb + np.zeros_like(lc))
    om = m * T(0) + one if defect == "one_minus_m" else one - m        # (1 - m) dropped from the background branch
    with np.errstate(under="ignore"):
        mx = np.maximum(lc, lb)
        l = mx + np.log(m * np.exp(lc - mx) + om * np.exp(lb - mx))
        shift = mx if prof else T(0)
        ec, eb = m * np.exp(lc - shift), om * np.exp(lb - shift)
        p = ec / (ec + eb)
    out.update(l=l, p=p, lb=lb, m=m)
    return out


def amplification(ex, rec, wp, model, free):
    """(A_l, A_p) of every (row, star), longdouble, from ex = term(rec, wp, model, free, L) on the float64 records; A_p is
    None without a background.  The formulas of the module docstring."""
    prof, bg = model in PROFILE, BG[model]
    rec, wp = np.asarray(rec, dtype=L), np.asarray(wp, dtype=L)
    v = np.abs(rec[:, 0])[None, :]
    vsys, rot = np.abs(wp[:, 0])[:, None], (np.abs(wp[:, 2]) + np.abs(wp[:, 3]))[:, None]
    d, n, lc = np.abs(ex["d"]), ex["n"], ex["lc"]
    q = d * d / n
    big_d = v + vsys + rot
    g, extra = L(0), L(0)
    if free and not prof:
        g = rot / ex["r"]
    elif free:
        r, a2, rp2, rp_2 = ex["r"], wp[:, 11][:, None], wp[:, 13][:, None], wp[:, 14][:, None]
        g = rp_2 / (rp2 + r * r) * rot * ARCSEC * (1 + 2 * r * r / (rp2 + r * r))
        extra = (1 + q) / (2 * n) * (ex["sig2"] * r * ARCSEC / (a2 + r * r))
    a_c = d / n * (big_d + g) + q + 1 + np.abs(lc) + extra
    if bg == 0:
        return a_c, None
    lb, m, p = ex["lb"], ex["m"], ex["p"]
    if bg == 2:
        db, nb = np.abs(ex["db"]), ex["nb"]
        a_b = db / nb * (v + np.abs(wp[:, 8])[:, None]) + db * db / nb + 1 + np.abs(lb)
    else:
        a_b = np.abs(lb)
    a_l = p * a_c + (1 - p) * a_b + 1 + np.abs(ex["l"]) + (1 - p) / (1 - m)
    a_p = p * (1 - p) * (a_c + a_b + 1 / (m * (1 - m))) + p
    return a_l, a_p


class Terms(object):
    """One case at some rows: the oracle of the model (longdouble on the float64 records), the amplifications and bounds."""

    def __init__(self, case, rows):
        self.case, self.rows = case, list(rows)
        self.model, self.free = case["model"], case["centre"] is None
        self.rec, self.wp = records(case, rows)
        self.exact = term(self.rec, self.wp, self.model, self.free, L)
        self.a_l, self.a_p = amplification(self.exact, self.rec, self.wp, self.model, self.free)

    def bound_l(self, c=C):
        return c * U * self.a_l

    def bound_p(self, c=C):
        return c * U * self.a_p + L(FLOOR)

    def np32(self, defect=None, slice_len=None):
        return term(rounded(self.rec), rounded(self.wp), self.model, self.free, np.float32, defect, slice_len)

    def exact_at_rounded(self):
        return term(rounded(self.rec), rounded(self.wp), self.model, self.free, L)

    def oracle(self):
        """(l, p) of variant_helper.per_star: the reference's formulas in longdouble on the UNROUNDED catalogue columns (the
        arctan2 form, not the records): what the device is held to.  (S, n) each; p None without a background."""
        if getattr(self, "_oracle", None) is not None:
            return self._oracle
        c = self.case
        both = [vh.per_star(self.model, c["cat"], c["params"][r], c["centre"]) for r in self.rows]
        self._oracle = (np.array([b[0] for b in both], dtype=L),
                        None if both[0][1] is None else np.array([b[1] for b in both], dtype=L))
        return self._oracle


def ratio(got, want, bound):
    """|got - want| / bound per element, float64."""
    return (np.abs(np.asarray(got, dtype=L) - want) / bound).astype(np.float64)


def worst(r):
    """(largest ratio, its (row, star))."""
    r = np.atleast_2d(r)
    i = np.unravel_index(int(np.argmax(r)), r.shape)
    return float(r[i]), (int(i[0]), int(i[1]))


# ---- propagation to the per-star posterior summaries (csrc/mcd_posterior.h) -----------------------------------------------
POST_FIELDS = ("lppd", "lnl_var", "pmem_mean", "pmem_std")


def _var_bound(x, b):
    """First-order bound of the sample variance of x (S, n) whose terms are off by <= b: (2/(S-1)) sum |x - mean| b +
    (1/(S-1)) sum b^2."""
    s = x.shape[0]
    if s == 1:
        return np.zeros(x.shape[1], dtype=L)
    return (2 * (np.abs(x - x.mean(axis=0)) * b).sum(axis=0) + (b * b).sum(axis=0)) / (s - 1)


def _std_bound(var, dvar):
    """|sqrt(var + e) - sqrt(var)| for |e| <= dvar: min(dvar / (2 sd), sqrt(dvar)) -- the second where sd is ~0."""
    sd = np.sqrt(var)
    with np.errstate(divide="ignore", invalid="ignore"):
        first = np.where(sd > 0, dvar / (2 * sd), L(np.inf))
    return np.minimum(first, np.sqrt(dvar))


def posterior_summary(x, p, b_x, b_p):
    """The exact summaries of terms x, p (S, n) (longdouble; p, b_p None without membership) and their bounds: per-term
    bounds b propagated to first order through the exact reduction, plus the allowance the float64 tests give the
    float64 reduction itself (tests/test_gpu_posterior.py: lppd 1e-12 relative on max(|lppd|, 1); the variance by var_ok
    with rtol 1e-10 on the scale of lppd; pmem_mean 1e-12, pmem_std 1e-10 absolute).  Returns (want, bound): dicts."""
    s = x.shape[0]
    mx = x.max(axis=0)
    lppd = mx + np.log(np.exp(x - mx).sum(axis=0)) - np.log(L(s))
    soft = np.exp(x - lppd) / s
    var = x.var(axis=0, ddof=1) if s > 1 else np.zeros(x.shape[1], dtype=L)
    dd = L(1e-10) * np.abs(lppd)
    want = {"lppd": lppd, "lnl_var": var}
    bound = {"lppd": (soft * b_x).sum(axis=0) + L(1e-12) * np.maximum(np.abs(lppd), 1),
             "lnl_var": _var_bound(x, b_x) + L(1e-10) * var + 2 * dd * np.sqrt(var) + dd * dd}
    if p is not None:
        pvar = p.var(axis=0, ddof=1) if s > 1 else np.zeros(p.shape[1], dtype=L)
        want.update(pmem_mean=p.mean(axis=0), pmem_std=np.sqrt(pvar))
        bound.update(pmem_mean=b_p.mean(axis=0) + L(1e-12), pmem_std=_std_bound(pvar, _var_bound(p, b_p)) + L(1e-10))
    return want, bound


def reduce_terms(x, p):
    """The plain float64 reduction of given terms (the NumPy restatement's summaries)."""
    x = np.asarray(x, dtype=np.float64)
    want, _ = posterior_summary(x.astype(L), None if p is None else np.asarray(p, dtype=np.float64).astype(L),
                                np.zeros(x.shape, dtype=L), None if p is None else np.zeros(x.shape, dtype=L))
    return want


# ---- the posterior predictive fields (csrc/mcd_predictive.h) --------------------------------------------------------------
# d and n come from star_d_n<float>; everything after that is float64: z = d / sqrt(n), t = erfc(|z| / sqrt 2), pit,
# vlos = v - d, sig = sqrt(sigma_los^2).  Amplifications, derived as above:
#   z:    A_d/sqrt(n) + |z| K_n / 2,   A_d the amplification of vlos below (the same d),   K_n = 2 (CONST: e2, sigma^2 rounded, one addition) or 5 (profile: sigma_max^2 a,
#         a^2 + r^2, the root, the reciprocal, the multiply-add) + G_n / n: the relative error of n in units of u
#   vlos: 2 (|v| + |v_sys|) + K_r rot + G: vlos = v - d with d rounded to float; the rounding of v itself cancels, those of
#         v - v_sys and of d (each <= u (|v| + |v_sys| + rot)) do not, and every rounding on the way to the rotation term
#         counts once per amplitude: K_r = 5 for CONST with a fixed centre (amplitude, sin | cos, product, two sums), 12
#         otherwise (the offsets or dx | dy, r^2, r_peak^2 | 2 r_peak, the sum, the root | reciprocal, three products, the
#         cross difference, the amplitude, the last multiply-add)
#   sig:  sig K_s,     K_s = 1/2 (CONST: the rounding of sigma_max^2, halved by the root) or 2 (profile: sigma_max^2 a,
#         a^2, r^2, their sum, each halved or quartered by the roots) + G_n / (2 sigma_los^2)
#   t, pit: the amplification of z times the normal density: dt/dz = 2 phi(z), dpit/dz = phi(z)
#   pit_mix: m A_pit + (1 - m) phi(z_b) A_zb + |pit - Phi(z_b)| m (2 + 2 (1 - m)),  A_zb = (|v| + |v_back|)/sqrt(n_b) + 2 |z_b|
#         (m = rho / (rho + f_back) formed in float: rho and f_back rounded, m (1 - m) u each; the sum and the quotient, m u each)
PRED_STDS = (("z_std", "z"), ("vlos_std", "vlos"), ("sigma_std", "sig"))


def predictive_amplification(ex, rec, wp, model, free, mix):
    prof = model in PROFILE
    rec, wp = np.asarray(rec, dtype=L), np.asarray(wp, dtype=L)
    v = np.abs(rec[:, 0])[None, :]
    vsys, rot = np.abs(wp[:, 0])[:, None], (np.abs(wp[:, 2]) + np.abs(wp[:, 3]))[:, None]
    d, n, sig2 = ex["d"], ex["n"], ex["sig2"]
    z = d / np.sqrt(n)
    g, g_n = L(0), L(0)
    if free and not prof:
        g = rot / ex["r"]
    elif free:
        r, a2, rp2, rp_2 = ex["r"], wp[:, 11][:, None], wp[:, 13][:, None], wp[:, 14][:, None]
        g = rp_2 / (rp2 + r * r) * rot * ARCSEC * (1 + 2 * r * r / (rp2 + r * r))
        g_n = sig2 * r * ARCSEC / (a2 + r * r)
    phi = np.exp(-z * z / 2) / np.sqrt(2 * L(np.pi))
    k_r = 5 if not (prof or free) else 12
    a_d = 2 * (v + vsys) + k_r * rot + g
    a_z = a_d / np.sqrt(n) + np.abs(z) * ((5 if prof else 2) + g_n / n) / 2
    out = {"z": a_z, "vlos": a_d, "sig": np.sqrt(sig2) * ((2 if prof else L(0.5)) + g_n / (2 * sig2)),
           "t": 2 * phi * a_z, "pit": phi * a_z}
    if mix:
        from scipy import special
        db, nb, m = ex["db"], ex["nb"], ex["m"]
        zb = db / np.sqrt(nb)
        a_zb = (v + np.abs(wp[:, 8])[:, None]) / np.sqrt(nb) + 2 * np.abs(zb)
        cdf = lambda q: L(0.5) * special.erfc((-q / np.sqrt(L(2))).astype(np.float64)).astype(L)
        out["pit_mix"] = (m * out["pit"] + (1 - m) * np.exp(-zb * zb / 2) / np.sqrt(2 * L(np.pi)) * a_zb
                          + np.abs(cdf(z) - cdf(zb)) * m * (2 + 2 * (1 - m)))
    return out


def predictive_np32(rec32, wp32, model, free, mix):
    """predictive_term<..., float> restated: d, n (and m, d_b, n_b) in numpy.float32, everything after in float64."""
    from scipy import special
    t32 = term(rec32, wp32, model, free, np.float32, geometry_only=True)
    f = lambda a: np.asarray(a, dtype=np.float64)
    z = f(t32["d"]) / np.sqrt(f(t32["n"]))
    tail = special.erfc(np.abs(z) / np.sqrt(2.0))
    pit = np.where(z < 0, tail / 2, 1 - tail / 2)
    if model in PROFILE:
        sig = np.sqrt(f(wp32[:, 12][:, None]) / np.sqrt(f(t32["a2r2"])))     # star_sigma2: the sum a^2 + r^2 in float, then float64
    else:
        sig = np.sqrt(f(t32["sig2"]))
    out = {"z": z, "t": tail, "pit": pit, "vlos": f(rec32[:, 0][None, :]) - f(t32["d"]), "sig": sig}
    if mix:
        zb = f(t32["db"]) / np.sqrt(f(t32["nb"]))
        tb = special.erfc(np.abs(zb) / np.sqrt(2.0))
        m = f(t32["m"])
        out["pit_mix"] = m * pit + (1 - m) * np.where(zb < 0, tb / 2, 1 - tb / 2)
    return out


def predictive_summary(terms, amp, c=C):
    """terms: dict of exact (S, n) longdouble arrays z, t, pit, vlos, sig (and pit_mix); amp: predictive_amplification.
    Returns (want, bound) for the outputs of mcd_posterior_predictive; the float64 allowance is 1e-12 on the scale of the
    field (tests/predictive_helper.py: the rule's floor) and 1e-10 for the spreads."""
    want, bound = {}, {}
    for name, key in (("z_mean", "z"), ("tail_p", "t"), ("pit", "pit"), ("vlos_mean", "vlos"), ("sigma_mean", "sig"),
                      ("pit_mix", "pit_mix")):
        if key in terms:
            want[name] = terms[key].mean(axis=0)
            bound[name] = (c * U * amp[key]).mean(axis=0) + L(1e-12) * np.maximum(1, np.abs(want[name]))
    for name, key in PRED_STDS:
        x, b = terms[key], c * U * amp[key]
        var = x.var(axis=0, ddof=1) if x.shape[0] > 1 else np.zeros(x.shape[1], dtype=L)
        want[name] = np.sqrt(var)
        bound[name] = _std_bound(var, _var_bound(x, b)) + L(1e-10) * np.maximum(1, np.sqrt(var))
    return want, bound


_TERMS = {}


def cached_terms(model, free, n, rows):
    """Terms of f32_helper.f32_case(model, free, n) at `rows`, built once per process."""
    key = (model, bool(free), n, tuple(rows))
    if key not in _TERMS:
        _TERMS[key] = Terms(fh.cached_case(model, free, n)[0], rows)
    return _TERMS[key]

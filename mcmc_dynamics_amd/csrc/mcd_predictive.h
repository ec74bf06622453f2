// mcd_predictive.h -- per-star posterior predictive checks over posterior samples (mcd_posterior_predictive): the
// (star, sample) term and the running state it is folded into, written once as host+device code so that tests/emul
// compiles the same expressions.
//
// For star i and posterior sample s, with d = v_i - v_los,is and n = verr_i^2 + sigma_los,is^2 from star_d_n (plain form,
// in the record's precision) and everything after that in float64:
//   z       = d / sqrt(n)                      standardised residual against the cluster component
//   t       = erfc(|z| / sqrt 2)               two-sided tail probability of the cluster component
//   pit     = z < 0 ? t / 2 : 1 - t / 2        cluster-component CDF at v_i (one erfc; the small side is never 1 - ...)
//   vlos    = v_i - d                          the model's mean line-of-sight velocity at the star, v_sys included
//   sig     = sqrt(sigma_los^2)                sigma_los^2 formed directly (star_sigma2), never as n - verr^2
//   pit_mix = m pit + (1 - m) Phi(z_b)         MIX (the two models with a Gaussian background): m = rho_i / (rho_i + f_back),
//                                              z_b = (v_i - v_back) / sqrt(verr_i^2 + sigma_back^2), Phi as pit
// Reduced over the samples, not over the stars: Welford's running mean / M2 for z, vlos and sig, a running mean for t, pit
// and pit_mix.  The samples of a launch are cut into slices (mcd_posterior.h: posterior_slices); every slice starts from
// the empty state and the slices' states are merged in slice order (Chan et al.'s pairwise update).  No guard path: a
// non-finite term (sigma = 0 with verr = 0) makes that star's outputs non-finite and touches no other star.
#pragma once

#include "mcd_math.h"

namespace mcd {

constexpr double kInvSqrt2 = 0.707106781186547524400844362105;

// libm's erfc on both sides (the device library's on gfx950: no scratch)
MCD_HD double erfc_(double x) {
#if defined(__HIP_DEVICE_COMPILE__)
    return erfc(x);
#else
    return std::erfc(x);
#endif
}

// sigma_los^2 of one star for one sample: sigma_max^2 for the constant models, sigma_max^2 a / sqrt(a^2 + r^2) for the
// profile models (model.py:93-127), r^2 as star_d_n forms it.
template <int MODEL, bool FREE, class T>
MCD_HD double star_sigma2(RecPtr<T> r, const WalkerConsts<T>& w) {
    if constexpr (!is_profile(MODEL)) {
        return (double)w.s2;
    } else {
        T r2;
        if (FREE) {
            T x, y;
            free_centre_xy(r[2], r[3], r[4], w.sac, w.cac, w.sdc, w.cdc, x, y);
            const T dx = T(kArcsecPerRad) * x, dy = T(kArcsecPerRad) * y;
            r2 = fma_(dx, dx, dy * dy);
        } else {
            r2 = r[4];
        }
        return (double)w.s2a / sqrt_((double)(w.a2 + r2));
    }
}

// (cos theta, sin theta) of one star's position angle for one sample, the angle the model's own v_los uses: the record's
// fields 3 and 2 for the constant models with a fixed centre, else (x, y) / r with the offsets as star_d_n forms them.
// r == 0: (0, 0) for the profile models (their v_los has no angle there), numpy's arctan2(+0, -+0) for the constant ones
// (free_centre_residual: sin = 0, cos = -+1).
template <int MODEL, bool FREE, class T>
MCD_HD void star_unit(RecPtr<T> r, const WalkerConsts<T>& w, double& c, double& s) {
    if constexpr (!is_profile(MODEL) && !FREE) {
        c = (double)r[3];
        s = (double)r[2];
    } else {
        T x, y;
        if (FREE) {
            free_centre_xy(r[2], r[3], r[4], w.sac, w.cac, w.sdc, w.cdc, x, y);
            if constexpr (is_profile(MODEL)) { x = T(kArcsecPerRad) * x; y = T(kArcsecPerRad) * y; }
        } else {
            x = r[2];
            y = r[3];
        }
        const T r2 = (is_profile(MODEL) && !FREE) ? r[4] : fma_(x, x, y * y);
        const double inv = 1.0 / sqrt_((double)r2);
        const bool on = !(r2 > T(0));
        c = on ? (is_profile(MODEL) ? 0.0 : (std::signbit(x) ? -1.0 : 1.0)) : (double)x * inv;
        s = on ? 0.0 : (double)y * inv;
    }
}

// Normal tail and CDF of a standardised residual from ONE erfc: t = P(|Z| > |z|), cdf = P(Z < z).
MCD_HD void normal_tail_cdf(double z, double& t, double& cdf) {
    t = erfc_(fabs_(z) * kInvSqrt2);
    const double h = 0.5 * t;
    cdf = z < 0.0 ? h : 1.0 - h;
}

struct PredTerm { double z, t, pit, vlos, sig, pit_mix; };

template <int MODEL, bool FREE, bool MIX, class T>
MCD_HD void predictive_term(RecPtr<T> r, const WalkerConsts<T>& w, PredTerm& x) {
    static_assert(!MIX || bg_kind(MODEL) == BG_GAUSS, "pit_mix needs a background with a CDF");
    T d, n;
    star_d_n<MODEL, T, FREE>(r, w, d, n);
    x.z = (double)d / sqrt_((double)n);
    normal_tail_cdf(x.z, x.t, x.pit);
    x.vlos = (double)r[0] - (double)d;
    x.sig = sqrt_(star_sigma2<MODEL, FREE, T>(r, w));
    if constexpr (MIX) {
        constexpr int XB = geometry_doubles(MODEL, FREE);
        const T db = r[0] - w.vb, nb = r[1] + w.sb2;          // as star_components forms the background term
        const T rho = r[XB];
        const double m = (double)(rho / (rho + w.fb));
        double tb, cb;
        normal_tail_cdf((double)db / sqrt_((double)nb), tb, cb);
        x.pit_mix = m * x.pit + (1.0 - m) * cb;               // m == 1 gives pit, m == 0 the background CDF, bit for bit
    } else {
        x.pit_mix = 0.0;
    }
}

// Fields of one slice's partial state in the scratch array (each field a contiguous run of n stars) ...
enum PredField : int { PR_ZM = 0, PR_Z2 = 1, PR_VM = 2, PR_V2 = 3, PR_SM = 4, PR_S2 = 5, PR_T = 6, PR_PIT = 7, PR_MIX = 8 };
MCD_HD constexpr int pred_fields(bool mix) { return mix ? 9 : 8; }
// ... and of the result (include/mcd.h: MCD_PRED_*; pit_mix follows as a ninth field on the device)
enum PredOut : int { PO_Z_MEAN = 0, PO_Z_STD = 1, PO_TAIL_P = 2, PO_PIT = 3, PO_VLOS_MEAN = 4, PO_VLOS_STD = 5,
                     PO_SIGMA_MEAN = 6, PO_SIGMA_STD = 7, PO_PIT_MIX = 8 };

// One star's running state over a run of samples (the count is the same for every star of a launch: kept by the caller).
struct PredAcc {
    double zm, z2;                 // Welford on z
    double vm, v2;                 // Welford on vlos
    double sm, s2;                 // Welford on sig
    double tm, pm, qm;             // running means of t, pit, pit_mix

    MCD_HD void init() { zm = z2 = vm = v2 = sm = s2 = tm = pm = qm = 0.0; }

    static MCD_HD void welford(double x, double inv, double& mean, double& m2) {
        const double dx = x - mean;
        mean = fma_(dx, inv, mean);
        m2 = fma_(dx, x - mean, m2);
    }

    // Fold in the (j+1)-th term of the run; inv = 1 / (j + 1).  The first term (inv = 1) gives the term itself and zero
    // M2 exactly; a repeated term leaves both unchanged.
    template <bool MIX>
    MCD_HD void add(const PredTerm& x, double inv) {
        welford(x.z, inv, zm, z2);
        welford(x.vlos, inv, vm, v2);
        welford(x.sig, inv, sm, s2);
        tm = fma_(x.t - tm, inv, tm);
        pm = fma_(x.pit - pm, inv, pm);
        if constexpr (MIX) qm = fma_(x.pit_mix - qm, inv, qm);
    }

    // this (na terms) <- this followed by b (nb terms); na, nb > 0
    template <bool MIX>
    MCD_HD void merge(const PredAcc& b, double na, double nb) {
        const double n = na + nb, wb = nb / n, wab = na * nb / n;
        const double dz = b.zm - zm, dv = b.vm - vm, ds = b.sm - sm;
        zm = fma_(dz, wb, zm);
        z2 = fma_(dz * dz, wab, z2 + b.z2);
        vm = fma_(dv, wb, vm);
        v2 = fma_(dv * dv, wab, v2 + b.v2);
        sm = fma_(ds, wb, sm);
        s2 = fma_(ds * ds, wab, s2 + b.s2);
        tm = fma_(b.tm - tm, wb, tm);
        pm = fma_(b.pm - pm, wb, pm);
        if constexpr (MIX) qm = fma_(b.qm - qm, wb, qm);
    }

    template <bool MIX>
    MCD_HD void load(const double* __restrict__ src, int64_t n) {
        zm = src[PR_ZM * n]; z2 = src[PR_Z2 * n]; vm = src[PR_VM * n]; v2 = src[PR_V2 * n];
        sm = src[PR_SM * n]; s2 = src[PR_S2 * n]; tm = src[PR_T * n]; pm = src[PR_PIT * n];
        qm = MIX ? src[PR_MIX * n] : 0.0;
    }
    template <bool MIX>
    MCD_HD void store(double* __restrict__ dst, int64_t n) const {
        dst[PR_ZM * n] = zm; dst[PR_Z2 * n] = z2; dst[PR_VM * n] = vm; dst[PR_V2 * n] = v2;
        dst[PR_SM * n] = sm; dst[PR_S2 * n] = s2; dst[PR_T * n] = tm; dst[PR_PIT * n] = pm;
        if constexpr (MIX) dst[PR_MIX * n] = qm;
    }

    static MCD_HD double spread(double m2, double s) { return s > 1.0 ? sqrt_(max_(m2, 0.0) / (s - 1.0)) : 0.0; }

    // outputs for S samples in all (field stride n): means, sample standard deviations (0 for S == 1)
    template <bool MIX>
    MCD_HD void finish(double s, double* __restrict__ out, int64_t n) const {
        out[PO_Z_MEAN * n] = zm;
        out[PO_Z_STD * n] = spread(z2, s);
        out[PO_TAIL_P * n] = tm;
        out[PO_PIT * n] = pm;
        out[PO_VLOS_MEAN * n] = vm;
        out[PO_VLOS_STD * n] = spread(v2, s);
        out[PO_SIGMA_MEAN * n] = sm;
        out[PO_SIGMA_STD * n] = spread(s2, s);
        if constexpr (MIX) out[PO_PIT_MIX * n] = qm;
    }
};

#if defined(__HIPCC__)
// mcd_predictive.hip: one pass over n_samples derived sample rows (wpar, [n_samples][KD] in term precision) with the slice
// plan of posterior_slices, then the merge of its slices (and of the n_prev samples of earlier passes kept in `state`,
// [pred_fields][n]); the pass that reaches n_total samples writes out[pred_fields(mix)][n] in PredOut order.
// part: [n_slices][pred_fields(mix)][n] scratch; inv: 1 / (j + 1) for j < slice_len.
struct LaunchShape;
hipError_t launch_predictive(hipStream_t s, const LaunchShape& shape, bool mix, const void* records, int64_t n,
                             const void* wpar, int64_t n_samples, const double* inv, int64_t slice_len, int64_t n_slices,
                             double* part, double* state, int64_t n_prev, int64_t n_total, double* out);
#endif

}  // namespace mcd

// mcd_grad.h -- analytic gradient of the log-likelihood (mcd_loglike_grad_batch): for one star and one walker the term l
// and its partial derivatives with respect to the K kernel columns (C-ABI order, include/mcd.h: mcd_catalog_param_count),
// written once as host+device code so that tests/emul compiles the same expressions.  Plain arithmetic only: true
// division, log_, exp_, float64.
//
// Units are the kernel's: km/s, arcsec for a and r_peak, degrees for the centre (the centre columns carry pi / 180).
//
//   cluster term   lc = -1/2 (ln 2pi + ln n + d^2/n):   dlc/dd = -d/n,   dlc/dn = 1/2 (d^2/n^2 - 1/n)
//   CONST          d = v - v_sys - v_maxx sin(theta) + v_maxy cos(theta),  n = verr^2 + sigma_max^2
//                  dd/dv_sys = -1, dd/dv_maxx = -sin(theta), dd/dv_maxy = cos(theta), dn/dsigma_max = 2 sigma_max
//   PROFILE        d = v - v_sys - 2 r_p cross / (r_p^2 + r^2),  cross = v_maxx dy - v_maxy dx,
//                  n = verr^2 + sigma_max^2 a / sqrt(a^2 + r^2)
//                  dd/dv_maxx = -2 r_p dy / (r_p^2 + r^2), dd/dv_maxy = 2 r_p dx / (r_p^2 + r^2),
//                  dd/dr_p = -2 cross (r^2 - r_p^2) / (r_p^2 + r^2)^2,
//                  dn/dsigma_max = 2 sigma_max a / sqrt(a^2 + r^2),  dn/da = sigma_max^2 r^2 / (a^2 + r^2)^(3/2)
//   DOUBLE         d = v - v_sys - sum_k 2 rho_k cross_k / D_k,  rho_1 = r_p, rho_2 = ratio r_p, D_k = rho_k^2 + r^2,
//                  cross_k = v_maxx_k dy - v_maxy_k dx;  with f_k = 2 rho_k / D_k, g_k = -2 cross_k (r^2 - rho_k^2) / D_k^2:
//                  dd/dv_maxx_k = -f_k dy, dd/dv_maxy_k = f_k dx, dd/dr_p = g_1 + ratio g_2, dd/dratio = r_p g_2,
//                  dd/d(dx) = sum_k f_k (v_maxy_k + 2 cross_k dx / D_k), dd/d(dy) = sum_k f_k (-v_maxx_k + 2 cross_k dy / D_k);
//                  n and its partials are PROFILE's.  The value d itself is formed as the value path forms it (star_d_n).
//   ESCALE         n = err_scale^2 verr^2 + sigma_los^2: dn/derr_scale = 2 err_scale verr^2; d and the other partials are the
//                  base model's (dl/dn is the factor sigma_max's column already forms)
//   free centre    chain rule through free_centre_xy (mcd_math.h): with t = B cos(ra_c) + A sin(ra_c),
//                  dx/dra_c = t, dy/dra_c = sin(dec_c) x, dx/ddec_c = 0, dy/ddec_c = -(sd sin(dec_c) + cos(dec_c) t)
//                  CONST:   sin(theta) = y/r, cos(theta) = x/r, so with u = cross / r (cross = v_maxx y - v_maxy x)
//                           dd/dx = (v_maxy + u cos(theta)) / r,  dd/dy = (-v_maxx + u sin(theta)) / r
//                  PROFILE: dd/d(dx) = 2 r_p (v_maxy + 2 cross dx / D) / D,  dd/d(dy) = 2 r_p (-v_maxx + 2 cross dy / D) / D,
//                           D = r_p^2 + r^2;  dn/d(dx, dy) = -sigma_max^2 a (dx, dy) / (a^2 + r^2)^(3/2)
//   mixtures       l = log(p e^lc + (1 - p) e^lb),  gamma = p e^(lc - l):
//                  dl/dtheta_cluster = gamma dlc/dtheta,  dl/dtheta_background = (1 - gamma) dlb/dtheta,
//                  dlb/dv_back = d_b/n_b,  dlb/dsigma_back = sigma_back (d_b^2/n_b^2 - 1/n_b),
//                  dl/df_back = (e^(lb - l) - e^(lc - l)) rho / (rho + f_back)^2      (finite at f_back = 0)
//                  gamma and 1 - gamma are formed after subtracting max(lc, lb), as mixture_lnl does: neither overflows,
//                  and 1 - gamma is (1 - p) e^(lb - l) itself, not a difference.
//
// A star exactly on a walker's centre: the constant-rotation models have theta undefined there, the value path
// (free_centre_residual) takes numpy's arctan2(+0, -+0) convention, and the gradient uses the same predicate (r^2 > 0):
// such a star contributes sin(theta) = 0, cos(theta) = -+1 to the velocity columns and exactly 0 to the two centre
// columns.  The profile models are smooth at r = 0 and need no special case.
#pragma once

#include "mcd_math.h"

namespace mcd {

constexpr double kDegToRad = 0.017453292519943295769;
constexpr int kGradMaxColumns = 14;       // DOUBLE_BGGAUSS with a free centre

// kernel columns of a model (the C-ABI's parameter order, mcd_prep.h)
MCD_HD constexpr int grad_columns(int model, bool free_centre) {
    return cluster_columns(model) + (free_centre ? 2 : 0) +
           (bg_kind(model) == BG_GAUSS ? 3 : bg_kind(model) == BG_FIXED_DENSITY ? 1 : 0);
}
template <int MODEL, bool FREE> struct GradCols {
    static constexpr bool kProf = is_profile(MODEL);
    static constexpr int kVsys = 0, kSigma = 1, kA = 2, kVx = kProf ? 3 : 2, kVy = kProf ? 4 : 3, kRp = 5;
    static constexpr bool kDouble = is_double(MODEL);
    static constexpr int kVxc = 6, kVyc = 7, kRatio = 8;     // (double models)
    static constexpr bool kEscale = is_escale(MODEL);
    static constexpr int kEs = cluster_columns(MODEL) - 1;   // (error-scale models: err_scale, the last cluster column)
    static constexpr int kRa = cluster_columns(MODEL), kDec = kRa + 1;
    static constexpr int kBg = kRa + (FREE ? 2 : 0);          // v_back, sigma_back, f_back | f_back
    static constexpr int kFb = bg_kind(MODEL) == BG_GAUSS ? kBg + 2 : kBg;
    static constexpr int K = grad_columns(MODEL, FREE);
};

// what the derivatives need of the parameter row itself (WalkerConsts holds squares and products only)
template <class T> struct GradRaw {
    T sigma, a, rp, sb, ratio, es;
    template <int MODEL, bool FREE>
    MCD_HD void load(const double* __restrict__ p) {
        using C = GradCols<MODEL, FREE>;
        sigma = (T)p[C::kSigma];
        a = C::kProf ? (T)p[C::kA] : T(0);
        rp = C::kProf ? (T)p[C::kRp] : T(0);
        sb = bg_kind(MODEL) == BG_GAUSS ? (T)p[C::kBg + 1] : T(0);
        ratio = C::kDouble ? (T)p[C::kRatio] : T(0);
        es = C::kEscale ? (T)p[C::kEs] : T(0);
    }
};

// g[0 .. K) += dl/dtheta_k of one star for one walker; returns l (the value path's plain term: gauss_lnl / mixture_lnl).
// SIM (mcd_simulated_grad.h): the star's velocity is v, not the record's -- the residual becomes d + (v - r[0]) as
// simulated_term (mcd_simulated.h) forms it, the fitted background's v - v_back, and the fixed-background families take
// the Gaussian (bg_mean, bg_sigma2) at v in place of the stored lnlike_bg.  The partials of d and n do not depend on the
// velocity.  Without SIM the three arguments are not read.
template <int MODEL, bool FREE, class T, bool SIM>
MCD_HD T grad_term_at(RecPtr<T> r, const WalkerConsts<T>& w, const GradRaw<T>& q, T v, T bg_mean, T bg_sigma2,
                      T* __restrict__ g) {
    using C = GradCols<MODEL, FREE>;
    constexpr int XB = geometry_doubles(MODEL, FREE);
    constexpr int BG = bg_kind(MODEL);
    // ---- cluster part: d, n and their partials
    T d, n;
    T d_vx, d_vy, d_rp = T(0), n_sigma, n_a = T(0);
    T d_vxc = T(0), d_vyc = T(0), d_ratio = T(0);                  // (double models)
    T d_ra = T(0), d_dec = T(0), n_ra = T(0), n_dec = T(0);
    // free centre, in units of r0: dx/dra_c = t, dy/dra_c = y_ra, dx/ddec_c = 0, dy/ddec_c = y_dec
    T x = T(0), y = T(0), t = T(0), y_ra = T(0), y_dec = T(0);
    if constexpr (FREE) {
        free_centre_xy(r[2], r[3], r[4], w.sac, w.cac, w.sdc, w.cdc, x, y);
        t = fma_(r[3], w.cac, r[2] * w.sac);
        y_ra = w.sdc * x;
        y_dec = -fma_(r[4], w.sdc, w.cdc * t);
    }
    if constexpr (!C::kProf) {
        if constexpr (C::kEscale) n = w.es2 * r[1] + w.s2;         // star_d_n's plain forms, here and below
        else n = r[1] + w.s2;
        n_sigma = T(2) * q.sigma;
        if constexpr (FREE) {
            const T r2 = fma_(x, x, y * y);
            const bool off_centre = r2 > T(0);
            const T inv = off_centre ? T(1) / sqrt_(r2) : T(0);
            const T s = y * inv, c = off_centre ? x * inv : (std::signbit(x) ? T(-1) : T(1));
            const T u = fma_(w.vx, s, -(w.vy * c));
            d = (r[0] - w.vsys) - u;
            // (the value path rounds this residual otherwise, and a simulated term returns simulated_term's bits)
            if constexpr (SIM) d = free_centre_residual<false>(r[2], r[3], r[4], w.sac, w.cac, w.sdc, w.cdc, w.vx, w.vy, r[0] - w.vsys);
            d_vx = -s;
            d_vy = c;
            const T d_x = inv * fma_(u, c, w.vy), d_y = inv * fma_(u, s, -w.vx);     // inv = 0 on the centre
            d_ra = fma_(d_x, t, d_y * y_ra);
            d_dec = d_y * y_dec;
        } else {
            d = fma_(-w.vx, r[2], fma_(w.vy, r[3], r[0] - w.vsys));
            d_vx = -r[2];
            d_vy = r[3];
        }
    } else {
        T dx, dy, r2;
        if constexpr (FREE) {
            dx = T(kArcsecPerRad) * x;
            dy = T(kArcsecPerRad) * y;
            r2 = fma_(dx, dx, dy * dy);
        } else { dx = r[2]; dy = r[3]; r2 = r[4]; }
        const T tt = T(1) / sqrt_(w.a2 + r2);
        const T inv = T(1) / (w.rp2 + r2);
        const T cross = fma_(w.vx, dy, -(w.vy * dx));
        const T f = w.rp_2 * inv;                                  // 2 r_p / (r_p^2 + r^2)
        T f2 = T(0), inv2 = T(0), cross2 = T(0);                   // (double models: the second component's)
        if constexpr (C::kDouble) {
            const T m1 = w.rp2 + r2, m2 = w.rc2 + r2;
            inv2 = T(1) / m2;
            cross2 = fma_(w.vxc, dy, -(w.vyc * dx));
            f2 = w.rc_2 * inv2;
            const T num = fma_(w.rp_2 * cross, m2, (w.rc_2 * cross2) * m1);      // star_d_n's plain form
            d = fma_(-num, T(1) / (m1 * m2), r[0] - w.vsys);
            const T g1 = T(-2) * cross * (r2 - w.rp2) * inv * inv, g2 = T(-2) * cross2 * (r2 - w.rc2) * inv2 * inv2;
            d_rp = fma_(q.ratio, g2, g1);
            d_ratio = q.rp * g2;
            d_vxc = -(f2 * dy);
            d_vyc = f2 * dx;
        } else {
            d = fma_(-f, cross, r[0] - w.vsys);
            d_rp = T(-2) * cross * (r2 - w.rp2) * inv * inv;
        }
        if constexpr (C::kEscale) n = fma_(w.s2a, tt, w.es2 * r[1]);
        else n = fma_(w.s2a, tt, r[1]);
        d_vx = -(f * dy);
        d_vy = f * dx;
        n_sigma = T(2) * q.sigma * q.a * tt;
        const T tt3 = tt * tt * tt;
        n_a = w.s2 * r2 * tt3;
        if constexpr (FREE) {
            const T ci = T(2) * cross * inv;
            T d_dx = f * fma_(ci, dx, w.vy), d_dy = f * fma_(ci, dy, -w.vx);
            if constexpr (C::kDouble) {
                const T ci2 = T(2) * cross2 * inv2;
                d_dx = fma_(f2, fma_(ci2, dx, w.vyc), d_dx);
                d_dy = fma_(f2, fma_(ci2, dy, -w.vxc), d_dy);
            }
            const T n_r = -(w.s2a * tt3);                          // dn/d(dx) = n_r dx, dn/d(dy) = n_r dy
            const T dx_ra = T(kArcsecPerRad) * t, dy_ra = T(kArcsecPerRad) * y_ra, dy_dec = T(kArcsecPerRad) * y_dec;
            d_ra = fma_(d_dx, dx_ra, d_dy * dy_ra);
            d_dec = d_dy * dy_dec;
            n_ra = n_r * fma_(dx, dx_ra, dy * dy_ra);
            n_dec = n_r * (dy * dy_dec);
        }
    }
    if constexpr (SIM) d = d + (v - r[0]);
    const T dn = d / n;
    T c_d = -dn;                                                   // dlc/dd
    T c_n = T(0.5) * (dn * dn - T(1) / n);                         // dlc/dn
    const T lc = gauss_lnl(d, n);
    T l = lc;
    // ---- mixture: responsibilities after subtracting max(lc, lb)
    if constexpr (BG != BG_NONE) {
        T lb, p, rho = T(0), db = T(0), nb = T(1);
        if constexpr (SIM) {
            if constexpr (BG == BG_GAUSS) {
                nb = r[1] + w.sb2;
                db = v - w.vb;
                lb = gauss_lnl(db, nb);
                rho = r[XB];
            } else {
                lb = gauss_lnl(v - bg_mean, r[1] + bg_sigma2);
                if constexpr (BG == BG_FIXED) p = r[XB + 1];
                else rho = r[XB + 2];
            }
            if constexpr (BG != BG_FIXED) p = rho / (rho + w.fb);
        } else
        if (BG == BG_FIXED) { lb = r[XB]; p = r[XB + 1]; }
        else if (BG == BG_FIXED_DENSITY) { lb = r[XB]; rho = r[XB + 2]; p = rho / (rho + w.fb); }
        else {
            nb = r[1] + w.sb2;
            db = r[0] - w.vb;
            lb = gauss_lnl(db, nb);
            rho = r[XB];
            p = rho / (rho + w.fb);
        }
        const T mx = max_(lc, lb);
        const T ec = exp_(lc - mx), eb = exp_(lb - mx);
        const T sum = p * ec + (T(1) - p) * eb;
        l = mx + log_(sum);                                        // mixture_lnl(lc, lb, p), term by term
        const T gamma = p * ec / sum, rest = (T(1) - p) * eb / sum;
        c_d *= gamma;
        c_n *= gamma;
        if constexpr (BG == BG_GAUSS) {
            const T bn = db / nb;
            g[C::kBg] += rest * bn;
            g[C::kBg + 1] += rest * (q.sb * (bn * bn - T(1) / nb));
        }
        if constexpr (BG != BG_FIXED) {
            const T rf = rho + w.fb;
            g[C::kFb] += (eb - ec) / sum * (rho / (rf * rf));
        }
    }
    g[C::kVsys] -= c_d;
    g[C::kSigma] += c_n * n_sigma;
    g[C::kVx] += c_d * d_vx;
    g[C::kVy] += c_d * d_vy;
    if constexpr (C::kProf) {
        g[C::kA] += c_n * n_a;
        g[C::kRp] += c_d * d_rp;
    }
    if constexpr (C::kDouble) {
        g[C::kVxc] += c_d * d_vxc;
        g[C::kVyc] += c_d * d_vyc;
        g[C::kRatio] += c_d * d_ratio;
    }
    if constexpr (C::kEscale) g[C::kEs] += c_n * (T(2) * q.es * r[1]);      // dn/derr_scale = 2 err_scale verr^2
    if constexpr (FREE) {
        if constexpr (C::kProf) {
            g[C::kRa] += T(kDegToRad) * fma_(c_d, d_ra, c_n * n_ra);
            g[C::kDec] += T(kDegToRad) * fma_(c_d, d_dec, c_n * n_dec);
        } else {
            g[C::kRa] += T(kDegToRad) * (c_d * d_ra);
            g[C::kDec] += T(kDegToRad) * (c_d * d_dec);
        }
    }
    return l;
}

template <int MODEL, bool FREE, class T = double>
MCD_HD T grad_term(RecPtr<T> r, const WalkerConsts<T>& w, const GradRaw<T>& q, T* __restrict__ g) {
    return grad_term_at<MODEL, FREE, T, false>(r, w, q, T(0), T(0), T(0), g);
}

// One chunk of stars for one walker: acc[0] += sum of l, acc[1 + k] += sum of dl/dtheta_k (star order).
template <int MODEL, bool FREE, class T = double>
MCD_HD void chunk_grad(RecPtr<T> r, int count, const WalkerConsts<T>& w, const GradRaw<T>& q, T* __restrict__ acc) {
    constexpr int ND = record_doubles(MODEL, FREE);
    for (int j = 0; j < count; ++j, r += ND) acc[0] += grad_term<MODEL, FREE, T>(r, w, q, acc + 1);
}

#if defined(__HIPCC__)
// mcd_grad.hip: value and gradient partial sums of every (chunk, walker) of a work set, and their fixed-order
// reduction.  partials: [1 + K][roundup64(W) / 8][n_chunks][8];  out: [n_psets][1 + K][roundup64(W)] (field 0 the value).
struct LaunchShape;
struct Chunk;
hipError_t launch_loglike_grad(hipStream_t s, const LaunchShape& shape, const void* records, const Chunk* chunks,
                               int64_t n_chunks, const double* params, const void* wpar, double* partials,
                               int64_t n_walkers);
hipError_t launch_grad_reduce(hipStream_t s, const LaunchShape& shape, const double* partials, int64_t n_chunks,
                              const int64_t* pset_slot_offsets, int64_t n_psets, int64_t max_chunks_per_pset,
                              int64_t n_walkers, double* out);
#endif

}  // namespace mcd

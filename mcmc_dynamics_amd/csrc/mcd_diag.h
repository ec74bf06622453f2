// mcd_diag.h -- host+device: convergence diagnostics of a stored chain -- the integrated autocorrelation time of emcee's
// autocorr.integrated_time, split-R-hat (BDA3) and the pooled moments.  One text for the device kernels (mcd_diag.hip), the
// host loop behind mcd_chain_diagnostics(ctx = NULL) (mcd_api_diag.hip) and the CPU harness tests/emul/diag_emul.cpp.  No
// HIP types; compiled with -ffp-contract=off everywhere, fused multiply-adds are written out as fma_.  DESIGN.md 3.13.
//
// The chain is chain[T][G][W][P] float64 (steps, independent ensembles, walkers, parameters).  A SERIES is one (g, w, p):
// sample t of series s = (g W + w) P + p is x[t * stride + s], stride = G W P.
//
//   centring   d_t = x_t - x_0,  y_t = d_t - (sum_t d_t) / T        (the first value leaves before any sum: a column at
//              56.3 with a posterior width of 1e-6 keeps its digits)
//   lag sums   a_k = sum_{u = 0}^{T-1-k} y_u y_{u+k},  k = 0 .. L    (no 1 / (T - k))
//   per (g,p)  rho_k = (sum_w a_k[w] / a_0[w]) / W                   (each walker normalised, then the mean in walker order)
//              tau_k = 2 sum_{j <= k} rho_j - 1;  window = the smallest k with k >= c tau_k;  found = 1, tau = tau_window;
//              none up to L: found = 0, tau = tau_L, window = L.  A walker with a_0 = 0: rho, tau, rhat NaN, found = 0.
//   moments    per series the mean and M2 of the first and of the last n = floor(T / 2) steps (two passes over d_t)
//   split-Rhat m = 2 W half-chains of length n:  B = n / (m - 1) sum_j (mean_j - mean)^2,  Wv = mean of the ddof = 1
//              variances,  rhat = sqrt(((n - 1) / n Wv + B / n) / Wv);  NaN for T < 4, Wv = 0 or a walker with a_0 = 0
//   pooled     mean and ddof = 1 variance over the T W samples of (g, p)
//
// Order of every sum (what makes host and device agree bit for bit, and a result independent of how the series are tiled):
// sums over t or u ascend from 0.0, one fma or one addition per sample; sums over walkers ascend in w from 0.0; the prefix
// sum over lags ascends in k.  Means across walkers are taken relative to walker 0's first value (`ref`), so that they too
// are sums of small numbers.  A lag sum is walked in blocks of kDiagLags lags (diag_lag_walk): per step one new value meets
// a ring of kDiagLags older ones; the ring's slots are addressed by compile-time indices of an unrolled loop, and slots
// before the series' start / values past its end are 0.0, which a finite fma chain that starts at +0.0 does not notice.
// (A non-finite sample makes its series' rho NaN on either path.)
#pragma once

#include <cmath>
#include <cstdint>
#include <vector>

#include "mcd_math.h"   // MCD_HD, fma_, sqrt_

namespace mcd {

constexpr int kDiagLags = 16;        // lags per walk of a series
constexpr int kDiagMoments = 7;      // per-series fields of diag_series_moments
enum DiagMoment { DM_X0 = 0, DM_MEAN = 1, DM_M2 = 2, DM_MEAN_A = 3, DM_M2_A = 4, DM_MEAN_B = 5, DM_M2_B = 6 };

// One series: x_0, the mean of d_t = x_t - x_0 and M2 = sum (d_t - mean)^2 over all steps (M2 = a_0), over the first
// n = T / 2 steps (A) and over the last n (B).  out[f * out_stride].
MCD_HD void diag_series_moments(const double* x, int64_t stride, int64_t T, double* out, int64_t out_stride) {
    const int64_t n = T / 2;
    const double x0 = x[0];
    double s = 0.0, sa = 0.0, sb = 0.0;
#pragma unroll 8
    for (int64_t t = 0; t < T; ++t) {
        const double d = x[t * stride] - x0;
        s += d;
        if (t < n) sa += d;
        if (t >= T - n) sb += d;
    }
    const double mean = s / (double)T;
    const double ma = n > 0 ? sa / (double)n : 0.0, mb = n > 0 ? sb / (double)n : 0.0;
    double q = 0.0, qa = 0.0, qb = 0.0;
#pragma unroll 8
    for (int64_t t = 0; t < T; ++t) {
        const double d = x[t * stride] - x0;
        const double e = d - mean;
        q = fma_(e, e, q);
        if (t < n) {
            const double ea = d - ma;
            qa = fma_(ea, ea, qa);
        }
        if (t >= T - n) {
            const double eb = d - mb;
            qb = fma_(eb, eb, qb);
        }
    }
    out[DM_X0 * out_stride] = x0;
    out[DM_MEAN * out_stride] = mean;
    out[DM_M2 * out_stride] = q;
    out[DM_MEAN_A * out_stride] = ma;
    out[DM_M2_A * out_stride] = qa;
    out[DM_MEAN_B * out_stride] = mb;
    out[DM_M2_B * out_stride] = qb;
}

// kDiagLags steps of diag_lag_walk from step t on; GUARD: some of them may lie past the series' end
template <bool GUARD>
MCD_HD void diag_lag_steps(const double* x, int64_t stride, int64_t T, double x0, double mean, int64_t k0, int64_t t, double* r,
                           double* acc) {
#pragma unroll
    for (int i = 0; i < kDiagLags; ++i) {
        const int64_t tt = t + i;
        double lead = 0.0, old = 0.0;
        if (!GUARD || tt < T) {
            lead = (x[tt * stride] - x0) - mean;
            old = (x[(tt - k0) * stride] - x0) - mean;
        }
        r[i] = old;                                        // slot i held y_{tt - k0 - kDiagLags}
#pragma unroll
        for (int j = 0; j < kDiagLags; ++j) acc[j] = fma_(r[(i - j) & (kDiagLags - 1)], lead, acc[j]);
    }
}

// acc[j] = a_{k0 + j} of one series, j = 0 .. kDiagLags - 1 (lags beyond T - 1 come out 0.0; the caller keeps k <= L).
MCD_HD void diag_lag_walk(const double* x, int64_t stride, int64_t T, double x0, double mean, int64_t k0, double* acc) {
    double r[kDiagLags];
#pragma unroll
    for (int j = 0; j < kDiagLags; ++j) {
        r[j] = 0.0;
        acc[j] = 0.0;
    }
    int64_t t = k0;
    for (; t + kDiagLags <= T; t += kDiagLags) diag_lag_steps<false>(x, stride, T, x0, mean, k0, t, r, acc);
    if (t < T) diag_lag_steps<true>(x, stride, T, x0, mean, k0, t, r, acc);
}

// rho_k of one (g, p): a [L + 1][a_stride] lag sums with the group's series (w P + p) at column a_col0 + w P + p
MCD_HD double diag_rho_mean(const double* a, int64_t a_stride, int64_t col0, int64_t W, int P, int p, int64_t k) {
    double s = 0.0;
    for (int64_t w = 0; w < W; ++w) {
        const int64_t col = col0 + w * P + p;
        s += a[k * a_stride + col] / a[col];
    }
    return s / (double)W;
}

// The window search, fed with rho_0, rho_1, ... in order.
struct DiagWindow {
    double csum = 0.0, tau = 0.0;
    int64_t k = 0, window = 0;
    int found = 0;
    MCD_HD void feed(double rho, double c) {
        csum += rho;
        const double tau_k = 2.0 * csum - 1.0;
        if (!found) {
            tau = tau_k;
            window = k;
            if ((double)k >= c * tau_k) found = 1;
        }
        ++k;
    }
};

// rhat, mean, var of one (g, p) from the moments of its W series: mom [kDiagMoments][m_stride], columns as above.
MCD_HD void diag_group_moments(const double* mom, int64_t m_stride, int64_t col0, int64_t W, int P, int p, int64_t T,
                               double* rhat, double* mean, double* var) {
    const double* x0 = mom + DM_X0 * m_stride + col0 + p;
    const double* mu = mom + DM_MEAN * m_stride + col0 + p;
    const double* m2 = mom + DM_M2 * m_stride + col0 + p;
    const double ref = x0[0];
    bool flat = false;
    double s = 0.0;
    for (int64_t w = 0; w < W; ++w) {
        s += (x0[w * P] - ref) + mu[w * P];
        flat = flat || !(m2[w * P] != 0.0);                // (a_0 = 0; a NaN a_0 is not "flat": it is NaN already)
    }
    const double centre = s / (double)W;
    double ss = 0.0;
    for (int64_t w = 0; w < W; ++w) {
        const double d = ((x0[w * P] - ref) + mu[w * P]) - centre;
        const double dd = d * d;
        ss += m2[w * P] + (double)T * dd;
    }
    *mean = ref + centre;
    *var = ss / (double)(T * W - 1);

    const int64_t n = T / 2;
    const double nan = __builtin_nan("");
    *rhat = nan;
    if (T < 4 || flat) return;
    const double* ma = mom + DM_MEAN_A * m_stride + col0 + p;
    const double* qa = mom + DM_M2_A * m_stride + col0 + p;
    const double* mb = mom + DM_MEAN_B * m_stride + col0 + p;
    const double* qb = mom + DM_M2_B * m_stride + col0 + p;
    const double m = (double)(2 * W);
    double sh = 0.0;
    for (int64_t w = 0; w < W; ++w) {
        sh += (x0[w * P] - ref) + ma[w * P];
        sh += (x0[w * P] - ref) + mb[w * P];
    }
    const double tbar = sh / m;
    double bs = 0.0, ws = 0.0;
    for (int64_t w = 0; w < W; ++w) {
        const double da = ((x0[w * P] - ref) + ma[w * P]) - tbar;
        const double db = ((x0[w * P] - ref) + mb[w * P]) - tbar;
        const double da2 = da * da, db2 = db * db;
        bs += da2;
        bs += db2;
        ws += qa[w * P] / (double)(n - 1);
        ws += qb[w * P] / (double)(n - 1);
    }
    const double B = (double)n / (m - 1.0) * bs;
    const double Wv = ws / m;
    if (!(Wv > 0.0)) return;
    const double within = (double)(n - 1) / (double)n * Wv;
    const double between = B / (double)n;
    *rhat = sqrt_((within + between) / Wv);
}

// Bytes of device scratch one group needs: its series, their lag sums and moments, and its rho rows.
inline int64_t diag_group_bytes(int64_t T, int64_t W, int P, int64_t L) {
    return 8 * (W * P * (T + (L + 1) + kDiagMoments) + (int64_t)P * (L + 1));
}
// Whole groups per device tile under a budget of `budget` bytes; 0: not even one.
inline int64_t diag_tile_groups(int64_t T, int64_t G, int64_t W, int P, int64_t L, int64_t budget) {
    const int64_t n = budget / diag_group_bytes(T, W, P, L);
    return n < G ? n : G;
}

// The host loop: groups [g0, g0 + ng) of the chain; outputs indexed by the absolute (g, p), rho [G][P][L + 1] or null.
// Without rho the lag blocks of a group stop once every parameter's window is found: the result depends on that prefix only.
// a: [(L + 1)][W P] and mom: [kDiagMoments][W P] work arrays of the caller.
inline void diag_host_groups(const double* chain, int64_t T, int64_t G, int64_t W, int P, int64_t L, double c, int64_t g0,
                             int64_t ng, double* a, double* mom, double* tau, int64_t* window, int32_t* found, double* rhat,
                             double* mean, double* var, double* rho) {
    const int64_t stride = G * W * P, ns = W * P;
    for (int64_t g = g0; g < g0 + ng; ++g) {
        const double* x = chain + g * ns;
        for (int64_t s = 0; s < ns; ++s) diag_series_moments(x + s, stride, T, mom + s, ns);
        std::vector<DiagWindow> win((size_t)P);
        for (int64_t k0 = 0; k0 <= L; k0 += kDiagLags) {
            const int64_t nk = (L + 1 - k0) < kDiagLags ? (L + 1 - k0) : kDiagLags;
            for (int64_t s = 0; s < ns; ++s) {
                double acc[kDiagLags];
                diag_lag_walk(x + s, stride, T, mom[DM_X0 * ns + s], mom[DM_MEAN * ns + s], k0, acc);
                for (int64_t j = 0; j < nk; ++j) a[(k0 + j) * ns + s] = acc[j];
            }
            bool all = true;
            for (int p = 0; p < P; ++p) {
                for (int64_t j = 0; j < nk; ++j) {
                    const double r = diag_rho_mean(a, ns, 0, W, P, p, k0 + j);
                    if (rho) rho[(g * P + p) * (L + 1) + k0 + j] = r;
                    win[p].feed(r, c);
                }
                all = all && win[p].found;
            }
            if (all && !rho) break;
        }
        for (int p = 0; p < P; ++p) {
            const int64_t o = g * P + p;
            tau[o] = win[p].tau;
            window[o] = win[p].window;
            found[o] = win[p].found;
            diag_group_moments(mom, ns, 0, W, P, p, T, rhat + o, mean + o, var + o);
        }
    }
}

#if defined(__HIPCC__)
// x [T][ns] (the tile's series), a [L + 1][ns], mom [kDiagMoments][ns], rho_rows [ng P][L + 1]; outputs [ng P]
hipError_t launch_diag(hipStream_t s, const double* x, int64_t T, int64_t ng, int64_t W, int P, int64_t L, double c, double* a,
                       double* mom, double* rho_rows, double* tau, int64_t* window, int32_t* found, double* rhat, double* mean,
                       double* var);
#endif

}  // namespace mcd

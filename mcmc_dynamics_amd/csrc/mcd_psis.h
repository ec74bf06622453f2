// mcd_psis.h -- Pareto-smoothed importance-sampling leave-one-out cross-validation per star (mcd_psis_loo): the per-star
// arithmetic, written once as host+device code so that tests/emul compiles the same expressions.
//
// For star i the S posterior samples give lnL_is (the term of mcd_posterior.h: posterior_term) and the log importance
// ratios r_s = -lnL_is.  PSIS as the R package loo states it (psis() / loo(); Vehtari, Gelman & Gabry 2017; Vehtari,
// Simpson, Gelman, Yao & Gabry 2024):
//   M = min(ceil(0.2 S), ceil(3 sqrt(S / r_eff)))                            psis_tail_len
//   lw_s = r_s - max_s r_s; order ascending, ties by sample index           psis_key (order-preserving, -0 -> +0)
//   the tail: the last M of that order; the cutoff: the (M+1)-th largest
//   x = exp(tail) - exp(cutoff), fitted with Zhang & Stephens' (2009) GPD estimator as loo's gpdfit states it
//                                                                           gpd_grid_m, gpd_theta, gpd_mean_log1p,
//                                                                           gpd_profile, gpd_adjust
//   tail t (1..M, sorted) <- log(qgpd((t - 0.5) / M) + exp(cutoff))         psis_smoothed
//   lw_s <- min(lw_s, 0); elpd_loo_i = logsumexp(lw + lnL) - logsumexp(lw); n_eff_i = r_eff / sum_s w~_s^2
// One deliberate deviation from loo: a tail whose values are all equal (max - min < DBL_EPSILON / 100) is not smoothed
// and gets k^ = -inf (loo reports +inf): a constant tail is not a heavy tail.
#pragma once

#include <cfloat>

#include "mcd_math.h"

namespace mcd {

#if defined(__HIP_DEVICE_COMPILE__)
MCD_HD double log1p_(double x) { return log1p(x); }
MCD_HD double expm1_(double x) { return expm1(x); }
MCD_HD double ceil_(double x) { return ceil(x); }
MCD_HD double floor_(double x) { return floor(x); }
MCD_HD uint64_t dbits_(double x) { return (uint64_t)__double_as_longlong(x); }
MCD_HD double bitsd_(uint64_t u) { return __longlong_as_double((long long)u); }
#else
MCD_HD double log1p_(double x) { return std::log1p(x); }
MCD_HD double expm1_(double x) { return std::expm1(x); }
MCD_HD double ceil_(double x) { return std::ceil(x); }
MCD_HD double floor_(double x) { return std::floor(x); }
MCD_HD uint64_t dbits_(double x) { uint64_t u; std::memcpy(&u, &x, 8); return u; }
MCD_HD double bitsd_(uint64_t u) { double x; std::memcpy(&x, &u, 8); return x; }
#endif

// Largest tail the device keeps in LDS (mcd_psis.hip): M <= kPsisMaxTail, i.e. S / r_eff up to (2560 / 3)^2 ~ 7.3e5.
constexpr int64_t kPsisMaxTail = 2560;
// Largest GPD grid: m = 30 + floor(sqrt(M)) <= 30 + 50 for M <= kPsisMaxTail.
constexpr int kPsisMaxGrid = 96;

// Tail length M for S samples and relative efficiency r_eff (> 0).
MCD_HD int64_t psis_tail_len(int64_t S, double r_eff) {
    const double a = ceil_(0.2 * (double)S);
    const double b = ceil_(3.0 * sqrt_(1.0 * (double)S / r_eff));
    return (int64_t)(a < b ? a : b);
}

// Order-preserving unsigned key of a double (NaN aside): key(a) < key(b) iff a < b; -0 and +0 share the key of +0, so
// equal values always tie and the sample index decides.
MCD_HD uint64_t psis_key(double v) {
    const uint64_t u = dbits_(v == 0.0 ? 0.0 : v);
    return (u >> 63) ? ~u : (u | 0x8000000000000000ull);
}
MCD_HD double psis_unkey(uint64_t k) { return bitsd_((k >> 63) ? (k & 0x7fffffffffffffffull) : ~k); }

// The k^ threshold above which a star's leave-one-out estimate is unreliable: min(1 - 1/log10(S), 0.7).
MCD_HD double psis_k_threshold(int64_t S) {
    const double t = 1.0 - 1.0 / (log_((double)S) / log_(10.0));
    return t < 0.7 ? t : 0.7;
}

// A tail whose values span less than this is constant: no fit, k^ = -inf.
constexpr double kPsisConstTail = DBL_EPSILON / 100.0;

// ---- generalized Pareto fit (Zhang & Stephens 2009, as loo's gpdfit states it); x ascending, length M -------------
MCD_HD int gpd_grid_m(int64_t M) { return 30 + (int)floor_(sqrt_((double)M)); }
// x* = x[floor(M/4 + 0.5) - 1]
MCD_HD int64_t gpd_xstar_index(int64_t M) { return (int64_t)floor_((double)M / 4.0 + 0.5) - 1; }
// theta_j, j = 1..m
MCD_HD double gpd_theta(int j, int m, double x_last, double x_star) {
    return 1.0 / x_last + (1.0 - sqrt_((double)m / ((double)j - 0.5))) / (3.0 * x_star);
}
// mean_t log1p(-theta x_t), summed in t order (x may live in LDS)
MCD_HD double gpd_mean_log1p(double theta, const double* x, int64_t M) {
    double s = 0.0;
    for (int64_t t = 0; t < M; ++t) s += log1p_(-theta * x[t]);
    return s / (double)M;
}
// profile log-likelihood l_j = M (log(-theta/k) - k - 1) of grid point theta with k = gpd_mean_log1p(theta)
MCD_HD double gpd_profile(double theta, double k, int64_t M) { return (double)M * (log_(-theta / k) - k - 1.0); }
// the weakly informative prior's adjustment of k (a NaN becomes +inf)
MCD_HD double gpd_adjust(double k, int64_t M) {
    const double kh = ((double)M * k + 5.0) / ((double)M + 10.0);
    return kh != kh ? INFINITY : kh;
}

// Smoothed log weight of sorted tail position t (0-based) for a finite k^: log(qgpd(p_t) + exp(cutoff)), p_t = (t+0.5)/M,
// truncated at 0.
MCD_HD double psis_smoothed(int64_t t, int64_t M, double khat, double sigma, double exp_cutoff) {
    const double p = ((double)t + 0.5) / (double)M;
    const double l = log1p_(-p);
    const double q = khat == 0.0 ? -sigma * l : sigma * expm1_(-khat * l) / khat;
    const double v = log_(q + exp_cutoff);
    return v < 0.0 ? v : 0.0;
}

// Output fields of mcd_psis_loo in the device's out[4][n].
enum PsisField : int { PSF_ELPD = 0, PSF_K = 1, PSF_LPPD = 2, PSF_NEFF = 3 };

// Term-tile plan of a device call: stars per tile so that the tile's [star][S] terms plus the sample table and the
// parameter pass fit `budget` bytes.  A multiple of 64 stars when >= 64; 0 when not even one star fits.
MCD_HD int64_t psis_tile_stars(int64_t n, int64_t S, int64_t fixed_bytes, int64_t budget) {
    const int64_t row = S * 8;
    if (budget - fixed_bytes < row) return 0;
    int64_t t = (budget - fixed_bytes) / row;
    if (t >= 64) t -= t % 64;
    return t < n ? t : n;
}

// ---- leave-one-out expectations under the same weights (mcd_psis_loo_expect) ---------------
// Rows of one star in the term tile [star][rows][S]: lnL first, then what the call asked for.
enum LooxRow : int { LR_LNL = 0, LR_PIT = 1, LR_Z = 2, LR_VLOS = 3, LR_SIG = 4, LR_MIX = 5 };
// What the term kernel writes next to lnL: nothing, the four predictive rows, or those and pit_mix.
enum LooxMode : int { LOOX_NONE = 0, LOOX_PRED = 1, LOOX_PRED_MIX = 2 };
MCD_HD constexpr int loox_rows(int mode) { return mode == LOOX_NONE ? 1 : mode == LOOX_PRED ? 5 : 6; }
// Most star-independent functions of the sample per call (include/mcd.h: MCD_LOO_MAX_FUNC).
constexpr int kLooMaxFunc = 16;
// Fields of the device's out[][n]: k^, n_eff, then the rows after lnL in LooxRow order, then the functions.
enum LooxField : int { LXF_K = 0, LXF_NEFF = 1, LXF_ROWS = 2 };

// Un-normalised weight of a sample whose (smoothed or raw) log weight is v <= 0, with the shift mw of the star: the
// e_s of a1 = sum_s e_s in psis_tail_kernel.
MCD_HD double loox_weight(double v, double mw) { return exp_(v - mw); }
// E_loo[x] = sum_s e_s x_s / sum_s e_s
MCD_HD double loox_ratio(double num, double den) { return num / den; }

// psis_tile_stars for tiles of `rows` rows of S terms per star.
MCD_HD int64_t psis_tile_stars_rows(int64_t n, int64_t S, int64_t rows, int64_t fixed_bytes, int64_t budget) {
    const int64_t row = S * 8 * rows;
    if (budget - fixed_bytes < row) return 0;
    int64_t t = (budget - fixed_bytes) / row;
    if (t >= 64) t -= t % 64;
    return t < n ? t : n;
}

#if defined(__HIPCC__)
// mcd_psis.hip: PSIS-LOO of the n stars of one tile (records: the tile's first record; wpar: the S derived sample rows,
// [S][KD] in term precision).  terms: [n][S] float64 scratch; out: out[f * out_stride + i] for the four PsisFields.
struct LaunchShape;
hipError_t launch_psis(hipStream_t s, const LaunchShape& shape, const void* records, int64_t n, const void* wpar,
                       int64_t S, int64_t M, double r_eff, double* terms, double* out, int64_t out_stride);
// mcd_loo_expect.hip: the leave-one-out expectations of the n stars of one tile.  mode: LooxMode; terms: [n][rows][S]
// float64 scratch; func: [S][n_func] on the device (null when n_func == 0); out: out[f * out_stride + i], LooxField.
hipError_t launch_loo_expect(hipStream_t s, const LaunchShape& shape, int mode, const void* records, int64_t n,
                             const void* wpar, int64_t S, int64_t M, double r_eff, const double* func, int n_func,
                             double* terms, double* out, int64_t out_stride);
#endif

}  // namespace mcd

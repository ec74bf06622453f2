// mcd_posterior.h -- per-star summaries over posterior samples (mcd_pointwise_posterior): the (star, sample) term and the
// running state it is folded into, written once as host+device code so that tests/emul compiles the same expressions.
//
// For star i and posterior sample s the term is lnL_is = the star's summand of lnlike (the mixture of runner.py:282-284 /
// constant.py:320-323 for the background models, the Gaussian term otherwise) and, for the background models, the
// membership probability p_is exactly as per_star_kernel mode 0 forms it (constant.py:366-374; the ModelFit classes
// subtract max(lc, lb) first, model.py:505-510, 680-687).  Reduced over the samples, not over the stars:
//   lppd_i    = log( (1/S) sum_s exp(lnL_is) )   running log-sum-exp: a shift (the largest term so far) and the sum of
//                                                exp(term - shift), rescaled when a larger term arrives -- never underflows
//                                                to -inf however negative the terms are (-1e4 and below)
//   lnl_var_i = sample variance of lnL_is        Welford's running mean / M2 (no E[x^2] - E[x]^2 cancellation)
//   pmem_*_i  = mean / sd of p_is                the same Welford update (a constant p gives an exactly-zero M2)
// The samples of a launch are cut into slices; every slice starts from the empty state and the slices' states are merged
// in slice order (Chan et al.'s pairwise update), so the result depends on the slice plan only at the rounding level.
#pragma once

#include "mcd_math.h"

namespace mcd {

// One star's running state over a run of samples (the count is the same for every star of a launch: kept by the caller).
struct PostAcc {
    double shift, sumexp;          // log-sum-exp: max term so far, sum of exp(term - shift)
    double mean, m2;               // Welford on lnL
    double pmean, pm2;             // Welford on the membership probability (background models)

    MCD_HD void init() {
        shift = -INFINITY; sumexp = 0.0; mean = 0.0; m2 = 0.0; pmean = 0.0; pm2 = 0.0;
    }

    // Fold in the (j+1)-th term of the run; inv = 1 / (j + 1).  The first term (inv = 1) gives shift = x, sumexp = 1,
    // mean = x, m2 = 0 exactly.
    template <bool MEM>
    MCD_HD void add(double x, double p, double inv) {
        const double d = x - shift;
        const bool up = d > 0.0;
        const double e = exp_(up ? -d : d);                  // exp(-|x - shift|) <= 1
        sumexp = up ? fma_(sumexp, e, 1.0) : sumexp + e;
        shift = up ? x : shift;
        const double dx = x - mean;
        mean = fma_(dx, inv, mean);
        m2 = fma_(dx, x - mean, m2);
        if constexpr (MEM) {
            const double dp = p - pmean;
            pmean = fma_(dp, inv, pmean);
            pm2 = fma_(dp, p - pmean, pm2);
        }
    }

    // this (na terms) <- this followed by b (nb terms); na, nb > 0
    template <bool MEM>
    MCD_HD void merge(const PostAcc& b, double na, double nb) {
        const double mx = max_(shift, b.shift);
        sumexp = fma_(sumexp, exp_(shift - mx), b.sumexp * exp_(b.shift - mx));
        shift = mx;
        const double n = na + nb, wb = nb / n, wab = na * nb / n;
        const double dx = b.mean - mean;
        mean = fma_(dx, wb, mean);
        m2 = fma_(dx * dx, wab, m2 + b.m2);
        if constexpr (MEM) {
            const double dp = b.pmean - pmean;
            pmean = fma_(dp, wb, pmean);
            pm2 = fma_(dp * dp, wab, pm2 + b.pm2);
        }
    }

    // outputs for S samples in all: lppd, sample variance of lnL (0 for S == 1), mean and sd of p
    MCD_HD void finish(double s, double& lppd, double& lnl_var, double& p_mean, double& p_std) const {
        lppd = shift + (log_(sumexp) - log_(s));
        lnl_var = s > 1.0 ? max_(m2, 0.0) / (s - 1.0) : 0.0;
        p_mean = pmean;
        p_std = s > 1.0 ? sqrt_(max_(pm2, 0.0) / (s - 1.0)) : 0.0;
    }
};

// Fields of one slice's partial state in the scratch array (each field a contiguous run of n stars).
enum PostField : int { PF_SHIFT = 0, PF_SUMEXP = 1, PF_MEAN = 2, PF_M2 = 3, PF_PMEAN = 4, PF_PM2 = 5 };
MCD_HD constexpr int post_fields(bool mem) { return mem ? 6 : 4; }

// The (star, sample) term: lnL_is into x, the membership probability into p (MEM: background models only).
template <int MODEL, bool FREE, bool MEM, class T>
MCD_HD void posterior_term(RecPtr<T> r, const WalkerConsts<T>& w, double& x, double& p) {
    T lc, lb, m;
    star_components<MODEL, FREE, T>(r, w, lc, lb, m);
    if constexpr (bg_kind(MODEL) == BG_NONE) {
        x = (double)lc;
        p = 0.0;
    } else {
        x = (double)mixture_lnl(lc, lb, m);
        if constexpr (MEM) {
            // per_star_kernel, mode 0 (mcd_kernels.hip)
            const T shift = is_profile(MODEL) ? max_(lc, lb) : T(0);
            const T ec = m * exp_(lc - shift), eb = (T(1) - m) * exp_(lb - shift);
            p = (double)(ec / (ec + eb));
        } else {
            p = 0.0;
        }
    }
}

// Slice plan of a launch over n stars (lane = star, 64 per wave) and s samples: enough slices that the chip holds
// >= 4 waves per SIMD twice over (256 CUs x 4 SIMDs x 4 waves x 2 = 8192 waves), no slice shorter than kMinSliceLen
// samples, at most kMaxSlices.  Returns the number of slices; *slice_len: samples per slice (the last may be shorter).
constexpr int64_t kPostTargetWaves = 8192;
constexpr int64_t kPostMinSliceLen = 64;
constexpr int64_t kPostMaxSlices = 1024;
MCD_HD int64_t posterior_slices(int64_t n, int64_t s, int64_t* slice_len) {
    const int64_t n_tiles = (n + 63) / 64;
    int64_t want = n_tiles > 0 ? (kPostTargetWaves + n_tiles - 1) / n_tiles : 1;
    const int64_t by_len = (s + kPostMinSliceLen - 1) / kPostMinSliceLen;
    if (want > by_len) want = by_len;
    if (want > kPostMaxSlices) want = kPostMaxSlices;
    if (want < 1) want = 1;
    const int64_t len = (s + want - 1) / want;
    *slice_len = len;
    return (s + len - 1) / len;
}

#if defined(__HIPCC__)
// mcd_posterior.hip: one pass over n_samples derived sample rows (wpar, [n_samples][KD] in term precision) with the slice
// plan above, then the merge of its slices (and of the n_prev samples of earlier passes kept in `state`,
// [post_fields][n]); the pass that reaches n_total samples writes out[4][n] = lppd, lnl_var, pmem_mean, pmem_std.
// part: [n_slices][post_fields(mem)][n] scratch; inv: 1 / (j + 1) for j < slice_len.
struct LaunchShape;
hipError_t launch_posterior(hipStream_t s, const LaunchShape& shape, bool mem, const void* records, int64_t n,
                            const void* wpar, int64_t n_samples, const double* inv, int64_t slice_len, int64_t n_slices,
                            double* part, double* state, int64_t n_prev, int64_t n_total, double* out);
#endif

}  // namespace mcd

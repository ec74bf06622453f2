// mcd_mmatch.h -- moment matching for PSIS-LOO (mcd_moment_match): the algebra of loo_moment_match.default of the R
// package loo (Paananen, Piironen, Buerkner & Vehtari 2021), written once as host+device text with no HIP types, so that
// the kernels of mcd_mmatch.hip, the host loop of mcd_api_mmatch.hip and tests/emul/mmatch_emul.cpp compile the same
// expressions.  Compiled with -ffp-contract=off everywhere.
//
// For a star i whose Pareto k^ is too large, the S posterior draws theta_s (P free parameters, their own units) are moved
// towards the leave-one-out posterior by affine maps theta -> A theta + b.  With w~ the normalised PSIS weights of the
// current rows, mu / v / C their plain mean, variance (S-1) and covariance, mu_w / v_w / C_w the weighted ones:
//   T1 shift            theta + (mu_w - mu)
//   T2 shift and scale  (theta - mu) sqrt(v_w / v) + mu_w,  v_w = sum w~ (theta - mu_w)^2 S / (S - 1); v == 0: scale 1
//   T3 covariance       (theta - mu) M^T + mu_w, M = L_w L^-1; L, L_w the lower Cholesky factors of C and of
//                       C_w = sum w~ (theta - mu_w)(theta - mu_w)^T / (1 - sum w~^2); a factor that fails skips T3
// A trial is accepted when it lowers k^; the star's total map is composed as A <- A_t A, b <- A_t b + b_t, and the rows of
// a star are ALWAYS the total map applied to the original draws (one matrix-vector product per row, whatever the number
// of accepted trials), so that (A, b) and the draws reproduce them.
// The loop of one star (MmState, mm_begin, mm_decide): while k^ > k_threshold and fewer than max_iters passes were begun,
// a pass tries T1, T2 [, T3] in this order; the first accepted trial ends the pass and the next one starts with T1; a pass
// without an accepted trial ends the loop.  `iterations` counts the passes begun, accepted[l] the trials accepted per
// level, so that sum(accepted) is iterations or iterations - 1.
#pragma once

#include <cstdint>
#include <vector>

#include "mcd_math.h"
#include "mcd_prior.h"

namespace mcd {

constexpr int kMmMaxDim = 12;                     // P of one call
constexpr int64_t kMmMaxRows = 65536;             // S of one call; stars run in groups of floor(kMmMaxRows / S)

// Levels of one launch, per star
enum MmLevel : int32_t { MM_KEEP = -1, MM_BASE = 0, MM_SHIFT = 1, MM_SCALE = 2, MM_COV = 3, MM_SPLIT_FWD = 4, MM_SPLIT_INV = 5 };
// What the weight kernel leaves per star: stat[MS_*]
enum MmStat : int { MS_K = 0, MS_ELPD = 1, MS_A1 = 2, MS_A2 = 3, MS_FIELDS = 4 };
// Layout of one star's moments: mu [P], mu_w [P], v_w [P], C [P][P], C_w [P][P]
MCD_HD constexpr int mm_moment_doubles(int P) { return 3 * P + 2 * P * P; }
// ... and of one affine map: A [P][P] row-major, b [P]
MCD_HD constexpr int mm_map_doubles(int P) { return P * P + P; }

MCD_HD void mm_identity(int P, double* A, double* b) {
    for (int r = 0; r < P; ++r) {
        for (int c = 0; c < P; ++c) A[r * P + c] = r == c ? 1.0 : 0.0;
        b[r] = 0.0;
    }
}

// y = A x + b, each row's sum in ascending column order from b
MCD_HD void mm_apply(int P, const double* A, const double* b, const double* x, double* y) {
    for (int r = 0; r < P; ++r) {
        double a = 0.0;
        for (int c = 0; c < P; ++c) a += A[r * P + c] * x[c];
        y[r] = a + b[r];
    }
}

// (A2, b2) = (At A, At b + bt); A2 / b2 must not alias the inputs
MCD_HD void mm_compose(int P, const double* At, const double* bt, const double* A, const double* b, double* A2, double* b2) {
    for (int r = 0; r < P; ++r) {
        for (int c = 0; c < P; ++c) {
            double a = 0.0;
            for (int j = 0; j < P; ++j) a += At[r * P + j] * A[j * P + c];
            A2[r * P + c] = a;
        }
        double a = 0.0;
        for (int j = 0; j < P; ++j) a += At[r * P + j] * b[j];
        b2[r] = a + bt[r];
    }
}

// Weighted variance and covariance from the centred weighted sums s = sum w~ d d^T, d = theta - mu_w
MCD_HD double mm_var_w(double s_cc, int64_t S) { return s_cc * ((double)S / (double)(S - 1)); }
MCD_HD double mm_cov_w(double s_rc, double sum_w2) { return s_rc / (1.0 - sum_w2); }

// One star's moments (layout: mm_moment_doubles) of rows [S][P] under the un-normalised weights w [S]: the two passes of
// mm_moment_kernel (means, then centred second moments) in plain sample order -- the device adds per lane and then over
// the wave, so the two agree to rounding, not bit for bit.
inline void mm_moments(int P, int64_t S, const double* rows, const double* w, double* mom) {
    double a1 = 0.0, a2 = 0.0;
    for (int64_t s = 0; s < S; ++s) { a1 += w[s]; a2 += w[s] * w[s]; }
    const double sum_w2 = a2 / (a1 * a1);
    double* mu = mom;
    double* mu_w = mom + P;
    for (int c = 0; c < P; ++c) {
        double m = 0.0, mw = 0.0;
        for (int64_t s = 0; s < S; ++s) { m += rows[s * P + c]; mw += w[s] * rows[s * P + c]; }
        mu[c] = m / (double)S;
        mu_w[c] = mw / a1;
    }
    for (int j = 0; j < P; ++j)
        for (int c = j; c < P; ++c) {
            double cs = 0.0, cw = 0.0;
            for (int64_t s = 0; s < S; ++s) {
                const double xj = rows[s * P + j], x = rows[s * P + c];
                cs += (x - mu[c]) * (xj - mu[j]);
                cw += (x - mu_w[c]) * (w[s] * (xj - mu_w[j]));
            }
            const double a = cs / (double)(S - 1), sw = cw / a1;
            mom[3 * P + c * P + j] = mom[3 * P + j * P + c] = a;
            mom[3 * P + P * P + c * P + j] = mom[3 * P + P * P + j * P + c] = mm_cov_w(sw, sum_w2);
            if (c == j) mom[2 * P + c] = mm_var_w(sw, S);
        }
}

// T1
MCD_HD void mm_trial_shift(int P, const double* mu, const double* mu_w, double* At, double* bt) {
    mm_identity(P, At, bt);
    for (int c = 0; c < P; ++c) bt[c] = mu_w[c] - mu[c];
}

// T2: v = diag C.  A column whose sample variance is 0 (or whose ratio is not a finite positive number) keeps scale 1
MCD_HD void mm_trial_scale(int P, const double* mu, const double* mu_w, const double* v_w, const double* C, double* At,
                           double* bt) {
    mm_identity(P, At, bt);
    for (int c = 0; c < P; ++c) {
        const double v = C[c * P + c];
        double s = 1.0;
        if (v > 0.0) {
            const double q = sqrt_(v_w[c] / v);
            if (q > 0.0 && q - q == 0.0) s = q;
        }
        At[c * P + c] = s;
        bt[c] = mu_w[c] - s * mu[c];
    }
}

// Lower Cholesky factor of the symmetric a [P][P] (its lower triangle is read) into l (upper triangle zeroed).  false: a
// pivot is not a finite positive number.
MCD_HD bool mm_cholesky(int P, const double* a, double* l) {
    for (int r = 0; r < P; ++r)
        for (int c = 0; c < P; ++c) l[r * P + c] = 0.0;
    for (int j = 0; j < P; ++j) {
        double d = a[j * P + j];
        for (int k = 0; k < j; ++k) d -= l[j * P + k] * l[j * P + k];
        if (!(d > 0.0) || d - d != 0.0) return false;
        const double ljj = sqrt_(d);
        l[j * P + j] = ljj;
        for (int r = j + 1; r < P; ++r) {
            double s = a[r * P + j];
            for (int k = 0; k < j; ++k) s -= l[r * P + k] * l[j * P + k];
            l[r * P + j] = s / ljj;
        }
    }
    return true;
}

// M = L_w L^-1 (both lower triangular, so is M): row by row, M L = L_w solved from the last column down
MCD_HD void mm_chol_map(int P, const double* lw, const double* l, double* m) {
    for (int r = 0; r < P; ++r) {
        for (int c = 0; c < P; ++c) m[r * P + c] = 0.0;
        for (int c = r; c >= 0; --c) {
            double s = lw[r * P + c];
            for (int k = c + 1; k <= r; ++k) s -= m[r * P + k] * l[k * P + c];
            m[r * P + c] = s / l[c * P + c];
        }
    }
}

// T3: At = M, bt = mu_w - M mu.  work: 2 P P doubles.  false: one of the factors failed (the trial is skipped)
MCD_HD bool mm_trial_cov(int P, const double* mu, const double* mu_w, const double* C, const double* C_w, double* At,
                         double* bt, double* work) {
    double* l = work;
    double* lw = work + P * P;
    if (!mm_cholesky(P, C, l) || !mm_cholesky(P, C_w, lw)) return false;
    mm_chol_map(P, lw, l, At);
    for (int r = 0; r < P; ++r) {
        double a = 0.0;
        for (int c = 0; c < P; ++c) a += At[r * P + c] * mu[c];
        bt[r] = mu_w[r] - a;
    }
    return true;
}

// The trial of `level` from one star's moments (mm_moment_doubles).  false: skipped (T3 only)
MCD_HD bool mm_trial(int P, int level, const double* mom, double* At, double* bt, double* work) {
    const double* mu = mom;
    const double* mu_w = mom + P;
    const double* v_w = mom + 2 * P;
    const double* C = mom + 3 * P;
    const double* C_w = C + P * P;
    if (level == MM_SHIFT) { mm_trial_shift(P, mu, mu_w, At, bt); return true; }
    if (level == MM_SCALE) { mm_trial_scale(P, mu, mu_w, v_w, C, At, bt); return true; }
    return mm_trial_cov(P, mu, mu_w, C, C_w, At, bt, work);
}

// (Ai, bi) with Ai (A x + b) + bi = x, and log |det A|: Gauss-Jordan with partial pivoting.  work: 2 P P doubles.
// false: A is singular to working precision (or not finite)
MCD_HD bool mm_inverse(int P, const double* A, const double* b, double* Ai, double* bi, double* log_abs_det, double* work) {
    double* m = work;
    for (int i = 0; i < P * P; ++i) m[i] = A[i];
    mm_identity(P, Ai, bi);
    double lad = 0.0;
    for (int j = 0; j < P; ++j) {
        int piv = j;
        double best = fabs_(m[j * P + j]);
        for (int r = j + 1; r < P; ++r)
            if (fabs_(m[r * P + j]) > best) { best = fabs_(m[r * P + j]); piv = r; }
        if (!(best > 0.0) || best - best != 0.0) return false;
        if (piv != j)
            for (int c = 0; c < P; ++c) {
                double t = m[j * P + c]; m[j * P + c] = m[piv * P + c]; m[piv * P + c] = t;
                t = Ai[j * P + c]; Ai[j * P + c] = Ai[piv * P + c]; Ai[piv * P + c] = t;
            }
        const double d = m[j * P + j];
        lad += log_(fabs_(d));
        for (int c = 0; c < P; ++c) { m[j * P + c] /= d; Ai[j * P + c] /= d; }
        for (int r = 0; r < P; ++r) {
            if (r == j) continue;
            const double f = m[r * P + j];
            if (f == 0.0) continue;
            for (int c = 0; c < P; ++c) { m[r * P + c] -= f * m[j * P + c]; Ai[r * P + c] -= f * Ai[j * P + c]; }
        }
    }
    for (int r = 0; r < P; ++r) {
        double a = 0.0;
        for (int c = 0; c < P; ++c) a += Ai[r * P + c] * b[c];
        bi[r] = -a;
    }
    *log_abs_det = lad;
    return true;
}

// Is the row inside the prior: the inclusive box (a NaN is outside), the support of every structured prior, fixed_ok
MCD_HD bool mm_row_inside(int P, const double* lo, const double* hi, const PriorTable& prior, int32_t fixed_ok, const double* x) {
    bool ok = fixed_ok != 0;
    for (int c = 0; c < P; ++c) ok = ok && x[c] >= lo[c] && x[c] <= hi[c];
    if (ok && prior.any()) ok = prior_row_inside(prior, P, x);
    return ok;
}

// log(exp(a) + exp(b)); -inf when both are
MCD_HD double mm_logaddexp(double a, double b) {
    const double m = a > b ? a : b;
    if (m == -INFINITY) return m;
    return m + log_(exp_(a - m) + exp_(b - m));
}

// Log weights of one row.  Baseline: -l_i.  Trial: train' + lnprior' - lp0, -inf outside the prior.  Split: numerator
// train + lnprior of the half-transformed rows over logaddexp(lp, lp_inv - log|det A|), lp_inv = -inf outside the prior.
MCD_HD double mm_lw_trial(bool inside, double train, double lnprior, double lp0) {
    return inside ? (train + lnprior) - lp0 : -INFINITY;
}
MCD_HD double mm_lw_split(double num, double lp_fwd, bool inv_inside, double lp_inv, double log_abs_det) {
    if (num == -INFINITY) return num;
    return num - mm_logaddexp(lp_fwd, inv_inside ? lp_inv - log_abs_det : -INFINITY);
}

// ---- the decision loop of one star ------------------------------------------------------------------------------------
struct MmState {
    double k = 0.0;               // current k^
    int32_t level = MM_SHIFT;     // the trial to make next
    int32_t iterations = 0;       // passes begun
    int32_t accepted[3] = {0, 0, 0};
    int32_t running = 0;
};

// The highest level of a call
MCD_HD int mm_max_level(int cov, int64_t S, int P) { return cov && S > (int64_t)10 * P ? MM_COV : MM_SCALE; }

MCD_HD void mm_begin(MmState& s, double k0, double k_threshold, int max_iters) {
    s.k = k0;
    s.level = MM_SHIFT;
    s.running = (k0 > k_threshold && max_iters > 0) ? 1 : 0;
    s.iterations = s.running;
}

// After the trial of s.level gave k_trial (usable: the trial could be made and left a row inside the prior): accept it?
MCD_HD bool mm_decide(MmState& s, double k_trial, bool usable, double k_threshold, int max_iters, int max_level) {
    const bool accept = usable && k_trial < s.k;
    if (accept) {
        s.k = k_trial;
        ++s.accepted[s.level - 1];
        s.level = MM_SHIFT;
        if (s.k > k_threshold && s.iterations < max_iters) ++s.iterations;
        else s.running = 0;
    } else if (++s.level > max_level) {
        s.running = 0;
    }
    return accept;
}

// ---- host only: the star ranges of one group --------------------------------------------------------------------------
// stars [g] ascending and distinct within [0, n_stars): the range offsets of plan_chunks (remainders before, between and
// after the singleton ranges, no empty range) and each star's own range
inline std::vector<int64_t> mm_ranges(int64_t n_stars, const int64_t* stars, int64_t g, std::vector<int64_t>& star_range) {
    std::vector<int64_t> r{0};
    star_range.assign((size_t)g, 0);
    for (int64_t e = 0; e < g; ++e) {
        if (stars[e] > r.back()) r.push_back(stars[e]);
        star_range[(size_t)e] = (int64_t)r.size() - 1;
        r.push_back(stars[e] + 1);
    }
    if (r.back() < n_stars) r.push_back(n_stars);
    return r;
}

inline const char* mm_stars_error(int64_t n_match, const int64_t* stars, int64_t n_stars) {
    if (n_match < 1) return "n_match must be >= 1";
    if (!stars) return "stars must not be NULL";
    for (int64_t e = 0; e < n_match; ++e) {
        if (stars[e] < 0 || stars[e] >= n_stars) return "a star index lies outside the catalogue";
        if (e && stars[e] <= stars[e - 1]) return "star indices must be ascending and distinct";
    }
    return nullptr;
}

#if defined(__HIPCC__)
// mcd_mmatch.hip.  Device pointers of one group of G stars with S rows each; buffers with a leading [2] are indexed by
// sel[e] (the star's current state) and 1 - sel[e] (what a launch writes).
struct MmDevice {
    int32_t P = 0, K = 0, fixed_ok = 1;
    int64_t S = 0, M = 0, G = 0;
    const double* draws = nullptr;          // [S][P]
    const int32_t* col_source = nullptr;    // [K]
    const double* col_const = nullptr;      // [K]
    const double* col_factor = nullptr;     // [K]
    const double* lo = nullptr;             // [P]
    const double* hi = nullptr;             // [P]
    PriorTable prior;
    const int32_t* level = nullptr;         // [G] MmLevel of this launch
    const int32_t* sel = nullptr;           // [G]
    double* rows = nullptr;                 // [2][G][S][P]
    double* wts = nullptr;                  // [2][G][S] un-normalised weights e_s (their sum is stat[MS_A1])
    double* li = nullptr;                   // [2][G][S] the star's own term at the rows
    double* stat = nullptr;                 // [2][G][MS_FIELDS]
    double* maps = nullptr;                 // [2][G][mm_map_doubles]
    const double* inv = nullptr;            // [G][mm_map_doubles] inverse of the total map (split step)
    const double* logdet = nullptr;         // [G]
    double* mom = nullptr;                  // [G][mm_moment_doubles]
    int32_t* inside = nullptr;              // [G][S]
    double* lnprior = nullptr;              // [G][S]
    double* lp0 = nullptr;                  // [G][S]
    double* lw = nullptr;                   // [G][S]
    double* num = nullptr;                  // [G][S] split: numerator
    double* lpf = nullptr;                  // [G][S] split: lp of the half-transformed rows
    int32_t* flags = nullptr;               // [G][2]: T3 skipped, rows outside the prior
    double* table = nullptr;                // [G][S][K] the kernel rows of the hold-out launch
    const double* out = nullptr;            // [2][G S] train, test of that launch
};
hipError_t launch_mm_moments(hipStream_t s, const MmDevice& d);
hipError_t launch_mm_transform(hipStream_t s, const MmDevice& d);
hipError_t launch_mm_weights(hipStream_t s, const MmDevice& d);
#endif

}  // namespace mcd

// mcd_simulated.h -- lock-step fits of simulated catalogues (mcd_simulate, mcd_simulated_set, mcd_simulated_loglike):
// every parameter row sees the catalogue with the velocities of its own simulation.  Positions and verr stay the observed
// ones; only the velocity column is replaced, by a table [n_stars][n_sims] that is drawn once from the model at one truth
// row per simulation (simulated_velocity) or uploaded by the caller.  Nothing of the per-star model is restated: star_d_n,
// gauss_lnl and mixture_lnl of mcd_math.h, rep_normal and rep_uniform of mcd_replicate.h.  Host+device text with no HIP
// types, so that tests/emul compiles the same expressions.
//
// The stream is mcd_replicate.h's own: simulation s at truth theta is the replicate of sample row s at theta that
// mcd_replicate_check draws, so mcd_replicate_numbers replays its numbers on the host bit for bit.  A velocity is a
// function of (seed, s, i, truth row) alone: the number of simulations of a call, the chunk plan and the launch shape never
// change it.
#pragma once

#include "mcd_holdout.h"
#include "mcd_replicate.h"

namespace mcd {

constexpr int64_t kSimulatedMaxRows = 65536;                     // parameter rows of one mcd_simulated_loglike
constexpr int64_t kSimulatedPassSims = 65536;                    // simulations drawn by one launch of mcd_simulate
constexpr int64_t kSimulatedMaxBytes = (int64_t)1 << 30;         // the resident table, n_sims x n_stars x 8 bytes

// The velocity of star i (index in catalogue order) in simulation s, drawn at the truth row whose constants are w:
//   (d*, n*) = star_d_n(r, w)                    g = rep_normal(seed, s, i)       u = rep_uniform(seed, s, i)
//   cluster star (no background, or u < m*):     v' = (v_i - d*) + sqrt(n*) g                [v_i - d* = v_los*]
//   background star:                             v' = mu_b + sqrt(verr_i^2 + s2_b) g
// m*, (mu_b, s2_b): as replicate_term takes them (the truth's membership prior; the truth's (v_back, sigma_back^2), or
// the call's (bg_mean, bg_sigma^2) for the fixed-background models).
template <int MODEL, bool FREE>
MCD_HD double simulated_velocity(RecPtr<double> r, const WalkerConsts<double>& w, uint64_t seed, int64_t s, int64_t i,
                                 double bg_mean, double bg_sigma2) {
    constexpr int BG = bg_kind(MODEL);
    constexpr int XB = geometry_doubles(MODEL, FREE);
    // the draw is finished before the term is formed: the divergent rejection loop holds no record value
    const double g = rep_normal(seed, s, i);
    double u = 0.0;
    if constexpr (BG != BG_NONE) u = rep_uniform(seed, s, i);
    double d, n;
    star_d_n<MODEL, double, FREE>(r, w, d, n);
    const double vc = (r[0] - d) + sqrt_(n) * g;
    if constexpr (BG == BG_NONE) {
        return vc;
    } else {
        double m, mu, s2;
        if constexpr (BG == BG_FIXED) {
            m = r[XB + 1]; mu = bg_mean; s2 = bg_sigma2;
        } else if constexpr (BG == BG_FIXED_DENSITY) {
            const double rho = r[XB + 2];
            m = rho / (rho + w.fb); mu = bg_mean; s2 = bg_sigma2;
        } else {
            const double rho = r[XB];
            m = rho / (rho + w.fb); mu = w.vb; s2 = w.sb2;
        }
        const double vb = mu + sqrt_(r[1] + s2) * g;
        return u < m ? vc : vb;
    }
}

// The term of one star under the simulated velocity v: holdout_term with v in place of the record's velocity.  With
// v == r[0] the no-background and Gaussian-background families give holdout_term's bits (d + 0.0 is d).  The stored
// lnlike_bg of the fixed-background records belongs to the observed velocity and is not read: their background term is
// the Gaussian (bg_mean, bg_sigma2) at v.
template <int MODEL, bool FREE>
MCD_HD double simulated_term(RecPtr<double> r, const WalkerConsts<double>& w, double v, double bg_mean, double bg_sigma2) {
    constexpr int BG = bg_kind(MODEL);
    constexpr int XB = geometry_doubles(MODEL, FREE);
    double d, n;
    star_d_n<MODEL, double, FREE>(r, w, d, n);
    const double ds = d + (v - r[0]);
    const double lc = gauss_lnl(ds, n);
    if constexpr (BG == BG_NONE) {
        return lc;
    } else {
        double lb, m;
        if constexpr (BG == BG_FIXED) {
            lb = gauss_lnl(v - bg_mean, r[1] + bg_sigma2); m = r[XB + 1];
        } else if constexpr (BG == BG_FIXED_DENSITY) {
            lb = gauss_lnl(v - bg_mean, r[1] + bg_sigma2);
            const double rho = r[XB + 2];
            m = rho / (rho + w.fb);
        } else {
            lb = gauss_lnl(v - w.vb, r[1] + w.sb2);
            const double rho = r[XB];
            m = rho / (rho + w.fb);
        }
        return mixture_lnl(lc, lb, m);
    }
}

// One chunk of stars [star0, star0 + count) for one row: the sum of the terms in star order, from +0.0.  The velocity of
// star i is col[i * stride]: the explicit-weight addressing of chunk_weighted_value (col = table + the row's simulation,
// stride = n_sims).
template <int MODEL, bool FREE>
MCD_HD double chunk_simulated_value(RecPtr<double> r, int64_t star0, int count, const WalkerConsts<double>& w,
                                    const double* __restrict__ col, int64_t stride, double bg_mean, double bg_sigma2) {
    constexpr int ND = record_doubles(MODEL, FREE);
    double acc = 0.0;
    for (int j = 0; j < count; ++j, r += ND)
        acc += simulated_term<MODEL, FREE>(r, w, col[(star0 + j) * stride], bg_mean, bg_sigma2);
    return acc;
}

// ---- host: validation --------------------------------------------------------------------------------------------------
// whether n_sims x n_stars doubles fit the resident table's budget
inline bool simulated_fits_budget(int64_t n_sims, int64_t n_stars) {
    const int64_t cap = kSimulatedMaxBytes / 8;
    return n_sims <= cap && (n_stars <= 0 || n_sims <= cap / n_stars);
}

#if defined(__HIPCC__)
// mcd_simulated.hip.  table: device, [n_stars][n_sims].
//   launch_simulate        draws the simulations sim_begin .. sim_begin + n_rows - 1 of the table (generator rows
//                          sim0 + sim_begin ..) at the truth rows wpar: [n_rows][KD]; bad: [n_chunks][n_rows], the first
//                          star of the chunk whose velocity is not finite, or -1
//   launch_simulate_first  first_bad[row] = the smallest such star over the chunks, or -1
//   launch_simulated_value the partial sum of every (chunk, row) in the layout of the value kernels
//                          (partials: [roundup64(R) / 8][n_chunks][8]), which launch_reduce adds up; row_sim: device, [R]
struct LaunchShape;
struct Chunk;
hipError_t launch_simulate(hipStream_t s, const LaunchShape& shape, const void* records, const Chunk* chunks, int64_t n_chunks,
                           const void* wpar, int64_t n_rows, int64_t sim_begin, int64_t n_sims, int64_t sim0, uint64_t seed,
                           double bg_mean, double bg_sigma2, double* table, int64_t* bad);
hipError_t launch_simulate_first(hipStream_t s, const int64_t* bad, int64_t n_chunks, int64_t n_rows, int64_t* first_bad);
hipError_t launch_simulated_value(hipStream_t s, const LaunchShape& shape, const void* records, const Chunk* chunks,
                                  int64_t n_chunks, const void* wpar, const int64_t* row_sim, const double* table,
                                  int64_t n_sims, double bg_mean, double bg_sigma2, double* partials, int64_t n_rows);
#endif

}  // namespace mcd

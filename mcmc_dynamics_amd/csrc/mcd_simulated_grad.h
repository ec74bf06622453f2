// mcd_simulated_grad.h -- value and gradient of the log-likelihood of simulated catalogues (mcd_simulated_loglike_grad):
// for row r on simulation s = row_sim[r],
//   sum_i l_i(theta_r; v'(s, i))      and      sum_i dl_i/dtheta_k(theta_r; v'(s, i)),
// with l_i the term of mcd_simulated.h (simulated_term: the value is its bits) and the partials those of mcd_grad.h
// (grad_term_at with its SIM flag: nothing of the derivative arithmetic is restated here).  The velocity of star i is read
// from the resident table [n_stars][n_sims] as chunk_simulated_value reads it.  Host+device text with no HIP types, so
// that tests/emul compiles the loop the gfx950 kernel runs.
#pragma once

#include "mcd_grad.h"
#include "mcd_simulated.h"

namespace mcd {

// g[0 .. K) += dl/dtheta_k of one star under the simulated velocity v; returns l, simulated_term's value
template <int MODEL, bool FREE>
MCD_HD double simulated_grad_term(RecPtr<double> r, const WalkerConsts<double>& w, const GradRaw<double>& q, double v,
                                  double bg_mean, double bg_sigma2, double* __restrict__ g) {
    return grad_term_at<MODEL, FREE, double, true>(r, w, q, v, bg_mean, bg_sigma2, g);
}

// One chunk of stars [star0, star0 + count) for one row: acc[0] += l, acc[1 + k] += dl/dtheta_k, in star order.  The
// velocity of star i is col[i * stride] (col = table + the row's simulation, stride = n_sims).
template <int MODEL, bool FREE>
MCD_HD void chunk_simulated_grad(RecPtr<double> r, int64_t star0, int count, const WalkerConsts<double>& w,
                                 const GradRaw<double>& q, const double* __restrict__ col, int64_t stride, double bg_mean,
                                 double bg_sigma2, double* __restrict__ acc) {
    constexpr int ND = record_doubles(MODEL, FREE);
    for (int j = 0; j < count; ++j, r += ND)
        acc[0] += simulated_grad_term<MODEL, FREE>(r, w, q, col[(star0 + j) * stride], bg_mean, bg_sigma2, acc + 1);
}

#if defined(__HIPCC__)
// mcd_simulated_grad.hip: the value and gradient partial sums of every (chunk, row), in the layout of mcd_grad.hip
// (partials: [1 + K][roundup64(R) / 8][n_chunks][8]), which launch_reduce adds up over (1 + K) x padded rows.
// row_sim: device, [R]; table: device, [n_stars][n_sims].
struct LaunchShape;
struct Chunk;
hipError_t launch_simulated_grad(hipStream_t s, const LaunchShape& shape, const void* records, const Chunk* chunks,
                                 int64_t n_chunks, const double* params, const void* wpar, const int64_t* row_sim,
                                 const double* table, int64_t n_sims, double bg_mean, double bg_sigma2, double* partials,
                                 int64_t n_rows);
#endif

}  // namespace mcd

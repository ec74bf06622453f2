// mcd_weighted_value.h -- the log-likelihood under per-row star weights WITHOUT its gradient (mcd_weighted_loglike): for
// row r with replicate b = row_replicate[r],
//   sum_i w(b, i) l_i(theta_r),
// with l_i the plain per-star term of mcd_holdout.h (holdout_term, what mcd_loglike_per_star returns: nothing is restated
// here) and w(b, i) the weight of mcd_weights.h, generated from (seed, b, i) or read from an array, through the WeightRow
// of mcd_weighted.h.  What a weighted chain needs: the gradient loop of mcd_weighted.h carries 1 + K sums and grad_term's
// partials per lane, a stretch move reads one number.  Written once as host+device code so that tests/emul compiles the
// loop the gfx950 kernel runs.
//
// Zero weights are selected out, not multiplied, and a generated weight does not depend on where a chunk starts: the
// rules of mcd_weighted.h (chunk_weighted), the same Philox block redrawn at the same stars.
#pragma once

#include "mcd_holdout.h"
#include "mcd_weighted.h"

namespace mcd {

// One chunk of stars [star0, star0 + count) for one row: the sum of w l in star order, from +0.0
template <int MODEL, bool FREE, int SCHEME>
MCD_HD double chunk_weighted_value(RecPtr<double> r, int64_t star0, int count, const WalkerConsts<double>& w,
                                   const WeightRow& src) {
    constexpr int ND = record_doubles(MODEL, FREE);
    Philox4x64 block = {};
    double acc = 0.0;
    for (int j = 0; j < count; ++j, r += ND) {
        const int64_t star = star0 + j;
        double wt;
        if constexpr (SCHEME == kWeightExplicit) {
            wt = src.col[star * src.stride];
        } else {
            const int word = (int)(star & 3);
            if (j == 0 || word == 0) block = weight_block(src.seed, src.replicate, (uint64_t)star >> 2);
            wt = weight_of_word<SCHEME>(weight_word(block, word));
        }
        const double l = holdout_term<MODEL, FREE, double>(r, w);
        acc += (wt != 0.0) ? wt * l : 0.0;
    }
    return acc;
}

#if defined(__HIPCC__)
// mcd_weighted_value.hip: the weighted value's partial sum of every (chunk, row), in the layout of the value kernels
// (partials: [roundup64(R) / 8][n_chunks][8]), which launch_reduce adds up.  row_replicate: device, [R]; weights: device,
// [n_stars][n_replicates] for kWeightExplicit, else unused.
struct LaunchShape;
struct Chunk;
hipError_t launch_weighted_value(hipStream_t s, const LaunchShape& shape, int scheme, const void* records, const Chunk* chunks,
                                 int64_t n_chunks, const void* wpar, const int64_t* row_replicate, uint64_t seed,
                                 const double* weights, int64_t n_replicates, double* partials, int64_t n_rows);
#endif

}  // namespace mcd

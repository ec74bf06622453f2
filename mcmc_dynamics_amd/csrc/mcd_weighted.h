// mcd_weighted.h -- value and gradient of the log-likelihood under per-row star weights (mcd_weighted_loglike_grad): for
// row r with replicate b = row_replicate[r],
//   sum_i w(b, i) l_i(theta_r)      and      sum_i w(b, i) dl_i/dtheta_k(theta_r),
// with l_i and its partials the term of mcd_grad.h (grad_term, the same expressions: nothing is restated here) and
// w(b, i) generated from (seed, b, i) (mcd_weights.h) or read from an array.  Written once as host+device code so that
// tests/emul compiles the loop the gfx950 kernel runs.
//
// Zero weights are selected out, not multiplied: a star with w == 0 adds exactly +0.0 to every field, whatever its term
// is -- 0 x (-inf) is never formed.  Poisson weights on catalogues with certain non-members are safe that way, and 0 / 1
// explicit weights reproduce a sum over the kept stars.
//
// A generated weight does not depend on where a chunk starts: a chunk that begins at star % 4 != 0 draws the block of
// star >> 2 and uses the word of star & 3.
#pragma once

#include "mcd_grad.h"
#include "mcd_weights.h"

namespace mcd {

constexpr int64_t kWeightedMaxRows = 65536;
constexpr int64_t kWeightedMaxExplicitBytes = (int64_t)256 << 20;

// Where one row's weights come from.  Generated: (seed, replicate).  Explicit: column `replicate` of the array
// [star][n_replicates] (the transpose of the caller's: the rows of a wave load adjacent doubles), col = base + replicate.
struct WeightRow {
    uint64_t seed = 0, replicate = 0;
    const double* col = nullptr;
    int64_t stride = 0;
};

// One chunk of stars [star0, star0 + count) for one row: acc[0] += sum of w l, acc[1 + k] += sum of w dl/dtheta_k, in
// star order.
template <int MODEL, bool FREE, int SCHEME>
MCD_HD void chunk_weighted(RecPtr<double> r, int64_t star0, int count, const WalkerConsts<double>& w,
                           const GradRaw<double>& q, const WeightRow& src, double* __restrict__ acc) {
    constexpr int ND = record_doubles(MODEL, FREE);
    constexpr int K = grad_columns(MODEL, FREE);
    Philox4x64 block = {};
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
        // the term on its own (-0.0 + x is x for every x, so these are grad_term's bits) ...
        double g[K];
#pragma unroll
        for (int k = 0; k < K; ++k) g[k] = -0.0;
        const double l = grad_term<MODEL, FREE, double>(r, w, q, g);
        // ... and selected in, never multiplied by a zero
        const bool in = wt != 0.0;
        acc[0] += in ? wt * l : 0.0;
#pragma unroll
        for (int k = 0; k < K; ++k) acc[1 + k] += in ? wt * g[k] : 0.0;
    }
}

#if defined(__HIPCC__)
// mcd_weighted.hip: the weighted value and gradient partial sums of every (chunk, row), in the layout of mcd_grad.hip
// (partials: [1 + K][roundup64(R) / 8][n_chunks][8]), which launch_grad_reduce adds up.  row_replicate: device, [R];
// weights: device, [n_stars][n_replicates] for kWeightExplicit, else unused.
struct LaunchShape;
struct Chunk;
hipError_t launch_weighted_grad(hipStream_t s, const LaunchShape& shape, int scheme, const void* records, const Chunk* chunks,
                                int64_t n_chunks, const double* params, const void* wpar, const int64_t* row_replicate,
                                uint64_t seed, const double* weights, int64_t n_replicates, double* partials,
                                int64_t n_rows);
#endif

}  // namespace mcd

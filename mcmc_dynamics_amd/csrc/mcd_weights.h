// mcd_weights.h -- the star weights of the weighted-likelihood bootstrap (mcd_weighted_loglike_grad), the same code on the
// device (mcd_weighted.hip draws them inside the gradient loop: no replicates x stars array exists anywhere) and on the host
// (mcd_bootstrap_weights, the CPU test harness tests/emul), so that a weight is a function of (scheme, seed, replicate,
// star) alone and can be replayed anywhere.
//
//   * generator: ONE philox4x64_10 call (mcd_rng.h) serves four stars: counter (star >> 2, replicate, 0, 0), key
//     (seed, kWeightKey1); the star's word is v[star & 3].  `star` is the index in catalogue order within the process
//     (the order of `records`, the index mcd_replicate_check uses), never a position in the verr-sorted copy.
//   * uniform: u = ((word >> 11) + 0.5) 2^-53.  The half keeps u away from 0, so the logarithm below is finite.  (In
//     float64 the sum rounds to even above 2^52; the one word value in 2^53 whose u rounds to 1.0 gives the exponential
//     weight 0, which the kernel selects out like any weight 0.)
//   * kWeightExponential: w = -det_log(u), Exp(1) -- Rubin's Bayesian bootstrap in the unnormalised form of Newton & Raftery
//     (1994).  det_log is a fixed sequence of IEEE operations, so host and device give the same bits (-ffp-contract=off).
//   * kWeightPoisson: w = the number of thresholds C_j <= u, C_j = e^-1 sum_{m <= j} 1 / m! the cumulative Poisson(1)
//     probabilities: the counts of the nonparametric bootstrap in its Poisson form, an exact small integer.
//
// The weights are NOT normalised: their sum over the stars is n_stars only in expectation (relative spread
// 1 / sqrt(n_stars)).  That is the weighted-likelihood bootstrap as published; a structured prior enters unweighted.
#pragma once

#include <cstdint>

#include "mcd_rng.h"

namespace mcd {

constexpr uint64_t kWeightKey1 = 0x6d63645f776768ull;         // "mcd_wgh"
constexpr int kWeightExponential = 0, kWeightPoisson = 1, kWeightExplicit = 2;   // include/mcd.h: MCD_WEIGHT_*

// cumulative Poisson(1) probabilities, correctly rounded; the last one is the first that equals 1.0 in float64.  HEAD: the
// five every draw is compared with; GATE: the sixth, which 5.9e-4 of the draws reach; TAIL: the thirteen behind it.
constexpr int kPoissonThresholds = 19;
#define MCD_POISSON_HEAD(X)                                                                                          \
    X(0.36787944117144233) X(0.7357588823428847) X(0.9196986029286058) X(0.9810118431238462) X(0.9963401531726563)
#define MCD_POISSON_GATE 0.9994058151824183
#define MCD_POISSON_TAIL(X)                                                                                          \
    X(0.999916758850712) X(0.9999897508033253) X(0.999998874797402) X(0.9999998885745217) X(0.9999999899522336)     \
    X(0.9999999991683892) X(0.9999999999364022) X(0.9999999999954802) X(0.9999999999997) X(0.9999999999999813)      \
    X(0.9999999999999989) X(0.9999999999999999) X(1.0)
#define MCD_POISSON_CUMULATIVE(X) MCD_POISSON_HEAD(X) X(MCD_POISSON_GATE) MCD_POISSON_TAIL(X)

MCD_HD double weight_uniform(uint64_t word) { return ((double)(word >> 11) + 0.5) * (1.0 / 9007199254740992.0); }

// The count of thresholds <= u.  The head is a chain of compares on literals; the tail sits behind a branch that a wave
// takes for 3.7 % of its stars and reads a constant table in a rolled loop: with all nineteen literals in the loop body
// the mixture families ran out of scalar registers (16 - 28 scalars parked in vector lanes and up to 40 more
// VGPRs, against 3 - 11 and none this way).
MCD_HD double poisson_count(double u) {
    double w = 0.0;
#define MCD_POISSON_STEP(C) w += u >= C ? 1.0 : 0.0;
    MCD_POISSON_HEAD(MCD_POISSON_STEP)
#undef MCD_POISSON_STEP
    if (__builtin_expect(u >= MCD_POISSON_GATE, 0)) {
        w += 1.0;
#define MCD_POISSON_ITEM(C) C,
        const double tail[13] = {MCD_POISSON_TAIL(MCD_POISSON_ITEM)};
#undef MCD_POISSON_ITEM
#pragma unroll 1
        for (int j = 0; j < 13; ++j) w += u >= tail[j] ? 1.0 : 0.0;
    }
    return w;
}

template <int SCHEME>
MCD_HD double weight_of_word(uint64_t word) {
    static_assert(SCHEME == kWeightExponential || SCHEME == kWeightPoisson, "a generated scheme");
    const double u = weight_uniform(word);
    if constexpr (SCHEME == kWeightExponential) return -det_log(u);
    else return poisson_count(u);
}

// the four words of the stars 4 block .. 4 block + 3 of a replicate
MCD_HD Philox4x64 weight_block(uint64_t seed, uint64_t replicate, uint64_t block) {
    return philox4x64_10(block, replicate, 0, 0, seed, kWeightKey1);
}

// word `k` (0 .. 3) of a block by selection: an index that is not a compile-time constant would put the block in memory
MCD_HD uint64_t weight_word(const Philox4x64& b, int k) {
    return k == 0 ? b.v[0] : k == 1 ? b.v[1] : k == 2 ? b.v[2] : b.v[3];
}

// scheme: kWeightExponential or kWeightPoisson (anything else: NaN)
MCD_HD double bootstrap_weight(int scheme, uint64_t seed, int64_t replicate, int64_t star) {
    const Philox4x64 b = weight_block(seed, (uint64_t)replicate, (uint64_t)star >> 2);
    const uint64_t word = weight_word(b, (int)(star & 3));
    if (scheme == kWeightExponential) return weight_of_word<kWeightExponential>(word);
    if (scheme == kWeightPoisson) return weight_of_word<kWeightPoisson>(word);
    return __builtin_nan("");
}

}  // namespace mcd

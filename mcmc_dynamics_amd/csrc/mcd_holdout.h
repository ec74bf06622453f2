// mcd_holdout.h -- exact leave-out refits (mcd_holdout_loglike): E ensembles that each leave out their own small set of
// stars share ONE evaluation of the whole catalogue.  Host+device text with no HIP types, so that tests/emul compiles the
// same validation, range table and combine rule.
//
//   hold-out sets    set_offsets[E + 1], non-decreasing, set_offsets[0] = 0, set_offsets[E] <= n_stars: set e is the
//                    stars [set_offsets[e], set_offsets[e + 1]) in catalogue order (the caller permutes the stars so that
//                    the sets are such prefixes); stars from set_offsets[E] on belong to no set.  A set may be empty.
//   ranges           set 0 .. set E - 1 [, remainder]: what plan_chunks (mcd_chunks.h) takes as its bin_offsets, so that
//                    no chunk straddles a set boundary and plan.offsets gives each range's slots
//   rows             e W + w over all E W parameter rows: every row is evaluated against EVERY star, and the partial
//                    sums of a range's chunks are added up apart from the others' (launch_reduce with the ranges as its
//                    parameter sets): M[r][row]
//   combine          test[row] = M[e][row],  train[row] = sum of M[r][row] over r != e in ascending r, from +0.0
// No difference of two large sums is formed anywhere: train is a sum of the other ranges' sums.
#pragma once

#include <cstdint>
#include <vector>

#include "mcd_math.h"

namespace mcd {

constexpr int64_t kHoldoutMaxRows = 65536;                       // E W of one call
constexpr int64_t kHoldoutScratchBytes = (int64_t)256 << 20;     // the [R][padded rows] intermediate of the reduction

// What is wrong with the offsets, or null
inline const char* holdout_offsets_error(int64_t n_sets, const int64_t* set_offsets, int64_t n_stars) {
    if (n_sets < 1) return "n_sets must be >= 1";
    if (!set_offsets) return "set_offsets must not be NULL";
    if (set_offsets[0] != 0) return "set_offsets[0] must be 0";
    for (int64_t e = 0; e < n_sets; ++e)
        if (set_offsets[e + 1] < set_offsets[e]) return "set_offsets must be non-decreasing";
    if (set_offsets[n_sets] > n_stars) return "set_offsets[n_sets] exceeds the catalogue's stars";
    return nullptr;
}

// [R + 1] range offsets: the sets, and the remainder where set_offsets[E] < n_stars (R = E + 1), else R = E
inline std::vector<int64_t> holdout_ranges(int64_t n_sets, const int64_t* set_offsets, int64_t n_stars) {
    std::vector<int64_t> r(set_offsets, set_offsets + n_sets + 1);
    if (r.back() < n_stars) r.push_back(n_stars);
    return r;
}

// m: [n_ranges][n_rows] range sums; row belongs to set e
MCD_HD void holdout_combine(const double* __restrict__ m, int64_t n_ranges, int64_t n_rows, int64_t row, int64_t e,
                            double& train, double& test) {
    double t = 0.0;
    for (int64_t r = 0; r < n_ranges; ++r)
        if (r != e) t += m[r * n_rows + row];
    train = t;
    test = m[e * n_rows + row];
}

// the plain per-star term l_i (what mcd_loglike_per_star returns; the value of grad_term)
template <int MODEL, bool FREE, class T = double>
MCD_HD T holdout_term(RecPtr<T> r, const WalkerConsts<T>& w) {
    T lc, lb, m;
    star_components<MODEL, FREE, T>(r, w, lc, lb, m);
    if constexpr (bg_kind(MODEL) == BG_NONE) return lc;
    else return mixture_lnl(lc, lb, m);
}

// One chunk of stars for one row: acc += l_i in star order
template <int MODEL, bool FREE, class T = double>
MCD_HD T chunk_holdout(RecPtr<T> r, int count, const WalkerConsts<T>& w) {
    constexpr int ND = record_doubles(MODEL, FREE);
    T acc = T(0);
    for (int j = 0; j < count; ++j, r += ND) acc += holdout_term<MODEL, FREE, T>(r, w);
    return acc;
}

#if defined(__HIPCC__)
// mcd_holdout.hip.  set_range (device, [rows / n_walkers], or null: set e is range e): each set's range.  partials: [roundup64(rows) / 8][n_chunks][8]; range_sums: [n_ranges][rows]; out: [2][rows] = train, test
struct LaunchShape;
struct Chunk;
hipError_t launch_holdout(hipStream_t s, const LaunchShape& shape, const void* records, const Chunk* chunks, int64_t n_chunks,
                          const void* wpar, double* partials, int64_t n_rows);
hipError_t launch_holdout_reduce(hipStream_t s, const double* partials, int64_t n_chunks, const int64_t* range_slot_offsets,
                                 int64_t n_ranges, int64_t max_chunks_per_range, int64_t n_rows, int64_t n_walkers,
                                 double* range_sums, double* out, const int64_t* set_range = nullptr);
#endif

}  // namespace mcd

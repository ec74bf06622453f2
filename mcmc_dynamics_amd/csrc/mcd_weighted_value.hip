// mcd_weighted_value.hip -- gfx950 kernel of mcd_weighted_loglike: the log-likelihood per parameter row, every row under
// the star weights of its own replicate, without the gradient (mcd_weighted_value.h holds the loop, mcd_holdout.h the
// per-star term, mcd_weights.h the generator).
//
// Work decomposition: weighted_grad_kernel's (mcd_weighted.hip; mcd_launch.h has the shared mapping and the partial-sum
// address).  lane = row; a wave evaluates 64 rows against one chunk of the chunk table over `records` (catalogue order);
// the record pointer and the star index are wave-uniform, so records arrive by scalar loads.  What differs per lane is the
// weight: the generated schemes draw one Philox block per four stars from (seed, the lane's replicate, star >> 2) in
// registers; the explicit scheme loads weights[star][replicate].  Each lane keeps ONE float64 sum and stores it as
// partials[row / 8][chunk][row % 8], the value kernels' layout, so the value path's fixed-order reduction (launch_reduce)
// adds it up unchanged.  Plain C++, vector stores only, no atomics, no LDS: results are bitwise repeatable.
//
// Workgroup: 256 threads (4 waves, one per SIMD of a CU).  No instantiation uses scratch; DESIGN 3.21 lists the compiler's
// resource usage per family and scheme.
#include "mcd_internal.h"
#include "mcd_dispatch.h"
#include "mcd_weighted_value.h"
#include "mcd_reduce.h"

namespace mcd {

namespace {

template <int MODEL, bool FREE, int SCHEME>
__global__ __launch_bounds__(kBlock) void weighted_value_kernel(const double* __restrict__ recs,
                                                                 const Chunk* __restrict__ chunks,
                                                                 const double* __restrict__ wpar,
                                                                 const int64_t* __restrict__ row_replicate, uint64_t seed,
                                                                 const double* __restrict__ weights, int64_t n_replicates,
                                                                 double* __restrict__ partials, int64_t n_tasks,
                                                                 int n_wtiles, int64_t n_rows, int64_t n_chunks) {
    constexpr int ND = record_doubles(MODEL, FREE);
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int lane = threadIdx.x & (kWave - 1);
    int64_t chunk_id;
    int wtile;
    if (!wave_task(wave, n_tasks, n_wtiles, n_chunks, chunk_id, wtile)) return;
    const Chunk ch = chunks[chunk_id];                                       // scalar load
    const int64_t w_raw = (int64_t)wtile * kWave + lane;
    const int64_t row = w_raw < n_rows ? w_raw : n_rows - 1;                 // idle lanes shadow the last row
    WalkerConsts<double> w;
    w.load(wpar + row * KD);
    WeightRow src;
    src.seed = seed;
    src.replicate = (uint64_t)row_replicate[row];
    if constexpr (SCHEME == kWeightExplicit) {
        src.col = weights + row_replicate[row];                              // (the host has checked 0 <= replicate < n_replicates)
        src.stride = n_replicates;
    }
    const double acc =
        chunk_weighted_value<MODEL, FREE, SCHEME>((RecPtr<double>)(recs + ch.begin * ND), ch.begin, ch.count, w, src);
    // rows are padded to whole tiles: idle lanes store their shadow sum into padding
    partials[partial_index(w_raw, n_chunks, chunk_id)] = acc;
}

template <int MODEL, bool FREE, int SCHEME>
hipError_t launch_weighted_value_main(hipStream_t s, const void* records, const Chunk* chunks, int64_t n_chunks,
                                      const void* wpar, const int64_t* row_replicate, uint64_t seed, const double* weights,
                                      int64_t n_replicates, double* partials, int64_t n_rows) {
    const int n_wtiles = (int)((n_rows + kWave - 1) / kWave);
    const int64_t grid = main_grid(n_chunks, n_rows);
    if (grid <= 0) return hipSuccess;
    hipLaunchKernelGGL((weighted_value_kernel<MODEL, FREE, SCHEME>), dim3((unsigned)grid), dim3(kBlock), 0, s,
                       (const double*)records, chunks, (const double*)wpar, row_replicate, seed, weights, n_replicates, partials,
                       n_chunks * n_wtiles, n_wtiles, n_rows, n_chunks);
    return hipGetLastError();
}

}  // namespace

hipError_t launch_weighted_value(hipStream_t s, const LaunchShape& sh, int scheme, const void* records, const Chunk* chunks,
                                 int64_t n_chunks, const void* wpar, const int64_t* row_replicate, uint64_t seed,
                                 const double* weights, int64_t n_replicates, double* partials, int64_t n_rows) {
    if (sh.precision != 0 || n_rows <= 0 || !row_replicate) return hipErrorInvalidValue;
    if (scheme == kWeightExplicit && (!weights || n_replicates <= 0)) return hipErrorInvalidValue;
    return dispatch_launch_model(sh.model, sh.free_centre, [&](auto M, auto FREE) {
        constexpr int MODEL = decltype(M)::value;
        constexpr bool kFree = decltype(FREE)::value;
        switch (scheme) {
        case kWeightExponential:
            return launch_weighted_value_main<MODEL, kFree, kWeightExponential>(s, records, chunks, n_chunks, wpar, row_replicate,
                                                                                seed, weights, n_replicates, partials, n_rows);
        case kWeightPoisson:
            return launch_weighted_value_main<MODEL, kFree, kWeightPoisson>(s, records, chunks, n_chunks, wpar, row_replicate,
                                                                            seed, weights, n_replicates, partials, n_rows);
        case kWeightExplicit:
            return launch_weighted_value_main<MODEL, kFree, kWeightExplicit>(s, records, chunks, n_chunks, wpar, row_replicate,
                                                                             seed, weights, n_replicates, partials, n_rows);
        }
        return hipErrorInvalidValue;
    }, hipErrorInvalidValue);
}

}  // namespace mcd

// mcd_holdout.hip -- gfx950 kernels of mcd_holdout_loglike: the plain terms of every star for E W parameter rows, kept
// apart per star range (mcd_holdout.h holds the ranges and the combine rule).
//
// Work decomposition: the gradient kernel's (mcd_grad.hip; mcd_launch.h has the shared mapping and the partial-sum
// address).  lane = row; a wave evaluates 64 rows against one chunk of the range plan's chunk table; the record pointer is
// wave-uniform, so records arrive by scalar loads and are SGPR operands of the f64 vector ops.  The row of a lane is
// e W + w over all E W rows and does not depend on the chunk (Chunk::pset, the chunk's RANGE, is not read here: it only
// decides where the reduction puts the chunk's sum).  Each lane keeps one float64 sum over its chunk and stores it as
// partials[row / 8][chunk][row % 8], the value kernel's layout, so the value path's fixed-order reduction (launch_reduce)
// adds up each range's slots unchanged.  No atomics, no LDS: results are bitwise repeatable.
//
// Workgroup: 256 threads (4 waves, one per SIMD of a CU).  No instantiation uses scratch; DESIGN 3.16 lists the
// compiler's resource usage per family.
#include "mcd_internal.h"
#include "mcd_dispatch.h"
#include "mcd_holdout.h"
#include "mcd_reduce.h"

namespace mcd {

namespace {

template <int MODEL, bool FREE>
__global__ __launch_bounds__(kBlock) void holdout_kernel(const double* __restrict__ recs, const Chunk* __restrict__ chunks,
                                                          const double* __restrict__ wpar, double* __restrict__ partials,
                                                          int64_t n_tasks, int n_wtiles, int64_t n_rows, int64_t n_chunks) {
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
    const double acc = chunk_holdout<MODEL, FREE, double>((RecPtr<double>)(recs + ch.begin * ND), ch.count, w);
    // rows are padded to whole tiles: idle lanes store their shadow sum into padding
    partials[partial_index(w_raw, n_chunks, chunk_id)] = acc;
}

// One thread per row: mcd_holdout.h: holdout_combine on the range sums.  out: [2][n_rows] = train, test.  set_range
// (null: set e is range e): the range of every set, for sets that are not the first ranges of the plan
__global__ __launch_bounds__(kBlock) void holdout_combine_kernel(const double* __restrict__ range_sums, int64_t n_ranges,
                                                                  int64_t n_rows, int64_t n_walkers,
                                                                  const int64_t* __restrict__ set_range,
                                                                  double* __restrict__ out) {
    const int64_t row = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (row >= n_rows) return;
    double train, test;
    const int64_t e = row / n_walkers;
    holdout_combine(range_sums, n_ranges, n_rows, row, set_range ? set_range[e] : e, train, test);
    out[row] = train;
    out[n_rows + row] = test;
}

template <int MODEL, bool FREE>
hipError_t launch_holdout_main(hipStream_t s, const void* records, const Chunk* chunks, int64_t n_chunks, const void* wpar,
                               double* partials, int64_t n_rows) {
    const int n_wtiles = (int)((n_rows + kWave - 1) / kWave);
    const int64_t grid = main_grid(n_chunks, n_rows);
    if (grid <= 0) return hipSuccess;
    hipLaunchKernelGGL((holdout_kernel<MODEL, FREE>), dim3((unsigned)grid), dim3(kBlock), 0, s, (const double*)records, chunks,
                       (const double*)wpar, partials, n_chunks * n_wtiles, n_wtiles, n_rows, n_chunks);
    return hipGetLastError();
}

}  // namespace

hipError_t launch_holdout(hipStream_t s, const LaunchShape& sh, const void* records, const Chunk* chunks, int64_t n_chunks,
                          const void* wpar, double* partials, int64_t n_rows) {
    if (sh.precision != 0 || n_rows <= 0) return hipErrorInvalidValue;
    return dispatch_launch_model(sh.model, sh.free_centre, [&](auto M, auto FREE) {
        return launch_holdout_main<decltype(M)::value, decltype(FREE)::value>(s, records, chunks, n_chunks, wpar, partials,
                                                                              n_rows);
    }, hipErrorInvalidValue);
}

// The value path's reduction with the ranges as its parameter sets (a range without chunks adds nothing to +0.0 and
// comes out as +0.0: reduce_group_kernel loads no slot), then the combine kernel.
hipError_t launch_holdout_reduce(hipStream_t s, const double* partials, int64_t n_chunks, const int64_t* range_slot_offsets,
                                 int64_t n_ranges, int64_t max_chunks_per_range, int64_t n_rows, int64_t n_walkers,
                                 double* range_sums, double* out, const int64_t* set_range) {
    if (n_rows <= 0 || n_ranges <= 0 || n_walkers <= 0) return hipErrorInvalidValue;
    const hipError_t e = launch_reduce(s, partials, range_slot_offsets, n_ranges, n_chunks,
                                       n_ranges == 1 ? n_chunks : max_chunks_per_range, n_rows, nullptr, range_sums);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(holdout_combine_kernel, dim3((unsigned)((n_rows + kBlock - 1) / kBlock)), dim3(kBlock), 0, s,
                       range_sums, n_ranges, n_rows, n_walkers, set_range, out);
    return hipGetLastError();
}

}  // namespace mcd

// mcd_replicate.hip -- gfx950 kernels of mcd_replicate_check: the replicated-data fields of every sample row, kept apart
// per range of stars (mcd_replicate.h holds the term, the generator and the plan).
//
// Work decomposition: the hold-out kernel's (mcd_holdout.hip; mcd_launch.h has the shared mapping).  lane = sample row; a
// wave evaluates 64 rows against one chunk of the range plan's chunk table.  A chunk is a run of the index array `order`
// (the stars of range 0, then of range 1, ...): the index and the record pointer made from it are wave-uniform, so both
// arrive by scalar loads from the constant address space and the catalogue is never re-ordered or re-uploaded.  The star
// index is also the generator's counter word, so a replicate does not depend on where the star sits.  Each lane keeps its
// 16 sums over the chunk and stores them with plain vector stores as partials[chunk][field][row]; the reduction combines
// a range's chunks in ascending order.  No atomics, no LDS: results are bitwise repeatable.
//
// Workgroup: 256 threads (4 waves, one per SIMD of a CU).  No instantiation uses scratch; DESIGN 3.18 lists the
// compiler's resource usage.
#include "mcd_internal.h"
#include "mcd_dispatch.h"
#include "mcd_replicate.h"

namespace mcd {

namespace {

template <int MODEL, bool FREE>
__global__ __launch_bounds__(kBlock) void replicate_kernel(const double* __restrict__ recs, const int64_t* __restrict__ order,
                                                            const Chunk* __restrict__ chunks,
                                                            const double* __restrict__ wpar, double* __restrict__ partials,
                                                            int64_t n_tasks, int n_wtiles, int64_t n_rows, int64_t n_chunks,
                                                            int64_t row0, uint64_t seed, double bg_mean, double bg_sigma2) {
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
    RepAcc acc;
    chunk_replicate<MODEL, FREE>((RecPtr<double>)recs, (RepOrderPtr)(order + ch.begin), ch.count, w, seed, row0 + row,
                                 bg_mean, bg_sigma2, acc);
    if (w_raw >= n_rows) return;                                             // (nothing is stored for a shadow)
    double* p = partials + chunk_id * kRepLaneDoubles * n_rows + row;
#pragma unroll
    for (int k = 0; k < kRepFields; ++k) {
        p[(int64_t)k * n_rows] = acc.obs.f[k];
        p[(int64_t)(kRepFields + k) * n_rows] = acc.rep.f[k];
    }
}

// One thread per (range, lane double, row): the range's slots in ascending order from +0.0 (an empty range stays +0.0).
// out: [n_rows][n_ranges][8][2] = observed, replicated.
__global__ __launch_bounds__(kBlock) void replicate_reduce_kernel(const double* __restrict__ partials,
                                                                   const int64_t* __restrict__ offsets, int64_t n_ranges,
                                                                   int64_t n_rows, double* __restrict__ out) {
    const int64_t t = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (t >= n_ranges * kRepLaneDoubles * n_rows) return;
    const int64_t row = t % n_rows, rest = t / n_rows;
    const int q = (int)(rest % kRepLaneDoubles);
    const int64_t r = rest / kRepLaneDoubles;
    const int field = q % kRepFields, which = q / kRepFields;
    double a = 0.0;
    for (int64_t c = offsets[r]; c < offsets[r + 1]; ++c) {
        const double b = partials[(c * kRepLaneDoubles + q) * n_rows + row];
        a = field == RP_MAX ? rep_max(a, b) : a + b;
    }
    out[((row * n_ranges + r) * kRepFields + field) * 2 + which] = a;
}

template <int MODEL, bool FREE>
hipError_t launch_replicate_main(hipStream_t s, const void* records, const int64_t* order, const Chunk* chunks,
                                 int64_t n_chunks, const void* wpar, int64_t n_rows, int64_t row0, uint64_t seed,
                                 double bg_mean, double bg_sigma2, double* partials) {
    const int n_wtiles = (int)((n_rows + kWave - 1) / kWave);
    const int64_t grid = main_grid(n_chunks, n_rows);
    if (grid <= 0) return hipSuccess;
    hipLaunchKernelGGL((replicate_kernel<MODEL, FREE>), dim3((unsigned)grid), dim3(kBlock), 0, s, (const double*)records, order,
                       chunks, (const double*)wpar, partials, n_chunks * n_wtiles, n_wtiles, n_rows, n_chunks, row0, seed,
                       bg_mean, bg_sigma2);
    return hipGetLastError();
}

}  // namespace

hipError_t launch_replicate(hipStream_t s, const LaunchShape& sh, const void* records, const int64_t* order,
                            const Chunk* chunks, int64_t n_chunks, const void* wpar, int64_t n_rows, int64_t row0,
                            uint64_t seed, double bg_mean, double bg_sigma2, double* partials) {
    if (sh.precision != 0 || n_rows <= 0 || n_rows > kRepMaxRows) return hipErrorInvalidValue;
    return dispatch_launch_model(sh.model, sh.free_centre, [&](auto M, auto FREE) {
        return launch_replicate_main<decltype(M)::value, decltype(FREE)::value>(s, records, order, chunks, n_chunks, wpar,
                                                                                n_rows, row0, seed, bg_mean, bg_sigma2,
                                                                                partials);
    }, hipErrorInvalidValue);
}

hipError_t launch_replicate_reduce(hipStream_t s, const double* partials, const int64_t* range_slot_offsets,
                                   int64_t n_ranges, int64_t n_rows, double* out) {
    if (n_rows <= 0 || n_ranges <= 0) return hipErrorInvalidValue;
    const int64_t n = n_ranges * kRepLaneDoubles * n_rows;
    hipLaunchKernelGGL(replicate_reduce_kernel, dim3((unsigned)((n + kBlock - 1) / kBlock)), dim3(kBlock), 0, s, partials,
                       range_slot_offsets, n_ranges, n_rows, out);
    return hipGetLastError();
}

}  // namespace mcd

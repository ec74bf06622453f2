// mcd_grad.hip -- gfx950 kernel of mcd_loglike_grad_batch: the log-likelihood and its gradient with respect to the K
// kernel columns, per walker (mcd_grad.h holds the per-term arithmetic).
//
// Work decomposition: the value kernel's (mcd_kernels.hip: loglike_kernel; mcd_launch.h has the shared mapping and the
// partial-sum address).  lane = walker; a wave evaluates 64 walkers against one
// chunk of the catalogue's chunk table; the record pointer is wave-uniform, so records arrive by scalar loads and are SGPR
// operands of the f64 vector ops.  Each lane keeps 1 + K float64 sums (at most 15) in registers over its chunk and
// stores them as partials[field][walker / 8][chunk][walker % 8] -- per field the layout of the value kernel's partial
// sums, so the value path's fixed-order reduction (launch_reduce) adds them up unchanged, with field f of walker w as its
// "walker" f x roundup64(W) + w.  No float atomics: results are bitwise repeatable.
//
// Workgroup: 256 threads (4 waves, one per SIMD of a CU), as the value kernel.  No instantiation uses scratch; all but
// one stay within the 128 VGPRs of 4 waves per SIMD (fixed-centre CONST_BGGAUSS: 134, 3 waves per SIMD; the loop is
// expected to be bound by f64 VALU issue, which three resident waves should saturate as well -- not measured).  DESIGN 3.9
// lists the compiler's resource usage per family.
#include "mcd_internal.h"
#include "mcd_dispatch.h"
#include "mcd_grad.h"
#include "mcd_reduce.h"

namespace mcd {

namespace {

template <int MODEL, bool FREE>
__global__ __launch_bounds__(kBlock) void loglike_grad_kernel(const double* __restrict__ recs,
                                                               const Chunk* __restrict__ chunks,
                                                               const double* __restrict__ params,
                                                               const double* __restrict__ wpar,
                                                               double* __restrict__ partials, int64_t n_tasks,
                                                               int n_wtiles, int64_t n_walkers, int64_t n_chunks) {
    constexpr int ND = record_doubles(MODEL, FREE);
    constexpr int K = grad_columns(MODEL, FREE);
    static_assert(K <= kGradMaxColumns, "at most 15 sums per lane");
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int lane = threadIdx.x & (kWave - 1);
    int64_t chunk_id;
    int wtile;
    if (!wave_task(wave, n_tasks, n_wtiles, n_chunks, chunk_id, wtile)) return;
    const Chunk ch = chunks[chunk_id];                                       // scalar load
    const int64_t w_raw = (int64_t)wtile * kWave + lane;
    const int64_t w_idx = w_raw < n_walkers ? w_raw : n_walkers - 1;        // idle lanes shadow the last walker
    const int64_t row = (int64_t)ch.pset * n_walkers + w_idx;
    WalkerConsts<double> w;
    w.load(wpar + row * KD);
    GradRaw<double> q;
    q.template load<MODEL, FREE>(params + row * K);

    double acc[1 + K];
#pragma unroll
    for (int f = 0; f <= K; ++f) acc[f] = 0.0;
    chunk_grad<MODEL, FREE, double>((RecPtr<double>)(recs + ch.begin * ND), ch.count, w, q, acc);

    // rows are padded to whole walker tiles: idle lanes store their shadow sums into padding
    const int64_t n_groups = (int64_t)n_wtiles * (kWave / kPartialGroup);
    const int64_t at = partial_index(w_raw, n_chunks, chunk_id);
    const int64_t field_stride = n_groups * n_chunks * kPartialGroup;
#pragma unroll
    for (int f = 0; f <= K; ++f) partials[f * field_stride + at] = acc[f];
}

template <int MODEL, bool FREE>
hipError_t launch_grad_main(hipStream_t s, const void* records, const Chunk* chunks, int64_t n_chunks, const double* params,
                            const void* wpar, double* partials, int64_t n_walkers) {
    const int n_wtiles = (int)((n_walkers + kWave - 1) / kWave);
    const int64_t grid = main_grid(n_chunks, n_walkers);
    if (grid <= 0) return hipSuccess;
    hipLaunchKernelGGL((loglike_grad_kernel<MODEL, FREE>), dim3((unsigned)grid), dim3(kBlock), 0, s, (const double*)records,
                       chunks, params, (const double*)wpar, partials, n_chunks * n_wtiles, n_wtiles, n_walkers, n_chunks);
    return hipGetLastError();
}

}  // namespace

hipError_t launch_loglike_grad(hipStream_t s, const LaunchShape& sh, const void* records, const Chunk* chunks,
                               int64_t n_chunks, const double* params, const void* wpar, double* partials,
                               int64_t n_walkers) {
    if (sh.precision != 0) return hipErrorInvalidValue;
    return dispatch_launch_model(sh.model, sh.free_centre, [&](auto M, auto FREE) {
        return launch_grad_main<decltype(M)::value, decltype(FREE)::value>(s, records, chunks, n_chunks, params, wpar, partials,
                                                                           n_walkers);
    }, hipErrorInvalidValue);
}

// the value path's reduction over (1 + K) x roundup64(W) "walkers": the same tree for every field, no constant added (the
// plain terms carry lnL_bg themselves)
hipError_t launch_grad_reduce(hipStream_t s, const LaunchShape& sh, const double* partials, int64_t n_chunks,
                              const int64_t* pset_slot_offsets, int64_t n_psets, int64_t max_chunks_per_pset,
                              int64_t n_walkers, double* out) {
    const int64_t fields = 1 + grad_columns(sh.model, sh.free_centre);
    return launch_reduce(s, partials, pset_slot_offsets, n_psets, n_chunks, n_psets == 1 ? n_chunks : max_chunks_per_pset,
                         fields * padded_walkers(n_walkers), nullptr, out);
}

}  // namespace mcd

// mcd_simulated_grad.hip -- gfx950 kernel of mcd_simulated_loglike_grad: the log-likelihood and its gradient with respect
// to the K kernel columns per parameter row, every row on the velocities of its own simulation (mcd_simulated_grad.h holds
// the loop, mcd_grad.h the per-term arithmetic, mcd_simulated.h the term whose value it returns).
//
// Work decomposition: the gradient kernel's (mcd_grad.hip; mcd_launch.h has the shared mapping and the partial-sum
// address).  lane = row; a wave evaluates 64 rows against one chunk of the chunk table over `records` (catalogue order);
// the record pointer and the star index are wave-uniform, so records arrive by scalar loads.  What differs per lane is the
// velocity: one vector load per star from col = table + row_sim[row], stride = n_sims (simulated_value_kernel's
// addressing; rows of a wave that share a simulation hit one address).  Each lane keeps 1 + K float64 sums and stores them
// as partials[field][row / 8][chunk][row % 8], the gradient kernel's layout, so its fixed-order reduction
// (launch_grad_reduce: launch_reduce over (1 + K) x padded rows) adds them up unchanged.  Plain C++, vector stores only, no
// atomics, no LDS: results are bitwise repeatable.
//
// Workgroup: 256 threads (4 waves, one per SIMD of a CU).  No instantiation uses scratch;
// profiles/simulated_grad_resources.json lists the compiler's resource usage per family.
#include "mcd_internal.h"
#include "mcd_dispatch.h"
#include "mcd_simulated_grad.h"
#include "mcd_reduce.h"

namespace mcd {

namespace {

template <int MODEL, bool FREE>
__global__ __launch_bounds__(kBlock) void simulated_grad_kernel(const double* __restrict__ recs,
                                                                 const Chunk* __restrict__ chunks,
                                                                 const double* __restrict__ params,
                                                                 const double* __restrict__ wpar,
                                                                 const int64_t* __restrict__ row_sim,
                                                                 const double* __restrict__ table, int64_t n_sims,
                                                                 double bg_mean, double bg_sigma2,
                                                                 double* __restrict__ partials, int64_t n_tasks,
                                                                 int n_wtiles, int64_t n_rows, int64_t n_chunks) {
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
    const int64_t row = w_raw < n_rows ? w_raw : n_rows - 1;                 // idle lanes shadow the last row
    WalkerConsts<double> w;
    w.load(wpar + row * KD);
    GradRaw<double> q;
    q.template load<MODEL, FREE>(params + row * K);
    const double* col = table + row_sim[row];                                // (the host has checked 0 <= simulation < n_sims)

    double acc[1 + K];
#pragma unroll
    for (int f = 0; f <= K; ++f) acc[f] = 0.0;
    chunk_simulated_grad<MODEL, FREE>((RecPtr<double>)(recs + ch.begin * ND), ch.begin, ch.count, w, q, col, n_sims, bg_mean,
                                      bg_sigma2, acc);

    // rows are padded to whole tiles: idle lanes store their shadow sums into padding
    const int64_t n_groups = (int64_t)n_wtiles * (kWave / kPartialGroup);
    const int64_t at = partial_index(w_raw, n_chunks, chunk_id);
    const int64_t field_stride = n_groups * n_chunks * kPartialGroup;
#pragma unroll
    for (int f = 0; f <= K; ++f) partials[f * field_stride + at] = acc[f];
}

template <int MODEL, bool FREE>
hipError_t launch_simulated_grad_main(hipStream_t s, const void* records, const Chunk* chunks, int64_t n_chunks,
                                      const double* params, const void* wpar, const int64_t* row_sim, const double* table,
                                      int64_t n_sims, double bg_mean, double bg_sigma2, double* partials, int64_t n_rows) {
    const int n_wtiles = (int)((n_rows + kWave - 1) / kWave);
    const int64_t grid = main_grid(n_chunks, n_rows);
    if (grid <= 0) return hipSuccess;
    hipLaunchKernelGGL((simulated_grad_kernel<MODEL, FREE>), dim3((unsigned)grid), dim3(kBlock), 0, s, (const double*)records,
                       chunks, params, (const double*)wpar, row_sim, table, n_sims, bg_mean, bg_sigma2, partials,
                       n_chunks * n_wtiles, n_wtiles, n_rows, n_chunks);
    return hipGetLastError();
}

}  // namespace

hipError_t launch_simulated_grad(hipStream_t s, const LaunchShape& sh, const void* records, const Chunk* chunks,
                                 int64_t n_chunks, const double* params, const void* wpar, const int64_t* row_sim,
                                 const double* table, int64_t n_sims, double bg_mean, double bg_sigma2, double* partials,
                                 int64_t n_rows) {
    if (sh.precision != 0 || n_rows <= 0 || n_rows > kSimulatedMaxRows || !params || !row_sim || !table || n_sims <= 0)
        return hipErrorInvalidValue;
    return dispatch_launch_model(sh.model, sh.free_centre, [&](auto M, auto FREE) {
        return launch_simulated_grad_main<decltype(M)::value, decltype(FREE)::value>(s, records, chunks, n_chunks, params, wpar,
                                                                                     row_sim, table, n_sims, bg_mean, bg_sigma2,
                                                                                     partials, n_rows);
    }, hipErrorInvalidValue);
}

}  // namespace mcd

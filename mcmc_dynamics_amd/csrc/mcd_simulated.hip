// mcd_simulated.hip -- gfx950 kernels of the simulated catalogues (mcd_simulated.h holds the velocity rule, the term and the
// loop; mcd_replicate.h the generator).
//
// Work decomposition: the value kernels' (mcd_launch.h has the shared mapping and the partial-sum address).  A wave takes
// 64 rows against one chunk of the chunk table over `records` (catalogue order); the record pointer and the star index
// are wave-uniform, so records arrive by scalar loads.
//   simulate_kernel         lane = simulation.  The rows are the truth rows; every lane writes table[star][simulation], so
//                           a wave writes 512 contiguous bytes per star.  Idle lanes shadow the last simulation and store
//                           nothing.  Each lane also keeps the first star of its chunk whose velocity is not finite (-1:
//                           none) and stores it as bad[chunk][simulation]; simulate_first_kernel takes the smallest per
//                           simulation, so the host reads one word per simulation.
//   simulated_value_kernel  lane = parameter row: weighted_value_kernel (mcd_weighted_value.hip) with the explicit table's
//                           addressing, col = table + row_sim[row], stride = n_sims.  Each lane keeps ONE float64 sum and
//                           stores it as partials[row / 8][chunk][row % 8], so launch_reduce adds it up unchanged.  When
//                           the rows of a wave share a simulation the 64 loads of a star hit one address.
// Plain C++, vector stores only, no atomics, no LDS: results are bitwise repeatable.
//
// Workgroup: 256 threads (4 waves, one per SIMD of a CU).  No instantiation uses scratch; profiles/simulated_resources.json
// lists the compiler's resource usage per family.
#include "mcd_internal.h"
#include "mcd_dispatch.h"
#include "mcd_simulated.h"
#include "mcd_reduce.h"

namespace mcd {

namespace {

template <int MODEL, bool FREE>
__global__ __launch_bounds__(kBlock) void simulate_kernel(const double* __restrict__ recs, const Chunk* __restrict__ chunks,
                                                           const double* __restrict__ wpar, double* __restrict__ table,
                                                           int64_t* __restrict__ bad, int64_t n_tasks, int n_wtiles,
                                                           int64_t n_rows, int64_t n_chunks, int64_t sim_begin, int64_t n_sims,
                                                           int64_t sim0, uint64_t seed, double bg_mean, double bg_sigma2) {
    constexpr int ND = record_doubles(MODEL, FREE);
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int lane = threadIdx.x & (kWave - 1);
    int64_t chunk_id;
    int wtile;
    if (!wave_task(wave, n_tasks, n_wtiles, n_chunks, chunk_id, wtile)) return;
    const Chunk ch = chunks[chunk_id];                                       // scalar load
    const int64_t w_raw = (int64_t)wtile * kWave + lane;
    const bool live = w_raw < n_rows;
    const int64_t row = live ? w_raw : n_rows - 1;                           // idle lanes shadow the last simulation
    WalkerConsts<double> w;
    w.load(wpar + row * KD);
    const int64_t e = sim_begin + row;                                       // column of the table; generator row sim0 + e
    RecPtr<double> r = (RecPtr<double>)(recs + ch.begin * ND);
    int64_t first = -1;
    for (int j = 0; j < ch.count; ++j, r += ND) {
        const int64_t star = ch.begin + j;
        const double v = simulated_velocity<MODEL, FREE>(r, w, seed, sim0 + e, star, bg_mean, bg_sigma2);
        if (!(v - v == 0.0) && first < 0) first = star;
        if (live) table[star * n_sims + e] = v;
    }
    if (live) bad[chunk_id * n_rows + row] = first;
}

// One thread per simulation of the pass: the chunks in ascending order hold ascending stars
__global__ __launch_bounds__(kBlock) void simulate_first_kernel(const int64_t* __restrict__ bad, int64_t n_chunks, int64_t n_rows,
                                                                 int64_t* __restrict__ first_bad) {
    const int64_t row = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (row >= n_rows) return;
    int64_t first = -1;
    for (int64_t c = 0; c < n_chunks; ++c) {
        const int64_t b = bad[c * n_rows + row];
        if (b >= 0 && (first < 0 || b < first)) first = b;
    }
    first_bad[row] = first;
}

template <int MODEL, bool FREE>
__global__ __launch_bounds__(kBlock) void simulated_value_kernel(const double* __restrict__ recs,
                                                                  const Chunk* __restrict__ chunks,
                                                                  const double* __restrict__ wpar,
                                                                  const int64_t* __restrict__ row_sim,
                                                                  const double* __restrict__ table, int64_t n_sims,
                                                                  double bg_mean, double bg_sigma2,
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
    const double* col = table + row_sim[row];                                // (the host has checked 0 <= simulation < n_sims)
    const double acc = chunk_simulated_value<MODEL, FREE>((RecPtr<double>)(recs + ch.begin * ND), ch.begin, ch.count, w, col,
                                                          n_sims, bg_mean, bg_sigma2);
    // rows are padded to whole tiles: idle lanes store their shadow sum into padding
    partials[partial_index(w_raw, n_chunks, chunk_id)] = acc;
}

template <int MODEL, bool FREE>
hipError_t launch_simulate_main(hipStream_t s, const void* records, const Chunk* chunks, int64_t n_chunks, const void* wpar,
                                int64_t n_rows, int64_t sim_begin, int64_t n_sims, int64_t sim0, uint64_t seed, double bg_mean,
                                double bg_sigma2, double* table, int64_t* bad) {
    const int n_wtiles = (int)((n_rows + kWave - 1) / kWave);
    const int64_t grid = main_grid(n_chunks, n_rows);
    if (grid <= 0) return hipSuccess;
    hipLaunchKernelGGL((simulate_kernel<MODEL, FREE>), dim3((unsigned)grid), dim3(kBlock), 0, s, (const double*)records, chunks,
                       (const double*)wpar, table, bad, n_chunks * n_wtiles, n_wtiles, n_rows, n_chunks, sim_begin, n_sims, sim0,
                       seed, bg_mean, bg_sigma2);
    return hipGetLastError();
}

template <int MODEL, bool FREE>
hipError_t launch_simulated_value_main(hipStream_t s, const void* records, const Chunk* chunks, int64_t n_chunks,
                                       const void* wpar, const int64_t* row_sim, const double* table, int64_t n_sims,
                                       double bg_mean, double bg_sigma2, double* partials, int64_t n_rows) {
    const int n_wtiles = (int)((n_rows + kWave - 1) / kWave);
    const int64_t grid = main_grid(n_chunks, n_rows);
    if (grid <= 0) return hipSuccess;
    hipLaunchKernelGGL((simulated_value_kernel<MODEL, FREE>), dim3((unsigned)grid), dim3(kBlock), 0, s, (const double*)records,
                       chunks, (const double*)wpar, row_sim, table, n_sims, bg_mean, bg_sigma2, partials, n_chunks * n_wtiles,
                       n_wtiles, n_rows, n_chunks);
    return hipGetLastError();
}

}  // namespace

hipError_t launch_simulate(hipStream_t s, const LaunchShape& sh, const void* records, const Chunk* chunks, int64_t n_chunks,
                           const void* wpar, int64_t n_rows, int64_t sim_begin, int64_t n_sims, int64_t sim0, uint64_t seed,
                           double bg_mean, double bg_sigma2, double* table, int64_t* bad) {
    if (sh.precision != 0 || n_rows <= 0 || n_rows > kSimulatedPassSims || sim_begin < 0 || sim_begin + n_rows > n_sims ||
        !table || !bad)
        return hipErrorInvalidValue;
    return dispatch_launch_model(sh.model, sh.free_centre, [&](auto M, auto FREE) {
        return launch_simulate_main<decltype(M)::value, decltype(FREE)::value>(s, records, chunks, n_chunks, wpar, n_rows,
                                                                               sim_begin, n_sims, sim0, seed, bg_mean, bg_sigma2,
                                                                               table, bad);
    }, hipErrorInvalidValue);
}

hipError_t launch_simulate_first(hipStream_t s, const int64_t* bad, int64_t n_chunks, int64_t n_rows, int64_t* first_bad) {
    if (n_rows <= 0 || n_chunks < 0) return hipErrorInvalidValue;
    hipLaunchKernelGGL(simulate_first_kernel, dim3((unsigned)((n_rows + kBlock - 1) / kBlock)), dim3(kBlock), 0, s, bad, n_chunks,
                       n_rows, first_bad);
    return hipGetLastError();
}

hipError_t launch_simulated_value(hipStream_t s, const LaunchShape& sh, const void* records, const Chunk* chunks,
                                  int64_t n_chunks, const void* wpar, const int64_t* row_sim, const double* table,
                                  int64_t n_sims, double bg_mean, double bg_sigma2, double* partials, int64_t n_rows) {
    if (sh.precision != 0 || n_rows <= 0 || n_rows > kSimulatedMaxRows || !row_sim || !table || n_sims <= 0)
        return hipErrorInvalidValue;
    return dispatch_launch_model(sh.model, sh.free_centre, [&](auto M, auto FREE) {
        return launch_simulated_value_main<decltype(M)::value, decltype(FREE)::value>(s, records, chunks, n_chunks, wpar, row_sim,
                                                                                      table, n_sims, bg_mean, bg_sigma2, partials,
                                                                                      n_rows);
    }, hipErrorInvalidValue);
}

}  // namespace mcd

// mcd_launch.h -- launch vocabulary shared by the device units: the workgroup shape, and how a wave of the main kernels
// (mcd_kernels.hip: loglike_kernel, mcd_grad.hip: loglike_grad_kernel) finds its work and where its partial sums go.  The
// reduction (mcd_reduce.h) and the resident chain's step kernel (mcd_stretch.hip) read the layout defined here.
#pragma once

#include <hip/hip_runtime.h>
#include <cstdint>

#include "mcd_reduce.h"   // kPartialGroup

namespace mcd {

constexpr int kWave = 64;
constexpr int kBlock = 256;               // 4 waves: one per SIMD of a CU
constexpr int kWavesPerBlock = kBlock / kWave;

// rows of the partial-sum and gradient arrays: the walkers rounded up to whole 64-walker tiles
constexpr int64_t padded_walkers(int64_t n_walkers) { return (n_walkers + kWave - 1) / kWave * kWave; }

// (chunk, walker tile) of wave `wave` of a 4-wave workgroup of the grid mcd_chunks.h: main_grid.  Returns whether the wave
// has work: the early-out is the caller's.  loglike_kernel (mcd_kernels.hip) holds the same mapping written out, because
// calling this function changes its vector code, and adds the workgroups of 8 and 16 waves that combine their chunks
// (the first branch with their wave count, idle waves kept for the barrier): a change here is a change there.
__device__ __forceinline__ bool wave_task(int wave, int64_t n_tasks, int n_wtiles, int64_t n_chunks, int64_t& chunk_id,
                                          int& wtile) {
    if (n_wtiles <= kWavesPerBlock) {
        // <= 256 walkers: consecutive waves share a chunk, so every chunk is read by one workgroup (one CU, one XCD)
        const int64_t task = (int64_t)blockIdx.x * kWavesPerBlock + wave;   // wave-uniform
        if (task >= n_tasks) return false;
        chunk_id = task / n_wtiles;
        wtile = (int)(task - chunk_id * n_wtiles);
        return true;
    }
    // > 256 walkers: a chunk needs m = ceil(n_wtiles / 4) workgroups.  Workgroups are dealt round-robin over the
    // 8 XCDs, so workgroups b and b + 8 share an XCD (and its L2): within a group of 8 m workgroups, workgroup j
    // takes chunk j % 8 and walker-tile quartet j / 8 -- all m readers of a chunk sit on one XCD and the chunk is
    // fetched from HBM once.  (Placement only affects traffic, never results.)
    const int m = (n_wtiles + kWavesPerBlock - 1) / kWavesPerBlock;
    const int64_t group = blockIdx.x / (8 * m);
    const int j = (int)(blockIdx.x - group * (8 * m));
    chunk_id = group * 8 + (j & 7);
    wtile = (j >> 3) * kWavesPerBlock + wave;
    return chunk_id < n_chunks && wtile < n_wtiles;
}

// partials[walker group of 8][slot][walker in group]: eight full 64-byte segments per wave store (the rows are padded to
// whole walker tiles, so idle lanes store their shadow value into padding), and the reduction streams one contiguous
// [slot][8] block per walker group.  slot = chunk, or the workgroup when its chunks are combined.
__device__ __forceinline__ int64_t partial_index(int64_t w_raw, int64_t n_slots, int64_t slot) {
    static_assert(kPartialGroup == 8, "the shift and the mask below");
    return ((w_raw >> 3) * n_slots + slot) * kPartialGroup + (w_raw & (kPartialGroup - 1));
}

}  // namespace mcd

// mcd_hmc.hip -- gfx950 kernels of the resident Hamiltonian Monte Carlo block (mcd_hmc_block; the algebra is mcd_hmc.h,
// the host side hmc_block_device in mcd_api_chain.hip).  The expensive part of a leapfrog point is the existing gradient
// kernel and its reduction (mcd_grad.hip); the two kernels here are what runs BETWEEN two gradient evaluations, so that a
// block of n_steps x n_leap evaluations is one chain of launches on one stream and nothing returns to the host:
//
//   hmc_begin_kernel   start of a step: momenta, H0, the step's eps, half kick, drift with the box rule, the next table row
//   hmc_leap_kernel    after an evaluation: chain rule on the reduced [1 + K][roundup64(W)] fields, kick, drift, next row;
//                      on the trajectory's last point half kick, accept / reject, and the step's chain rows
//
// One thread per walker: a handful of float64 operations over P <= 12 coordinates, plain C++ on per-walker rows
// (mcd_launch.h's workgroup of 256 threads, wave64; no LDS, no atomics, vector stores only).  Structured priors
// (mcd_prior.h) arrive through HmcShared::prior and the shared hmc_* functions; nothing here names them.  Built with
// -ffp-contract=off like the host: the chain is the host-driven block's bit for bit.
#include "mcd_internal.h"
#include "mcd_launch.h"
#include "mcd_hmc.h"

namespace mcd {

namespace {

__device__ __forceinline__ HmcWalker walker_of(const HmcDevice& d, int64_t w) {
    HmcWalker t;
    const int P = d.s.n_dim;
    t.q = d.q + w * P; t.p = d.p + w * P; t.h0 = d.h0 + w; t.eps = d.eps + w; t.alive = d.alive + w;
    return t;
}

__global__ __launch_bounds__(kBlock) void hmc_begin_kernel(const HmcDevice d, int64_t step) {
    const int64_t w = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (w >= d.n_walkers) return;
    const int P = d.s.n_dim;
    hmc_begin(d.s, d.seed, step, w, d.pos + w * P, d.lnp[w], d.grad + w * P, walker_of(d, w), d.table + w * d.s.k);
}

__global__ __launch_bounds__(kBlock) void hmc_leap_kernel(const HmcDevice d, int64_t step, int64_t row, int leap) {
    const int64_t w = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (w >= d.n_walkers) return;
    const int P = d.s.n_dim;
    const int64_t W = d.n_walkers;
    const HmcOutcome o = hmc_leap(d.s, d.seed, step, w, leap, d.fields[w], d.fields + d.padded + w, d.padded, walker_of(d, w),
                                  d.pos + w * P, d.lnp + w, d.grad + w * P, d.table + w * d.s.k);
    if (leap < d.s.n_leap) return;
    if (o.accepted) d.accepted[w] += 1;
    if (d.energy_error) d.energy_error[row * W + w] = o.energy_error;
    if (d.lnprob_chain) d.lnprob_chain[row * W + w] = d.lnp[w];
    if (d.chain)
        for (int c = 0; c < P; ++c) d.chain[(row * W + w) * P + c] = d.pos[w * P + c];
}

unsigned walker_grid(int64_t n_walkers) { return (unsigned)((n_walkers + kBlock - 1) / kBlock); }

}  // namespace

hipError_t launch_hmc_begin(hipStream_t s, const HmcDevice& d, int64_t step) {
    if (d.n_walkers < 1 || d.s.n_dim < 1 || d.s.n_dim > kHmcMaxDim) return hipErrorInvalidValue;
    hipLaunchKernelGGL(hmc_begin_kernel, dim3(walker_grid(d.n_walkers)), dim3(kBlock), 0, s, d, step);
    return hipGetLastError();
}

hipError_t launch_hmc_leap(hipStream_t s, const HmcDevice& d, int64_t step, int64_t row, int leap) {
    if (d.n_walkers < 1 || d.s.n_dim < 1 || d.s.n_dim > kHmcMaxDim || leap < 1 || leap > d.s.n_leap) return hipErrorInvalidValue;
    hipLaunchKernelGGL(hmc_leap_kernel, dim3(walker_grid(d.n_walkers)), dim3(kBlock), 0, s, d, step, row, leap);
    return hipGetLastError();
}

}  // namespace mcd

// mcd_temper.hip -- gfx950 kernels of the resident parallel-tempering block (mcd_temper_block; the algebra is mcd_temper.h,
// the host side temper_block_device in mcd_api_temper.hip).  The expensive part of a half step is the existing main kernel
// and its reduction over T W/2 parameter rows; the two kernels here are what runs BETWEEN two evaluations, so that a block
// of n_steps steps is one chain of launches on one stream and nothing returns to the host:
//
//   temper_step_kernel   accept-and-propose: accepts or rejects the previous half step from the reduced sums, then proposes
//                        the next one, checks the box and the prior and writes the resolved kernel rows (the walker
//                        constants follow from launch_prepare_walkers, the kernel the host-driven evaluation runs on the same
//                        table: the bits of the host-driven form).  Partners come from the walker's own rung only: ONE
//                        WORKGROUP PER RUNG, the accept and the propose separated by the workgroup's barrier.
//   temper_swap_kernel   swap-and-record: the swap phase of the step, one thread per (rung, walker) -- the lower rung of an
//                        active pair decides and exchanges both walkers -- then the step's chain rows and the swap counts.
//
// Plain C++ on per-walker rows (mcd_launch.h's workgroup of 256 threads, wave64; no LDS, no atomics, vector stores only:
// counts are per-thread words, summed by the host after the block).  The stretch numbers of the block are generated ahead
// by launch_chain_numbers with B = T (mcd_stretch.hip); the swap's one generator call per (step, t, w) is inline.  Built
// with -ffp-contract=off like the host: the chain is the host-driven block's bit for bit.
#include "mcd_internal.h"
#include "mcd_launch.h"
#include "mcd_temper.h"

namespace mcd {

namespace {

__global__ __launch_bounds__(kBlock) void temper_step_kernel(const TemperDevice d, int64_t acc_i, int acc_h, int64_t prop_i,
                                                             int prop_h) {
    const int64_t t = blockIdx.x;                        // the rung of this workgroup
    const int64_t T = d.s.n_temps, W = d.s.n_walkers, half = W / 2;
    const int P = d.s.n_dim, K = d.s.k;
    double* ens = d.pos + t * W * P;
    if (acc_i >= 0) {
        const int32_t* first = d.order + (acc_i * T + t) * W + (acc_h == 0 ? 0 : half);
        const int64_t base = ((acc_i * 2 + acc_h) * T + t) * half;
        const double beta = d.s.betas[t];
        for (int64_t j = threadIdx.x; j < half; j += kBlock) {
            const int64_t r = t * half + j, w = t * W + first[j];
            const int a = temper_accept(d.s, beta, d.thr[base + j], d.ok[r] != 0, d.out[r], d.lp_new[r], d.ll[w], d.lp[w]);
            if (a < 0) *d.status = 1;
            if (a > 0) {
                for (int c = 0; c < P; ++c) d.pos[w * P + c] = d.proposal[r * P + c];
                d.ll[w] = d.out[r];
                d.lp[w] = d.lp_new[r];
                d.accepted[w] += 1;
            }
        }
    }
    __syncthreads();                                     // the proposals below read positions the accepts above wrote
    if (prop_i >= 0) {
        const int32_t* ord = d.order + (prop_i * T + t) * W;
        const int32_t* first = ord + (prop_h == 0 ? 0 : half);
        const int32_t* second = ord + (prop_h == 0 ? half : 0);
        const int64_t base = ((prop_i * 2 + prop_h) * T + t) * half;
        for (int64_t j = threadIdx.x; j < half; j += kBlock) {
            const int64_t r = t * half + j;
            double lp_new;
            const bool good = temper_propose(d.s, ens + (int64_t)first[j] * P, ens + (int64_t)second[d.pick[base + j]] * P,
                                             d.zz[base + j], d.proposal + r * P, d.table + r * K, &lp_new);
            d.ok[r] = good ? 1 : 0;
            d.lp_new[r] = lp_new;
        }
    }
}

__global__ __launch_bounds__(kBlock) void temper_swap_kernel(const TemperDevice d, int64_t step, int64_t row) {
    const int64_t T = d.s.n_temps, W = d.s.n_walkers;
    const int P = d.s.n_dim;
    const int64_t x = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (x >= T * W) return;
    const int64_t t = x / W, w = x - t * W;
    if (t > 0 && temper_pair_active(step, t - 1, T)) return;        // the upper rung of an active pair: its partner's thread
    const bool pair = temper_pair_active(step, t, T);
    const int64_t a = x, b = x + W;
    if (pair && temper_swap_accept(d.s, t, temper_swap_thr(d.seed, step, t, w), d.ll[a], d.ll[b])) {
        for (int c = 0; c < P; ++c) { const double v = d.pos[a * P + c]; d.pos[a * P + c] = d.pos[b * P + c]; d.pos[b * P + c] = v; }
        { const double v = d.ll[a]; d.ll[a] = d.ll[b]; d.ll[b] = v; }
        { const double v = d.lp[a]; d.lp[a] = d.lp[b]; d.lp[b] = v; }
        d.swap_accepted[a] += 1;
    }
    for (int64_t y = a; y <= (pair ? b : a); y += W) {            // the step's rows of this thread's one or two walkers
        if (d.lnlike_chain) d.lnlike_chain[row * T * W + y] = d.ll[y];
        if (d.chain && y < (int64_t)d.n_chain_temps * W)
            for (int c = 0; c < P; ++c) d.chain[(row * d.n_chain_temps * W + y) * P + c] = d.pos[y * P + c];
    }
}

bool shape_ok(const TemperDevice& d) {
    return d.s.n_temps >= 1 && d.s.n_temps <= 0x7fffffff && d.s.n_walkers >= 2 && !(d.s.n_walkers & 1) && d.s.n_dim >= 1 &&
           d.s.n_dim <= kTemperMaxDim && d.s.k >= 1 && d.n_chain_temps >= 1 && d.n_chain_temps <= d.s.n_temps;
}

}  // namespace

hipError_t launch_temper_step(hipStream_t s, const TemperDevice& d, int64_t acc_i, int acc_h, int64_t prop_i, int prop_h) {
    if (!shape_ok(d) || (acc_i < 0 && prop_i < 0) || (acc_h & ~1) || (prop_h & ~1)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(temper_step_kernel, dim3((unsigned)d.s.n_temps), dim3(kBlock), 0, s, d, acc_i, acc_h, prop_i, prop_h);
    return hipGetLastError();
}

hipError_t launch_temper_swap(hipStream_t s, const TemperDevice& d, int64_t step, int64_t row) {
    const int64_t n = (int64_t)d.s.n_temps * d.s.n_walkers;
    if (!shape_ok(d) || step < 0 || row < 0 || (n + kBlock - 1) / kBlock > 0x7fffffff) return hipErrorInvalidValue;
    hipLaunchKernelGGL(temper_swap_kernel, dim3((unsigned)((n + kBlock - 1) / kBlock)), dim3(kBlock), 0, s, d, step, row);
    return hipGetLastError();
}

}  // namespace mcd

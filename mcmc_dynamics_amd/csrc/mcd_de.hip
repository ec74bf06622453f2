// mcd_de.hip -- the differential-evolution move of mcd_de.h with the ensembles resident on the device: the counterpart of
// mcd_stretch.hip's general step kernel, and of its numbers kernel.
//
// ONE small kernel per half step does what the host loop (mcd_de.h: de_block) does between two evaluations:
//
//     accept / reject the previous half step  ->  [end of a step: chain row]  ->  propose the next half step
//     (s + (x_a - x_b) g), box and structured priors, resolved parameter rows, derived walker constants, the ranges the
//     guard judges
//
// one workgroup per ensemble, strided loops over the slots of a half step: any W, un-binned or binned.  The arithmetic is
// the host loop's, operation for operation (no FMA contraction: -ffp-contract=off); the walker constants come from the prep
// kernel's device function (mcd_prep.h) and the guard is the same code (mcd_guard.h), so the chain is bit-identical to the
// host-driven one.
//
// The guard's verdict is on the table of ALL ensembles: every workgroup leaves its ensemble's ranges in memory (per
// half-step parity) and workgroup 0 of the NEXT launch -- the one that accepts from that table's sums -- judges them
// together; the block's last launch only accepts and judges.  What the device cannot decide alone it only detects, with the
// stretch kernel's status bits (mcd_internal.h: ChainStatus): a NaN sum, a re-run request of the fast mixture kernels, a
// verdict that differs from the kernel family the host enqueued, an ensemble without a proposal inside the prior.  The host
// then discards the block and runs it host-driven from the same inputs (mcd_api_de.hip).
#include "mcd_internal.h"   // first: <hip/hip_runtime.h> before the MCD_HD headers
#include "mcd_de.h"
#include "mcd_guard.h"
#include "mcd_math.h"
#include "mcd_prep.h"
#include "mcd_prior.h"

namespace mcd {

namespace {

constexpr int kDeBlock = 256;

__device__ __forceinline__ double de_wave_lesser(double v) {
    for (int off = 32; off > 0; off >>= 1) v = ParamRanges::lesser(v, __shfl_xor(v, off));
    return v;
}
__device__ __forceinline__ double de_wave_greater(double v) {
    for (int off = 32; off > 0; off >>= 1) v = ParamRanges::greater(v, __shfl_xor(v, off));
    return v;
}
// (minima and maxima: any order of merging gives the same bits)
__device__ __forceinline__ void de_wave_merge(ParamRanges& r) {
    r.s2_min = de_wave_lesser(r.s2_min); r.s2_max = de_wave_greater(r.s2_max); r.amp = de_wave_greater(r.amp);
    r.sb2_min = de_wave_lesser(r.sb2_min); r.sb2_max = de_wave_greater(r.sb2_max);
    r.f_min = de_wave_lesser(r.f_min); r.f_max = de_wave_greater(r.f_max);
    r.len_min = de_wave_lesser(r.len_min); r.len_max = de_wave_greater(r.len_max);
    r.es2_min = de_wave_lesser(r.es2_min); r.es2_max = de_wave_greater(r.es2_max);
    r.finite = __all(r.finite ? 1 : 0) != 0;
}
__device__ __forceinline__ void de_store_ranges(const ParamRanges& r, double* o) {
    o[0] = r.s2_min; o[1] = r.s2_max; o[2] = r.amp; o[3] = r.sb2_min; o[4] = r.sb2_max; o[5] = r.f_min; o[6] = r.f_max;
    o[7] = r.len_min; o[8] = r.len_max; o[9] = r.finite ? 1.0 : 0.0; o[10] = r.es2_min; o[11] = r.es2_max;
}
__device__ __forceinline__ ParamRanges de_load_ranges(const double* o) {
    ParamRanges r;
    r.s2_min = o[0]; r.s2_max = o[1]; r.amp = o[2]; r.sb2_min = o[3]; r.sb2_max = o[4]; r.f_min = o[5]; r.f_max = o[6];
    r.len_min = o[7]; r.len_max = o[8]; r.finite = o[9] != 0.0; r.es2_min = o[10]; r.es2_max = o[11];
    return r;
}

// the workgroup's ranges: every thread's -> one per wave -> thread 0 holds the merge of all in `out`
__device__ __forceinline__ void de_block_merge(ParamRanges& mine, double (*s_ranges)[kRangeDoubles], ParamRanges& out) {
    const int tid = threadIdx.x;
    de_wave_merge(mine);
    if ((tid & 63) == 0) de_store_ranges(mine, s_ranges[tid >> 6]);
    __syncthreads();
    if (tid == 0) {
        out = de_load_ranges(s_ranges[0]);
        for (int i = 1; i < kDeBlock / 64; ++i) out.merge(de_load_ranges(s_ranges[i]));
    }
}

// kPrior: the block has structured priors (mcd_prior.h) -- a proposal's log-prior is evaluated when it is proposed, kept in
// prior_val and added to the reduced sum when the proposal is accepted or rejected; a log-normal coordinate <= 0 counts as
// outside the prior.
template <bool kPrior>
__global__ __launch_bounds__(kDeBlock) void de_step_kernel(DeDevice dd, int64_t acc_step, int acc_h, int64_t prop_step,
                                                           int prop_h, const double* __restrict__ ll, double rerun_tag) {
    const StretchDevice& d = dd.s;
    const int64_t B = d.n_bins, b = blockIdx.x, W = d.n_walkers, half = W / 2;
    const int P = d.n_dim, K = d.k;
    const int tid = threadIdx.x;
    __shared__ int s_n_ok, s_donor;
    __shared__ double s_ranges[kDeBlock / 64][kRangeDoubles];           // ParamRanges of each wave (a type with initialisers cannot be __shared__)
    // arrays carry the ensemble index in front of the walker index
    double* const pos_b = d.pos + b * W * P;
    double* const lnp_b = d.lnp + b * W;
    long long* const accepted_b = d.accepted + b * W;
    double* const proposal_b = d.proposal + b * half * P;
    uint8_t* const ok_b = d.ok + b * half;
    double* const prior_val_b = kPrior ? d.prior_val + b * half : nullptr;
    // n_ok and the guard's ranges are kept per half-step parity: workgroup 0 judges the PREVIOUS table of all ensembles while
    // the other workgroups already write the next one's
    const int64_t slot_acc = (int64_t)(acc_h & 1) * B, slot_prop = (int64_t)(prop_h & 1) * B;

    if (acc_step >= 0) {
        if (b == 0) {
            // single device: the fast mixture kernels write the launch's tag behind the sums when they want the plain kernels
            if (tid == 0 && rerun_tag != 0.0 && ll[B * half] == rerun_tag) atomicOr(&d.meta[META_STATUS], CHAIN_RERUN);
            // was the kernel family of the launch whose sums arrive now the one the guard picks for its table?  (an ensemble
            // without a valid proposal raised CHAIN_NO_PROPOSAL itself: the block is given back whatever the verdict)
            ParamRanges mine, all;
            for (int64_t e = tid; e < B; e += kDeBlock)
                if (d.n_ok[slot_acc + e] > 0) mine.merge(de_load_ranges(d.ranges + (slot_acc + e) * kRangeDoubles));
            de_block_merge(mine, s_ranges, all);
            if (tid == 0 && !(d.meta[META_STATUS] & CHAIN_NO_PROPOSAL)) {
                int level = 0;
                if (d.allow_fast) {
                    level = level_verdict(d.stats, d.model, false, B * half, all);
                    if (d.allow_fast == 2 && level > 1) level = 1;
                }
                if (level != d.expected_level) {
                    if (!(d.meta[META_STATUS] & CHAIN_LEVEL)) d.meta[META_LEVEL] = level;   // the first verdict that differed
                    atomicOr(&d.meta[META_STATUS], CHAIN_LEVEL);
                }
            }
            __syncthreads();                                   // (s_ranges is used again by the propose phase)
        }
        const int32_t* first = d.order + (acc_step * B + b) * W + (acc_h == 0 ? 0 : half);
        const double* t = d.thr + ((acc_step * 2 + acc_h) * B + b) * half;
        const double* ll_b = ll + b * half;
        const int n_ok = d.n_ok[slot_acc + b];
        for (int64_t j = tid; j < half; j += kDeBlock) {       // (walkers of one half step are distinct: no two threads share a row)
            double new_lnp = (n_ok > 0 && ok_b[j]) ? ll_b[j] : -kInfinity;
            if constexpr (kPrior) { if (n_ok > 0 && ok_b[j]) new_lnp = ll_b[j] + prior_val_b[j]; }
            if (new_lnp != new_lnp) atomicOr(&d.meta[META_STATUS], CHAIN_NAN);
            const int64_t w = first[j];
            if (t[j] < new_lnp - lnp_b[w]) {                   // accept iff thr < new_lnp - old_lnp
                const double* p = proposal_b + j * P;
                for (int c = 0; c < P; ++c) pos_b[w * P + c] = p[c];
                lnp_b[w] = new_lnp;
                accepted_b[w] += 1;
            }
        }
        __syncthreads();                                       // the ensemble is final for this half step
        if (acc_h == 1) {
            if (d.chain) for (int64_t x = tid; x < W * P; x += kDeBlock) d.chain[(acc_step * B + b) * W * P + x] = pos_b[x];
            if (d.lnprob_chain) for (int64_t w = tid; w < W; w += kDeBlock) d.lnprob_chain[(acc_step * B + b) * W + w] = lnp_b[w];
        }
    }
    if (prop_step < 0) return;

    const int32_t* first = d.order + (prop_step * B + b) * W + (prop_h == 0 ? 0 : half);
    const int32_t* second = d.order + (prop_step * B + b) * W + (prop_h == 0 ? half : 0);
    const int64_t at = ((prop_step * 2 + prop_h) * B + b) * half;
    const double* g = d.zz + at;
    const int32_t* pa = d.pick + at;
    const int32_t* pb = dd.pick_b + at;
    if (tid == 0) { s_n_ok = 0; s_donor = 0x7fffffff; }
    __syncthreads();
    // proposal = s + (x_a - x_b) * g, inside the inclusive box prior (false for NaN)
    for (int64_t j = tid; j < half; j += kDeBlock) {
        const double* s = pos_b + (int64_t)first[j] * P;
        const double* xa = pos_b + (int64_t)second[pa[j]] * P;
        const double* xb = pos_b + (int64_t)second[pb[j]] * P;
        const double gj = g[j];
        double* p = proposal_b + j * P;
        bool good = d.fixed_ok != 0;
        for (int c = 0; c < P; ++c) {
            const double v = s[c] + (xa[c] - xb[c]) * gj;
            p[c] = v;
            good = good && (v >= d.lo[c]) && (v <= d.hi[c]);
        }
        if constexpr (kPrior) {
            good = good && prior_row_inside(d.prior, P, p);
            prior_val_b[j] = good ? prior_row(d.prior, P, p) : 0.0;
        }
        ok_b[j] = good;
        if (good) { atomicAdd(&s_n_ok, 1); atomicMin(&s_donor, (int)j); }
    }
    __syncthreads();
    const int n_ok = s_n_ok, donor = s_donor;
    ParamRanges mine, all;
    if (n_ok > 0) {
        // rows outside the prior take the first valid row's place in the launch and are masked when the sums come back
        for (int64_t j = tid; j < half; j += kDeBlock) {
            const double* p = proposal_b + (ok_b[j] ? j : (int64_t)donor) * P;
            double* row = d.table + (b * half + j) * K;
            for (int c = 0; c < K; ++c) {
                const int src = d.col_source[c];
                row[c] = src < 0 ? d.col_const[c] : (d.col_factor[c] == 1.0 ? p[src] : p[src] * d.col_factor[c]);
            }
            walker_constants<double>(row, d.model, d.free_centre != 0, d.wpar + (b * half + j) * KD);
            mine.add_row(row, K, d.model, d.free_centre != 0);
        }
    }
    de_block_merge(mine, s_ranges, all);
    if (tid == 0) {
        d.n_ok[slot_prop + b] = n_ok;
        if (n_ok == 0) atomicOr(&d.meta[META_STATUS], CHAIN_NO_PROPOSAL);   // (the host loop lends the ensemble another's row)
        else de_store_ranges(all, d.ranges + (slot_prop + b) * kRangeDoubles);
    }
}

// ---- seeded blocks (mcd_de_move_seeded): the random numbers of steps [i0, i1) of a block, written where the host's upload
// would have put them (order [i][B][W], pick_a / pick_b / gamma / thr [i][2][B][W/2]).  One workgroup per (ensemble, step):
// one draw per walker (mcd_de.h: de_draw), the split of the ensemble by counting, as chain_numbers_kernel (mcd_stretch.hip).
constexpr int kDeNumbersBlock = 256;
__global__ __launch_bounds__(kDeNumbersBlock) void de_numbers_kernel(uint64_t seed, int64_t step0, int64_t i0, int64_t B, int64_t W,
                                                                     double gamma0, double sigma, int32_t* __restrict__ order,
                                                                     int32_t* __restrict__ pick_a, int32_t* __restrict__ pick_b,
                                                                     double* __restrict__ gamma, double* __restrict__ thr) {
    extern __shared__ unsigned long long s_de_keys[];                   // [W]
    const int64_t b = blockIdx.x, i = i0 + blockIdx.y, half = W / 2;
    const int t = threadIdx.x;
    for (int64_t w = t; w < W; w += kDeNumbersBlock) {
        const int h = w >= half ? 1 : 0;
        const int64_t j = w - h * half;
        const DeDraw dr = de_draw(seed, step0 + i, h, b, j, half, gamma0, sigma);
        const int64_t at = ((i * 2 + h) * B + b) * half + j;
        pick_a[at] = dr.pick_a;
        pick_b[at] = dr.pick_b;
        gamma[at] = dr.gamma;
        thr[at] = dr.thr;
        s_de_keys[w] = dr.order_key;
    }
    __syncthreads();
    for (int64_t w = t; w < W; w += kDeNumbersBlock) {
        const unsigned long long mine = s_de_keys[w];
        int rank = 0;
        for (int64_t v = 0; v < W; ++v) rank += s_de_keys[v] < mine ? 1 : 0;      // (every lane reads the same address: a broadcast)
        order[(i * B + b) * W + rank] = (int32_t)w;
    }
}

}  // namespace

hipError_t launch_de_step(hipStream_t s, const DeDevice& d, int64_t acc_step, int acc_h, int64_t prop_step, int prop_h,
                          const double* ll, double rerun_tag) {
    const bool prior = d.s.prior.any();
    if (prior && !d.s.prior_val) return hipErrorInvalidValue;
    if (d.s.n_bins < 1 || d.s.n_bins > 0x7fffffff || d.s.n_walkers < 4 || (d.s.n_walkers & 1) || !d.pick_b || !d.s.n_ok || !d.s.ranges)
        return hipErrorInvalidValue;
    if (prior)
        hipLaunchKernelGGL(de_step_kernel<true>, dim3((unsigned)d.s.n_bins), dim3(kDeBlock), 0, s, d, acc_step, acc_h, prop_step,
                           prop_h, ll, rerun_tag);
    else
        hipLaunchKernelGGL(de_step_kernel<false>, dim3((unsigned)d.s.n_bins), dim3(kDeBlock), 0, s, d, acc_step, acc_h, prop_step,
                           prop_h, ll, rerun_tag);
    return hipGetLastError();
}

hipError_t launch_de_numbers(hipStream_t s, uint64_t seed, int64_t step0, int64_t i0, int64_t i1, int64_t n_bins,
                             int64_t n_walkers, double gamma0, double sigma, int32_t* order, int32_t* pick_a, int32_t* pick_b,
                             double* gamma, double* thr) {
    if (!chain_numbers_on_device(n_walkers) || n_walkers < 4 || (n_walkers & 1) || n_bins < 1 || n_bins > 0x7fffffff)
        return hipErrorInvalidValue;
    for (int64_t at = i0; at < i1; at += 65535) {                        // (gridDim.y <= 65535)
        const int64_t n = i1 - at < 65535 ? i1 - at : 65535;
        hipLaunchKernelGGL(de_numbers_kernel, dim3((unsigned)n_bins, (unsigned)n), dim3(kDeNumbersBlock), (size_t)n_walkers * 8, s,
                           seed, step0, at, n_bins, n_walkers, gamma0, sigma, order, pick_a, pick_b, gamma, thr);
    }
    return hipGetLastError();
}

}  // namespace mcd

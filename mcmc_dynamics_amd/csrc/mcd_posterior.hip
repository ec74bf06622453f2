// mcd_posterior.hip -- gfx950 kernels of mcd_pointwise_posterior: per-star summaries over S posterior samples (lppd and
// the variance of lnL for WAIC, mean and spread of the membership probability).  The arithmetic is in mcd_posterior.h.
//
// Mapping: the mirror of the main kernel.  lane = star: a wave holds 64 stars, each lane loads
// its star's record once (global loads, hoisted out of the sample loop) and keeps it in VGPRs.  The samples are
// wave-uniform: every lane of a wave walks the same slice of samples, so the derived constants of sample s (one
// WalkerConsts row of KD values, written by launch_prepare_walkers) arrive through the scalar cache as SGPR operands.
// The samples are cut into slices (mcd_posterior.h: posterior_slices) so that small catalogues still fill the chip; a
// wave evaluates one (64-star tile, slice) pair and writes its stars' partial states; posterior_merge_kernel merges them
// per star in slice order.  No atomics: repeated calls give identical bits.
#include <hip/hip_runtime.h>
#include <cstdint>

#include "mcd_internal.h"
#include "mcd_dispatch.h"
#include "mcd_posterior.h"

namespace mcd {
namespace {

// part: [n_slices][post_fields(MEM)][n]   inv: 1 / (j + 1) for j < slice_len
template <int MODEL, bool FREE, bool MEM, class T>
__global__ __launch_bounds__(kBlock) void posterior_slice_kernel(const T* __restrict__ recs, int64_t n,
                                                                  const T* __restrict__ wpar, int64_t n_samples,
                                                                  const double* __restrict__ inv, int64_t slice_len,
                                                                  int64_t n_slices, double* __restrict__ part) {
    constexpr int ND = record_doubles(MODEL, FREE);
    constexpr int F = post_fields(MEM);
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int lane = (int)(threadIdx.x & 63);
    const int64_t task = (int64_t)blockIdx.x * kWavesPerBlock + wave;
    const int64_t n_tiles = (n + kWave - 1) / kWave;
    if (task >= n_tiles * n_slices) return;
    const int64_t slice = task % n_slices;               // neighbouring waves share a tile (its records hit L2)
    const int64_t tile = task / n_slices;
    const int64_t i = tile * kWave + lane;
    const int64_t ic = i < n ? i : n - 1;
    const int64_t j0 = slice * slice_len;
    const int64_t count = (n_samples - j0) < slice_len ? (n_samples - j0) : slice_len;

    const RecPtr<T> r = (RecPtr<T>)(recs + ic * ND);                          // per lane, loop-invariant
    const T MCD_CONST_AS* row = (const T MCD_CONST_AS*)(wpar + j0 * KD);      // wave-uniform: scalar loads
    const double MCD_CONST_AS* iv = (const double MCD_CONST_AS*)inv;

    PostAcc acc;
    acc.init();
    for (int64_t j = 0; j < count; ++j, row += KD) {
        WalkerConsts<T> w;
        w.load(row);
        double x, p;
        posterior_term<MODEL, FREE, MEM, T>(r, w, x, p);
        acc.add<MEM>(x, p, iv[j]);
    }
    if (i < n) {
        double* o = part + slice * F * n + i;
        o[PF_SHIFT * n] = acc.shift;
        o[PF_SUMEXP * n] = acc.sumexp;
        o[PF_MEAN * n] = acc.mean;
        o[PF_M2 * n] = acc.m2;
        if constexpr (MEM) {
            o[PF_PMEAN * n] = acc.pmean;
            o[PF_PM2 * n] = acc.pm2;
        }
    }
}

template <bool MEM>
__device__ __forceinline__ void load_state(const double* __restrict__ src, int64_t n, int64_t i, PostAcc& a) {
    a.shift = src[PF_SHIFT * n + i];
    a.sumexp = src[PF_SUMEXP * n + i];
    a.mean = src[PF_MEAN * n + i];
    a.m2 = src[PF_M2 * n + i];
    a.pmean = MEM ? src[PF_PMEAN * n + i] : 0.0;
    a.pm2 = MEM ? src[PF_PM2 * n + i] : 0.0;
}

// One thread per star: merge the pass's slices in slice order, then fold the pass into the state of the earlier passes
// (n_prev samples; none for the first pass); the last pass writes out[4][n] = lppd, lnl_var, pmem_mean, pmem_std.
template <bool MEM>
__global__ __launch_bounds__(kBlock) void posterior_merge_kernel(const double* __restrict__ part, int64_t n,
                                                                  int64_t n_samples, int64_t slice_len, int64_t n_slices,
                                                                  double* __restrict__ state, int64_t n_prev,
                                                                  int64_t n_total, double* __restrict__ out) {
    constexpr int F = post_fields(MEM);
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    PostAcc acc;
    load_state<MEM>(part, n, i, acc);
    int64_t na = slice_len < n_samples ? slice_len : n_samples;
    for (int64_t s = 1; s < n_slices; ++s) {
        const int64_t left = n_samples - s * slice_len;
        const int64_t nb = left < slice_len ? left : slice_len;
        PostAcc b;
        load_state<MEM>(part + s * F * n, n, i, b);
        acc.merge<MEM>(b, (double)na, (double)nb);
        na += nb;
    }
    if (n_prev > 0) {
        PostAcc prev;
        load_state<MEM>(state, n, i, prev);
        prev.merge<MEM>(acc, (double)n_prev, (double)na);
        acc = prev;
    }
    if (n_prev + na < n_total) {
        state[PF_SHIFT * n + i] = acc.shift;
        state[PF_SUMEXP * n + i] = acc.sumexp;
        state[PF_MEAN * n + i] = acc.mean;
        state[PF_M2 * n + i] = acc.m2;
        if constexpr (MEM) {
            state[PF_PMEAN * n + i] = acc.pmean;
            state[PF_PM2 * n + i] = acc.pm2;
        }
        return;
    }
    double lppd, var, pm, ps;
    acc.finish((double)n_total, lppd, var, pm, ps);
    out[i] = lppd;
    out[n + i] = var;
    out[2 * n + i] = pm;
    out[3 * n + i] = ps;
}

template <int MODEL, bool FREE, bool MEM>
hipError_t slice_launch(hipStream_t s, int precision, const void* records, int64_t n, const void* wpar, int64_t n_samples,
                        const double* inv, int64_t slice_len, int64_t n_slices, double* part) {
    const int64_t n_tasks = (n + kWave - 1) / kWave * n_slices;
    const dim3 grid((unsigned)((n_tasks + kWavesPerBlock - 1) / kWavesPerBlock));
    return dispatch_model_term_type<MODEL>(precision, [&](auto t) {
        using T = decltype(t);
        hipLaunchKernelGGL((posterior_slice_kernel<MODEL, FREE, MEM, T>), grid, dim3(kBlock), 0, s, (const T*)records, n,
                           (const T*)wpar, n_samples, inv, slice_len, n_slices, part);
        return hipGetLastError();
    }, hipErrorInvalidValue);
}

}  // namespace

hipError_t launch_posterior(hipStream_t s, const LaunchShape& sh, bool mem, const void* records, int64_t n,
                            const void* wpar, int64_t n_samples, const double* inv, int64_t slice_len, int64_t n_slices,
                            double* part, double* state, int64_t n_prev, int64_t n_total, double* out) {
    if (n <= 0 || n_samples <= 0) return hipSuccess;
    const hipError_t e = dispatch_launch_model(sh.model, sh.free_centre, [&](auto M, auto FREE) {
        constexpr int MODEL = decltype(M)::value;
        constexpr bool kFree = decltype(FREE)::value;
        // the membership fields exist for the models with a background only
        if constexpr (bg_kind(MODEL) != BG_NONE) {
            if (mem) return slice_launch<MODEL, kFree, true>(s, sh.precision, records, n, wpar, n_samples, inv, slice_len, n_slices, part);
        }
        if (mem) return hipErrorInvalidValue;
        return slice_launch<MODEL, kFree, false>(s, sh.precision, records, n, wpar, n_samples, inv, slice_len, n_slices, part);
    }, hipErrorInvalidValue);
    if (e != hipSuccess) return e;
    const dim3 grid((unsigned)((n + kBlock - 1) / kBlock));
    if (mem)
        hipLaunchKernelGGL(posterior_merge_kernel<true>, grid, dim3(kBlock), 0, s, part, n, n_samples, slice_len, n_slices,
                           state, n_prev, n_total, out);
    else
        hipLaunchKernelGGL(posterior_merge_kernel<false>, grid, dim3(kBlock), 0, s, part, n, n_samples, slice_len, n_slices,
                           state, n_prev, n_total, out);
    return hipGetLastError();
}

}  // namespace mcd

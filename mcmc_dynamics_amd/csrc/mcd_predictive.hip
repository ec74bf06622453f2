// mcd_predictive.hip -- gfx950 kernels of mcd_posterior_predictive: per-star posterior predictive checks over S posterior
// samples (standardised residual, tail probability, PIT, the model's v_los and sigma_los with their spreads).  The
// arithmetic is in mcd_predictive.h.
//
// Mapping: that of mcd_posterior.hip (DESIGN.md sections 3.7 and 3.12).  lane = star: a wave holds 64 stars, each lane
// loads its star's record once and keeps it in VGPRs.  The samples are wave-uniform: every lane of a wave walks the same
// slice of samples, so the derived constants of sample s (one WalkerConsts row of KD values) and the 1 / (j + 1) table
// arrive through the scalar cache as SGPR operands.  A wave evaluates one (64-star tile, slice) pair and writes its stars'
// partial states [slice][field][star]; predictive_merge_kernel merges them per star in slice order and folds the passes.
// No atomics, no LDS: repeated calls give identical bits.
#include <hip/hip_runtime.h>
#include <cstdint>

#include "mcd_internal.h"
#include "mcd_dispatch.h"
#include "mcd_predictive.h"

namespace mcd {
namespace {

// part: [n_slices][pred_fields(MIX)][n]   inv: 1 / (j + 1) for j < slice_len
template <int MODEL, bool FREE, bool MIX, class T>
__global__ __launch_bounds__(kBlock) void predictive_slice_kernel(const T* __restrict__ recs, int64_t n,
                                                                   const T* __restrict__ wpar, int64_t n_samples,
                                                                   const double* __restrict__ inv, int64_t slice_len,
                                                                   int64_t n_slices, double* __restrict__ part) {
    constexpr int ND = record_doubles(MODEL, FREE);
    constexpr int F = pred_fields(MIX);
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int lane = (int)(threadIdx.x & 63);
    const int64_t task = (int64_t)blockIdx.x * kWavesPerBlock + wave;
    const int64_t n_tiles = (n + kWave - 1) / kWave;
    if (task >= n_tiles * n_slices) return;
    const int64_t slice = task % n_slices;               // neighbouring waves share a tile (its records hit L2)
    const int64_t tile = task / n_slices;
    const int64_t i = tile * kWave + lane;
    const int64_t ic = i < n ? i : n - 1;                // lanes past the end re-read the last star and store nothing
    const int64_t j0 = slice * slice_len;
    const int64_t count = (n_samples - j0) < slice_len ? (n_samples - j0) : slice_len;

    const RecPtr<T> r = (RecPtr<T>)(recs + ic * ND);                          // per lane, loop-invariant
    const T MCD_CONST_AS* row = (const T MCD_CONST_AS*)(wpar + j0 * KD);      // wave-uniform: scalar loads
    const double MCD_CONST_AS* iv = (const double MCD_CONST_AS*)inv;

    PredAcc acc;
    acc.init();
    for (int64_t j = 0; j < count; ++j, row += KD) {
        WalkerConsts<T> w;
        w.load(row);
        PredTerm x;
        predictive_term<MODEL, FREE, MIX, T>(r, w, x);
        acc.add<MIX>(x, iv[j]);
    }
    if (i < n) acc.store<MIX>(part + slice * F * n + i, n);
}

// One thread per star: merge the pass's slices in slice order, then fold the pass into the state of the earlier passes
// (n_prev samples; none for the first pass); the last pass writes out[pred_fields(MIX)][n].
template <bool MIX>
__global__ __launch_bounds__(kBlock) void predictive_merge_kernel(const double* __restrict__ part, int64_t n,
                                                                   int64_t n_samples, int64_t slice_len, int64_t n_slices,
                                                                   double* __restrict__ state, int64_t n_prev,
                                                                   int64_t n_total, double* __restrict__ out) {
    constexpr int F = pred_fields(MIX);
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    PredAcc acc;
    acc.load<MIX>(part + i, n);
    int64_t na = slice_len < n_samples ? slice_len : n_samples;
    for (int64_t s = 1; s < n_slices; ++s) {
        const int64_t left = n_samples - s * slice_len;
        const int64_t nb = left < slice_len ? left : slice_len;
        PredAcc b;
        b.load<MIX>(part + s * F * n + i, n);
        acc.merge<MIX>(b, (double)na, (double)nb);
        na += nb;
    }
    if (n_prev > 0) {
        PredAcc prev;
        prev.load<MIX>(state + i, n);
        prev.merge<MIX>(acc, (double)n_prev, (double)na);
        acc = prev;
    }
    if (n_prev + na < n_total) {
        acc.store<MIX>(state + i, n);
        return;
    }
    acc.finish<MIX>((double)n_total, out + i, n);
}

template <int MODEL, bool FREE, bool MIX>
hipError_t slice_launch(hipStream_t s, int precision, const void* records, int64_t n, const void* wpar, int64_t n_samples,
                        const double* inv, int64_t slice_len, int64_t n_slices, double* part) {
    const int64_t n_tasks = (n + kWave - 1) / kWave * n_slices;
    const dim3 grid((unsigned)((n_tasks + kWavesPerBlock - 1) / kWavesPerBlock));
    return dispatch_model_term_type<MODEL>(precision, [&](auto t) {
        using T = decltype(t);
        hipLaunchKernelGGL((predictive_slice_kernel<MODEL, FREE, MIX, T>), grid, dim3(kBlock), 0, s, (const T*)records, n,
                           (const T*)wpar, n_samples, inv, slice_len, n_slices, part);
        return hipGetLastError();
    }, hipErrorInvalidValue);
}

}  // namespace

hipError_t launch_predictive(hipStream_t s, const LaunchShape& sh, bool mix, const void* records, int64_t n,
                             const void* wpar, int64_t n_samples, const double* inv, int64_t slice_len, int64_t n_slices,
                             double* part, double* state, int64_t n_prev, int64_t n_total, double* out) {
    if (n <= 0 || n_samples <= 0) return hipSuccess;
    const hipError_t e = dispatch_launch_model(sh.model, sh.free_centre, [&](auto M, auto FREE) {
        constexpr int MODEL = decltype(M)::value;
        constexpr bool kFree = decltype(FREE)::value;
        // pit_mix exists for the two models whose background has a CDF only
        if constexpr (bg_kind(MODEL) == BG_GAUSS) {
            if (mix) return slice_launch<MODEL, kFree, true>(s, sh.precision, records, n, wpar, n_samples, inv, slice_len, n_slices, part);
        }
        if (mix) return hipErrorInvalidValue;
        return slice_launch<MODEL, kFree, false>(s, sh.precision, records, n, wpar, n_samples, inv, slice_len, n_slices, part);
    }, hipErrorInvalidValue);
    if (e != hipSuccess) return e;
    const dim3 grid((unsigned)((n + kBlock - 1) / kBlock));
    if (mix)
        hipLaunchKernelGGL(predictive_merge_kernel<true>, grid, dim3(kBlock), 0, s, part, n, n_samples, slice_len, n_slices,
                           state, n_prev, n_total, out);
    else
        hipLaunchKernelGGL(predictive_merge_kernel<false>, grid, dim3(kBlock), 0, s, part, n, n_samples, slice_len, n_slices,
                           state, n_prev, n_total, out);
    return hipGetLastError();
}

}  // namespace mcd

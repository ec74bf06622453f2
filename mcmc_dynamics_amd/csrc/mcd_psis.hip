// mcd_psis.hip -- gfx950 kernels of mcd_psis_loo: PSIS-LOO per star over S posterior samples.  The per-star arithmetic
// is in mcd_psis.h; DESIGN.md section 3.8 has the mapping and the measurements.
//
// Two kernels per tile of stars:
//   psis_term_kernel   lnL_is of the tile into a [star][S] float64 scratch.  The mapping of posterior_slice_kernel
//                      (section 3.7): lane = star with its record in VGPRs, the samples wave-uniform with their derived
//                      constants read through the scalar cache.  A wave evaluates 16 samples of its 64 stars into LDS and
//                      writes them transposed, so that every star's row is written 128 contiguous bytes at a time.
//   psis_tail_kernel   one wave per star (mcd_psis_row.h, shared with moment matching): the largest log ratio, a radix select of the cutoff over an order-preserving
//                      64-bit key (8-bit digits, LDS histograms with integer atomics, ties by sample index), the M tail
//                      values gathered and ranked in LDS, the GPD fit with lanes = grid points, the smoothing, and the
//                      log-sum-exps over the row.  Every sum has a fixed order (per lane in sample order, then a butterfly
//                      across the wave): the bits depend on nothing but the star's row.
#include <hip/hip_runtime.h>
#include <cstdint>

#include "mcd_internal.h"
#include "mcd_dispatch.h"
#include "mcd_posterior.h"
#include "mcd_psis.h"
#include "mcd_psis_row.h"

namespace mcd {
namespace {

constexpr int kChunk = 16;                 // samples per LDS transpose of the term kernel

// terms: [n][S]; one wave per (64-star group, sample slice)
template <int MODEL, bool FREE, class T>
__global__ __launch_bounds__(kWave) void psis_term_kernel(const T* __restrict__ recs, int64_t n, const T* __restrict__ wpar,
                                                          int64_t S, int64_t slice_len, int64_t n_slices,
                                                          double* __restrict__ terms) {
    constexpr int ND = record_doubles(MODEL, FREE);
    __shared__ double buf[kChunk][kWave + 1];
    const int lane = lane_id();
    const int64_t task = blockIdx.x;
    const int64_t slice = task % n_slices;
    const int64_t group = task / n_slices;
    const int64_t i0 = group * kWave;
    const int64_t i = i0 + lane;
    const int64_t ic = i < n ? i : n - 1;
    const int64_t j0 = slice * slice_len;
    const int64_t count = (S - j0) < slice_len ? (S - j0) : slice_len;

    const RecPtr<T> r = (RecPtr<T>)(recs + ic * ND);                          // per lane, loop-invariant
    const T MCD_CONST_AS* row = (const T MCD_CONST_AS*)(wpar + j0 * KD);      // wave-uniform: scalar loads
    const int wj = lane & (kChunk - 1), wq = lane >> 4;                       // write phase: sample, star within 4
    for (int64_t c0 = 0; c0 < count; c0 += kChunk) {
        const int cn = (int)((count - c0) < kChunk ? (count - c0) : kChunk);
        for (int j = 0; j < cn; ++j, row += KD) {
            WalkerConsts<T> w;
            w.load(row);
            double x, p;
            posterior_term<MODEL, FREE, false, T>(r, w, x, p);
            buf[j][lane] = x;
        }
        __syncthreads();
        for (int q = 0; q < kWave; q += kWave / kChunk) {
            const int64_t st = i0 + q + wq;
            if (wj < cn && st < n) terms[st * S + j0 + c0 + wj] = buf[wj][q + wq];
        }
        __syncthreads();
    }
}

// One wave per star of the tile (mcd_psis_row.h: psis_row with the ratios -lnL; dynamic LDS: psis_tail_lds_bytes)
__global__ __launch_bounds__(kWave) void psis_tail_kernel(const double* __restrict__ terms, int64_t S, int64_t M,
                                                          double r_eff, double* __restrict__ out, int64_t out_stride) {
    extern __shared__ uint64_t lds64[];
    const int64_t star = blockIdx.x;
    const double* __restrict__ row = terms + star * S;
    const PsisRow r = psis_row<true>([&](int64_t s) { return -row[s]; }, [&](int64_t s) { return row[s]; }, S, M, lds64,
                                     nullptr);
    if (lane_id() == 0) {
        out[PSF_ELPD * out_stride + star] = (r.m2 + log_(r.a3)) - (r.mw + log_(r.a1));
        out[PSF_K * out_stride + star] = r.khat;
        out[PSF_LPPD * out_stride + star] = r.lmax + (log_(r.a4) - log_((double)S));
        out[PSF_NEFF * out_stride + star] = r_eff * (r.a1 * r.a1) / r.a2;
    }
}

template <int MODEL, bool FREE>
hipError_t term_launch(hipStream_t s, int precision, const void* records, int64_t n, const void* wpar, int64_t S,
                       double* terms) {
    int64_t slice_len = 0;
    const int64_t n_slices = posterior_slices(n, S, &slice_len);
    const dim3 grid((unsigned)((n + kWave - 1) / kWave * n_slices));
    return dispatch_model_term_type<MODEL>(precision, [&](auto t) {
        using T = decltype(t);
        hipLaunchKernelGGL((psis_term_kernel<MODEL, FREE, T>), grid, dim3(kWave), 0, s, (const T*)records, n, (const T*)wpar,
                           S, slice_len, n_slices, terms);
        return hipGetLastError();
    }, hipErrorInvalidValue);
}

}  // namespace

hipError_t launch_psis(hipStream_t s, const LaunchShape& sh, const void* records, int64_t n, const void* wpar, int64_t S,
                       int64_t M, double r_eff, double* terms, double* out, int64_t out_stride) {
    if (n <= 0 || S <= 0) return hipSuccess;
    if (M > kPsisMaxTail) return hipErrorInvalidValue;
    const hipError_t e = dispatch_launch_model(sh.model, sh.free_centre, [&](auto M, auto FREE) {
        return term_launch<decltype(M)::value, decltype(FREE)::value>(s, sh.precision, records, n, wpar, S, terms);
    }, hipErrorInvalidValue);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(psis_tail_kernel, dim3((unsigned)n), dim3(kWave), psis_tail_lds_bytes(M), s, terms, S, M, r_eff,
                       out, out_stride);
    return hipGetLastError();
}

}  // namespace mcd

// mcd_loo_expect.hip -- gfx950 kernels of mcd_psis_loo_expect: per-star expectations under the PSIS leave-one-out
// weights of mcd_psis_loo (LOO-PIT, case-deletion means).  The per-star arithmetic is in mcd_psis.h and
// mcd_predictive.h; DESIGN.md section 3.15 has the mapping and the measurements.
//
// Two kernels per tile of stars, the pair of mcd_psis.hip with more rows per star:
//   loox_term_kernel   lnL_is and, next to it, the rows the call asked for (pit, z, vlos, sig, pit_mix of
//                      predictive_term) into a [star][rows][S] float64 scratch.  Mapping of psis_term_kernel: lane = star
//                      with its record in VGPRs, the samples wave-uniform through the scalar cache, 16 samples of the
//                      wave's 64 stars through LDS so that every row is written 128 contiguous bytes at a time.
//   loox_tail_kernel   one wave per star: psis_tail_kernel's select, fit and smoothing, statement for statement (k^ and
//                      n_eff have mcd_psis_loo's bits), and in its last pass over the row, where e_s = exp(lw_s - mw) is
//                      formed for sum_s e_s, the sums sum_s e_s x_s over the extra rows and over the [S][Q] table of
//                      star-independent functions (lanes = samples).  Every sum has the order of that kernel: per lane in
//                      sample order (body, then tail), then a butterfly across the wave.
// psis_tail_kernel itself (mcd_psis.hip) is left as it is: mcd_psis_loo compiles from unchanged text.
#include <hip/hip_runtime.h>
#include <cstdint>

#include "mcd_internal.h"
#include "mcd_dispatch.h"
#include "mcd_posterior.h"
#include "mcd_predictive.h"
#include "mcd_psis.h"

namespace mcd {
namespace {

#ifndef MCD_LOOX_CHUNK
#define MCD_LOOX_CHUNK 16
#endif
constexpr int kChunk = MCD_LOOX_CHUNK;     // samples per LDS transpose of the term kernel (a power of two <= 64)

__device__ __forceinline__ double wave_sum(double v) {
    for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o);        // a + b == b + a: every lane ends with the same bits
    return v;
}
__device__ __forceinline__ double wave_max(double v) {
    for (int o = 32; o >= 1; o >>= 1) v = max_(v, __shfl_xor(v, o));
    return v;
}
__device__ __forceinline__ int lane_id() { return (int)(threadIdx.x & 63); }
__device__ __forceinline__ int prefix_count(uint64_t mask) {             // set bits of mask below this lane
    return __builtin_amdgcn_mbcnt_hi((uint32_t)(mask >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mask, 0));
}

// terms: [n][R][S], R = loox_rows(MODE); one wave per (64-star group, sample slice)
// Dynamic LDS: buf[R][kChunk][kWave + 1] doubles.  Four waves per SIMD asked for: with a static 41 KiB buffer the compiler
// plans for one wave per SIMD, takes all 512 VGPRs and keeps erfc's constants in ~180 of them across the loop.
constexpr size_t term_lds_bytes(int rows) { return (size_t)rows * kChunk * (kWave + 1) * sizeof(double); }

template <int MODEL, bool FREE, int MODE, class T>
__global__ __launch_bounds__(kWave, 4) void loox_term_kernel(const T* __restrict__ recs, int64_t n, const T* __restrict__ wpar,
                                                          int64_t S, int64_t slice_len, int64_t n_slices,
                                                          double* __restrict__ terms) {
    constexpr int ND = record_doubles(MODEL, FREE);
    constexpr int R = loox_rows(MODE);
    extern __shared__ double term_lds[];
    double (*buf)[kChunk][kWave + 1] = (double (*)[kChunk][kWave + 1])term_lds;
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
    const int wj = lane & (kChunk - 1), wq = lane / kChunk;                   // write phase: sample, star within 64 / kChunk
    for (int64_t c0 = 0; c0 < count; c0 += kChunk) {
        const int cn = (int)((count - c0) < kChunk ? (count - c0) : kChunk);
        for (int j = 0; j < cn; ++j, row += KD) {
            WalkerConsts<T> w;
            w.load(row);
            double x, p;
            posterior_term<MODEL, FREE, false, T>(r, w, x, p);
            buf[LR_LNL][j][lane] = x;
            if constexpr (MODE != LOOX_NONE) {
                PredTerm t;
                predictive_term<MODEL, FREE, MODE == LOOX_PRED_MIX, T>(r, w, t);
                buf[LR_PIT][j][lane] = t.pit;
                buf[LR_Z][j][lane] = t.z;
                buf[LR_VLOS][j][lane] = t.vlos;
                buf[LR_SIG][j][lane] = t.sig;
                if constexpr (MODE == LOOX_PRED_MIX) buf[LR_MIX][j][lane] = t.pit_mix;
            }
        }
        __syncthreads();
#pragma unroll 1                       // (unrolled, the 16 x R store addresses are kept across the chunks: 160 VGPRs at R = 5)
        for (int q = 0; q < kWave; q += kWave / kChunk) {
            const int64_t st = i0 + q + wq;
            if (wj < cn && st < n) {
                double* __restrict__ dst = terms + st * R * S + j0 + c0 + wj;
#pragma unroll
                for (int rr = 0; rr < R; ++rr) dst[rr * S] = buf[rr][wj][q + wq];
            }
        }
        __syncthreads();
    }
}

// One wave per star of the tile; XR rows follow lnL in the star's [1 + XR][S] block; func: [S][Q], Q <= kLooMaxFunc.
// Dynamic LDS as psis_tail_kernel: hist[256] u32 | key[M] u64 | idx[M] i32 | skey[M] u64 | sidx[M] i32 |
// theta[kPsisMaxGrid] | lj[kPsisMaxGrid]
template <int XR>
__global__ __launch_bounds__(kWave) void loox_tail_kernel(const double* __restrict__ terms, int64_t S, int64_t M,
                                                          double r_eff, const double* __restrict__ func, int Q,
                                                          double* __restrict__ out, int64_t out_stride) {
    extern __shared__ uint64_t lds64[];
    uint32_t* hist = (uint32_t*)lds64;                                        // 256 x 4 B = 128 x 8 B
    uint64_t* tkey = lds64 + 128;
    uint64_t* skey = tkey + M;
    double* theta = (double*)(skey + M);
    double* lj = theta + kPsisMaxGrid;
    int32_t* tidx = (int32_t*)(lj + kPsisMaxGrid);
    int32_t* sidx = tidx + M;
    double* x = (double*)tkey;                                                // x_t reuses the unsorted keys

    const int lane = lane_id();
    const int64_t star = blockIdx.x;
    const double* __restrict__ row = terms + star * (1 + XR) * S;    // the lnL row; row r at row + r * S

    // the largest log ratio (max r = -min lnL)
    double rmax = -INFINITY;
    for (int64_t s = lane; s < S; s += kWave) rmax = max_(rmax, -row[s]);
    rmax = wave_max(rmax);

    // cutoff = the (M+1)-th largest (lw, index): the key by radix select, then the index among equal keys
    bool tail = M >= 5;
    uint64_t key_c = 0;
    int64_t idx_c = -1;
    if (tail) {
        uint64_t prefix = 0, mask = 0;
        int64_t kth = M + 1;                                                  // rank from the top among the candidates
        for (int shift = 56; shift >= 0; shift -= 8) {
            for (int b = lane; b < 256; b += kWave) hist[b] = 0u;
            __syncthreads();
            for (int64_t s = lane; s < S; s += kWave) {
                const uint64_t k = psis_key(-row[s] - rmax);
                if ((k & mask) == prefix) atomicAdd(&hist[(k >> shift) & 255u], 1u);
            }
            __syncthreads();
            uint32_t c[4];
            uint32_t mine = 0;
            for (int b = 0; b < 4; ++b) {
                c[b] = hist[4 * lane + b];
                mine += c[b];
            }
            // counts in the bins above this lane's four (lanes above hold higher bins)
            uint32_t inc = mine;                                              // inclusive suffix sum over lanes
            for (int o = 1; o < kWave; o <<= 1) {
                const uint32_t v = __shfl_down(inc, o);
                if (lane + o < kWave) inc += v;
            }
            uint32_t above = inc - mine;
            int found = -1;
            uint32_t above_b = 0;
            for (int b = 3; b >= 0; --b) {
                if (found < 0 && (int64_t)above < kth && (int64_t)(above + c[b]) >= kth) {
                    found = 4 * lane + b;
                    above_b = above;
                }
                above += c[b];
            }
            const uint64_t who = __ballot(found >= 0);
            const int src = __ffsll((unsigned long long)who) - 1;
            const int bucket = __shfl(found, src);
            const uint32_t gt = __shfl(above_b, src);
            const uint32_t cnt = hist[bucket];
            kth -= gt;
            prefix |= (uint64_t)bucket << shift;
            mask |= (uint64_t)255u << shift;
            __syncthreads();
            if (cnt == 1u) break;                                             // the cutoff is the only candidate left
        }
        // the kth candidate counted from the highest sample index
        int64_t seen = 0;
        for (int64_t top = S; top > 0; top -= kWave) {
            const int64_t s = top - 1 - lane;
            uint64_t k = 0;
            bool match = false;
            if (s >= 0) {
                k = psis_key(-row[s] - rmax);
                match = (k & mask) == prefix;
            }
            const uint64_t bm = __ballot(match);
            const int64_t pc = __popcll(bm);
            if (seen + pc >= kth) {
                const bool hit = match && (seen + prefix_count(bm) + 1 == kth);
                const int src = __ffsll((unsigned long long)__ballot(hit)) - 1;
                key_c = ((uint64_t)__shfl((int)(uint32_t)(k >> 32), src) << 32) | (uint32_t)__shfl((int)(uint32_t)k, src);
                idx_c = __shfl((int)s, src);
                break;
            }
            seen += pc;
        }
        // gather the tail, (key, index) > (key_c, idx_c), in sample order
        int64_t base = 0;
        for (int64_t s0 = 0; s0 < S; s0 += kWave) {
            const int64_t s = s0 + lane;
            bool in = false;
            uint64_t k = 0;
            if (s < S) {
                k = psis_key(-row[s] - rmax);
                in = k > key_c || (k == key_c && s > idx_c);
            }
            const uint64_t bm = __ballot(in);
            if (in) {
                const int64_t pos = base + prefix_count(bm);
                tkey[pos] = k;
                tidx[pos] = (int32_t)s;
            }
            base += __popcll(bm);
        }
        __syncthreads();
        // rank sort of the M tail entries by (key, index)
        for (int64_t t = lane; t < M; t += kWave) {
            const uint64_t k = tkey[t];
            const int32_t id = tidx[t];
            int64_t rank = 0;
            for (int64_t u = 0; u < M; ++u) {
                const uint64_t ku = tkey[u];
                rank += (ku < k || (ku == k && tidx[u] < id)) ? 1 : 0;
            }
            skey[rank] = k;
            sidx[rank] = id;
        }
        __syncthreads();
    }

    const double cutoff = tail ? psis_unkey(key_c) : 0.0;
    const double ec = exp_(cutoff);
    double khat = INFINITY;
    double sigma = 0.0;
    bool smooth = false;
    if (tail) {
        const double lo = psis_unkey(skey[0]), hi = psis_unkey(skey[M - 1]);
        if (hi - lo < kPsisConstTail) {
            khat = -INFINITY;
        } else {
            for (int64_t t = lane; t < M; t += kWave) x[t] = exp_(psis_unkey(skey[t])) - ec;
            __syncthreads();
            const int m = gpd_grid_m(M);
            const double x_last = x[M - 1], x_star = x[gpd_xstar_index(M)];
            bool bad = false;
            double lmx = -INFINITY;
            for (int j = lane; j < m; j += kWave) {
                const double th = gpd_theta(j + 1, m, x_last, x_star);
                const double l = gpd_profile(th, gpd_mean_log1p(th, x, M), M);
                theta[j] = th;
                lj[j] = l;
                bad = bad || l != l;
                lmx = max_(lmx, l);
            }
            __syncthreads();
            bad = __ballot(bad) != 0;
            lmx = wave_max(lmx);
            double se = 0.0;
            for (int j = lane; j < m; j += kWave) se += exp_(lj[j] - lmx);
            const double lse = lmx + log_(wave_sum(se));
            double th = 0.0;
            for (int j = lane; j < m; j += kWave) th += theta[j] * exp_(lj[j] - lse);
            const double theta_hat = bad ? NAN : wave_sum(th);
            double kk = 0.0;
            for (int64_t t = lane; t < M; t += kWave) kk += log1p_(-theta_hat * x[t]);
            const double k = wave_sum(kk) / (double)M;
            sigma = -k / theta_hat;
            khat = gpd_adjust(k, M);
            smooth = khat < INFINITY && khat > -INFINITY;
        }
    }
    // smoothed (or kept) tail log weights, truncated at 0, into x[]
    double tmax = -INFINITY;
    if (tail) {
        __syncthreads();
        for (int64_t t = lane; t < M; t += kWave) {
            double v = psis_unkey(skey[t]);
            if (smooth) v = psis_smoothed(t, M, khat, sigma, ec);
            v = v < 0.0 ? v : 0.0;
            x[t] = v;
            tmax = max_(tmax, v);
        }
        __syncthreads();
        tmax = wave_max(tmax);
    }
    // the shift: lw's largest value
    const double mw = tail ? max_(tmax, cutoff) : 0.0;                       // the body's largest lw: cutoff, or 0
    double a1 = 0.0, a2 = 0.0;
    double ax[XR > 0 ? XR : 1] = {}, af[kLooMaxFunc] = {};                      // sum_s e_s x_s: rows, functions
    auto fold = [&](double e, int64_t s) {
#pragma unroll
        for (int rr = 0; rr < XR; ++rr) ax[rr] += e * row[(rr + 1) * S + s];
#pragma unroll
        for (int q = 0; q < kLooMaxFunc; ++q)
            if (q < Q) af[q] += e * func[s * Q + q];
    };
    for (int64_t s = lane; s < S; s += kWave) {
        const double l = row[s];
        const double lw = -l - rmax;
        bool in = false;
        if (tail) {
            const uint64_t k = psis_key(lw);
            in = k > key_c || (k == key_c && s > idx_c);
        }
        if (!in) {
            const double v = lw < 0.0 ? lw : 0.0;
            const double e = loox_weight(v, mw);
            a1 += e;
            a2 += e * e;
            fold(e, s);
        }
    }
    if (tail) {
        for (int64_t t = lane; t < M; t += kWave) {
            const double v = x[t];
            const double e = loox_weight(v, mw);
            a1 += e;
            a2 += e * e;
            fold(e, sidx[t]);
        }
    }
    a1 = wave_sum(a1);
    a2 = wave_sum(a2);
#pragma unroll
    for (int rr = 0; rr < XR; ++rr) ax[rr] = wave_sum(ax[rr]);
#pragma unroll
    for (int q = 0; q < kLooMaxFunc; ++q)
        if (q < Q) af[q] = wave_sum(af[q]);
    if (lane == 0) {
        out[LXF_K * out_stride + star] = khat;
        out[LXF_NEFF * out_stride + star] = r_eff * (a1 * a1) / a2;
#pragma unroll
        for (int rr = 0; rr < XR; ++rr) out[(LXF_ROWS + rr) * out_stride + star] = loox_ratio(ax[rr], a1);
#pragma unroll
        for (int q = 0; q < kLooMaxFunc; ++q)
            if (q < Q) out[(LXF_ROWS + XR + q) * out_stride + star] = loox_ratio(af[q], a1);
    }
}

template <int MODEL, bool FREE, int MODE>
hipError_t term_launch(hipStream_t s, int precision, const void* records, int64_t n, const void* wpar, int64_t S,
                       double* terms) {
    int64_t slice_len = 0;
    const int64_t n_slices = posterior_slices(n, S, &slice_len);
    const dim3 grid((unsigned)((n + kWave - 1) / kWave * n_slices));
    return dispatch_model_term_type<MODEL>(precision, [&](auto t) {
        using T = decltype(t);
        hipLaunchKernelGGL((loox_term_kernel<MODEL, FREE, MODE, T>), grid, dim3(kWave), term_lds_bytes(loox_rows(MODE)), s, (const T*)records, n,
                           (const T*)wpar, S, slice_len, n_slices, terms);
        return hipGetLastError();
    }, hipErrorInvalidValue);
}

template <int XR>
hipError_t tail_launch(hipStream_t s, int64_t n, const double* terms, int64_t S, int64_t M, double r_eff, const double* func,
                       int n_func, double* out, int64_t out_stride) {
    const size_t lds = 256 * 4 + (size_t)M * (8 + 8 + 4 + 4) + 2 * kPsisMaxGrid * 8;      // psis_tail_kernel's layout
    hipLaunchKernelGGL(loox_tail_kernel<XR>, dim3((unsigned)n), dim3(kWave), lds, s, terms, S, M, r_eff, func, n_func, out,
                       out_stride);
    return hipGetLastError();
}

}  // namespace

hipError_t launch_loo_expect(hipStream_t s, const LaunchShape& sh, int mode, const void* records, int64_t n,
                             const void* wpar, int64_t S, int64_t M, double r_eff, const double* func, int n_func,
                             double* terms, double* out, int64_t out_stride) {
    if (n <= 0 || S <= 0) return hipSuccess;
    if (M > kPsisMaxTail || n_func < 0 || n_func > kLooMaxFunc) return hipErrorInvalidValue;
    const hipError_t e = dispatch_launch_model(sh.model, sh.free_centre, [&](auto M, auto FREE) {
        constexpr int MODEL = decltype(M)::value;
        constexpr bool kFree = decltype(FREE)::value;
        // pit_mix exists for the two models whose background has a CDF only
        if constexpr (bg_kind(MODEL) == BG_GAUSS) {
            if (mode == LOOX_PRED_MIX) return term_launch<MODEL, kFree, LOOX_PRED_MIX>(s, sh.precision, records, n, wpar, S, terms);
        }
        if (mode == LOOX_PRED) return term_launch<MODEL, kFree, LOOX_PRED>(s, sh.precision, records, n, wpar, S, terms);
        if (mode == LOOX_NONE) return term_launch<MODEL, kFree, LOOX_NONE>(s, sh.precision, records, n, wpar, S, terms);
        return hipErrorInvalidValue;
    }, hipErrorInvalidValue);
    if (e != hipSuccess) return e;
    if (mode == LOOX_PRED_MIX) return tail_launch<loox_rows(LOOX_PRED_MIX) - 1>(s, n, terms, S, M, r_eff, func, n_func, out, out_stride);
    if (mode == LOOX_PRED) return tail_launch<loox_rows(LOOX_PRED) - 1>(s, n, terms, S, M, r_eff, func, n_func, out, out_stride);
    return tail_launch<0>(s, n, terms, S, M, r_eff, func, n_func, out, out_stride);
}

}  // namespace mcd

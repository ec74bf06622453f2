// mcd_mmatch.hip -- gfx950 kernels of mcd_moment_match: what runs between two hold-out evaluations of a group of G stars
// with S rows each.  The algebra is mcd_mmatch.h; DESIGN.md section 3.17 has the mapping.
//
//   mm_moment_kernel     one wave per star: the plain and the weighted mean of its current rows, then the centred second
//                        moments column by column (at most 2 x 12 accumulators per lane).  Sums run in sample order per
//                        lane, then through the wave's butterfly.
//   mm_transform_kernel  one workgroup per star: lane 0 forms the trial of the star's level from its moments (Cholesky
//                        factors and the triangular solve in LDS) and composes it with the star's total map; all lanes then
//                        apply the total map to the ORIGINAL draws, check box and priors, pick the donor (the star's first
//                        row inside the prior) and resolve the kernel rows of the hold-out launch.
//   mm_weight_kernel     one wave per star: the step's log weights from train / test / lnprior / lp0, then the PSIS tail of
//                        mcd_psis_row.h, which leaves k^, the un-normalised weights and the sums of elpd and n_eff.
// Plain C++ with vector stores; the only atomics are integer ones in LDS (radix histogram, first valid row, counts), whose
// results do not depend on their order: a call is bit-identical from run to run.
#include <hip/hip_runtime.h>
#include <cstdint>

#include "mcd_launch.h"
#include "mcd_mmatch.h"
#include "mcd_psis_row.h"

namespace mcd {
namespace {

constexpr int P_MAX = kMmMaxDim;

__global__ __launch_bounds__(kWave) void mm_moment_kernel(MmDevice d) {
    const int e = blockIdx.x;
    if (d.level[e] < MM_SHIFT || d.level[e] > MM_COV) return;
    const int lane = lane_id();
    const int P = d.P;
    const int64_t S = d.S;
    const int sel = d.sel[e];
    const double* __restrict__ rows = d.rows + ((size_t)sel * d.G + e) * S * P;
    const double* __restrict__ w = d.wts + ((size_t)sel * d.G + e) * S;
    const double* __restrict__ st = d.stat + ((size_t)sel * d.G + e) * MS_FIELDS;
    double* __restrict__ mom = d.mom + (size_t)e * mm_moment_doubles(P);
    const double a1 = st[MS_A1];
    const double sum_w2 = st[MS_A2] / (a1 * a1);

    double m[P_MAX], mw[P_MAX];
#pragma unroll
    for (int c = 0; c < P_MAX; ++c) { m[c] = 0.0; mw[c] = 0.0; }
    for (int64_t s = lane; s < S; s += kWave) {
        const double ws = w[s];
#pragma unroll
        for (int c = 0; c < P_MAX; ++c)
            if (c < P) {
                const double x = rows[s * P + c];
                m[c] += x;
                mw[c] += ws * x;
            }
    }
#pragma unroll
    for (int c = 0; c < P_MAX; ++c) {
        m[c] = wave_sum(m[c]) / (double)S;
        mw[c] = wave_sum(mw[c]) / a1;
    }
    // column j of the centred sums, rows r >= j (the matrices are symmetric)
    for (int j = 0; j < P; ++j) {
        double cs[P_MAX], cw[P_MAX];
        double mj = 0.0, mwj = 0.0;
#pragma unroll
        for (int c = 0; c < P_MAX; ++c) {
            cs[c] = 0.0; cw[c] = 0.0;
            if (c == j) { mj = m[c]; mwj = mw[c]; }
        }
        for (int64_t s = lane; s < S; s += kWave) {
            const double ws = w[s];
            const double xj = rows[s * P + j];
            const double dj = xj - mj, dwj = ws * (xj - mwj);
#pragma unroll
            for (int c = 0; c < P_MAX; ++c)
                if (c >= j && c < P) {
                    const double x = rows[s * P + c];
                    cs[c] += (x - m[c]) * dj;
                    cw[c] += (x - mw[c]) * dwj;
                }
        }
#pragma unroll
        for (int c = 0; c < P_MAX; ++c)
            if (c >= j && c < P) {
                const double a = wave_sum(cs[c]) / (double)(S - 1);
                const double sw = wave_sum(cw[c]) / a1;
                if (lane == 0) {
                    mom[3 * P + c * P + j] = a;
                    mom[3 * P + j * P + c] = a;
                    const double b = mm_cov_w(sw, sum_w2);
                    mom[3 * P + P * P + c * P + j] = b;
                    mom[3 * P + P * P + j * P + c] = b;
                    if (c == j) mom[2 * P + c] = mm_var_w(sw, S);
                }
            }
    }
    if (lane == 0) {
#pragma unroll
        for (int c = 0; c < P_MAX; ++c)
            if (c < P) { mom[c] = m[c]; mom[P + c] = mw[c]; }
    }
}

__global__ __launch_bounds__(kBlock) void mm_transform_kernel(MmDevice d) {
    __shared__ double sA[P_MAX * P_MAX], sb[P_MAX], sAt[P_MAX * P_MAX], sbt[P_MAX], swork[2 * P_MAX * P_MAX];
    __shared__ int s_first, s_outside, s_lo, s_hi;
    const int e = blockIdx.x;
    const int tid = threadIdx.x;
    const int P = d.P, K = d.K;
    const int64_t S = d.S;
    const int level = d.level[e];
    const int sel = d.sel[e];
    const int nm = mm_map_doubles(P);
    const double* cur = d.maps + ((size_t)sel * d.G + e) * nm;
    double* dst_map = d.maps + ((size_t)(1 - sel) * d.G + e) * nm;
    double* __restrict__ rows = d.rows + ((size_t)(1 - sel) * d.G + e) * S * P;

    if (tid == 0) {
        int skipped = 0;
        s_first = (int)S;
        s_outside = 0;
        s_lo = 0;
        s_hi = (int)S;
        if (level == MM_BASE) {
            mm_identity(P, sA, sb);
        } else if (level >= MM_SHIFT && level <= MM_COV) {
            if (mm_trial(P, level, d.mom + (size_t)e * mm_moment_doubles(P), sAt, sbt, swork)) {
                mm_compose(P, sAt, sbt, cur, cur + P * P, sA, sb);
            } else {
                skipped = 1;
                for (int i = 0; i < P * P; ++i) sA[i] = cur[i];
                for (int i = 0; i < P; ++i) sb[i] = cur[P * P + i];
            }
        } else if (level == MM_SPLIT_INV) {
            const double* inv = d.inv + (size_t)e * nm;
            for (int i = 0; i < P * P; ++i) sA[i] = inv[i];
            for (int i = 0; i < P; ++i) sb[i] = inv[P * P + i];
            s_lo = (int)(S / 2);
        } else {                                                             // MM_KEEP, MM_SPLIT_FWD: the total map
            for (int i = 0; i < P * P; ++i) sA[i] = cur[i];
            for (int i = 0; i < P; ++i) sb[i] = cur[P * P + i];
            if (level == MM_SPLIT_FWD) s_hi = (int)(S / 2);
        }
        for (int i = 0; i < P * P; ++i) dst_map[i] = sA[i];
        for (int i = 0; i < P; ++i) dst_map[P * P + i] = sb[i];
        d.flags[2 * e] = skipped;
    }
    __syncthreads();
    const int r0 = s_lo, r1 = s_hi;
    PriorTable prior = d.prior;
    for (int64_t s = tid; s < S; s += kBlock) {
        double x[P_MAX], y[P_MAX];
        for (int c = 0; c < P; ++c) x[c] = d.draws[s * P + c];
        if (s >= r0 && s < r1) mm_apply(P, sA, sb, x, y);
        else
            for (int c = 0; c < P; ++c) y[c] = x[c];
        const bool ok = mm_row_inside(P, d.lo, d.hi, prior, d.fixed_ok, y);
        double lp = 0.0;
        if (ok && prior.any()) lp = prior_row(prior, P, y);
        for (int c = 0; c < P; ++c) rows[s * P + c] = y[c];
        d.inside[(size_t)e * S + s] = ok ? 1 : 0;
        d.lnprior[(size_t)e * S + s] = lp;
        if (ok) atomicMin(&s_first, (int)s);
        else atomicAdd(&s_outside, 1);
    }
    __syncthreads();
    const int first = s_first;
    if (tid == 0) d.flags[2 * e + 1] = s_outside;
    // the kernel rows: a row outside the prior is replaced by the star's first row inside it (without one the draws
    // themselves go up: the host discards the launch)
    double* __restrict__ table = d.table + (size_t)e * S * K;
    for (int64_t s = tid; s < S; s += kBlock) {
        const bool ok = d.inside[(size_t)e * S + s] != 0;
        const double* src = ok ? rows + s * P : (first < S ? rows + (int64_t)first * P : d.draws + s * P);
        for (int c = 0; c < K; ++c) {
            const int j = d.col_source[c];
            table[s * K + c] = j < 0 ? d.col_const[c] : (d.col_factor[c] == 1.0 ? src[j] : src[j] * d.col_factor[c]);
        }
    }
}

__global__ __launch_bounds__(kWave) void mm_weight_kernel(MmDevice d) {
    extern __shared__ uint64_t lds64[];
    const int e = blockIdx.x;
    const int level = d.level[e];
    if (level < MM_BASE) return;
    const int lane = lane_id();
    const int64_t S = d.S;
    const int dst = 1 - d.sel[e];
    const int64_t n_rows = d.G * S;
    const double* __restrict__ train = d.out + (size_t)e * S;
    const double* __restrict__ test = d.out + n_rows + (size_t)e * S;
    const int32_t* __restrict__ inside = d.inside + (size_t)e * S;
    const double* __restrict__ lnprior = d.lnprior + (size_t)e * S;
    double* __restrict__ lp0 = d.lp0 + (size_t)e * S;
    double* __restrict__ lw = d.lw + (size_t)e * S;
    double* __restrict__ num = d.num + (size_t)e * S;
    double* __restrict__ lpf = d.lpf + (size_t)e * S;
    double* __restrict__ li = d.li + ((size_t)dst * d.G + e) * S;
    double* __restrict__ wts = d.wts + ((size_t)dst * d.G + e) * S;
    double* __restrict__ st = d.stat + ((size_t)dst * d.G + e) * MS_FIELDS;

    for (int64_t s = lane; s < S; s += kWave) {
        const bool in = inside[s] != 0;
        const double tr = train[s], te = test[s], pr = lnprior[s];
        if (level == MM_BASE) {
            lp0[s] = (tr + te) + pr;
            li[s] = te;
            lw[s] = in ? -te : -INFINITY;
        } else if (level <= MM_COV) {
            li[s] = te;
            lw[s] = mm_lw_trial(in, tr, pr, lp0[s]);
        } else if (level == MM_SPLIT_FWD) {
            li[s] = te;
            num[s] = in ? tr + pr : -INFINITY;
            lpf[s] = (tr + te) + pr;
        } else {
            lw[s] = mm_lw_split(num[s], lpf[s], in, (tr + te) + pr, d.logdet[e]);
        }
    }
    if (level == MM_SPLIT_FWD) return;
    __syncthreads();                                                         // the wave's own stores, read by other lanes below
    const PsisRow r = psis_row<false>([&](int64_t s) { return lw[s]; }, [&](int64_t s) { return li[s]; }, S, d.M, lds64, wts);
    if (lane == 0) {
        st[MS_K] = r.khat;
        st[MS_ELPD] = (r.m2 + log_(r.a3)) - (r.mw + log_(r.a1));
        st[MS_A1] = r.a1;
        st[MS_A2] = r.a2;
    }
}

}  // namespace

hipError_t launch_mm_moments(hipStream_t s, const MmDevice& d) {
    hipLaunchKernelGGL(mm_moment_kernel, dim3((unsigned)d.G), dim3(kWave), 0, s, d);
    return hipGetLastError();
}

hipError_t launch_mm_transform(hipStream_t s, const MmDevice& d) {
    hipLaunchKernelGGL(mm_transform_kernel, dim3((unsigned)d.G), dim3(kBlock), 0, s, d);
    return hipGetLastError();
}

hipError_t launch_mm_weights(hipStream_t s, const MmDevice& d) {
    if (d.M > kPsisMaxTail) return hipErrorInvalidValue;
    hipLaunchKernelGGL(mm_weight_kernel, dim3((unsigned)d.G), dim3(kWave), psis_tail_lds_bytes(d.M), s, d);
    return hipGetLastError();
}

}  // namespace mcd

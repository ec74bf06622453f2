// mcd_psis_row.h -- device only: the PSIS tail of ONE row of S log ratios by one wave, shared by psis_tail_kernel
// (mcd_psis.hip: the ratios are -lnL of the row) and the weight kernel of moment matching (mcd_mmatch.hip: the ratios are
// whatever the step defines, -inf for a row outside the prior).  The arithmetic is mcd_psis.h's; every sum has a fixed
// order (per lane in sample order, then a butterfly across the wave).
#pragma once

#include <hip/hip_runtime.h>
#include <cstdint>

#include "mcd_launch.h"
#include "mcd_psis.h"

namespace mcd {

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

// Dynamic LDS of one wave: hist[256] u32 | key[M] u64 | skey[M] u64 | theta[kPsisMaxGrid] | lj[kPsisMaxGrid] | idx[M] i32 |
// sidx[M] i32
inline size_t psis_tail_lds_bytes(int64_t M) { return 256 * 4 + (size_t)M * (8 + 8 + 4 + 4) + 2 * kPsisMaxGrid * 8; }

// What the row leaves: elpd = (m2 + log a3) - (mw + log a1), n_eff = r_eff a1^2 / a2, lppd = lmax + (log a4 - log S)
struct PsisRow {
    double khat, mw, m2, a1, a2, a3, a4, lmax;
};

// ratio(s): the log ratio of sample s; lnl(s): the value whose weighted mean is wanted.  LOO: ratio(s) == -lnl(s), so
// that lw + lnl is one constant over the body (the shift m2 needs no pass of its own) and lppd is accumulated.
// wout (may be null): [S], the un-normalised weight e_s = exp(lw_s - mw) of every sample (their sum is a1).
template <bool LOO, class Ratio, class Lnl>
__device__ __forceinline__ PsisRow psis_row(Ratio ratio, Lnl lnl, int64_t S, int64_t M, uint64_t* lds64,
                                            double* __restrict__ wout) {
    uint32_t* hist = (uint32_t*)lds64;                                        // 256 x 4 B = 128 x 8 B
    uint64_t* tkey = lds64 + 128;
    uint64_t* skey = tkey + M;
    double* theta = (double*)(skey + M);
    double* lj = theta + kPsisMaxGrid;
    int32_t* tidx = (int32_t*)(lj + kPsisMaxGrid);
    int32_t* sidx = tidx + M;
    double* x = (double*)tkey;                                                // x_t reuses the unsorted keys

    const int lane = lane_id();

    // the largest log ratio and the largest lnL
    double rmax = -INFINITY, lmax = -INFINITY;
    for (int64_t s = lane; s < S; s += kWave) {
        rmax = max_(rmax, ratio(s));
        if constexpr (LOO) lmax = max_(lmax, lnl(s));
    }
    rmax = wave_max(rmax);
    if constexpr (LOO) lmax = wave_max(lmax);

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
                const uint64_t k = psis_key(ratio(s) - rmax);
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
                k = psis_key(ratio(s) - rmax);
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
                k = psis_key(ratio(s) - rmax);
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
    double tmax = -INFINITY, tmax2 = -INFINITY;
    if (tail) {
        __syncthreads();
        for (int64_t t = lane; t < M; t += kWave) {
            double v = psis_unkey(skey[t]);
            if (smooth) v = psis_smoothed(t, M, khat, sigma, ec);
            v = v < 0.0 ? v : 0.0;
            x[t] = v;
            tmax = max_(tmax, v);
            tmax2 = max_(tmax2, v + lnl(sidx[t]));
        }
        __syncthreads();
        tmax = wave_max(tmax);
        tmax2 = wave_max(tmax2);
    }
    // shifts: lw's largest value, and for lw + lnL the body's common value -rmax (LOO; else the body's largest) or the
    // tail's largest
    const double mw = tail ? max_(tmax, cutoff) : 0.0;                       // the body's largest lw: cutoff, or 0
    double m2;
    if constexpr (LOO) {
        m2 = max_(-rmax, tmax2);
    } else {
        double bmax2 = -INFINITY;
        for (int64_t s = lane; s < S; s += kWave) {
            const double lw = ratio(s) - rmax;
            bool in = false;
            if (tail) {
                const uint64_t k = psis_key(lw);
                in = k > key_c || (k == key_c && s > idx_c);
            }
            if (!in) bmax2 = max_(bmax2, (lw < 0.0 ? lw : 0.0) + lnl(s));
        }
        m2 = max_(wave_max(bmax2), tmax2);
    }
    double a1 = 0.0, a2 = 0.0, a3 = 0.0, a4 = 0.0;
    for (int64_t s = lane; s < S; s += kWave) {
        const double l = lnl(s);
        const double lw = ratio(s) - rmax;
        if constexpr (LOO) a4 += exp_(l - lmax);
        bool in = false;
        if (tail) {
            const uint64_t k = psis_key(lw);
            in = k > key_c || (k == key_c && s > idx_c);
        }
        if (!in) {
            const double v = lw < 0.0 ? lw : 0.0;
            const double e = exp_(v - mw);
            a1 += e;
            a2 += e * e;
            a3 += exp_(v + l - m2);
            if (wout) wout[s] = e;
        }
    }
    if (tail) {
        for (int64_t t = lane; t < M; t += kWave) {
            const double v = x[t];
            const double e = exp_(v - mw);
            a1 += e;
            a2 += e * e;
            a3 += exp_(v + lnl(sidx[t]) - m2);
            if (wout) wout[sidx[t]] = e;
        }
    }
    PsisRow r;
    r.khat = khat;
    r.mw = mw;
    r.m2 = m2;
    r.a1 = wave_sum(a1);
    r.a2 = wave_sum(a2);
    r.a3 = wave_sum(a3);
    r.a4 = wave_sum(a4);
    r.lmax = lmax;
    return r;
}

}  // namespace mcd

// TEST INFRASTRUCTURE ONLY -- compiles the per-star arithmetic of mcd_psis_loo_expect (csrc/mcd_psis.h and
// csrc/mcd_predictive.h on top of csrc/mcd_math.h) for the CPU: the weights of psis_emul.cpp's one_star (the same tail
// length, key / tie rule, GPD fit pieces and smoothing as loox_tail_kernel, csrc/mcd_loo_expect.hip) and the expectations
// sum_s e_s x_s / sum_s e_s with the kernel's e_s (loox_weight) and ratio (loox_ratio), with a serial sort and serial sums
// in place of the wave's radix select and reductions.  Never loaded by the product package.
#include <algorithm>
#include <cstdint>
#include <vector>

#include "mcd_dispatch.h"
#include "mcd_posterior.h"
#include "mcd_predictive.h"
#include "mcd_psis.h"

using namespace mcd;

namespace {

// x ascending, length M: returns k^ (gpd_adjust; +inf for a failed fit) and sigma
double gpd_fit(const double* x, int64_t M, double& sigma) {
    const int m = gpd_grid_m(M);
    const double x_last = x[M - 1], x_star = x[gpd_xstar_index(M)];
    std::vector<double> th((size_t)m), l((size_t)m);
    bool bad = false;
    double lmx = -INFINITY;
    for (int j = 0; j < m; ++j) {
        th[j] = gpd_theta(j + 1, m, x_last, x_star);
        l[j] = gpd_profile(th[j], gpd_mean_log1p(th[j], x, M), M);
        bad = bad || l[j] != l[j];
        lmx = max_(lmx, l[j]);
    }
    double se = 0.0;
    for (int j = 0; j < m; ++j) se += exp_(l[j] - lmx);
    const double lse = lmx + log_(se);
    double theta_hat = 0.0;
    for (int j = 0; j < m; ++j) theta_hat += th[j] * exp_(l[j] - lse);
    if (bad) theta_hat = NAN;
    double kk = 0.0;
    for (int64_t t = 0; t < M; ++t) kk += log1p_(-theta_hat * x[t]);
    const double k = kk / (double)M;
    sigma = -k / theta_hat;
    return gpd_adjust(k, M);
}

// One star: e[s] = exp(lw_s - mw) of the smoothed, truncated log weights; returns k^; a1 = sum e, a2 = sum e^2
double star_weights(const double* lnl, int64_t S, double r_eff, std::vector<double>& e, double& a1, double& a2) {
    const int64_t M = psis_tail_len(S, r_eff);
    double rmax = -INFINITY;
    for (int64_t s = 0; s < S; ++s) rmax = max_(rmax, -lnl[s]);
    std::vector<double> lw((size_t)S);
    for (int64_t s = 0; s < S; ++s) lw[s] = -lnl[s] - rmax;
    double khat = INFINITY;
    if (M >= 5) {
        std::vector<int64_t> order((size_t)S);
        for (int64_t s = 0; s < S; ++s) order[s] = s;
        std::sort(order.begin(), order.end(), [&](int64_t a, int64_t b) {
            const uint64_t ka = psis_key(lw[a]), kb = psis_key(lw[b]);
            return ka < kb || (ka == kb && a < b);
        });
        const int64_t first = S - M;
        const double cutoff = lw[order[first - 1]];
        const double ec = exp_(cutoff);
        if (lw[order[S - 1]] - lw[order[first]] < kPsisConstTail) {
            khat = -INFINITY;
        } else {
            std::vector<double> x((size_t)M);
            for (int64_t t = 0; t < M; ++t) x[t] = exp_(lw[order[first + t]]) - ec;
            double sigma = 0.0;
            khat = gpd_fit(x.data(), M, sigma);
            if (khat < INFINITY && khat > -INFINITY)
                for (int64_t t = 0; t < M; ++t) lw[order[first + t]] = psis_smoothed(t, M, khat, sigma, ec);
        }
    }
    double mw = -INFINITY;
    for (int64_t s = 0; s < S; ++s) {
        lw[s] = lw[s] < 0.0 ? lw[s] : 0.0;
        mw = max_(mw, lw[s]);
    }
    e.resize((size_t)S);
    a1 = a2 = 0.0;
    for (int64_t s = 0; s < S; ++s) {
        e[s] = loox_weight(lw[s], mw);
        a1 += e[s];
        a2 += e[s] * e[s];
    }
    return khat;
}

// sum_s e_s x[s * stride] / a1
double expect(const std::vector<double>& e, double a1, const double* x, int64_t stride) {
    double acc = 0.0;
    for (size_t s = 0; s < e.size(); ++s) acc += e[s] * x[(int64_t)s * stride];
    return loox_ratio(acc, a1);
}

// records and derived sample rows arrive as doubles; T = float rounds both once, as the float32 catalogues hold them
template <int MODEL, bool FREE, bool MIX, class T>
void run_model(int64_t n, const double* recs, const double* wrows, int64_t S, double r_eff, double* out) {
    constexpr int ND = record_doubles(MODEL, FREE);
    constexpr int XR = MIX ? 5 : 4;
    std::vector<WalkerConsts<T>> w((size_t)S);
    std::vector<T> row(KD), rec(ND);
    for (int64_t s = 0; s < S; ++s) {
        for (int c = 0; c < KD; ++c) row[c] = (T)wrows[s * KD + c];
        w[s].load(row.data());
    }
    std::vector<double> rows((size_t)(1 + XR) * S), e;
    for (int64_t i = 0; i < n; ++i) {
        for (int c = 0; c < ND; ++c) rec[c] = (T)recs[i * ND + c];
        for (int64_t s = 0; s < S; ++s) {
            double x, p;
            posterior_term<MODEL, FREE, false, T>(rec.data(), w[s], x, p);
            PredTerm t;
            predictive_term<MODEL, FREE, MIX, T>(rec.data(), w[s], t);
            rows[LR_LNL * S + s] = x;
            rows[LR_PIT * S + s] = t.pit;
            rows[LR_Z * S + s] = t.z;
            rows[LR_VLOS * S + s] = t.vlos;
            rows[LR_SIG * S + s] = t.sig;
            if (MIX) rows[LR_MIX * S + s] = t.pit_mix;
        }
        double a1, a2;
        out[LXF_K * n + i] = star_weights(rows.data(), S, r_eff, e, a1, a2);
        out[LXF_NEFF * n + i] = r_eff * (a1 * a1) / a2;
        for (int rr = 0; rr < XR; ++rr) out[(LXF_ROWS + rr) * n + i] = expect(e, a1, rows.data() + (rr + 1) * S, 1);
    }
}

template <int MODEL, bool FREE, bool MIX>
void run_precision(int f32, int64_t n, const double* recs, const double* wrows, int64_t S, double r_eff, double* out) {
    if (f32) run_model<MODEL, FREE, MIX, float>(n, recs, wrows, S, r_eff, out);
    else run_model<MODEL, FREE, MIX, double>(n, recs, wrows, S, r_eff, out);
}

}  // namespace

// lnl: [n][S]; x: [n][R][S] rows per star; func: [S][Q] -> out[2 + R + Q][n] = k^, n_eff, E_loo[x_r], E_loo[func_q]
extern "C" int emul_loo_expect(int64_t n, int64_t S, const double* lnl, double r_eff, int R, const double* x, int Q,
                               const double* func, double* out) {
    if (Q < 0 || Q > kLooMaxFunc) return -1;
    std::vector<double> e;
    for (int64_t i = 0; i < n; ++i) {
        double a1, a2;
        out[LXF_K * n + i] = star_weights(lnl + i * S, S, r_eff, e, a1, a2);
        out[LXF_NEFF * n + i] = r_eff * (a1 * a1) / a2;
        for (int rr = 0; rr < R; ++rr) out[(LXF_ROWS + rr) * n + i] = expect(e, a1, x + (i * R + rr) * S, 1);
        for (int q = 0; q < Q; ++q) out[(LXF_ROWS + R + q) * n + i] = expect(e, a1, func + q, Q);
    }
    return 0;
}

// the whole call from records and derived sample rows: out[2 + 4 (+ 1 with mix)][n], rows in LooxRow order after lnL
extern "C" int emul_loo_expect_model(int model, int free_centre, int mix, int f32, int64_t n, const double* recs,
                                     const double* wrows, int64_t S, double r_eff, double* out) {
    return dispatch_any_model(model, free_centre != 0, [&](auto M, auto FREE) {
        constexpr int MODEL = decltype(M)::value;
        constexpr bool kFree = decltype(FREE)::value;
        if constexpr (bg_kind(MODEL) == BG_GAUSS) {
            if (mix) { run_precision<MODEL, kFree, true>(f32, n, recs, wrows, S, r_eff, out); return 0; }
        }
        if (mix) return -1;
        run_precision<MODEL, kFree, false>(f32, n, recs, wrows, S, r_eff, out);
        return 0;
    }, -1);
}

extern "C" int64_t emul_psis_tile_stars_rows(int64_t n, int64_t S, int64_t rows, int64_t fixed, int64_t budget) {
    return psis_tile_stars_rows(n, S, rows, fixed, budget);
}

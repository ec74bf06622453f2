// TEST INFRASTRUCTURE ONLY -- compiles the per-star PSIS-LOO arithmetic of mcd_psis_loo (csrc/mcd_psis.h on top of
// csrc/mcd_math.h) for the CPU: the same tail length, key / tie rule, GPD fit pieces and smoothing as psis_tail_kernel
// (csrc/mcd_psis.hip), with a serial sort and serial sums in place of the wave's radix select and reductions.  Never
// loaded by the product package.
#include <algorithm>
#include <cstdint>
#include <vector>

#include "mcd_psis.h"

using namespace mcd;

namespace {

// x ascending, length M: k (unadjusted), sigma; returns k^ (gpd_adjust; +inf for a failed fit)
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

void one_star(const double* lnl, int64_t S, double r_eff, double* o4) {
    const int64_t M = psis_tail_len(S, r_eff);
    double rmax = -INFINITY, lmax = -INFINITY;
    for (int64_t s = 0; s < S; ++s) {
        rmax = max_(rmax, -lnl[s]);
        lmax = max_(lmax, lnl[s]);
    }
    std::vector<double> lw((size_t)S);
    for (int64_t s = 0; s < S; ++s) lw[s] = -lnl[s] - rmax;
    double khat = INFINITY;
    std::vector<char> in_tail((size_t)S, 0);
    std::vector<int64_t> order((size_t)S);
    if (M >= 5) {
        for (int64_t s = 0; s < S; ++s) order[s] = s;
        std::sort(order.begin(), order.end(), [&](int64_t a, int64_t b) {
            const uint64_t ka = psis_key(lw[a]), kb = psis_key(lw[b]);
            return ka < kb || (ka == kb && a < b);
        });
        const int64_t first = S - M;                                 // sorted position of the tail's first entry
        const double cutoff = lw[order[first - 1]];
        const double ec = exp_(cutoff);
        for (int64_t t = 0; t < M; ++t) in_tail[order[first + t]] = 1;
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
    double mw = -INFINITY, m2 = -INFINITY;
    for (int64_t s = 0; s < S; ++s) {
        lw[s] = lw[s] < 0.0 ? lw[s] : 0.0;
        mw = max_(mw, lw[s]);
        m2 = max_(m2, lw[s] + lnl[s]);
    }
    double a1 = 0.0, a2 = 0.0, a3 = 0.0, a4 = 0.0;
    for (int64_t s = 0; s < S; ++s) {
        const double e = exp_(lw[s] - mw);
        a1 += e;
        a2 += e * e;
        a3 += exp_(lw[s] + lnl[s] - m2);
        a4 += exp_(lnl[s] - lmax);
    }
    o4[PSF_ELPD] = (m2 + log_(a3)) - (mw + log_(a1));
    o4[PSF_K] = khat;
    o4[PSF_LPPD] = lmax + (log_(a4) - log_((double)S));
    o4[PSF_NEFF] = r_eff * (a1 * a1) / a2;
}

}  // namespace

// lnl: [n][S] -> out[4][n] = elpd_loo, pareto_k, lppd, n_eff
extern "C" int emul_psis(int64_t n, int64_t S, const double* lnl, double r_eff, double* out) {
    for (int64_t i = 0; i < n; ++i) {
        double o4[4];
        one_star(lnl + i * S, S, r_eff, o4);
        for (int f = 0; f < 4; ++f) out[f * n + i] = o4[f];
    }
    return 0;
}

// the GPD fit alone: x ascending, length M -> k^, sigma
extern "C" double emul_gpd_fit(const double* x, int64_t M, double* sigma) { return gpd_fit(x, M, *sigma); }

// the order-preserving key the select works on
extern "C" uint64_t emul_psis_key(double v) { return psis_key(v); }

extern "C" int64_t emul_psis_tail_len(int64_t S, double r_eff) { return psis_tail_len(S, r_eff); }

extern "C" int64_t emul_psis_tile_stars(int64_t n, int64_t S, int64_t fixed, int64_t budget) {
    return psis_tile_stars(n, S, fixed, budget);
}

// CPU build of the chain diagnostics (csrc/mcd_diag.h) for the tests: the same text the device kernels and the library's
// host code compile.  Loaded by tests/diag_helper.py.
#include <cstdint>
#include <vector>

#include "mcd_diag.h"

using namespace mcd;

// groups [g0, g0 + ng) of chain [T][G][W][P]; outputs indexed by the absolute (g, p), rho [G][P][L + 1] or null
extern "C" int emul_diag_groups(int64_t T, int64_t G, int64_t W, int P, int64_t L, double c, int64_t g0, int64_t ng,
                                const double* chain, double* tau, int64_t* window, int32_t* found, double* rhat, double* mean,
                                double* var, double* rho) {
    if (T < 2 || L < 1 || L > T - 1 || g0 < 0 || g0 + ng > G) return -1;
    std::vector<double> a((size_t)((L + 1) * W * P)), mom((size_t)(kDiagMoments * W * P));
    diag_host_groups(chain, T, G, W, P, L, c, g0, ng, a.data(), mom.data(), tau, window, found, rhat, mean, var, rho);
    return 0;
}

// a_k of ONE series by the walk in blocks of kDiagLags lags, k = 0 .. L
extern "C" void emul_diag_lag_sums(const double* x, int64_t stride, int64_t T, int64_t L, double* a) {
    double mom[kDiagMoments];
    diag_series_moments(x, stride, T, mom, 1);
    for (int64_t k0 = 0; k0 <= L; k0 += kDiagLags) {
        double acc[kDiagLags];
        diag_lag_walk(x, stride, T, mom[DM_X0], mom[DM_MEAN], k0, acc);
        for (int64_t j = 0; j < kDiagLags && k0 + j <= L; ++j) a[k0 + j] = acc[j];
    }
}

extern "C" int64_t emul_diag_tile_groups(int64_t T, int64_t G, int64_t W, int P, int64_t L, int64_t budget) {
    return diag_tile_groups(T, G, W, P, L, budget);
}

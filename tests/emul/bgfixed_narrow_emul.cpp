// CPU build of the narrow-range MODEL_BGFIXED chunk arithmetic on the exponent-biased table (csrc/mcd_math.h:
// exp_tab_bias, exp_tab_scaled, chunk_bgfixed_fast<.., TAB_BIASED>), next to the same chunk on the plain sqrt(2) table.
// Test infrastructure only (tests/test_bgfixed_narrow_loop.py).
#include <cstdint>

#include "mcd_math.h"

using namespace mcd;

static const double kTab[kExpTabSize] = {MCD_EXP_TABLE_SQRT2_VALUES};

extern "C" {

// out[4 w + i] for walker row w (KD doubles) over `count` BGFIXED fixed-centre records (8 doubles each):
//   i = 0 narrow on the plain table, 1 narrow on the biased table, 2 general on the plain table, 3 general on the biased one
int emul_bgfixed_biased(int64_t count, const double* recs, int64_t n_walkers, const double* walkers, double* out) {
    double biased[kExpTabSize];
    for (int j = 0; j < kExpTabSize; ++j) biased[j] = exp_tab_bias(kTab[j], j);
    for (int64_t w = 0; w < n_walkers; ++w) {
        WalkerConsts<double> c;
        c.load(walkers + w * KD);
        bool den;
        const int n = (int)count;
        out[4 * w + 0] = chunk_loglike<MODEL_BGFIXED, false, double, double, 2, true>(recs, n, c, den, kTab);
        out[4 * w + 1] = chunk_loglike<MODEL_BGFIXED, false, double, double, 2, true, true>(recs, n, c, den, biased);
        out[4 * w + 2] = chunk_loglike<MODEL_BGFIXED, false, double, double, 1, true>(recs, n, c, den, kTab);
        out[4 * w + 3] = chunk_loglike<MODEL_BGFIXED, false, double, double, 1, true, true>(recs, n, c, den, biased);
    }
    return 0;
}

// e^u term by term: ldexp(exp_tab(u), e) on the plain table (out[2 i]) and exp_tab_scaled on the biased one (out[2 i + 1])
int emul_exp_scaled(int64_t n, const double* u, double* out) {
    double biased[kExpTabSize];
    for (int j = 0; j < kExpTabSize; ++j) biased[j] = exp_tab_bias(kTab[j], j);
    for (int64_t i = 0; i < n; ++i) {
        int k;
        const double er = exp_tab<false>(u[i], k, kTab);
        out[2 * i] = std::ldexp(er, k);
        out[2 * i + 1] = exp_tab_scaled<false>(u[i], biased);
    }
    return 0;
}
}

// CPU build of the bounded sub-variant of the narrow-range MODEL_BGFIXED loop (csrc/mcd_math.h: chunk_bgfixed_fast<.., BOUNDED>,
// exp_tab_scaled<.., false>) and of its host guard (csrc/mcd_guard.h: bounded_rescale), next to the level-2 loop it replaces.
// Test infrastructure only (tests/test_bgfixed_bounded.py).
#include <cstdint>

#include "mcd_guard.h"

using namespace mcd;

static const double kTab[kExpTabSize] = {MCD_EXP_TABLE_SQRT2_VALUES};

static void biased_table(double* out) {
    for (int j = 0; j < kExpTabSize; ++j) out[j] = exp_tab_bias(kTab[j], j);
}

extern "C" {

// R of the bounded verdict (0: level 2 as is) for a fixed-centre MODEL_BGFIXED catalogue and a 4-column parameter table;
// info = nbp_min, nbp_max, pm_max, n_min, d_max, level
int emul_bounded_verdict(int64_t n, const double* v, const double* verr, const double* lnbg, const double* pmember,
                         const double* params, int64_t n_rows, double* info) {
    const CatalogStats st = compute_stats(n, v, verr, lnbg, pmember, nullptr, BG_FIXED);
    const ParamRanges pr = table_ranges(MODEL_BGFIXED, false, 4, params, n_rows);
    GuardRanges g;
    guard_verdict(st, MODEL_BGFIXED, false, n_rows, pr, &g);
    info[0] = st.nbp_min; info[1] = st.nbp_max; info[2] = st.pm_max; info[3] = g.n_min; info[4] = g.d_max;
    info[5] = level_verdict(st, MODEL_BGFIXED, false, n_rows, pr);
    return bounded_rescale(st, MODEL_BGFIXED, false, n_rows, pr);
}

// Every (star, walker) term with the arithmetic of BgFixedAcc::add<true, true, true, true, false>: the smallest k of the
// exponent (out_k[0]) and the range of the mixture values y (out_y[0], out_y[1]) over `count` fixed-centre records.
int emul_bounded_terms(int64_t count, const double* recs, int64_t n_walkers, const double* walkers, int32_t* out_k,
                       double* out_y) {
    double biased[kExpTabSize];
    biased_table(biased);
    constexpr int ND = record_doubles(MODEL_BGFIXED, false), XB = geometry_doubles(MODEL_BGFIXED, false);
    int kmin = 0x7fffffff;
    double ylo = kInfinity, yhi = -kInfinity;
    for (int64_t w = 0; w < n_walkers; ++w) {
        WalkerConsts<double> c;
        c.load(walkers + w * KD);
        const double s2x = 8.0 * c.s2;
        for (int64_t i = 0; i < count; ++i) {
            const double* r = recs + i * ND;
            double d, n;
            star_d_n<MODEL_BGFIXED, double, false, true>(r, c, d, n);
            n = fma_(8.0, r[1], s2x);
            const double g = rsqrt2_newton(n);
            const double dg = d * g;
            const double u = fnma_sgpr_addend(dg, dg, r[XB + 3]);
            int k;
            (void)exp_tab_reduce<false>(u, k);
            kmin = k < kmin ? k : kmin;
            const double y = fma_(g, exp_tab_scaled<false, false>(u, biased), r[XB + 2]);
            ylo = y < ylo ? y : ylo;
            yhi = y > yhi ? y : yhi;
        }
    }
    out_k[0] = kmin;
    out_y[0] = ylo; out_y[1] = yhi;
    return 0;
}

// out[2 w + i] for walker row w over one chunk of `count` records: i = 0 the level-2 loop (biased table, with prefetch),
// 1 the bounded loop rescaling every `rescale_iters` 8-star iterations
int emul_bounded_chunk(int64_t count, const double* recs, int64_t n_walkers, const double* walkers, int rescale_iters,
                       double* out) {
    double biased[kExpTabSize];
    biased_table(biased);
    for (int64_t w = 0; w < n_walkers; ++w) {
        WalkerConsts<double> c;
        c.load(walkers + w * KD);
        bool den;
        const int n = (int)count;
        out[2 * w] = chunk_loglike<MODEL_BGFIXED, false, double, double, 2, true, true>(recs, n, c, den, biased);
        out[2 * w + 1] = chunk_loglike<MODEL_BGFIXED, false, double, double, 2, true, true, true>(recs, n, c, den, biased,
                                                                                                  rescale_iters);
    }
    return 0;
}
}

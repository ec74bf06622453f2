// TEST INFRASTRUCTURE ONLY -- the block step of the bounded quadratic loop (option "block_step"; csrc/mcd_math.h:
// chunk_bgfixed_fast<.., BOUNDED, BLOCK>; host guard csrc/mcd_guard.h: block_step_admitted) compiled for the CPU, next to
// the bounded loop it replaces (tests/test_block_step_cpu.py).  Never loaded by the product package.
#include <cmath>
#include <cstdint>
#include <vector>

#include "mcd_chunks.h"
#include "mcd_exp_split.h"
#include "mcd_guard.h"
#include "mcd_math.h"

using namespace mcd;

static const double kTab[kExpTabSize] = {MCD_EXP_TABLE_SQRT2_VALUES};

extern "C" {

// out = {bounded_rescale, block_step_admitted} for a fixed-centre MODEL_BGFIXED catalogue and a 4-column parameter table
void emul_block_verdict(int64_t n, const double* v, const double* verr, const double* lnbg, const double* pmember,
                        const double* params, int64_t n_rows, int32_t* out) {
    const CatalogStats st = compute_stats(n, v, verr, lnbg, pmember, nullptr, BG_FIXED);
    out[0] = bounded_rescale(st, MODEL_BGFIXED, false, 4, params, n_rows);
    out[1] = block_step_admitted(st, MODEL_BGFIXED, false, 4, params, n_rows) ? 1 : 0;
}

// Sum of log y of ONE chunk (records begin .. begin + count - 1 of the n sorted records `recs`) for W walkers, as the main
// kernel calls chunk_loglike for it with the quadratic form offered: out[w] = {bounded loop, bounded loop with the block
// step}.  took[w]: 1 when the block-step call took the quadratic loop -- observed as in root_quad_emul.cpp, from a call on
// a split array whose block constants are NaN.
void emul_block_chunk(int64_t n, const double* recs, int64_t begin, int64_t count, int64_t W, const double* wpar,
                      int rescale_iters, double* out, int32_t* took) {
    constexpr int ND = record_doubles(MODEL_BGFIXED, false);
    static double tab[kExpTabSize];
    for (int j = 0; j < kExpTabSize; ++j) tab[j] = exp_tab_bias(kTab[j], j);
    std::vector<double> split((size_t)n * ND), nbf((size_t)n), e2((size_t)n);
    exp_split_records(recs, n, split.data(), nbf.data());
    for (int64_t i = 0; i < n; ++i) e2[i] = recs[i * ND + 1];
    const double cc[2] = {exp_split_chunk_const(nbf.data() + begin, count), quad_chunk_width(e2.data(), n, begin, count)};
    const QuadArgs qa = quad_args(begin, n, true);
    const double* r = recs + begin * ND;
    const double* rs = split.data() + begin * ND;
    std::vector<double> poisoned(split);
    for (int64_t i = 0; i < n; ++i) poisoned[i * ND + 6] = poisoned[i * ND + 7] = std::nan("");
    const int cnt = (int)count;
    for (int64_t w = 0; w < W; ++w) {
        WalkerConsts<double> c;
        c.load(wpar + w * KD);
        bool den;
        out[2 * w] = chunk_loglike<MODEL_BGFIXED, false, double, double, 2, true, true, true>(
                     r, cnt, c, den, tab, rescale_iters, true, true, rs, cc, qa);
        out[2 * w + 1] = chunk_loglike<MODEL_BGFIXED, false, double, double, 2, true, true, true, true>(
                         r, cnt, c, den, tab, rescale_iters, true, true, rs, cc, qa);
        took[w] = std::isnan(chunk_loglike<MODEL_BGFIXED, false, double, double, 2, true, true, true, true>(
                             r, cnt, c, den, tab, rescale_iters, true, true, poisoned.data() + begin * ND, cc, qa)) ? 1 : 0;
    }
}

}  // extern "C"

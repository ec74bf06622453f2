// TEST INFRASTRUCTURE ONLY -- the quadratic series root on 32-star bands of the level-2 BGFIXED fixed-centre loops
// (csrc/mcd_math.h: RootQuad, chunk_bgfixed_fast; csrc/mcd_exp_split.h: quad_block, quad_fill_records, quad_chunk_width;
// csrc/mcd_chunks.h: quad_thresholds) compiled for the CPU, so that its accuracy, the third vote, the block constants and
// the three loop shapes can be checked without a GPU (tests/root_quad_helper.py).  Never loaded by the product package.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <vector>

#include "mcd_chunks.h"
#include "mcd_exp_split.h"
#include "mcd_guard.h"
#include "mcd_math.h"

using namespace mcd;

static const double kTab[kExpTabSize] = {MCD_EXP_TABLE_SQRT2_VALUES};

static const double* biased_table() {
    static double biased[kExpTabSize];
    static bool made = false;
    if (!made) {
        for (int j = 0; j < kExpTabSize; ++j) biased[j] = exp_tab_bias(kTab[j], j);
        made = true;
    }
    return biased;
}

extern "C" {

double emul_quad_max_t() { return RootQuad::kMaxT; }
double emul_quad_error_bound() { return RootQuad::kErrorBound; }
double emul_quad_scale() { return kExpSplitC; }

// the scaled root of a lane with sigma^2 = s2[i] on a chunk centred on eb[i], at verr^2 = e[i] inside the block whose verr^2
// runs from e_lo[i] to e_hi[i]: quad[i] from RootQuad (the block's constants folded in), cubic[i] from RootDirectSplit
void emul_quad_root(int64_t n, const double* eb, const double* s2, const double* e_lo, const double* e_hi, const double* e,
                    double* quad, double* cubic) {
    for (int64_t i = 0; i < n; ++i) {
        RootQuadCentre c;
        c.setup_quad(eb[i], s2[i], kExpSplitC);
        const QuadBlock b = quad_block(e_lo[i], e_hi[i]);
        RootQuad q;
        q.fold(c, b.a2, b.a1, b.a0);
        quad[i] = q.g_quad(e[i]);
        RootDirectSplit d;
        d.setup_scaled(eb[i], s2[i], kExpSplitC);
        cubic[i] = d.g_direct(e[i]);
    }
}

int emul_quad_ok(double H, double eb, double s2) { return wave_all(RootQuad::quad_ok(H, eb, s2)) ? 1 : 0; }

// block constants of the sorted verr^2 column e2[0 .. n): out[b] = {a2, a1, a0, h}; returns the number of blocks
int64_t emul_quad_blocks(int64_t n, const double* e2, double* out) {
    for (int64_t b = 0; b < quad_blocks(n); ++b) {
        const QuadBlock q = quad_block_consts(e2, n, b);
        out[4 * b] = q.a2; out[4 * b + 1] = q.a1; out[4 * b + 2] = q.a0; out[4 * b + 3] = q.h;
    }
    return quad_blocks(n);
}

// the spare slots of a split array made from n records whose verr^2 is e2: slots[i] = {slot 6, slot 7} of record i
void emul_quad_slots(int64_t n, const double* e2, double* slots) {
    constexpr int ND = record_doubles(MODEL_BGFIXED, false);
    std::vector<double> rec((size_t)n * ND, 0.0), split((size_t)n * ND), nbf((size_t)n);
    for (int64_t i = 0; i < n; ++i) { rec[i * ND + 1] = e2[i]; rec[i * ND + 6] = 0.5; rec[i * ND + 7] = -3.0; }
    exp_split_records(rec.data(), n, split.data(), nbf.data());
    for (int64_t i = 0; i < n; ++i) { slots[2 * i] = split[i * ND + 6]; slots[2 * i + 1] = split[i * ND + 7]; }
}

// per chunk [cuts[c], cuts[c + 1]) of the column: H (quad_chunk_width), quad_threshold and direct_threshold; the sorted
// vectors of quad_thresholds / direct_thresholds of the same plan go to sorted_quad / sorted_direct
void emul_quad_plan(int64_t n, const double* e2, int64_t n_cuts, const int64_t* cuts, double* H, double* need_quad,
                    double* need_direct, double* sorted_quad, double* sorted_direct) {
    ChunkPlan plan;
    for (int64_t c = 0; c < n_cuts; ++c) {
        Chunk ch;
        ch.begin = cuts[c];
        ch.count = (int32_t)(cuts[c + 1] - cuts[c]);
        ch.pset = 0;
        plan.chunks.push_back(ch);
    }
    std::vector<double> nbf((size_t)n, 0.0);
    const std::vector<double> consts = exp_split_chunk_consts(plan, nbf.data(), e2, n);
    for (int64_t c = 0; c < n_cuts; ++c) {
        const double first = e2[cuts[c]], last = e2[cuts[c + 1] - 1];
        H[c] = consts[2 * c + 1];
        need_quad[c] = quad_threshold(first, last, H[c]);
        need_direct[c] = direct_threshold(first, last);
    }
    const std::vector<double> sq = quad_thresholds(plan, e2, consts.data() + 1, 2), sd = direct_thresholds(plan, e2);
    std::copy(sq.begin(), sq.end(), sorted_quad);
    std::copy(sd.begin(), sd.end(), sorted_direct);
}

// Sum of log y of ONE chunk (records begin .. begin + count - 1 of the n sorted records `recs`) for W walkers, as the main
// kernel calls chunk_loglike for it: out[w] = {4-star loop, 8-star prefetch loop, bounded loop, each with the quadratic form
// offered; the 8-star loop with the split offset only}.  took[w]: 1 when chunk_loglike itself took the quadratic loop for
// this lane -- observed, not recomputed: the same call on a split array whose block constants are NaN returns NaN exactly
// when the fold read them (no other loop touches slots 6 and 7 of the split records).
void emul_quad_chunk(int64_t n, const double* recs, int64_t begin, int64_t count, int64_t W, const double* wpar,
                     int rescale_iters, double* out, int32_t* took) {
    constexpr int ND = record_doubles(MODEL_BGFIXED, false);
    const double* tab = biased_table();
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
        out[4 * w] = chunk_loglike<MODEL_BGFIXED, false, double, double, 2, false, true>(r, cnt, c, den, tab, 1, true, true, rs, cc, qa);
        out[4 * w + 1] = chunk_loglike<MODEL_BGFIXED, false, double, double, 2, true, true>(r, cnt, c, den, tab, 1, true, true, rs, cc, qa);
        out[4 * w + 2] = chunk_loglike<MODEL_BGFIXED, false, double, double, 2, true, true, true>(r, cnt, c, den, tab, rescale_iters,
                                                                                                true, true, rs, cc, qa);
        out[4 * w + 3] = chunk_loglike<MODEL_BGFIXED, false, double, double, 2, true, true>(r, cnt, c, den, tab, 1, true, true, rs, cc);
        took[w] = std::isnan(chunk_loglike<MODEL_BGFIXED, false, double, double, 2, true, true>(r, cnt, c, den, tab, 1, true, true,
                                                                                               poisoned.data() + begin * ND, cc, qa)) ? 1 : 0;
    }
}

}  // extern "C"

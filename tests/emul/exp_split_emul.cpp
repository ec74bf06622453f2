// TEST INFRASTRUCTURE ONLY -- the split exponent offset of the direct BGFIXED loops (csrc/mcd_math.h: kExpSplitC,
// BgFixedAcc::add_gs; csrc/mcd_exp_split.h; csrc/mcd_guard.h: exp_split_admitted) compiled for the CPU, so that the record
// split, the reduced argument, the per-term error, the chunk constants and the guard can be checked without a GPU
// (tests/exp_split_helper.py).  Never loaded by the product package.
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

double emul_split_c() { return kExpSplitC; }
int emul_split_table_size() { return kExpTabSize; }
int emul_split_shift() { return kExpSplitShift; }
int emul_split_k_min_table() { return kExpTabKMin; }
int emul_split_k_min_bounded() { return kExpSplitKMinBounded; }
double emul_split_log2_kappa_max() { return kExpSplitLog2KappaMax; }

// the record split of nbp[i], omp[i]; back[i] = |(nbi + nbf) ln2/N - nbp| evaluated in long double (nbi: M's integer with
// the 5 N shift taken back)
void emul_split_record(int64_t n, const double* nbp, const double* omp, double* M, double* ompk, double* nbf, double* back) {
    for (int64_t i = 0; i < n; ++i) {
        const ExpSplitRecord s = exp_split_record(nbp[i], omp[i]);
        M[i] = s.M;
        ompk[i] = s.ompk;
        nbf[i] = s.nbf;
        const long double nbi = (long double)s.M - (long double)kExpSplitMagic + (long double)(kExpSplitShift * kExpTabSize);
        back[i] = (double)fabsl((nbi + (long double)s.nbf) * kExpSplitStepL - (long double)nbp[i]);
    }
}

// k and rv of exp_split_reduce
void emul_split_reduce(int64_t n, const double* dgs, const double* M, int32_t* k, double* rv) {
    for (int64_t i = 0; i < n; ++i) {
        int kk;
        rv[i] = exp_split_reduce(dgs[i], M[i], kk);
        k[i] = kk;
    }
}

// One term per sample through the kernels' own code (the exponent-biased table, with the clamp): a chunk centred on eb[i]
// for sigma^2 = s2[i], a star with verr^2 = e[i], residual d[i], offset nbp[i] and omp[i] = 1 - p.  err[0][i]: relative
// error of the parent's direct form (RootDirect + add_g), err[1][i]: of the split form (RootDirectSplit + add_gs) with
// kappa divided out in long double, both against y = omp + (e + s2)^(-1/2) e^{nbp - d^2 / (2 (e + s2))} in long double.
void emul_split_term_error(int64_t n, const double* eb, const double* s2, const double* e, const double* d, const double* nbp,
                           const double* omp, double* err_parent, double* err_split) {
    const double* tab = biased_table();
    for (int64_t i = 0; i < n; ++i) {
        const long double nn = (long double)e[i] + (long double)s2[i];
        const long double want = (long double)omp[i] + expl((long double)nbp[i] - (long double)d[i] * d[i] / (2.0L * nn)) / sqrtl(nn);
        RootDirect sd;
        sd.setup(eb[i], s2[i]);
        BgFixedAcc a;
        a.init();
        a.add_g<true, true, true, true, true>(d[i], sd.g_direct(e[i]), omp[i], nbp[i], tab);
        err_parent[i] = (double)fabsl(((long double)a.l.p - want) / want);
        RootDirectSplit ss;
        ss.setup_scaled(eb[i], s2[i], kExpSplitC);
        const ExpSplitRecord r = exp_split_record(nbp[i], omp[i]);
        BgFixedAcc b;
        b.init();
        b.add_gs<true, true>(d[i], ss.g_direct(e[i]), r.M, r.ompk, kExpSplitS1, tab);
        const long double kappa = ((long double)kExpSplitC / (1 << kExpSplitShift)) * expl(-(long double)r.nbf * kExpSplitStepL);
        err_split[i] = (double)fabsl(((long double)b.l.p / kappa - want) / want);
    }
}

// the chunk constants of an array of n stars with offsets nbp cut at `cuts` (n_cuts + 1 ascending positions, 0 .. n)
void emul_split_chunk_consts(int64_t n, const double* nbp, int64_t n_cuts, const int64_t* cuts, double* consts, double* nbf) {
    for (int64_t i = 0; i < n; ++i) nbf[i] = exp_split_record(nbp[i], 0.5).nbf;
    for (int64_t c = 0; c < n_cuts; ++c) consts[c] = exp_split_chunk_const(nbf + cuts[c], cuts[c + 1] - cuts[c]);
}

// sum of log y of ONE chunk of `count` (sorted) records for W walkers, every lane taking the direct form: the
// prefetching level-2 loop (8-star iterations, a 4-star group, single stars) and the bounded loop, each in the parent's
// direct form and with the split offset.  out[w][0..3] = {level-2 direct, level-2 split, bounded direct, bounded split}
void emul_split_chunk(int64_t count, const double* recs, int64_t W, const double* wpar, int rescale_iters, double* out) {
    constexpr int ND = record_doubles(MODEL_BGFIXED, false);
    const double* tab = biased_table();
    std::vector<double> split((size_t)count * ND), nbf((size_t)count);
    exp_split_records(recs, count, split.data(), nbf.data());
    const double cc = exp_split_chunk_const(nbf.data(), count);
    for (int64_t w = 0; w < W; ++w) {
        WalkerConsts<double> c;
        c.load(wpar + w * KD);
        bool den;
        const int n = (int)count;
        out[4 * w] = chunk_loglike<MODEL_BGFIXED, false, double, double, 2, true, true>(recs, n, c, den, tab, 1, true, true);
        out[4 * w + 1] = chunk_loglike<MODEL_BGFIXED, false, double, double, 2, true, true>(recs, n, c, den, tab, 1, true, true,
                                                                                          split.data(), &cc);
        out[4 * w + 2] = chunk_loglike<MODEL_BGFIXED, false, double, double, 2, true, true, true>(recs, n, c, den, tab,
                                                                                                rescale_iters, true, true);
        out[4 * w + 3] = chunk_loglike<MODEL_BGFIXED, false, double, double, 2, true, true, true>(recs, n, c, den, tab,
                                                                                                rescale_iters, true, true,
                                                                                                split.data(), &cc);
    }
}

// The guard on the statistics of a fixed-centre MODEL_BGFIXED catalogue and a 4-column parameter table, with nbp_max
// replaced (r_hi2 > 0) by the value that puts 32 hi2 of bounded_rescale at r_hi2:
// out = {bounded_rescale, exp_split_admitted for that loop, exp_split_admitted for the loops that keep the clamp}
void emul_split_guard(int64_t n, const double* v, const double* verr, const double* lnbg, const double* pmember,
                      const double* params, int64_t n_rows, double r_hi2, int32_t* out) {
    CatalogStats st = compute_stats(n, v, verr, lnbg, pmember, nullptr, BG_FIXED);
    const ParamRanges pr = table_ranges(MODEL_BGFIXED, false, 4, params, n_rows);
    if (r_hi2 > 0.0) {
        GuardRanges g;
        guard_verdict(st, MODEL_BGFIXED, false, n_rows, pr, &g);
        st.nbp_max = std::log((std::exp2(r_hi2 / 32.0) - 1.0) * std::sqrt(g.n_min));
    }
    out[0] = bounded_rescale(st, MODEL_BGFIXED, false, n_rows, pr);
    out[1] = exp_split_admitted(st, MODEL_BGFIXED, false, n_rows, pr, out[0]) ? 1 : 0;
    out[2] = exp_split_admitted(st, MODEL_BGFIXED, false, n_rows, pr, 0) ? 1 : 0;
}

}  // extern "C"

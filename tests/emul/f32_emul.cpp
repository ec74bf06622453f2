// TEST INFRASTRUCTURE ONLY -- CPU build of the float32 instantiations of the main kernel's per-chunk arithmetic
// (csrc/mcd_math.h: chunk_loglike<MODEL, FREE, float, float | double, 0 | 1>: chunk_plain / chunk_plain_mixture,
// chunk_const_f32, chunk_mixture_f32 with ConstAccF, BgFixedAccF, BgGaussAccF), so that their tails (single stars, the lone
// 4-star tree, the per-star rescale, finish(count)) can be held to the 80-bit oracle without a GPU
// (tests/test_f32_emul_cpu.py), and of the per-star terms and posterior summaries of a float32 catalogue
// (star_components<..., float>, posterior_term<..., float> through PostAcc; tests/test_f32_terms_cpu.py).  Never loaded by
// the product package.
//
// Where the device has v_rcp_f32 / v_rsq_f32 / v_exp_f32 (1 ulp) this build has the division, 1 / sqrt and libm's exp
// (mcd_math.h: MCD_ON_DEVICE): the same formulation, not the same bits.
#include <cstdint>
#include <vector>

#include "mcd_chunks.h"
#include "mcd_dispatch.h"
#include "mcd_math.h"
#include "mcd_posterior.h"

using namespace mcd;

// recs / wpar: the float64 records and walker constants of emul_helper.pack_records / pack_walkers.  Each field is rounded
// to float here, as prepare_records_kernel<float> and walker_constants<float> round the float64 expressions they evaluate.
template <int MODEL, bool FREE, class A, int FAST>
static void run(int64_t n, const double* recs, const double* wpar, int64_t W, int64_t chunk_len, double* out) {
    constexpr int ND = record_doubles(MODEL, FREE);
    constexpr int BG = bg_kind(MODEL);
    std::vector<float> rf((size_t)(n * ND));
    for (int64_t i = 0; i < n * ND; ++i) rf[i] = (float)recs[i];
    double bg_sum = 0.0;
    if (FAST && (BG == BG_FIXED || BG == BG_FIXED_DENSITY)) {
        // Walker-independent sum of lnL_bg, which the fast mixtures leave out.  The library forms it ONCE PER CATALOGUE ON THE
        // HOST from the caller's float64 column -- mcd_api_catalog.hip: pset_background_sums (mcd_chunks.h, Neumaier-
        // compensated), whatever the catalogue's precision -- and the reduce kernel adds it: it is NOT a sum over the
        // float32 records.  The same function on the same unrounded column here.
        constexpr int XB = geometry_doubles(MODEL, FREE);
        std::vector<double> lnbg((size_t)n);
        for (int64_t i = 0; i < n; ++i) lnbg[i] = recs[i * ND + XB];
        bg_sum = pset_background_sums(lnbg.data(), std::vector<int64_t>{0, n}, 0, n)[0];
    }
    for (int64_t w = 0; w < W; ++w) {
        float wf[KD];
        for (int j = 0; j < KD; ++j) wf[j] = (float)wpar[w * KD + j];
        WalkerConsts<float> c;
        c.load(wf);
        double total = 0.0;                               // the partial sums of the chunks are float64 on the device too
        for (int64_t s = 0; s < n; s += chunk_len) {
            const int count = (int)((n - s) < chunk_len ? (n - s) : chunk_len);
            bool denormal;                                // never set by the float32 forms: they have no re-run
            total += chunk_loglike<MODEL, FREE, float, A, FAST>(rf.data() + s * ND, count, c, denormal, nullptr);
        }
        out[w] = total + bg_sum;
    }
}

// ---- the per-star terms and the per-star posterior summaries of a float32 catalogue (tests/test_f32_terms_cpu.py) ----------
// star_components<MODEL, FREE, float> -> gauss_lnl<float> / mixture_lnl<float>: the literal float32 log-sum-exp that
// per_star_kernel (mcd_kernels.hip), posterior_slice_kernel, predictive_slice_kernel, psis_term_kernel and loox_term_kernel
// run on a float32 catalogue.  per_star_kernel's body lives in a .hip unit; its two modes are restated here word for word
// (as mcd_posterior.h: posterior_term restates mode 0).

template <int MODEL, bool FREE>
static void round_inputs(int64_t n, const double* recs, const double* wrows, int64_t S, std::vector<float>& rf,
                         std::vector<WalkerConsts<float>>& w) {
    constexpr int ND = record_doubles(MODEL, FREE);
    rf.resize((size_t)(n * ND));
    for (int64_t i = 0; i < n * ND; ++i) rf[i] = (float)recs[i];
    w.resize((size_t)S);
    for (int64_t s = 0; s < S; ++s) {
        float wf[KD];
        for (int j = 0; j < KD; ++j) wf[j] = (float)wrows[s * KD + j];
        w[s].load(wf);
    }
}

// out_l, out_p [S][n]: per_star_kernel<MODEL, FREE, float> mode 1 and mode 0 of every (sample row, star); the models
// without a background (which the API refuses) give the Gaussian term and p = 1.
template <int MODEL, bool FREE>
static void per_star_f32(int64_t n, const double* recs, const double* wrows, int64_t S, double* out_l, double* out_p) {
    constexpr int ND = record_doubles(MODEL, FREE);
    std::vector<float> rf;
    std::vector<WalkerConsts<float>> w;
    round_inputs<MODEL, FREE>(n, recs, wrows, S, rf, w);
    for (int64_t s = 0; s < S; ++s)
        for (int64_t i = 0; i < n; ++i) {
            float lc, lb, m;
            star_components<MODEL, FREE, float>(rf.data() + i * ND, w[s], lc, lb, m);
            if constexpr (bg_kind(MODEL) == BG_NONE) {
                out_l[s * n + i] = (double)lc;
                out_p[s * n + i] = 1.0;
            } else {
                out_l[s * n + i] = (double)mixture_lnl(lc, lb, m);                              // mode 1
                const float shift = is_profile(MODEL) ? max_(lc, lb) : 0.0f;                    // mode 0
                const float ec = m * exp_(lc - shift), eb = (1.0f - m) * exp_(lb - shift);
                out_p[s * n + i] = (double)(ec / (ec + eb));
            }
        }
}

extern "C" int emul_per_star_f32(int model, int free_centre, int64_t n, const double* recs, const double* wrows, int64_t S,
                                 double* out_l, double* out_p) {
    return dispatch_model(model, free_centre != 0, [&](auto M, auto FREE) {
        per_star_f32<decltype(M)::value, decltype(FREE)::value>(n, recs, wrows, S, out_l, out_p);
        return 0;
    }, -1);
}

// out[4][n] = lppd, lnl_var, pmem_mean, pmem_std: posterior_term<..., float> folded through PostAcc with posterior_slices'
// plan, the slices merged in order (posterior_slice_kernel / posterior_merge_kernel, one pass).
template <int MODEL, bool FREE, bool MEM>
static void posterior_f32(int64_t n, const double* recs, const double* wrows, int64_t S, double* out) {
    constexpr int ND = record_doubles(MODEL, FREE);
    std::vector<float> rf;
    std::vector<WalkerConsts<float>> w;
    round_inputs<MODEL, FREE>(n, recs, wrows, S, rf, w);
    int64_t slice_len = 0;
    posterior_slices(n, S, &slice_len);
    for (int64_t i = 0; i < n; ++i) {
        PostAcc acc;
        int64_t na = 0;
        for (int64_t j0 = 0; j0 < S; j0 += slice_len) {
            const int64_t count = (S - j0) < slice_len ? (S - j0) : slice_len;
            PostAcc b;
            b.init();
            for (int64_t j = 0; j < count; ++j) {
                double x, p;
                posterior_term<MODEL, FREE, MEM, float>(rf.data() + i * ND, w[j0 + j], x, p);
                b.add<MEM>(x, p, 1.0 / (double)(j + 1));
            }
            if (na == 0) acc = b;
            else acc.merge<MEM>(b, (double)na, (double)count);
            na += count;
        }
        acc.finish((double)S, out[0 * n + i], out[1 * n + i], out[2 * n + i], out[3 * n + i]);
    }
}

extern "C" int emul_posterior_f32(int model, int free_centre, int mem, int64_t n, const double* recs, const double* wrows,
                                  int64_t S, double* out) {
    return dispatch_model(model, free_centre != 0, [&](auto M, auto FREE) {
        constexpr int MODEL = decltype(M)::value;
        constexpr bool kFree = decltype(FREE)::value;
        if constexpr (bg_kind(MODEL) != BG_NONE) {
            if (mem) { posterior_f32<MODEL, kFree, true>(n, recs, wrows, S, out); return 0; }
        }
        if (mem) return -1;
        posterior_f32<MODEL, kFree, false>(n, recs, wrows, S, out);
        return 0;
    }, -1);
}

// fast: 0 the plain float32 kernels, else the float32 fast formulations; acc64: sums and products in double (MCD_F32_ACC64)
// or in float (MCD_F32).  -1 for the double models (float64 only) and unknown models.
extern "C" int emul_loglike_f32(int model, int free_centre, int fast, int acc64, int64_t n, const double* recs,
                                const double* wpar, int64_t W, int64_t chunk_len, double* out) {
    if (chunk_len <= 0) return -1;
    return dispatch_model(model, free_centre != 0, [&](auto M, auto FREE) {
        constexpr int MODEL = decltype(M)::value;
        constexpr bool kFree = decltype(FREE)::value;
        if (fast && acc64) run<MODEL, kFree, double, 1>(n, recs, wpar, W, chunk_len, out);
        else if (fast) run<MODEL, kFree, float, 1>(n, recs, wpar, W, chunk_len, out);
        else if (acc64) run<MODEL, kFree, double, 0>(n, recs, wpar, W, chunk_len, out);
        else run<MODEL, kFree, float, 0>(n, recs, wpar, W, chunk_len, out);
        return 0;
    }, -1);
}

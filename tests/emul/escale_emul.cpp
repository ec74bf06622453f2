// TEST INFRASTRUCTURE ONLY -- the host build of the error-scale models' arithmetic (models 10 and 11) and of their base
// models' through the same entry points: the launchers' dispatcher (csrc/mcd_dispatch.h: dispatch_launch_model),
// walker_constants (csrc/mcd_prep.h), star_d_n in its plain and fast general forms through chunk_loglike (csrc/mcd_math.h),
// grad_term (csrc/mcd_grad.h) and the guard (csrc/mcd_guard.h).  Never loaded by the product package.
#include <cmath>
#include <cstdint>

#include "mcd_dispatch.h"
#include "mcd_grad.h"
#include "mcd_guard.h"
#include "mcd_math.h"

// mcd_prep.h is device text (walker_constants runs in the prep kernel and in the resident chains); the host pass reads the
// same lines with the two qualifiers taken out and glibc's sincos
#define __device__
#define __forceinline__ inline
#include "mcd_prep.h"
#undef __device__
#undef __forceinline__

using namespace mcd;

static const double kExpTabHost[kExpTabSize] = {MCD_EXP_TABLE_VALUES};

extern "C" int escale_emul_kd() { return KD; }
extern "C" int escale_emul_slot() { return W_ES2; }
extern "C" int escale_emul_counts(int which) { return which == 0 ? kNumModels : which == 1 ? kNumAllModels : kNumLaunchModels; }
extern "C" int escale_emul_is_profile(int model) { return is_profile(model) ? 1 : 0; }
extern "C" int escale_emul_is_escale(int model) { return is_escale(model) ? 1 : 0; }
extern "C" int escale_emul_cluster_columns(int model) { return cluster_columns(model); }
extern "C" int escale_emul_bg_kind(int model) { return bg_kind(model); }
extern "C" int escale_emul_columns(int model, int free_centre) { return grad_columns(model, free_centre != 0); }
extern "C" int escale_emul_record_doubles(int model, int free_centre) { return record_doubles(model, free_centre != 0); }
extern "C" int escale_emul_grad_max_columns() { return kGradMaxColumns; }
extern "C" int escale_emul_range_doubles() { return kRangeDoubles; }

// M * 2 + FREE of the pair the dispatcher calls the functor with, or `fallback`; *calls counts the calls.
// which: 0 dispatch_launch_model (every launcher's), 1 dispatch_any_model
extern "C" int escale_emul_dispatch(int which, int model, int free_centre, int fallback, int* calls) {
    auto f = [&](auto M, auto FREE) {
        ++*calls;
        return decltype(M)::value * 2 + (decltype(FREE)::value ? 1 : 0);
    };
    return which == 0 ? dispatch_launch_model(model, free_centre != 0, f, fallback)
                      : dispatch_any_model(model, free_centre != 0, f, fallback);
}

// walker_constants of every row: params [W][k] -> wpar [W][KD]
extern "C" void escale_emul_walkers(int model, int free_centre, int k, int64_t W, const double* params, double* wpar) {
    for (int64_t w = 0; w < W; ++w) walker_constants<double>(params + w * k, model, free_centre != 0, wpar + w * KD);
}

// out[w] = log-likelihood of walker row w; fast: 0 the plain form, 1 the fast form.  Chunks of chunk_len stars are summed on
// their own and added in chunk order.
extern "C" int escale_emul_loglike(int model, int free_centre, int fast, int64_t n, const double* recs, const double* wpar,
                                   int64_t W, int64_t chunk_len, double* out) {
    if (bg_kind(model) != BG_NONE) return -1;
    return dispatch_launch_model(model, free_centre != 0, [&](auto M, auto FREE) {
        constexpr int MODEL = decltype(M)::value;
        constexpr bool kFree = decltype(FREE)::value;
        if constexpr (bg_kind(MODEL) != BG_NONE) {
            return -1;
        } else {
            constexpr int ND = record_doubles(MODEL, kFree);
            for (int64_t w = 0; w < W; ++w) {
                WalkerConsts<double> c;
                c.load(wpar + w * KD);
                double total = 0.0;
                for (int64_t s = 0; s < n; s += chunk_len) {
                    const int count = (int)((n - s) < chunk_len ? (n - s) : chunk_len);
                    bool denormal = false;
                    if (fast) total += chunk_loglike<MODEL, kFree, double, double, 1>(recs + s * ND, count, c, denormal, kExpTabHost);
                    else total += chunk_loglike<MODEL, kFree, double, double, 0>(recs + s * ND, count, c, denormal, kExpTabHost);
                }
                out[w] = total;
            }
            return 0;
        }
    }, -1);
}

// d[i], nn[i] and the plain Gaussian term l[i] of every star for ONE walker row; fast: star_d_n's FASTMATH form
extern "C" int escale_emul_terms(int model, int free_centre, int fast, int64_t n, const double* recs, const double* wrow,
                                 double* d, double* nn, double* l) {
    return dispatch_launch_model(model, free_centre != 0, [&](auto M, auto FREE) {
        constexpr int MODEL = decltype(M)::value;
        constexpr bool kFree = decltype(FREE)::value;
        constexpr int ND = record_doubles(MODEL, kFree);
        WalkerConsts<double> c;
        c.load(wrow);
        for (int64_t i = 0; i < n; ++i) {
            if (fast) star_d_n<MODEL, double, kFree, true>(recs + i * ND, c, d[i], nn[i]);
            else star_d_n<MODEL, double, kFree, false>(recs + i * ND, c, d[i], nn[i]);
            l[i] = gauss_lnl(d[i], nn[i]);
        }
        return 0;
    }, -1);
}

// out[w][0] = sum of l, out[w][1 + k] = sum of dl/dtheta_k (grad_emul.cpp's loop)
extern "C" int escale_emul_grad(int model, int free_centre, int64_t n, const double* recs, const double* wpar,
                                const double* params, int64_t W, int64_t chunk_len, double* out) {
    if (bg_kind(model) != BG_NONE) return -1;
    return dispatch_launch_model(model, free_centre != 0, [&](auto M, auto FREE) {
        constexpr int MODEL = decltype(M)::value;
        constexpr bool kFree = decltype(FREE)::value;
        constexpr int ND = record_doubles(MODEL, kFree);
        constexpr int K = grad_columns(MODEL, kFree);
        for (int64_t w = 0; w < W; ++w) {
            WalkerConsts<double> c;
            c.load(wpar + w * KD);
            GradRaw<double> q;
            q.template load<MODEL, kFree>(params + w * K);
            double total[1 + K] = {};
            for (int64_t s = 0; s < n; s += chunk_len) {
                const int count = (int)((n - s) < chunk_len ? (n - s) : chunk_len);
                double acc[1 + K] = {};
                chunk_grad<MODEL, kFree, double>(recs + s * ND, count, c, q, acc);
                for (int f = 0; f <= K; ++f) total[f] += acc[f];
            }
            for (int f = 0; f <= K; ++f) out[w * (1 + K) + f] = total[f];
        }
        return 0;
    }, -1);
}

// the library's launch level for a parameter table (csrc/mcd_guard.h: fast_level) with the statistics gathered as
// mcd_catalog_create gathers them for a float64 catalogue; ranges[0 .. 1] = (es2_min, es2_max) of the table
extern "C" int escale_emul_level(int model, int free_centre, int64_t n, const double* ra, const double* dec, const double* v,
                                 const double* verr, const double* lnbg, const double* pmember, const double* density,
                                 double ra_c, double dec_c, int k, const double* params, int64_t n_rows, double* ranges) {
    const CatalogStats st = compute_stats(n, v, verr, lnbg, pmember, density, bg_kind(model), is_profile(model) ? ra : nullptr,
                                          dec, free_centre == 0, ra_c, dec_c);
    const ParamRanges pr = table_ranges(model, free_centre != 0, k, params, n_rows);
    if (ranges) { ranges[0] = pr.es2_min; ranges[1] = pr.es2_max; }
    return fast_level(st, model, free_centre != 0, false, k, params, n_rows);
}

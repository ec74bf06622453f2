// mcd_api_summaries.hip -- C-ABI of the MI355X log-likelihood library (see include/mcd.h; mcd_host.h lists the host
// units): host drivers of the per-star posterior summaries (kernels: mcd_posterior.hip), of PSIS-LOO (mcd_psis.hip) and the expectations under its weights (mcd_loo_expect.hip),
// of the kernel-density background (mcd_kde.hip), and of the posterior predictive checks (mcd_predictive.hip).
#include "mcd_host.h"
#include "mcd_posterior.h"
#include "mcd_predictive.h"
#include "mcd_psis.h"

using namespace mcd::host;

namespace {

// What mcd_pointwise_posterior and mcd_psis_loo share per shard.  One pass of sample rows: `ns` rows from row `s0` on go
// to the pass buffer `d_params`, their derived rows to row `wpar_row` of `d_wpar`; `mark` (may be null) is recorded
// between the copy and the kernel.
int upload_samples(const mcd_catalog* cat, const DeviceSlot& slot, const double* params, int64_t s0, int64_t ns, int32_t k,
                   double* d_params, void* d_wpar, int64_t wpar_row, hipEvent_t mark) {
    const size_t term_bytes = cat->precision == MCD_F64 ? 8 : 4;
    MCD_HIP(hipMemcpyAsync(d_params, params + s0 * k, (size_t)ns * k * sizeof(double), hipMemcpyHostToDevice, slot.stream));
    if (mark) MCD_HIP(hipEventRecord(mark, slot.stream));
    MCD_HIP(mcd::launch_prepare_walkers(slot.stream, d_params, ns, k, cat->model, cat->free_centre, cat->precision,
                                        (char*)d_wpar + (size_t)wpar_row * mcd::KD * term_bytes));
    return MCD_OK;
}

// ... the shard's four per-star outputs [4][sh.n] to the caller's arrays (those that are not null), the wait for the
// shard's stream, and the time between the scratch's events (when it has them) added to *kernel_ms ...
int fetch_outputs(const Shard& sh, const DeviceSlot& slot, const DeviceScratch& d, const double* d_out, double* const outs[4],
                  double* kernel_ms) {
    for (int f = 0; f < 4; ++f)
        if (outs[f])
            MCD_HIP(hipMemcpyAsync(outs[f] + sh.star_begin, d_out + f * sh.n, (size_t)sh.n * sizeof(double),
                                   hipMemcpyDeviceToHost, slot.stream));
    MCD_HIP(hipStreamSynchronize(slot.stream));
    if (d.e0) {
        float ms = 0.f;
        MCD_HIP(hipEventElapsedTime(&ms, d.e0, d.e1));
        *kernel_ms += ms;
    }
    return MCD_OK;
}

// ... and, after the last shard, what mcd_last_kernel_ms reports.
void note_kernel_ms(mcd_catalog* cat, double kernel_ms) {
    if (cat->timing) {
        cat->last_kernel_ms = kernel_ms;
        cat->timing_pending = false;
    }
}

// What mcd_pointwise_posterior and mcd_posterior_predictive share: per shard, the scratch of the slice plan for `nf` state
// fields and `n_out` output fields per star, the samples in passes of posterior_pass rows through `launch` (launch_posterior's
// argument list after the shape and its flag), then `fetch(shard, slot, scratch, d_out, &kernel_ms)`.
template <class Launch, class Fetch>
int sliced_sample_passes(mcd_catalog* cat, int64_t S, int32_t k, const double* params, int nf, int n_out, Launch launch,
                         Fetch fetch) {
    const size_t term_bytes = cat->precision == MCD_F64 ? 8 : 4;
    const int64_t pass_len = std::min<int64_t>(S, cat->posterior_pass);
    const int64_t n_passes = (S + pass_len - 1) / pass_len;
    double kernel_ms = 0.0;
    for (Shard& sh : cat->shards) {
        if (sh.n == 0) continue;
        const DeviceSlot& slot = cat->ctx->slots[sh.slot];
        MCD_HIP(hipSetDevice(slot.device));
        // scratch for the longest pass and for the plan with the most slices (the first pass or the shorter last one)
        int64_t len_full = 0, len_last = 0;
        const int64_t sl_full = mcd::posterior_slices(sh.n, pass_len, &len_full);
        const int64_t sl_last = mcd::posterior_slices(sh.n, S - (n_passes - 1) * pass_len, &len_last);
        const int64_t max_slices = std::max(sl_full, sl_last), max_len = std::max(len_full, len_last);
        DeviceScratch d;                                    // (one shard's)
        double *d_params = nullptr, *d_inv = nullptr, *d_part = nullptr, *d_state = nullptr, *d_out = nullptr;
        void* d_wpar = nullptr;
        MCD_HIP(d.malloc(&d_params, (size_t)pass_len * k * sizeof(double)));
        MCD_HIP(d.malloc(&d_wpar, (size_t)pass_len * mcd::KD * term_bytes));
        MCD_HIP(d.malloc(&d_inv, (size_t)max_len * sizeof(double)));
        MCD_HIP(d.malloc(&d_part, (size_t)max_slices * nf * sh.n * sizeof(double)));
        if (n_passes > 1) MCD_HIP(d.malloc(&d_state, (size_t)nf * sh.n * sizeof(double)));
        MCD_HIP(d.malloc(&d_out, (size_t)n_out * sh.n * sizeof(double)));
        std::vector<double> inv((size_t)max_len);
        for (int64_t j = 0; j < max_len; ++j) inv[j] = 1.0 / (double)(j + 1);
        MCD_HIP(hipMemcpy(d_inv, inv.data(), inv.size() * sizeof(double), hipMemcpyHostToDevice));
        if (cat->timing) MCD_HIP(d.create_events());
        const mcd::LaunchShape shape{cat->model, cat->free_centre, cat->precision, 0};
        for (int64_t p = 0; p < n_passes; ++p) {
            const int64_t s0 = p * pass_len, ns = std::min(pass_len, S - s0);
            int64_t slice_len = 0;
            const int64_t n_slices = mcd::posterior_slices(sh.n, ns, &slice_len);
            // (every pass reuses the one pass buffer of derived rows)
            if (int rc = upload_samples(cat, slot, params, s0, ns, k, d_params, d_wpar, 0, p == 0 ? d.e0 : nullptr)) return rc;
            MCD_HIP(launch(slot.stream, shape, sh.records, sh.n, d_wpar, ns, d_inv, slice_len, n_slices, d_part, d_state, s0, S,
                           d_out));
            if (d.e1 && p == n_passes - 1) MCD_HIP(hipEventRecord(d.e1, slot.stream));
        }
        if (int rc = fetch(sh, slot, d, d_out, &kernel_ms)) return rc;
    }
    note_kernel_ms(cat, kernel_ms);
    return MCD_OK;
}

int pointwise_posterior(mcd_catalog* cat, int64_t S, int32_t k, const double* params, double* const outs[4]) {
    if (!cat || !params) return fail(MCD_ERR_INVALID, "mcd_pointwise_posterior: null catalogue or params");
    if (S < 1) return fail(MCD_ERR_INVALID, "mcd_pointwise_posterior: n_samples must be >= 1");
    if (k != cat->k) return fail(MCD_ERR_INVALID, "mcd_pointwise_posterior: parameter rows have the wrong number of columns");
    if (cat->n_psets != 1) return fail(MCD_ERR_INVALID, "mcd_pointwise_posterior: defined for un-binned catalogues only");
    const bool mem = outs[2] || outs[3];
    if (mem && mcd::bg_kind(cat->model) == mcd::BG_NONE)
        return fail(MCD_ERR_INVALID, "mcd_pointwise_posterior: membership outputs need a background model (pmem_* must be NULL)");
    if (cat->n_stars == 0 || !(outs[0] || outs[1] || mem)) return MCD_OK;
    return sliced_sample_passes(
        cat, S, k, params, mcd::post_fields(mem), 4,
        [&](hipStream_t s, const mcd::LaunchShape& shape, auto... rest) { return mcd::launch_posterior(s, shape, mem, rest...); },
        [&](const Shard& sh, const DeviceSlot& slot, const DeviceScratch& d, const double* d_out, double* kernel_ms) {
            return fetch_outputs(sh, slot, d, d_out, outs, kernel_ms);
        });
}

// out [MCD_PRED_FIELDS][n_stars], pit_mix [n_stars] or null
int posterior_predictive(mcd_catalog* cat, int64_t S, int32_t k, const double* params, double* out, double* pit_mix) {
    if (!cat || !params) return fail(MCD_ERR_INVALID, "mcd_posterior_predictive: null catalogue or params");
    if (!out) return fail(MCD_ERR_INVALID, "mcd_posterior_predictive: out must not be NULL");
    if (S < 1) return fail(MCD_ERR_INVALID, "mcd_posterior_predictive: n_samples must be >= 1");
    if (k != cat->k) return fail(MCD_ERR_INVALID, "mcd_posterior_predictive: parameter rows have the wrong number of columns");
    if (cat->n_psets != 1) return fail(MCD_ERR_INVALID, "mcd_posterior_predictive: defined for un-binned catalogues only");
    const bool mix = pit_mix != nullptr;
    if (mix && mcd::bg_kind(cat->model) != mcd::BG_GAUSS)
        return fail(MCD_ERR_INVALID, "mcd_posterior_predictive: pit_mix needs a Gaussian background model (pit_mix must be NULL)");
    if (cat->n_stars == 0) return MCD_OK;
    const int nf = mcd::pred_fields(mix);
    return sliced_sample_passes(
        cat, S, k, params, nf, nf,
        [&](hipStream_t s, const mcd::LaunchShape& shape, auto... rest) { return mcd::launch_predictive(s, shape, mix, rest...); },
        [&](const Shard& sh, const DeviceSlot& slot, const DeviceScratch& d, const double* d_out, double* kernel_ms) {
            // the shard's stars at star_begin of every field, as fetch_outputs places them; it copies pit_mix and waits
            for (int f = 0; f < MCD_PRED_FIELDS; ++f)
                MCD_HIP(hipMemcpyAsync(out + (size_t)f * cat->n_stars + sh.star_begin, d_out + (size_t)f * sh.n,
                                       (size_t)sh.n * sizeof(double), hipMemcpyDeviceToHost, slot.stream));
            double* const rest[4] = {pit_mix, nullptr, nullptr, nullptr};
            return fetch_outputs(sh, slot, d, mix ? d_out + (size_t)mcd::PO_PIT_MIX * sh.n : d_out, rest, kernel_ms);
        });
}

// Per shard: the S derived sample rows once (uploaded in passes of posterior_pass rows), then tiles of stars whose
// [star][S] terms fit the scratch budget with them: the term kernel fills the tile, the tail kernel reduces it.
int psis_loo(mcd_catalog* cat, int64_t S, int32_t k, const double* params, double r_eff, double* const outs[4]) {
    if (!cat || !params) return fail(MCD_ERR_INVALID, "mcd_psis_loo: null catalogue or params");
    if (S < 1) return fail(MCD_ERR_INVALID, "mcd_psis_loo: n_samples must be >= 1");
    if (S > INT32_MAX) return fail(MCD_ERR_INVALID, "mcd_psis_loo: n_samples must be < 2^31");
    if (!(r_eff > 0.0) || !std::isfinite(r_eff)) return fail(MCD_ERR_INVALID, "mcd_psis_loo: r_eff must be > 0 and finite");
    if (k != cat->k) return fail(MCD_ERR_INVALID, "mcd_psis_loo: parameter rows have the wrong number of columns");
    if (cat->n_psets != 1) return fail(MCD_ERR_INVALID, "mcd_psis_loo: defined for un-binned catalogues only");
    const int64_t M = mcd::psis_tail_len(S, r_eff);
    if (M > mcd::kPsisMaxTail)
        return fail(MCD_ERR_INVALID, "mcd_psis_loo: the Pareto tail of " + std::to_string(M) + " samples exceeds " +
                                         std::to_string(mcd::kPsisMaxTail) + " (S / r_eff too large)");
    if (cat->n_stars == 0 || !(outs[0] || outs[1] || outs[2] || outs[3])) return MCD_OK;
    const size_t term_bytes = cat->precision == MCD_F64 ? 8 : 4;
    const size_t rec_bytes = term_bytes * (size_t)mcd::record_doubles(cat->model, cat->free_centre);
    const int64_t pass_len = std::min<int64_t>(S, cat->posterior_pass);
    const int64_t fixed = (int64_t)((size_t)pass_len * k * sizeof(double) + (size_t)S * mcd::KD * term_bytes);
    const int64_t budget = cat->loo_scratch_mb * (int64_t)1048576;
    double kernel_ms = 0.0;
    for (Shard& sh : cat->shards) {
        if (sh.n == 0) continue;
        const int64_t tile = mcd::psis_tile_stars(sh.n, S, fixed, budget);
        if (tile < 1)
            return fail(MCD_ERR_INVALID, "mcd_psis_loo: option loo_scratch_mb = " + std::to_string(cat->loo_scratch_mb) +
                                             " cannot hold the sample table and one star's " + std::to_string(S) + " terms");
        const DeviceSlot& slot = cat->ctx->slots[sh.slot];
        MCD_HIP(hipSetDevice(slot.device));
        DeviceScratch d;                                    // (one shard's)
        double *d_params = nullptr, *d_terms = nullptr, *d_out = nullptr;
        void* d_wpar = nullptr;
        MCD_HIP(d.malloc(&d_params, (size_t)pass_len * k * sizeof(double)));
        MCD_HIP(d.malloc(&d_wpar, (size_t)S * mcd::KD * term_bytes));
        MCD_HIP(d.malloc(&d_terms, (size_t)tile * S * sizeof(double)));
        MCD_HIP(d.malloc(&d_out, (size_t)4 * sh.n * sizeof(double)));
        if (cat->timing) MCD_HIP(d.create_events());
        for (int64_t s0 = 0; s0 < S; s0 += pass_len) {      // (the passes fill the whole [S][KD] table)
            const int64_t ns = std::min(pass_len, S - s0);
            if (int rc = upload_samples(cat, slot, params, s0, ns, k, d_params, d_wpar, s0, s0 == 0 ? d.e0 : nullptr)) return rc;
        }
        const mcd::LaunchShape shape{cat->model, cat->free_centre, cat->precision, 0};
        for (int64_t t0 = 0; t0 < sh.n; t0 += tile) {
            const int64_t nt = std::min(tile, sh.n - t0);
            MCD_HIP(mcd::launch_psis(slot.stream, shape, (const char*)sh.records + (size_t)t0 * rec_bytes, nt, d_wpar, S, M,
                                     r_eff, d_terms, d_out + t0, sh.n));
        }
        if (d.e1) MCD_HIP(hipEventRecord(d.e1, slot.stream));
        if (int rc = fetch_outputs(sh, slot, d, d_out, outs, &kernel_ms)) return rc;
    }
    note_kernel_ms(cat, kernel_ms);
    return MCD_OK;
}

// mcd_psis_loo's plan with `rows` rows per star in the tile and the function table in the fixed part of the budget.
int psis_loo_expect(mcd_catalog* cat, int64_t S, int32_t k, const double* params, double r_eff, int32_t n_func,
                    const double* func, double* loo_func, double* loo_pred, double* loo_pit_mix, double* pareto_k,
                    double* n_eff) {
    if (!cat || !params) return fail(MCD_ERR_INVALID, "mcd_psis_loo_expect: null catalogue or params");
    if (S < 1) return fail(MCD_ERR_INVALID, "mcd_psis_loo_expect: n_samples must be >= 1");
    if (S > INT32_MAX) return fail(MCD_ERR_INVALID, "mcd_psis_loo_expect: n_samples must be < 2^31");
    if (!(r_eff > 0.0) || !std::isfinite(r_eff))
        return fail(MCD_ERR_INVALID, "mcd_psis_loo_expect: r_eff must be > 0 and finite");
    if (k != cat->k) return fail(MCD_ERR_INVALID, "mcd_psis_loo_expect: parameter rows have the wrong number of columns");
    if (cat->n_psets != 1) return fail(MCD_ERR_INVALID, "mcd_psis_loo_expect: defined for un-binned catalogues only");
    if (n_func < 0 || n_func > MCD_LOO_MAX_FUNC)
        return fail(MCD_ERR_INVALID, "mcd_psis_loo_expect: n_func must be in [0, " + std::to_string(MCD_LOO_MAX_FUNC) + "]");
    if (n_func > 0 && (!func || !loo_func))
        return fail(MCD_ERR_INVALID, "mcd_psis_loo_expect: func and loo_func must not be NULL when n_func > 0");
    if (loo_pit_mix && mcd::bg_kind(cat->model) != mcd::BG_GAUSS)
        return fail(MCD_ERR_INVALID,
                    "mcd_psis_loo_expect: loo_pit_mix needs a Gaussian background model (loo_pit_mix must be NULL)");
    const int64_t M = mcd::psis_tail_len(S, r_eff);
    if (M > mcd::kPsisMaxTail)
        return fail(MCD_ERR_INVALID, "mcd_psis_loo_expect: the Pareto tail of " + std::to_string(M) + " samples exceeds " +
                                         std::to_string(mcd::kPsisMaxTail) + " (S / r_eff too large)");
    if (cat->n_stars == 0 || !(n_func > 0 || loo_pred || loo_pit_mix || pareto_k || n_eff)) return MCD_OK;
    const int mode = loo_pit_mix ? mcd::LOOX_PRED_MIX : loo_pred ? mcd::LOOX_PRED : mcd::LOOX_NONE;
    const int rows = mcd::loox_rows(mode), n_out = mcd::LXF_ROWS + rows - 1 + n_func;
    const size_t term_bytes = cat->precision == MCD_F64 ? 8 : 4;
    const size_t rec_bytes = term_bytes * (size_t)mcd::record_doubles(cat->model, cat->free_centre);
    const int64_t pass_len = std::min<int64_t>(S, cat->posterior_pass);
    const size_t func_bytes = (size_t)S * n_func * sizeof(double);
    const int64_t fixed = (int64_t)((size_t)pass_len * k * sizeof(double) + (size_t)S * mcd::KD * term_bytes + func_bytes);
    const int64_t budget = cat->loo_scratch_mb * (int64_t)1048576;
    double kernel_ms = 0.0;
    for (Shard& sh : cat->shards) {
        if (sh.n == 0) continue;
        const int64_t tile = mcd::psis_tile_stars_rows(sh.n, S, rows, fixed, budget);
        if (tile < 1)
            return fail(MCD_ERR_INVALID, "mcd_psis_loo_expect: option loo_scratch_mb = " + std::to_string(cat->loo_scratch_mb) +
                                             " cannot hold the sample table and one star's " + std::to_string(rows) +
                                             " rows of " + std::to_string(S) + " terms");
        const DeviceSlot& slot = cat->ctx->slots[sh.slot];
        MCD_HIP(hipSetDevice(slot.device));
        DeviceScratch d;                                    // (one shard's)
        double *d_params = nullptr, *d_terms = nullptr, *d_out = nullptr, *d_func = nullptr;
        void* d_wpar = nullptr;
        MCD_HIP(d.malloc(&d_params, (size_t)pass_len * k * sizeof(double)));
        MCD_HIP(d.malloc(&d_wpar, (size_t)S * mcd::KD * term_bytes));
        MCD_HIP(d.malloc(&d_terms, (size_t)tile * rows * S * sizeof(double)));
        MCD_HIP(d.malloc(&d_out, (size_t)n_out * sh.n * sizeof(double)));
        if (n_func > 0) {
            MCD_HIP(d.malloc(&d_func, func_bytes));
            MCD_HIP(hipMemcpyAsync(d_func, func, func_bytes, hipMemcpyHostToDevice, slot.stream));
        }
        if (cat->timing) MCD_HIP(d.create_events());
        for (int64_t s0 = 0; s0 < S; s0 += pass_len) {      // (the passes fill the whole [S][KD] table)
            const int64_t ns = std::min(pass_len, S - s0);
            if (int rc = upload_samples(cat, slot, params, s0, ns, k, d_params, d_wpar, s0, s0 == 0 ? d.e0 : nullptr)) return rc;
        }
        const mcd::LaunchShape shape{cat->model, cat->free_centre, cat->precision, 0};
        for (int64_t t0 = 0; t0 < sh.n; t0 += tile) {
            const int64_t nt = std::min(tile, sh.n - t0);
            MCD_HIP(mcd::launch_loo_expect(slot.stream, shape, mode, (const char*)sh.records + (size_t)t0 * rec_bytes, nt, d_wpar,
                                           S, M, r_eff, d_func, n_func, d_terms, d_out + t0, sh.n));
        }
        if (d.e1) MCD_HIP(hipEventRecord(d.e1, slot.stream));
        // the shard's stars at star_begin of every field; fetch_outputs copies k^ and n_eff and waits
        auto field = [&](double* dst, int f) {
            return hipMemcpyAsync(dst + sh.star_begin, d_out + (size_t)f * sh.n, (size_t)sh.n * sizeof(double),
                                  hipMemcpyDeviceToHost, slot.stream);
        };
        if (loo_pred)
            for (int f = 0; f < MCD_LOOX_FIELDS; ++f) MCD_HIP(field(loo_pred + (size_t)f * cat->n_stars, mcd::LXF_ROWS + f));
        if (loo_pit_mix) MCD_HIP(field(loo_pit_mix, mcd::LXF_ROWS + mcd::LR_MIX - 1));
        for (int q = 0; q < n_func; ++q) MCD_HIP(field(loo_func + (size_t)q * cat->n_stars, mcd::LXF_ROWS + rows - 1 + q));
        double* const rest[4] = {pareto_k, n_eff, nullptr, nullptr};
        if (int rc = fetch_outputs(sh, slot, d, d_out, rest, &kernel_ms)) return rc;
    }
    note_kernel_ms(cat, kernel_ms);
    return MCD_OK;
}

}  // namespace

extern "C" {

int mcd_pointwise_posterior(mcd_catalog* cat, int64_t n_samples, int32_t k, const double* params, double* lppd,
                            double* lnl_var, double* pmem_mean, double* pmem_std) {
    try {
    double* const outs[4] = {lppd, lnl_var, pmem_mean, pmem_std};
    return pointwise_posterior(cat, n_samples, k, params, outs);
    } catch (...) { return on_exception("mcd_pointwise_posterior"); }
}

int mcd_psis_loo(mcd_catalog* cat, int64_t n_samples, int32_t k, const double* params, double r_eff, double* elpd_loo,
                 double* pareto_k, double* lppd, double* n_eff) {
    try {
    double* const outs[4] = {elpd_loo, pareto_k, lppd, n_eff};
    return psis_loo(cat, n_samples, k, params, r_eff, outs);
    } catch (...) { return on_exception("mcd_psis_loo"); }
}

int mcd_psis_loo_expect(mcd_catalog* cat, int64_t n_samples, int32_t k, const double* params, double r_eff,
                        int32_t n_func, const double* func, double* loo_func, double* loo_pred, double* loo_pit_mix,
                        double* pareto_k, double* n_eff) {
    try {
    return psis_loo_expect(cat, n_samples, k, params, r_eff, n_func, func, loo_func, loo_pred, loo_pit_mix, pareto_k, n_eff);
    } catch (...) { return on_exception("mcd_psis_loo_expect"); }
}

int mcd_posterior_predictive(mcd_catalog* cat, int64_t n_samples, int32_t k, const double* params, double* out,
                             double* pit_mix) {
    try {
    return posterior_predictive(cat, n_samples, k, params, out, pit_mix);
    } catch (...) { return on_exception("mcd_posterior_predictive"); }
}

int mcd_kde_background(mcd_ctx* ctx, int64_t n_comp, const double* comp, int64_t n, const double* v,
                       const double* verr, double sigma_int, double* out, double* kernel_ms) {
    try {
    if (kernel_ms) *kernel_ms = 0.0;
    if (!ctx || ctx->slots.empty()) return fail(MCD_ERR_INVALID, "kde background: null context");
    if (n < 0 || n_comp < 0) return fail(MCD_ERR_INVALID, "kde background: negative size");
    if (n == 0) return MCD_OK;
    if (n_comp == 0) return fail(MCD_ERR_INVALID, "kde background: no comparison stars");
    if (!comp || !v || !verr || !out) return fail(MCD_ERR_INVALID, "kde background: null argument");
    if (!(sigma_int == sigma_int)) return fail(MCD_ERR_INVALID, "kde background: sigma_int is NaN");
    const DeviceSlot& slot = ctx->slots[0];
    MCD_HIP(hipSetDevice(slot.device));
    int slice_len = 0;
    const int n_slices = mcd::kde_slices(n, n_comp, &slice_len);
    DeviceScratch d;
    double *d_comp = nullptr, *d_v = nullptr, *d_verr = nullptr, *d_dmin = nullptr, *d_sum = nullptr, *d_out = nullptr;
    MCD_HIP(d.malloc(&d_comp, (size_t)n_comp * sizeof(double)));
    MCD_HIP(d.malloc(&d_v, (size_t)n * sizeof(double)));
    MCD_HIP(d.malloc(&d_verr, (size_t)n * sizeof(double)));
    MCD_HIP(d.malloc(&d_dmin, (size_t)n * n_slices * sizeof(double)));
    MCD_HIP(d.malloc(&d_sum, (size_t)n * n_slices * sizeof(double)));
    MCD_HIP(d.malloc(&d_out, (size_t)n * sizeof(double)));
    MCD_HIP(d.create_events());
    MCD_HIP(hipMemcpyAsync(d_comp, comp, (size_t)n_comp * sizeof(double), hipMemcpyHostToDevice, slot.stream));
    MCD_HIP(hipMemcpyAsync(d_v, v, (size_t)n * sizeof(double), hipMemcpyHostToDevice, slot.stream));
    MCD_HIP(hipMemcpyAsync(d_verr, verr, (size_t)n * sizeof(double), hipMemcpyHostToDevice, slot.stream));
    MCD_HIP(hipEventRecord(d.e0, slot.stream));
    MCD_HIP(mcd::launch_kde(slot.stream, d_comp, n_comp, d_v, d_verr, n, sigma_int, slice_len, n_slices, d_dmin, d_sum,
                            d_out));
    MCD_HIP(hipEventRecord(d.e1, slot.stream));
    MCD_HIP(hipMemcpyAsync(out, d_out, (size_t)n * sizeof(double), hipMemcpyDeviceToHost, slot.stream));
    MCD_HIP(hipStreamSynchronize(slot.stream));
    if (kernel_ms) {
        float ms = 0.f;
        MCD_HIP(hipEventElapsedTime(&ms, d.e0, d.e1));
        *kernel_ms = ms;
    }
    return MCD_OK;
    } catch (...) { return on_exception("mcd_kde_background"); }
}

}  // extern "C"

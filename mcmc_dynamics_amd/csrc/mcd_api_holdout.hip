// mcd_api_holdout.hip -- C-ABI of the MI355X log-likelihood library (see include/mcd.h; mcd_host.h lists the host units):
// host drivers of the exact leave-out refits.  mcd_holdout_loglike: E W parameter rows against the whole catalogue in one
// launch, the sums kept apart per hold-out set (kernels: mcd_holdout.hip; rules: mcd_holdout.h).  mcd_holdout_pointwise:
// every held-out star's predictive density under its own set's samples, a host loop over the sets around the kernels of
// mcd_pointwise_posterior (mcd_posterior.hip) on the set's record range.
#include "mcd_host.h"
#include "mcd_holdout.h"
#include "mcd_posterior.h"

using namespace mcd::host;

MCD_HOST_BEGIN

static void free_holdout_work(HoldoutWork& w) {
    if (w.d_chunks) (void)hipFree(w.d_chunks);
    if (w.d_offsets) (void)hipFree(w.d_offsets);
    if (w.d_params) (void)hipFree(w.d_params);
    if (w.d_wpar) (void)hipFree(w.d_wpar);
    if (w.d_partials) (void)hipFree(w.d_partials);
    if (w.d_sums) (void)hipFree(w.d_sums);
    if (w.d_out) (void)hipFree(w.d_out);
    if (w.h_params) (void)hipHostFree(w.h_params);
    if (w.h_out) (void)hipHostFree(w.h_out);
    if (w.e0) (void)hipEventDestroy(w.e0);
    if (w.e1) (void)hipEventDestroy(w.e1);
    w = HoldoutWork();
}

// the catalogue's hold-out plans and their buffers (the device of the catalogue's one shard is current, its stream idle)
void release_holdout(mcd_catalog* cat) {
    for (auto& kv : cat->holdout) free_holdout_work(kv.second);
    cat->holdout.clear();
}

MCD_HOST_END

namespace {

// What both entry points refuse, in the order of include/mcd.h; `who` opens the message
int holdout_usable(mcd_catalog* cat, const char* who, int32_t n_sets, const int64_t* set_offsets, int64_t n_rows_per_set,
                   int32_t k) {
    const std::string name(who);
    if (int rc = ctx_usable(cat->ctx)) return rc;
    if (cat->n_psets != 1) return fail(MCD_ERR_INVALID, name + ": defined for un-binned catalogues only");
    if (cat->precision != MCD_F64) return fail(MCD_ERR_INVALID, name + ": needs an MCD_F64 catalogue");
    if (cat->ctx->has_comm() || cat->shards.size() != 1)
        return fail(MCD_ERR_INVALID, name + ": one device per process (no several devices, no communicator)");
    if (const char* why = mcd::holdout_offsets_error(n_sets, set_offsets, cat->n_stars))
        return fail(MCD_ERR_INVALID, name + ": " + why);
    if (n_rows_per_set < 1) return fail(MCD_ERR_INVALID, name + ": needs at least one parameter row per set");
    if (k != cat->k) return fail(MCD_ERR_INVALID, name + ": parameter rows have the wrong number of columns");
    return MCD_OK;
}

// The plan of (set_offsets, rows) and its buffers, from the catalogue's cache or built now
int holdout_work(mcd_catalog* cat, const Shard& sh, const std::vector<int64_t>& ranges, int32_t n_sets, int64_t n_rows,
                 HoldoutWork** out) {
    const std::pair<std::vector<int64_t>, int64_t> key(std::vector<int64_t>(ranges.begin(), ranges.begin() + n_sets + 1), n_rows);
    auto it = cat->holdout.find(key);
    if (it != cat->holdout.end()) { *out = &it->second; return MCD_OK; }
    if (cat->holdout.size() >= 8) release_holdout(cat);               // bound the cache (a refit uses one plan throughout)
    const mcd::ChunkPlan plan = mcd::plan_chunks(ranges, 0, sh.n, n_rows, cat->target_waves, cat->tail_split, {}, cat->chunk_len);
    HoldoutWork w;
    w.n_rows = n_rows;
    w.n_ranges = (int64_t)ranges.size() - 1;
    w.n_chunks = (int64_t)plan.chunks.size();
    w.max_chunks_per_range = plan.max_chunks_per_pset;
    const size_t padded = (size_t)mcd::padded_walkers(n_rows);
    // (a failure half-way releases what it got)
    auto build = [&]() -> int {
        MCD_HIP(hipMalloc(&w.d_chunks, std::max<size_t>(1, plan.chunks.size()) * sizeof(mcd::Chunk)));
        MCD_HIP(hipMalloc(&w.d_offsets, plan.offsets.size() * sizeof(int64_t)));
        MCD_HIP(hipMalloc(&w.d_params, (size_t)n_rows * cat->k * sizeof(double)));
        MCD_HIP(hipMalloc(&w.d_wpar, (size_t)n_rows * mcd::KD * sizeof(double)));
        MCD_HIP(hipMalloc(&w.d_partials, std::max<size_t>(1, padded * plan.chunks.size()) * sizeof(double)));
        MCD_HIP(hipMalloc(&w.d_sums, (size_t)w.n_ranges * n_rows * sizeof(double)));
        MCD_HIP(hipMalloc(&w.d_out, (size_t)2 * n_rows * sizeof(double)));
        MCD_HIP(hipHostMalloc(&w.h_params, (size_t)n_rows * cat->k * sizeof(double), hipHostMallocDefault));
        MCD_HIP(hipHostMalloc(&w.h_out, (size_t)2 * n_rows * sizeof(double), hipHostMallocDefault));
        MCD_HIP(hipEventCreate(&w.e0));
        MCD_HIP(hipEventCreate(&w.e1));
        if (!plan.chunks.empty())
            MCD_HIP(hipMemcpy(w.d_chunks, plan.chunks.data(), plan.chunks.size() * sizeof(mcd::Chunk), hipMemcpyHostToDevice));
        MCD_HIP(hipMemcpy(w.d_offsets, plan.offsets.data(), plan.offsets.size() * sizeof(int64_t), hipMemcpyHostToDevice));
        return MCD_OK;
    };
    if (int rc = build()) { free_holdout_work(w); return rc; }
    *out = &(cat->holdout[key] = w);
    return MCD_OK;
}

int holdout_loglike(mcd_catalog* cat, int32_t n_sets, const int64_t* set_offsets, int64_t n_walkers, int32_t k,
                    const double* params, double* train, double* test) {
    if (!cat || !params || !train) return fail(MCD_ERR_INVALID, "mcd_holdout_loglike: null catalogue, params or train");
    if (int rc = holdout_usable(cat, "mcd_holdout_loglike", n_sets, set_offsets, n_walkers, k)) return rc;
    if (n_walkers > mcd::kHoldoutMaxRows || (int64_t)n_sets * n_walkers > mcd::kHoldoutMaxRows)
        return fail(MCD_ERR_INVALID, "mcd_holdout_loglike: n_sets x n_walkers exceeds " + std::to_string(mcd::kHoldoutMaxRows));
    const int64_t n_rows = (int64_t)n_sets * n_walkers;
    const std::vector<int64_t> ranges = mcd::holdout_ranges(n_sets, set_offsets, cat->n_stars);
    const int64_t n_ranges = (int64_t)ranges.size() - 1;
    if (n_ranges * mcd::padded_walkers(n_rows) * (int64_t)sizeof(double) > mcd::kHoldoutScratchBytes)
        return fail(MCD_ERR_INVALID, "mcd_holdout_loglike: the range sums of " + std::to_string(n_ranges) + " ranges x " +
                                         std::to_string(n_rows) + " rows exceed the scratch budget of " +
                                         std::to_string(mcd::kHoldoutScratchBytes >> 20) + " MiB (fewer sets or walkers per call)");
    Shard& sh = cat->shards[0];
    const DeviceSlot& slot = cat->ctx->slots[sh.slot];
    MCD_HIP(hipSetDevice(slot.device));
    // (an earlier pipelined evaluation may still be in flight on the stream the plans are released and built on)
    MCD_WAIT(cat->ctx, slot.stream, cat->spin_us, "mcd_holdout_loglike (previous evaluation)");
    HoldoutWork* wp = nullptr;
    if (int rc = holdout_work(cat, sh, ranges, n_sets, n_rows, &wp)) return rc;
    HoldoutWork& w = *wp;
    // the gradient path's staging: params H2D, walker prep
    std::memcpy(w.h_params, params, (size_t)n_rows * k * sizeof(double));
    MCD_HIP(hipMemcpyAsync(w.d_params, w.h_params, (size_t)n_rows * k * sizeof(double), hipMemcpyHostToDevice, slot.stream));
    MCD_HIP(mcd::launch_prepare_walkers(slot.stream, w.d_params, n_rows, k, cat->model, cat->free_centre, cat->precision,
                                        w.d_wpar));
    const mcd::LaunchShape shape{cat->model, cat->free_centre, cat->precision, 0};
    if (cat->timing) MCD_HIP(hipEventRecord(w.e0, slot.stream));
    MCD_HIP(mcd::launch_holdout(slot.stream, shape, sh.records, w.d_chunks, w.n_chunks, w.d_wpar, w.d_partials, n_rows));
    if (cat->timing) MCD_HIP(hipEventRecord(w.e1, slot.stream));
    MCD_HIP(mcd::launch_holdout_reduce(slot.stream, w.d_partials, w.n_chunks, w.d_offsets, w.n_ranges, w.max_chunks_per_range,
                                       n_rows, n_walkers, w.d_sums, w.d_out));
    MCD_HIP(hipMemcpyAsync(w.h_out, w.d_out, (size_t)2 * n_rows * sizeof(double), hipMemcpyDeviceToHost, slot.stream));
    MCD_WAIT(cat->ctx, slot.stream, cat->spin_us, "mcd_holdout_loglike");
    if (cat->timing) {
        float ms = 0.f;
        MCD_HIP(hipEventElapsedTime(&ms, w.e0, w.e1));
        cat->last_kernel_ms = ms;
        cat->timing_pending = false;
    }
    cat->last_chunks = w.n_chunks;
    cat->last_grid = mcd::main_grid(w.n_chunks, n_rows);
    std::memcpy(train, w.h_out, (size_t)n_rows * sizeof(double));
    if (test) std::memcpy(test, w.h_out + n_rows, (size_t)n_rows * sizeof(double));
    return MCD_OK;
}

}  // namespace

MCD_HOST_BEGIN

// For callers whose parameter table is made ON the device (mcd_api_mmatch.hip): the plan over any ranges with offsets
// 0 .. n_stars and its buffers, from the same cache ...
int holdout_device_plan(mcd_catalog* cat, const std::vector<int64_t>& ranges, int64_t n_rows, HoldoutWork** out) {
    return holdout_work(cat, cat->shards[0], ranges, (int32_t)ranges.size() - 1, n_rows, out);
}

// ... and one evaluation of the table the caller left in w.d_params: the launch sequence of mcd_holdout_loglike on the
// catalogue's stream, without a copy and without a wait.  Row e n_walkers + i belongs to the set whose range is
// d_set_range[e] (device memory); train and test stay in w.d_out ([2][n_rows]).  The device is current.
int holdout_device_eval(mcd_catalog* cat, HoldoutWork& w, int64_t n_walkers, const int64_t* d_set_range) {
    Shard& sh = cat->shards[0];
    const DeviceSlot& slot = cat->ctx->slots[sh.slot];
    MCD_HIP(mcd::launch_prepare_walkers(slot.stream, w.d_params, w.n_rows, cat->k, cat->model, cat->free_centre,
                                        cat->precision, w.d_wpar));
    const mcd::LaunchShape shape{cat->model, cat->free_centre, cat->precision, 0};
    if (cat->timing) MCD_HIP(hipEventRecord(w.e0, slot.stream));
    MCD_HIP(mcd::launch_holdout(slot.stream, shape, sh.records, w.d_chunks, w.n_chunks, w.d_wpar, w.d_partials, w.n_rows));
    if (cat->timing) MCD_HIP(hipEventRecord(w.e1, slot.stream));
    MCD_HIP(mcd::launch_holdout_reduce(slot.stream, w.d_partials, w.n_chunks, w.d_offsets, w.n_ranges, w.max_chunks_per_range,
                                       w.n_rows, n_walkers, w.d_sums, w.d_out, d_set_range));
    cat->last_chunks = w.n_chunks;
    cat->last_grid = mcd::main_grid(w.n_chunks, w.n_rows);
    return MCD_OK;
}

MCD_HOST_END

namespace {

// Per set: its S sample rows in passes of posterior_pass rows through the slice and merge kernels of
// mcd_pointwise_posterior on the set's records (the slice plan of a catalogue of the set's size: one set that covers the
// catalogue gives mcd_pointwise_posterior's bits).  The scratch is sized for the largest set and shared by all.
int holdout_pointwise(mcd_catalog* cat, int32_t n_sets, const int64_t* set_offsets, int64_t S, int32_t k, const double* params,
                      double* lppd, double* lnl_var) {
    if (!cat || !params) return fail(MCD_ERR_INVALID, "mcd_holdout_pointwise: null catalogue or params");
    if (int rc = holdout_usable(cat, "mcd_holdout_pointwise", n_sets, set_offsets, S, k)) return rc;
    const int64_t total = set_offsets[n_sets];
    if (total == 0 || !(lppd || lnl_var)) return MCD_OK;
    int64_t n_max = 0;
    for (int32_t e = 0; e < n_sets; ++e) n_max = std::max(n_max, set_offsets[e + 1] - set_offsets[e]);
    Shard& sh = cat->shards[0];
    const DeviceSlot& slot = cat->ctx->slots[sh.slot];
    MCD_HIP(hipSetDevice(slot.device));
    const size_t rec_bytes = sizeof(double) * (size_t)mcd::record_doubles(cat->model, cat->free_centre);
    const int64_t pass_len = std::min<int64_t>(S, cat->posterior_pass);
    const int64_t n_passes = (S + pass_len - 1) / pass_len;
    const int64_t last_len = S - (n_passes - 1) * pass_len;
    constexpr int nf = mcd::post_fields(false);
    // the plan with the most slices and the longest slice over the sets (a smaller set is cut into more slices)
    int64_t max_part = 0, max_len = 0;
    for (int32_t e = 0; e < n_sets; ++e) {
        const int64_t n = set_offsets[e + 1] - set_offsets[e];
        if (n == 0) continue;
        for (const int64_t ns : {pass_len, last_len}) {
            int64_t len = 0;
            const int64_t slices = mcd::posterior_slices(n, ns, &len);
            max_part = std::max(max_part, slices * n);
            max_len = std::max(max_len, len);
        }
    }
    DeviceScratch d;
    double *d_params = nullptr, *d_inv = nullptr, *d_part = nullptr, *d_state = nullptr, *d_out = nullptr;
    void* d_wpar = nullptr;
    MCD_HIP(d.malloc(&d_params, (size_t)pass_len * k * sizeof(double)));
    MCD_HIP(d.malloc(&d_wpar, (size_t)pass_len * mcd::KD * sizeof(double)));
    MCD_HIP(d.malloc(&d_inv, (size_t)max_len * sizeof(double)));
    MCD_HIP(d.malloc(&d_part, (size_t)max_part * nf * sizeof(double)));
    if (n_passes > 1) MCD_HIP(d.malloc(&d_state, (size_t)nf * n_max * sizeof(double)));
    MCD_HIP(d.malloc(&d_out, (size_t)4 * total * sizeof(double)));      // set e: [4][n_e] from 4 set_offsets[e] on
    std::vector<double> inv((size_t)max_len);
    for (int64_t j = 0; j < max_len; ++j) inv[j] = 1.0 / (double)(j + 1);
    MCD_HIP(hipMemcpy(d_inv, inv.data(), inv.size() * sizeof(double), hipMemcpyHostToDevice));
    if (cat->timing) {
        MCD_HIP(d.create_events());
        MCD_HIP(hipEventRecord(d.e0, slot.stream));
    }
    const mcd::LaunchShape shape{cat->model, cat->free_centre, cat->precision, 0};
    for (int32_t e = 0; e < n_sets; ++e) {
        const int64_t b = set_offsets[e], n = set_offsets[e + 1] - b;
        if (n == 0) continue;
        const double* table = params + (size_t)e * S * k;
        for (int64_t p = 0; p < n_passes; ++p) {
            const int64_t s0 = p * pass_len, ns = std::min(pass_len, S - s0);
            int64_t slice_len = 0;
            const int64_t n_slices = mcd::posterior_slices(n, ns, &slice_len);
            MCD_HIP(hipMemcpyAsync(d_params, table + s0 * k, (size_t)ns * k * sizeof(double), hipMemcpyHostToDevice, slot.stream));
            MCD_HIP(mcd::launch_prepare_walkers(slot.stream, d_params, ns, k, cat->model, cat->free_centre, cat->precision,
                                                d_wpar));
            MCD_HIP(mcd::launch_posterior(slot.stream, shape, false, (const char*)sh.records + (size_t)b * rec_bytes, n, d_wpar,
                                          ns, d_inv, slice_len, n_slices, d_part, d_state, s0, S, d_out + 4 * b));
        }
    }
    if (d.e1) MCD_HIP(hipEventRecord(d.e1, slot.stream));
    for (int32_t e = 0; e < n_sets; ++e) {
        const int64_t b = set_offsets[e], n = set_offsets[e + 1] - b;
        if (n == 0) continue;
        if (lppd) MCD_HIP(hipMemcpyAsync(lppd + b, d_out + 4 * b, (size_t)n * sizeof(double), hipMemcpyDeviceToHost, slot.stream));
        if (lnl_var)
            MCD_HIP(hipMemcpyAsync(lnl_var + b, d_out + 4 * b + n, (size_t)n * sizeof(double), hipMemcpyDeviceToHost, slot.stream));
    }
    MCD_WAIT(cat->ctx, slot.stream, cat->spin_us, "mcd_holdout_pointwise");
    if (cat->timing) {
        float ms = 0.f;
        MCD_HIP(hipEventElapsedTime(&ms, d.e0, d.e1));
        cat->last_kernel_ms = ms;
        cat->timing_pending = false;
    }
    return MCD_OK;
}

}  // namespace

extern "C" {

int mcd_holdout_loglike(mcd_catalog* cat, int32_t n_sets, const int64_t* set_offsets, int64_t n_walkers, int32_t k,
                        const double* params, double* train, double* test) {
    try {
    return holdout_loglike(cat, n_sets, set_offsets, n_walkers, k, params, train, test);
    } catch (...) { return on_exception("mcd_holdout_loglike"); }
}

int mcd_holdout_pointwise(mcd_catalog* cat, int32_t n_sets, const int64_t* set_offsets, int64_t n_samples, int32_t k,
                          const double* params, double* lppd, double* lnl_var) {
    try {
    return holdout_pointwise(cat, n_sets, set_offsets, n_samples, k, params, lppd, lnl_var);
    } catch (...) { return on_exception("mcd_holdout_pointwise"); }
}

}  // extern "C"

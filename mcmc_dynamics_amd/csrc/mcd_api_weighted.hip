// mcd_api_weighted.hip -- C-ABI of the MI355X log-likelihood library (see include/mcd.h; mcd_host.h lists the host units):
// host driver of the weighted value and gradient.  mcd_weighted_loglike_grad: R parameter rows against the whole catalogue
// in one launch, every row under the star weights of its own replicate (kernel: mcd_weighted.hip; loop: mcd_weighted.h;
// generator: mcd_weights.h).  mcd_weighted_loglike: the value alone (kernel: mcd_weighted_value.hip; loop:
// mcd_weighted_value.h), behind the same validation and the same explicit-table pass.  mcd_bootstrap_weights: the generated
// weights on the host.
#include "mcd_host.h"
#include "mcd_weighted.h"
#include "mcd_weighted_value.h"

using namespace mcd::host;

MCD_HOST_BEGIN

void free_weighted_work(WeightedWork& w) {
    if (w.d_chunks) (void)hipFree(w.d_chunks);
    if (w.d_offsets) (void)hipFree(w.d_offsets);
    if (w.d_params) (void)hipFree(w.d_params);
    if (w.d_wpar) (void)hipFree(w.d_wpar);
    if (w.d_replicate) (void)hipFree(w.d_replicate);
    if (w.d_partials) (void)hipFree(w.d_partials);
    if (w.d_out) (void)hipFree(w.d_out);
    if (w.h_params) (void)hipHostFree(w.h_params);
    if (w.h_replicate) (void)hipHostFree(w.h_replicate);
    if (w.h_out) (void)hipHostFree(w.h_out);
    if (w.e0) (void)hipEventDestroy(w.e0);
    if (w.e1) (void)hipEventDestroy(w.e1);
    w = WeightedWork();
}

// the catalogue's weighted plans, their buffers and the uploaded weights (the device of the catalogue's one shard is
// current, its stream idle)
void release_weighted(mcd_catalog* cat) {
    for (auto& kv : cat->weighted) free_weighted_work(kv.second);
    cat->weighted.clear();
    for (auto& kv : cat->weighted_value) free_weighted_work(kv.second);
    cat->weighted_value.clear();
    if (cat->d_weights) (void)hipFree(cat->d_weights);
    cat->d_weights = nullptr;
    cat->d_weights_bytes = 0;
    cat->weights_replicates = -1;
}

// The chunk table over `records` for n_rows rows and its buffers, from `cache` (the catalogue's for the gradient call,
// 1 + K fields per row, the one for the value call or the one of mcd_simulated_loglike, one field) or built now
int weighted_work(mcd_catalog* cat, std::map<int64_t, WeightedWork>& cache, size_t fields, const Shard& sh, int64_t n_rows,
                  WeightedWork** out) {
    auto it = cache.find(n_rows);
    if (it != cache.end()) { *out = &it->second; return MCD_OK; }
    if (cache.size() >= 8) {                                           // bound the cache (a bootstrap, a bagged run use one row count)
        for (auto& kv : cache) free_weighted_work(kv.second);
        cache.clear();
    }
    // catalogue order always: the weights are indexed by the star's position in `records`, so the verr-sorted copy and
    // the plans made for it are not used
    const mcd::ChunkPlan plan = mcd::plan_chunks({0, sh.n}, 0, sh.n, n_rows, cat->target_waves, cat->tail_split, {}, cat->chunk_len);
    WeightedWork w;
    w.n_rows = n_rows;
    w.n_chunks = (int64_t)plan.chunks.size();
    const size_t padded = (size_t)mcd::padded_walkers(n_rows);
    // (a failure half-way releases what it got)
    auto build = [&]() -> int {
        MCD_HIP(hipMalloc(&w.d_chunks, std::max<size_t>(1, plan.chunks.size()) * sizeof(mcd::Chunk)));
        MCD_HIP(hipMalloc(&w.d_offsets, plan.offsets.size() * sizeof(int64_t)));
        MCD_HIP(hipMalloc(&w.d_params, (size_t)n_rows * cat->k * sizeof(double)));
        MCD_HIP(hipMalloc(&w.d_wpar, (size_t)n_rows * mcd::KD * sizeof(double)));
        MCD_HIP(hipMalloc(&w.d_replicate, (size_t)n_rows * sizeof(int64_t)));
        MCD_HIP(hipMalloc(&w.d_partials, std::max<size_t>(1, fields * padded * plan.chunks.size()) * sizeof(double)));
        MCD_HIP(hipMalloc(&w.d_out, fields * padded * sizeof(double)));
        MCD_HIP(hipHostMalloc(&w.h_params, (size_t)n_rows * cat->k * sizeof(double), hipHostMallocDefault));
        MCD_HIP(hipHostMalloc(&w.h_replicate, (size_t)n_rows * sizeof(int64_t), hipHostMallocDefault));
        MCD_HIP(hipHostMalloc(&w.h_out, fields * padded * sizeof(double), hipHostMallocDefault));
        MCD_HIP(hipEventCreate(&w.e0));
        MCD_HIP(hipEventCreate(&w.e1));
        if (!plan.chunks.empty())
            MCD_HIP(hipMemcpy(w.d_chunks, plan.chunks.data(), plan.chunks.size() * sizeof(mcd::Chunk), hipMemcpyHostToDevice));
        MCD_HIP(hipMemcpy(w.d_offsets, plan.offsets.data(), plan.offsets.size() * sizeof(int64_t), hipMemcpyHostToDevice));
        return MCD_OK;
    };
    if (int rc = build()) { free_weighted_work(w); return rc; }
    *out = &(cache[n_rows] = w);
    return MCD_OK;
}

// After the D2H copy of a call's results is enqueued: the wait, option "timing", the launch record
int weighted_finish(mcd_catalog* cat, const std::string& name, WeightedWork& w, int64_t n_rows) {
    const DeviceSlot& slot = cat->ctx->slots[cat->shards[0].slot];
    MCD_WAIT(cat->ctx, slot.stream, cat->spin_us, name.c_str());
    if (cat->timing) {
        float ms = 0.f;
        MCD_HIP(hipEventElapsedTime(&ms, w.e0, w.e1));
        cat->last_kernel_ms = ms;
        cat->timing_pending = false;
    }
    cat->last_chunks = w.n_chunks;
    cat->last_grid = mcd::main_grid(w.n_chunks, n_rows);
    return MCD_OK;
}

MCD_HOST_END

namespace {

// What both entry points refuse, in the order of include/mcd.h; `name` opens the message
int weighted_usable(mcd_catalog* cat, const std::string& name, int64_t n_rows, int32_t k, const double* params,
                    const mcd_weight_desc* wd) {
    if (!cat || !params || !wd) return fail(MCD_ERR_INVALID, name + ": null catalogue, params or weight description");
    if (int rc = ctx_usable(cat->ctx)) return rc;
    if (cat->n_psets != 1) return fail(MCD_ERR_INVALID, name + ": defined for un-binned catalogues only");
    if (cat->precision != MCD_F64) return fail(MCD_ERR_INVALID, name + ": needs an MCD_F64 catalogue");
    if (cat->ctx->has_comm() || cat->shards.size() != 1)
        return fail(MCD_ERR_INVALID, name + ": one device per process (no several devices, no communicator)");
    if (k != cat->k) return fail(MCD_ERR_INVALID, name + ": parameter rows have the wrong number of columns");
    if (n_rows < 1 || n_rows > mcd::kWeightedMaxRows)
        return fail(MCD_ERR_INVALID, name + ": needs 1 .. " + std::to_string(mcd::kWeightedMaxRows) + " parameter rows");
    const int scheme = wd->scheme;
    if (scheme != MCD_WEIGHT_EXPONENTIAL && scheme != MCD_WEIGHT_POISSON && scheme != MCD_WEIGHT_EXPLICIT)
        return fail(MCD_ERR_INVALID, name + ": unknown weight scheme " + std::to_string(scheme));
    if (!wd->row_replicate) return fail(MCD_ERR_INVALID, name + ": row_replicate is null");
    const bool explicit_w = scheme == MCD_WEIGHT_EXPLICIT;
    const int64_t B = explicit_w ? wd->n_replicates : 0, N = cat->n_stars;
    if (explicit_w) {
        if (!wd->weights) return fail(MCD_ERR_INVALID, name + ": explicit weights are null");
        if (B < 1) return fail(MCD_ERR_INVALID, name + ": explicit weights need n_replicates >= 1");
        if (B > mcd::kWeightedMaxExplicitBytes / 8 || (N > 0 && B > mcd::kWeightedMaxExplicitBytes / 8 / N))
            return fail(MCD_ERR_INVALID, name + ": explicit weights of " + std::to_string(B) + " replicates x " + std::to_string(N) +
                                             " stars exceed " + std::to_string(mcd::kWeightedMaxExplicitBytes >> 20) + " MiB");
    }
    for (int64_t r = 0; r < n_rows; ++r) {
        const int64_t b = wd->row_replicate[r];
        if (b < 0 || (explicit_w && b >= B))
            return fail(MCD_ERR_INVALID, name + ": row_replicate[" + std::to_string(r) + "] = " + std::to_string(b) +
                                             (explicit_w ? " is outside [0, n_replicates)" : " is negative"));
    }
    return MCD_OK;
}

// explicit weights: every call checks them and fingerprints their contents in one sequential pass (two independent
// 64-bit mixes of the bit patterns, with the shape): the transposed copy on the device is kept while the fingerprint
// stands, whatever the address and whichever of the two calls uploaded it, so that the trial steps of an optimiser and
// the half steps of a chain pay the pass and not the upload
int weights_fingerprint(const mcd_catalog* cat, const std::string& name, const mcd_weight_desc* wd, uint64_t print[2]) {
    print[0] = 0x6d63645f776768ull;
    print[1] = 0x9E3779B97F4A7C15ull;
    if (wd->scheme != MCD_WEIGHT_EXPLICIT) return MCD_OK;
    const int64_t B = wd->n_replicates, N = cat->n_stars;
    const size_t total = (size_t)(B * N);
    for (size_t at = 0; at < total; ++at) {
        const double x = wd->weights[at];
        if (!(x >= 0.0) || !std::isfinite(x))
            return fail(MCD_ERR_INVALID, name + ": weight [" + std::to_string(at / (size_t)N) + "][" +
                                             std::to_string(at % (size_t)N) + "] is negative or not finite");
        uint64_t bits;
        std::memcpy(&bits, &x, sizeof bits);
        print[0] = (print[0] ^ bits) * 0xD2E7470EE14C6C93ull;
        print[0] ^= print[0] >> 32;
        print[1] = (print[1] + bits) * 0xCA5A826395121157ull;
        print[1] = (print[1] << 23) | (print[1] >> 41);
    }
    return MCD_OK;
}

// ... and the device copy of the table with fingerprint `print`: kept, or transposed and uploaded now (the device is
// current, its stream idle)
int weights_on_device(mcd_catalog* cat, const mcd_weight_desc* wd, const uint64_t print[2]) {
    const int64_t B = wd->n_replicates, N = cat->n_stars;
    if (cat->d_weights && cat->weights_replicates == B && cat->weights_print[0] == print[0] && cat->weights_print[1] == print[1])
        return MCD_OK;
    // transposed to [star][replicate], in blocks of stars whose rows of the copy stay in cache
    std::vector<double> transposed((size_t)(B * N));
    constexpr int64_t kBlockStars = 256;
    for (int64_t i0 = 0; i0 < N; i0 += kBlockStars) {
        const int64_t i1 = std::min(N, i0 + kBlockStars);
        for (int64_t b = 0; b < B; ++b) {
            const double* row = wd->weights + (size_t)(b * N);
            for (int64_t i = i0; i < i1; ++i) transposed[(size_t)(i * B + b)] = row[i];
        }
    }
    cat->weights_replicates = -1;                                   // (nothing is cached while the copy is in the making)
    const size_t bytes = std::max<size_t>(8, transposed.size() * sizeof(double));
    if (bytes > cat->d_weights_bytes) {
        if (cat->d_weights) MCD_HIP(hipFree(cat->d_weights));
        cat->d_weights = nullptr;
        cat->d_weights_bytes = 0;
        MCD_HIP(hipMalloc(&cat->d_weights, bytes));
        cat->d_weights_bytes = bytes;
    }
    // (from pageable memory: the copy has left `transposed` when the call returns)
    if (!transposed.empty())
        MCD_HIP(hipMemcpy(cat->d_weights, transposed.data(), transposed.size() * sizeof(double), hipMemcpyHostToDevice));
    cat->weights_replicates = B;
    cat->weights_print[0] = print[0];
    cat->weights_print[1] = print[1];
    return MCD_OK;
}

// What both calls do between their validation and their kernel: the explicit table's pass, the plan and buffers of the
// row count from `cache` (`fields` sums per row), the table's device copy, params and replicates H2D, walker prep; the
// device is current and the first timing event recorded when this returns
int weighted_stage(mcd_catalog* cat, const std::string& name, std::map<int64_t, WeightedWork>& cache, size_t fields,
                   int64_t n_rows, int32_t k, const double* params, const mcd_weight_desc* wd, WeightedWork** out) {
    uint64_t print[2];
    if (int rc = weights_fingerprint(cat, name, wd, print)) return rc;
    Shard& sh = cat->shards[0];
    const DeviceSlot& slot = cat->ctx->slots[sh.slot];
    MCD_HIP(hipSetDevice(slot.device));
    // (an earlier pipelined evaluation may still be in flight on the stream the plans are released and built on)
    MCD_WAIT(cat->ctx, slot.stream, cat->spin_us, (name + " (previous evaluation)").c_str());
    if (int rc = weighted_work(cat, cache, fields, sh, n_rows, out)) return rc;
    WeightedWork& w = **out;
    if (wd->scheme == MCD_WEIGHT_EXPLICIT)
        if (int rc = weights_on_device(cat, wd, print)) return rc;
    // the gradient path's staging: params H2D, walker prep
    std::memcpy(w.h_params, params, (size_t)n_rows * k * sizeof(double));
    std::memcpy(w.h_replicate, wd->row_replicate, (size_t)n_rows * sizeof(int64_t));
    MCD_HIP(hipMemcpyAsync(w.d_params, w.h_params, (size_t)n_rows * k * sizeof(double), hipMemcpyHostToDevice, slot.stream));
    MCD_HIP(hipMemcpyAsync(w.d_replicate, w.h_replicate, (size_t)n_rows * sizeof(int64_t), hipMemcpyHostToDevice, slot.stream));
    MCD_HIP(mcd::launch_prepare_walkers(slot.stream, w.d_params, n_rows, k, cat->model, cat->free_centre, cat->precision,
                                        w.d_wpar));
    if (cat->timing) MCD_HIP(hipEventRecord(w.e0, slot.stream));
    return MCD_OK;
}

// ... and after the D2H copy of their results is enqueued: weighted_finish (above)

int weighted_loglike_grad(mcd_catalog* cat, int64_t n_rows, int32_t k, const double* params, const mcd_weight_desc* wd,
                          double* out, double* grad) {
    const std::string name("mcd_weighted_loglike_grad");
    if (int rc = weighted_usable(cat, name, n_rows, k, params, wd)) return rc;
    if (!out && !grad) return MCD_OK;
    WeightedWork* wp = nullptr;
    if (int rc = weighted_stage(cat, name, cat->weighted, (size_t)(1 + k), n_rows, k, params, wd, &wp)) return rc;
    WeightedWork& w = *wp;
    const Shard& sh = cat->shards[0];
    const DeviceSlot& slot = cat->ctx->slots[sh.slot];
    const bool explicit_w = wd->scheme == MCD_WEIGHT_EXPLICIT;
    const size_t fields = (size_t)(1 + k), padded = (size_t)mcd::padded_walkers(n_rows);
    const mcd::LaunchShape shape{cat->model, cat->free_centre, cat->precision, 0};
    MCD_HIP(mcd::launch_weighted_grad(slot.stream, shape, wd->scheme, sh.records, w.d_chunks, w.n_chunks, w.d_params, w.d_wpar,
                                      w.d_replicate, wd->seed, explicit_w ? cat->d_weights : nullptr,
                                      explicit_w ? wd->n_replicates : 0, w.d_partials, n_rows));
    if (cat->timing) MCD_HIP(hipEventRecord(w.e1, slot.stream));
    MCD_HIP(mcd::launch_grad_reduce(slot.stream, shape, w.d_partials, w.n_chunks, w.d_offsets, 1, w.n_chunks, n_rows, w.d_out));
    MCD_HIP(hipMemcpyAsync(w.h_out, w.d_out, fields * padded * sizeof(double), hipMemcpyDeviceToHost, slot.stream));
    if (int rc = weighted_finish(cat, name, w, n_rows)) return rc;
    if (out) std::memcpy(out, w.h_out, (size_t)n_rows * sizeof(double));
    if (grad)
        for (int64_t j = 0; j < k; ++j) {
            const double* col = w.h_out + (1 + j) * padded;
            for (int64_t i = 0; i < n_rows; ++i) grad[i * k + j] = col[i];
        }
    return MCD_OK;
}

// The value alone: the value kernel (one sum per row) and the value path's reduction of one range
int weighted_loglike(mcd_catalog* cat, int64_t n_rows, int32_t k, const double* params, const mcd_weight_desc* wd, double* out) {
    const std::string name("mcd_weighted_loglike");
    if (int rc = weighted_usable(cat, name, n_rows, k, params, wd)) return rc;
    if (!out) return MCD_OK;
    WeightedWork* wp = nullptr;
    if (int rc = weighted_stage(cat, name, cat->weighted_value, 1, n_rows, k, params, wd, &wp)) return rc;
    WeightedWork& w = *wp;
    const Shard& sh = cat->shards[0];
    const DeviceSlot& slot = cat->ctx->slots[sh.slot];
    const bool explicit_w = wd->scheme == MCD_WEIGHT_EXPLICIT;
    const mcd::LaunchShape shape{cat->model, cat->free_centre, cat->precision, 0};
    MCD_HIP(mcd::launch_weighted_value(slot.stream, shape, wd->scheme, sh.records, w.d_chunks, w.n_chunks, w.d_wpar, w.d_replicate,
                                       wd->seed, explicit_w ? cat->d_weights : nullptr, explicit_w ? wd->n_replicates : 0,
                                       w.d_partials, n_rows));
    if (cat->timing) MCD_HIP(hipEventRecord(w.e1, slot.stream));
    MCD_HIP(mcd::launch_reduce(slot.stream, w.d_partials, w.d_offsets, 1, w.n_chunks, w.n_chunks, n_rows, nullptr, w.d_out));
    MCD_HIP(hipMemcpyAsync(w.h_out, w.d_out, (size_t)n_rows * sizeof(double), hipMemcpyDeviceToHost, slot.stream));
    if (int rc = weighted_finish(cat, name, w, n_rows)) return rc;
    std::memcpy(out, w.h_out, (size_t)n_rows * sizeof(double));
    return MCD_OK;
}

}  // namespace

extern "C" {

int mcd_weighted_loglike_grad(mcd_catalog* cat, int64_t n_rows, int32_t k, const double* params, const mcd_weight_desc* w,
                              double* out, double* grad) {
    try {
    return weighted_loglike_grad(cat, n_rows, k, params, w, out, grad);
    } catch (...) { return on_exception("mcd_weighted_loglike_grad"); }
}

int mcd_weighted_loglike(mcd_catalog* cat, int64_t n_rows, int32_t k, const double* params, const mcd_weight_desc* w,
                         double* out) {
    try {
    return weighted_loglike(cat, n_rows, k, params, w, out);
    } catch (...) { return on_exception("mcd_weighted_loglike"); }
}

int mcd_bootstrap_weights(int32_t scheme, uint64_t seed, int64_t rep0, int64_t n_reps, int64_t star0, int64_t n_stars,
                          double* w) {
    try {
    if ((scheme != MCD_WEIGHT_EXPONENTIAL && scheme != MCD_WEIGHT_POISSON) || rep0 < 0 || n_reps < 0 || star0 < 0 ||
        n_stars < 0 || !w)
        return fail(MCD_ERR_INVALID, "mcd_bootstrap_weights: bad arguments (a generated scheme, non-negative ranges, an output)");
    for (int64_t b = 0; b < n_reps; ++b)
        for (int64_t i = 0; i < n_stars; ++i) w[b * n_stars + i] = mcd::bootstrap_weight(scheme, seed, rep0 + b, star0 + i);
    return MCD_OK;
    } catch (...) { return on_exception("mcd_bootstrap_weights"); }
}

}  // extern "C"

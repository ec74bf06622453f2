// mcd_api_simulated.hip -- C-ABI of the MI355X log-likelihood library (see include/mcd.h; mcd_host.h lists the host units):
// host driver of the simulated catalogues.  mcd_simulate draws n_sims catalogues' velocities from the model, one truth row
// each, into a table resident on the catalogue's device; mcd_simulated_set uploads a caller's own; mcd_simulated_loglike
// evaluates R parameter rows in one launch, every row against the velocities of its own simulation (kernels:
// mcd_simulated.hip; velocity rule, term and loop: mcd_simulated.h; generator: mcd_replicate.h);
// mcd_simulated_loglike_grad adds the gradient (kernel: mcd_simulated_grad.hip; loop: mcd_simulated_grad.h).
#include "mcd_host.h"
#include "mcd_simulated_grad.h"

using namespace mcd::host;

MCD_HOST_BEGIN

// mcd_simulated_loglike's plans and buffers and, unless keep_set, the resident table (the device of the catalogue's one
// shard is current, its stream idle)
void release_simulated(mcd_catalog* cat, bool keep_set) {
    for (auto& kv : cat->simulated) free_weighted_work(kv.second);
    cat->simulated.clear();
    for (auto& kv : cat->simulated_grad) free_weighted_work(kv.second);
    cat->simulated_grad.clear();
    if (keep_set) return;
    if (cat->d_sim) (void)hipFree(cat->d_sim);
    cat->d_sim = nullptr;
    cat->d_sim_bytes = 0;
    cat->sim_count = 0;
}

MCD_HOST_END

namespace {

// What the three calls refuse about the catalogue itself; `name` opens the message
int simulated_usable(mcd_catalog* cat, const std::string& name) {
    if (!cat) return fail(MCD_ERR_INVALID, name + ": null catalogue");
    if (int rc = ctx_usable(cat->ctx)) return rc;
    if (cat->n_psets != 1) return fail(MCD_ERR_INVALID, name + ": defined for un-binned catalogues only");
    if (cat->precision != MCD_F64) return fail(MCD_ERR_INVALID, name + ": needs an MCD_F64 catalogue");
    if (cat->ctx->has_comm() || cat->shards.size() != 1)
        return fail(MCD_ERR_INVALID, name + ": one device per process (no several devices, no communicator)");
    return MCD_OK;
}

// ... and about the set they are to make
int simulated_set_usable(mcd_catalog* cat, const std::string& name, int64_t n_sims, double bg_mean, double bg_sigma) {
    if (n_sims < 1) return fail(MCD_ERR_INVALID, name + ": needs at least one simulation");
    if (!mcd::simulated_fits_budget(n_sims, cat->n_stars))
        return fail(MCD_ERR_INVALID, name + ": velocities of " + std::to_string(n_sims) + " simulations x " +
                                         std::to_string(cat->n_stars) + " stars exceed the simulated-set budget of " +
                                         std::to_string(mcd::kSimulatedMaxBytes >> 20) + " MiB");
    if (const char* why = mcd::replicate_background_error(cat->model, bg_mean, bg_sigma))
        return fail(MCD_ERR_INVALID, name + ": " + why);
    return MCD_OK;
}

// Room for a table of n_sims simulations; no set is resident while it is in the making (the device is current, its stream
// idle)
int simulated_room(mcd_catalog* cat, int64_t n_sims) {
    cat->sim_count = 0;
    const size_t bytes = std::max<size_t>(8, (size_t)n_sims * (size_t)cat->n_stars * sizeof(double));
    if (bytes > cat->d_sim_bytes) {
        if (cat->d_sim) MCD_HIP(hipFree(cat->d_sim));
        cat->d_sim = nullptr;
        cat->d_sim_bytes = 0;
        MCD_HIP(hipMalloc(&cat->d_sim, bytes));
        cat->d_sim_bytes = bytes;
    }
    return MCD_OK;
}

void simulated_keep(mcd_catalog* cat, int64_t n_sims, double bg_mean, double bg_sigma) {
    const bool needs = mcd::replicate_needs_background(cat->model);
    cat->sim_bg_mean = needs ? bg_mean : 0.0;
    cat->sim_bg_sigma2 = needs ? bg_sigma * bg_sigma : 0.0;
    cat->sim_count = n_sims;
}

// [a][b] -> [b][a], in blocks whose rows of the copy stay in cache
void transpose(const double* src, int64_t a, int64_t b, double* dst) {
    constexpr int64_t kBlockCols = 256;
    for (int64_t j0 = 0; j0 < b; j0 += kBlockCols) {
        const int64_t j1 = std::min(b, j0 + kBlockCols);
        for (int64_t i = 0; i < a; ++i) {
            const double* row = src + (size_t)(i * b);
            for (int64_t j = j0; j < j1; ++j) dst[(size_t)(j * a + i)] = row[j];
        }
    }
}

int simulate(mcd_catalog* cat, int64_t E, int32_t k, const double* truths, uint64_t seed, int64_t sim0, double bg_mean,
             double bg_sigma, double* velocities) {
    const std::string name("mcd_simulate");
    if (int rc = simulated_usable(cat, name)) return rc;
    if (!truths) return fail(MCD_ERR_INVALID, name + ": truths is null");
    if (k != cat->k) return fail(MCD_ERR_INVALID, name + ": truth rows have the wrong number of columns");
    if (sim0 < 0) return fail(MCD_ERR_INVALID, name + ": sim0 is negative");
    if (int rc = simulated_set_usable(cat, name, E, bg_mean, bg_sigma)) return rc;
    const int64_t N = cat->n_stars;
    Shard& sh = cat->shards[0];
    const DeviceSlot& slot = cat->ctx->slots[sh.slot];
    MCD_HIP(hipSetDevice(slot.device));
    // (an earlier pipelined evaluation may still be in flight on the stream)
    MCD_WAIT(cat->ctx, slot.stream, cat->spin_us, "mcd_simulate (previous evaluation)");
    // catalogue order always: a velocity is indexed by the star's position in `records`
    const int64_t P = std::min(E, mcd::kSimulatedPassSims);
    const mcd::ChunkPlan plan = mcd::plan_chunks({0, sh.n}, 0, sh.n, P, cat->target_waves, cat->tail_split, {}, cat->chunk_len);
    const int64_t n_chunks = (int64_t)plan.chunks.size();
    DeviceScratch d;
    mcd::Chunk* d_chunks = nullptr;
    double* d_params = nullptr;
    void* d_wpar = nullptr;
    int64_t *d_bad = nullptr, *d_first = nullptr;
    MCD_HIP(d.malloc(&d_chunks, std::max<size_t>(1, (size_t)n_chunks) * sizeof(mcd::Chunk)));
    MCD_HIP(d.malloc(&d_params, (size_t)P * k * sizeof(double)));
    MCD_HIP(d.malloc(&d_wpar, (size_t)P * mcd::KD * sizeof(double)));
    MCD_HIP(d.malloc(&d_bad, std::max<size_t>(1, (size_t)(n_chunks * P)) * sizeof(int64_t)));
    MCD_HIP(d.malloc(&d_first, (size_t)P * sizeof(int64_t)));
    if (n_chunks > 0)
        MCD_HIP(hipMemcpy(d_chunks, plan.chunks.data(), (size_t)n_chunks * sizeof(mcd::Chunk), hipMemcpyHostToDevice));
    if (cat->timing) MCD_HIP(d.create_events());
    if (int rc = simulated_room(cat, E)) return rc;
    const mcd::LaunchShape shape{cat->model, cat->free_centre, cat->precision, 0};
    const double bg_sigma2 = bg_sigma * bg_sigma;
    std::vector<int64_t> first((size_t)P);
    double kernel_ms = 0.0;
    int64_t bad_sim = -1, bad_star = -1;
    // Simulations are independent: a pass is the staging of the truth rows (H2D, walker prep), the kernel on its columns
    // of the table, and the first non-finite star of each of its simulations
    for (int64_t e0 = 0; e0 < E; e0 += P) {
        const int64_t ne = std::min(P, E - e0);
        MCD_HIP(hipMemcpyAsync(d_params, truths + (size_t)e0 * k, (size_t)ne * k * sizeof(double), hipMemcpyHostToDevice, slot.stream));
        MCD_HIP(mcd::launch_prepare_walkers(slot.stream, d_params, ne, k, cat->model, cat->free_centre, cat->precision, d_wpar));
        if (cat->timing) MCD_HIP(hipEventRecord(d.e0, slot.stream));
        MCD_HIP(mcd::launch_simulate(slot.stream, shape, sh.records, d_chunks, n_chunks, d_wpar, ne, e0, E, sim0, seed, bg_mean,
                                     bg_sigma2, cat->d_sim, d_bad));
        if (cat->timing) MCD_HIP(hipEventRecord(d.e1, slot.stream));
        MCD_HIP(mcd::launch_simulate_first(slot.stream, d_bad, n_chunks, ne, d_first));
        MCD_HIP(hipMemcpyAsync(first.data(), d_first, (size_t)ne * sizeof(int64_t), hipMemcpyDeviceToHost, slot.stream));
        MCD_WAIT(cat->ctx, slot.stream, cat->spin_us, "mcd_simulate");
        if (cat->timing) {
            float ms = 0.f;
            MCD_HIP(hipEventElapsedTime(&ms, d.e0, d.e1));
            kernel_ms += ms;
        }
        for (int64_t e = 0; e < ne && bad_sim < 0; ++e)
            if (first[(size_t)e] >= 0) { bad_sim = e0 + e; bad_star = first[(size_t)e]; }
        if (bad_sim >= 0) break;
    }
    if (cat->timing) {
        cat->last_kernel_ms = kernel_ms;
        cat->timing_pending = false;
    }
    cat->last_chunks = n_chunks;
    cat->last_grid = mcd::main_grid(n_chunks, P);
    if (bad_sim >= 0)
        return fail(MCD_ERR_NONFINITE, name + ": the velocity of simulation " + std::to_string(bad_sim) + ", star " +
                                           std::to_string(bad_star) + " is not finite (a truth row outside the model's domain); " +
                                           "no set is resident");
    if (velocities && N > 0) {
        std::vector<double> table((size_t)(N * E));
        MCD_HIP(hipMemcpy(table.data(), cat->d_sim, table.size() * sizeof(double), hipMemcpyDeviceToHost));
        transpose(table.data(), N, E, velocities);
    }
    simulated_keep(cat, E, bg_mean, bg_sigma);
    return MCD_OK;
}

int simulated_set(mcd_catalog* cat, int64_t E, const double* velocities, double bg_mean, double bg_sigma) {
    const std::string name("mcd_simulated_set");
    if (int rc = simulated_usable(cat, name)) return rc;
    if (!velocities) return fail(MCD_ERR_INVALID, name + ": velocities is null");
    if (int rc = simulated_set_usable(cat, name, E, bg_mean, bg_sigma)) return rc;
    const int64_t N = cat->n_stars;
    const size_t total = (size_t)(E * N);
    for (size_t at = 0; at < total; ++at)
        if (!std::isfinite(velocities[at]))
            return fail(MCD_ERR_INVALID, name + ": velocity [" + std::to_string(at / (size_t)N) + "][" +
                                             std::to_string(at % (size_t)N) + "] is not finite");
    std::vector<double> table(total);
    transpose(velocities, E, N, table.data());
    const DeviceSlot& slot = cat->ctx->slots[cat->shards[0].slot];
    MCD_HIP(hipSetDevice(slot.device));
    MCD_WAIT(cat->ctx, slot.stream, cat->spin_us, "mcd_simulated_set (previous evaluation)");
    if (int rc = simulated_room(cat, E)) return rc;
    // (from pageable memory: the copy has left `table` when the call returns)
    if (total > 0) MCD_HIP(hipMemcpy(cat->d_sim, table.data(), total * sizeof(double), hipMemcpyHostToDevice));
    simulated_keep(cat, E, bg_mean, bg_sigma);
    return MCD_OK;
}

int simulated_loglike(mcd_catalog* cat, int64_t n_rows, int32_t k, const double* params, const int64_t* row_sim, double* out) {
    const std::string name("mcd_simulated_loglike");
    if (int rc = simulated_usable(cat, name)) return rc;
    if (!params || !row_sim) return fail(MCD_ERR_INVALID, name + ": null params or row_sim");
    if (k != cat->k) return fail(MCD_ERR_INVALID, name + ": parameter rows have the wrong number of columns");
    if (n_rows < 1 || n_rows > mcd::kSimulatedMaxRows)
        return fail(MCD_ERR_INVALID, name + ": needs 1 .. " + std::to_string(mcd::kSimulatedMaxRows) + " parameter rows");
    if (cat->sim_count < 1 || !cat->d_sim)
        return fail(MCD_ERR_INVALID, name + ": no simulated set is resident (mcd_simulate or mcd_simulated_set first)");
    for (int64_t r = 0; r < n_rows; ++r)
        if (row_sim[r] < 0 || row_sim[r] >= cat->sim_count)
            return fail(MCD_ERR_INVALID, name + ": row_sim[" + std::to_string(r) + "] = " + std::to_string(row_sim[r]) +
                                             " is outside [0, " + std::to_string(cat->sim_count) + ")");
    if (!out) return MCD_OK;
    Shard& sh = cat->shards[0];
    const DeviceSlot& slot = cat->ctx->slots[sh.slot];
    MCD_HIP(hipSetDevice(slot.device));
    // (an earlier pipelined evaluation may still be in flight on the stream the plans are released and built on)
    MCD_WAIT(cat->ctx, slot.stream, cat->spin_us, "mcd_simulated_loglike (previous evaluation)");
    WeightedWork* wp = nullptr;
    if (int rc = weighted_work(cat, cat->simulated, 1, sh, n_rows, &wp)) return rc;
    WeightedWork& w = *wp;
    // the weighted path's staging: params and simulation ids H2D, walker prep
    std::memcpy(w.h_params, params, (size_t)n_rows * k * sizeof(double));
    std::memcpy(w.h_replicate, row_sim, (size_t)n_rows * sizeof(int64_t));
    MCD_HIP(hipMemcpyAsync(w.d_params, w.h_params, (size_t)n_rows * k * sizeof(double), hipMemcpyHostToDevice, slot.stream));
    MCD_HIP(hipMemcpyAsync(w.d_replicate, w.h_replicate, (size_t)n_rows * sizeof(int64_t), hipMemcpyHostToDevice, slot.stream));
    MCD_HIP(mcd::launch_prepare_walkers(slot.stream, w.d_params, n_rows, k, cat->model, cat->free_centre, cat->precision,
                                        w.d_wpar));
    if (cat->timing) MCD_HIP(hipEventRecord(w.e0, slot.stream));
    const mcd::LaunchShape shape{cat->model, cat->free_centre, cat->precision, 0};
    MCD_HIP(mcd::launch_simulated_value(slot.stream, shape, sh.records, w.d_chunks, w.n_chunks, w.d_wpar, w.d_replicate,
                                        cat->d_sim, cat->sim_count, cat->sim_bg_mean, cat->sim_bg_sigma2, w.d_partials, n_rows));
    if (cat->timing) MCD_HIP(hipEventRecord(w.e1, slot.stream));
    MCD_HIP(mcd::launch_reduce(slot.stream, w.d_partials, w.d_offsets, 1, w.n_chunks, w.n_chunks, n_rows, nullptr, w.d_out));
    MCD_HIP(hipMemcpyAsync(w.h_out, w.d_out, (size_t)n_rows * sizeof(double), hipMemcpyDeviceToHost, slot.stream));
    if (int rc = weighted_finish(cat, name, w, n_rows)) return rc;
    std::memcpy(out, w.h_out, (size_t)n_rows * sizeof(double));
    return MCD_OK;
}

// What the two evaluations refuse, in the order of include/mcd.h; `name` opens the message, `nulls` names the pointers
int simulated_rows_usable(mcd_catalog* cat, const std::string& name, int64_t n_rows, int32_t k, bool any_null,
                          const char* nulls, const int64_t* row_sim) {
    if (int rc = simulated_usable(cat, name)) return rc;
    if (any_null) return fail(MCD_ERR_INVALID, name + ": null " + nulls);
    if (k != cat->k) return fail(MCD_ERR_INVALID, name + ": parameter rows have the wrong number of columns");
    if (n_rows < 1 || n_rows > mcd::kSimulatedMaxRows)
        return fail(MCD_ERR_INVALID, name + ": needs 1 .. " + std::to_string(mcd::kSimulatedMaxRows) + " parameter rows");
    if (cat->sim_count < 1 || !cat->d_sim)
        return fail(MCD_ERR_INVALID, name + ": no simulated set is resident (mcd_simulate or mcd_simulated_set first)");
    for (int64_t r = 0; r < n_rows; ++r)
        if (row_sim[r] < 0 || row_sim[r] >= cat->sim_count)
            return fail(MCD_ERR_INVALID, name + ": row_sim[" + std::to_string(r) + "] = " + std::to_string(row_sim[r]) +
                                             " is outside [0, " + std::to_string(cat->sim_count) + ")");
    return MCD_OK;
}

// ... and what both do between their validation and their kernel: the plan and buffers of the row count from `cache`
// (`fields` sums per row), params and simulation ids H2D, walker prep (the weighted path's staging); the device is current
// and the first timing event recorded when this returns
int simulated_stage(mcd_catalog* cat, const std::string& name, std::map<int64_t, WeightedWork>& cache, size_t fields,
                    int64_t n_rows, int32_t k, const double* params, const int64_t* row_sim, WeightedWork** out) {
    Shard& sh = cat->shards[0];
    const DeviceSlot& slot = cat->ctx->slots[sh.slot];
    MCD_HIP(hipSetDevice(slot.device));
    // (an earlier pipelined evaluation may still be in flight on the stream the plans are released and built on)
    MCD_WAIT(cat->ctx, slot.stream, cat->spin_us, (name + " (previous evaluation)").c_str());
    if (int rc = weighted_work(cat, cache, fields, sh, n_rows, out)) return rc;
    WeightedWork& w = **out;
    std::memcpy(w.h_params, params, (size_t)n_rows * k * sizeof(double));
    std::memcpy(w.h_replicate, row_sim, (size_t)n_rows * sizeof(int64_t));
    MCD_HIP(hipMemcpyAsync(w.d_params, w.h_params, (size_t)n_rows * k * sizeof(double), hipMemcpyHostToDevice, slot.stream));
    MCD_HIP(hipMemcpyAsync(w.d_replicate, w.h_replicate, (size_t)n_rows * sizeof(int64_t), hipMemcpyHostToDevice, slot.stream));
    MCD_HIP(mcd::launch_prepare_walkers(slot.stream, w.d_params, n_rows, k, cat->model, cat->free_centre, cat->precision,
                                        w.d_wpar));
    if (cat->timing) MCD_HIP(hipEventRecord(w.e0, slot.stream));
    return MCD_OK;
}

int simulated_loglike_grad(mcd_catalog* cat, int64_t n_rows, int32_t k, const double* params, const int64_t* row_sim,
                           double* out, double* grad) {
    const std::string name("mcd_simulated_loglike_grad");
    if (int rc = simulated_rows_usable(cat, name, n_rows, k, !params || !row_sim || !grad, "params, row_sim or grad", row_sim))
        return rc;
    WeightedWork* wp = nullptr;
    if (int rc = simulated_stage(cat, name, cat->simulated_grad, (size_t)(1 + k), n_rows, k, params, row_sim, &wp)) return rc;
    WeightedWork& w = *wp;
    const Shard& sh = cat->shards[0];
    const DeviceSlot& slot = cat->ctx->slots[sh.slot];
    const size_t fields = (size_t)(1 + k), padded = (size_t)mcd::padded_walkers(n_rows);
    const mcd::LaunchShape shape{cat->model, cat->free_centre, cat->precision, 0};
    MCD_HIP(mcd::launch_simulated_grad(slot.stream, shape, sh.records, w.d_chunks, w.n_chunks, w.d_params, w.d_wpar,
                                       w.d_replicate, cat->d_sim, cat->sim_count, cat->sim_bg_mean, cat->sim_bg_sigma2,
                                       w.d_partials, n_rows));
    if (cat->timing) MCD_HIP(hipEventRecord(w.e1, slot.stream));
    MCD_HIP(mcd::launch_grad_reduce(slot.stream, shape, w.d_partials, w.n_chunks, w.d_offsets, 1, w.n_chunks, n_rows, w.d_out));
    MCD_HIP(hipMemcpyAsync(w.h_out, w.d_out, fields * padded * sizeof(double), hipMemcpyDeviceToHost, slot.stream));
    if (int rc = weighted_finish(cat, name, w, n_rows)) return rc;
    if (out) std::memcpy(out, w.h_out, (size_t)n_rows * sizeof(double));
    for (int64_t j = 0; j < k; ++j) {
        const double* col = w.h_out + (1 + j) * padded;
        for (int64_t i = 0; i < n_rows; ++i) grad[i * k + j] = col[i];
    }
    return MCD_OK;
}

}  // namespace

extern "C" {

int mcd_simulate(mcd_catalog* cat, int64_t n_sims, int32_t k, const double* truths, uint64_t seed, int64_t sim0, double bg_mean,
                 double bg_sigma, double* velocities) {
    try {
    return simulate(cat, n_sims, k, truths, seed, sim0, bg_mean, bg_sigma, velocities);
    } catch (...) { return on_exception("mcd_simulate"); }
}

int mcd_simulated_set(mcd_catalog* cat, int64_t n_sims, const double* velocities, double bg_mean, double bg_sigma) {
    try {
    return simulated_set(cat, n_sims, velocities, bg_mean, bg_sigma);
    } catch (...) { return on_exception("mcd_simulated_set"); }
}

int mcd_simulated_loglike(mcd_catalog* cat, int64_t n_rows, int32_t k, const double* params, const int64_t* row_sim,
                          double* out) {
    try {
    return simulated_loglike(cat, n_rows, k, params, row_sim, out);
    } catch (...) { return on_exception("mcd_simulated_loglike"); }
}

int mcd_simulated_loglike_grad(mcd_catalog* cat, int64_t n_rows, int32_t k, const double* params, const int64_t* row_sim,
                               double* out, double* grad) {
    try {
    return simulated_loglike_grad(cat, n_rows, k, params, row_sim, out, grad);
    } catch (...) { return on_exception("mcd_simulated_loglike_grad"); }
}

int mcd_simulated_info(const mcd_catalog* cat, int64_t* n_sims) {
    try {
    if (!cat || !n_sims) return fail(MCD_ERR_INVALID, "mcd_simulated_info: null argument");
    *n_sims = cat->sim_count;
    return MCD_OK;
    } catch (...) { return on_exception("mcd_simulated_info"); }
}

}  // extern "C"

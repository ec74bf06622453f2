// mcd_api_replicate.hip -- C-ABI of the MI355X log-likelihood library (see include/mcd.h; mcd_host.h lists the host units):
// host driver of the replicated-data predictive checks.  mcd_replicate_check: S sample rows against the stars of R ranges
// of an index array, in passes over the rows (kernels: mcd_replicate.hip; term, generator, validation and plan:
// mcd_replicate.h).  mcd_replicate_numbers: the generator's numbers on the host.
#include "mcd_host.h"
#include "mcd_replicate.h"

using namespace mcd::host;

namespace {

int replicate_check(mcd_catalog* cat, int64_t S, int32_t k, const double* params, uint64_t seed, int32_t R,
                    const int64_t* offs, const int64_t* order, double bg_mean, double bg_sigma, double* out) {
    const std::string name("mcd_replicate_check");
    if (!cat || !params || !out) return fail(MCD_ERR_INVALID, name + ": null catalogue, params or out");
    if (int rc = ctx_usable(cat->ctx)) return rc;
    if (cat->n_psets != 1) return fail(MCD_ERR_INVALID, name + ": defined for un-binned catalogues only");
    if (cat->precision != MCD_F64) return fail(MCD_ERR_INVALID, name + ": needs an MCD_F64 catalogue");
    if (cat->ctx->has_comm() || cat->shards.size() != 1)
        return fail(MCD_ERR_INVALID, name + ": one device per process (no several devices, no communicator)");
    std::vector<uint8_t> seen;
    if (const char* why = mcd::replicate_groups_error(R, offs, order, cat->n_stars, seen))
        return fail(MCD_ERR_INVALID, name + ": " + why);
    if (const char* why = mcd::replicate_background_error(cat->model, bg_mean, bg_sigma))
        return fail(MCD_ERR_INVALID, name + ": " + why);
    if (S < 1) return fail(MCD_ERR_INVALID, name + ": needs at least one sample row");
    if (k != cat->k) return fail(MCD_ERR_INVALID, name + ": parameter rows have the wrong number of columns");
    const int64_t n_used = offs[R];
    const mcd::ReplicatePlan plan = mcd::replicate_plan(R, offs, S, cat->chunk_len);
    const int64_t P = plan.pass_rows, n_chunks = (int64_t)plan.chunks.chunks.size();
    const int64_t lane_bytes = (int64_t)mcd::kRepLaneDoubles * (int64_t)sizeof(double);
    if (n_chunks * P * lane_bytes > mcd::kRepScratchBytes || (int64_t)R * P * lane_bytes > mcd::kRepScratchBytes)
        return fail(MCD_ERR_INVALID, name + ": the partial sums of " + std::to_string(n_chunks) + " chunks in " +
                                         std::to_string(R) + " ranges exceed the scratch budget of " +
                                         std::to_string(mcd::kRepScratchBytes >> 20) + " MiB (fewer ranges per call)");
    Shard& sh = cat->shards[0];
    const DeviceSlot& slot = cat->ctx->slots[sh.slot];
    MCD_HIP(hipSetDevice(slot.device));
    // (an earlier pipelined evaluation may still be in flight on the stream)
    MCD_WAIT(cat->ctx, slot.stream, cat->spin_us, "mcd_replicate_check (previous evaluation)");
    DeviceScratch d;
    int64_t *d_order = nullptr, *d_offsets = nullptr;
    mcd::Chunk* d_chunks = nullptr;
    double *d_params = nullptr, *d_partials = nullptr, *d_out = nullptr;
    void* d_wpar = nullptr;
    const size_t out_row = (size_t)R * mcd::kRepLaneDoubles;
    MCD_HIP(d.malloc(&d_order, std::max<size_t>(1, (size_t)n_used) * sizeof(int64_t)));
    MCD_HIP(d.malloc(&d_offsets, plan.chunks.offsets.size() * sizeof(int64_t)));
    MCD_HIP(d.malloc(&d_chunks, std::max<size_t>(1, (size_t)n_chunks) * sizeof(mcd::Chunk)));
    MCD_HIP(d.malloc(&d_params, (size_t)P * k * sizeof(double)));
    MCD_HIP(d.malloc(&d_wpar, (size_t)P * mcd::KD * sizeof(double)));
    MCD_HIP(d.malloc(&d_partials, std::max<size_t>(1, (size_t)(n_chunks * P)) * lane_bytes));
    MCD_HIP(d.malloc(&d_out, (size_t)P * out_row * sizeof(double)));
    if (n_used > 0) MCD_HIP(hipMemcpy(d_order, order, (size_t)n_used * sizeof(int64_t), hipMemcpyHostToDevice));
    if (n_chunks > 0)
        MCD_HIP(hipMemcpy(d_chunks, plan.chunks.chunks.data(), (size_t)n_chunks * sizeof(mcd::Chunk), hipMemcpyHostToDevice));
    MCD_HIP(hipMemcpy(d_offsets, plan.chunks.offsets.data(), plan.chunks.offsets.size() * sizeof(int64_t), hipMemcpyHostToDevice));
    if (cat->timing) MCD_HIP(d.create_events());
    const mcd::LaunchShape shape{cat->model, cat->free_centre, cat->precision, 0};
    const double bg_sigma2 = bg_sigma * bg_sigma;
    double kernel_ms = 0.0;
    // Samples are independent: a pass is the staging of section 3.9 (params H2D, walker prep), the main kernel with the
    // generator's row index of its first row, the reduction, and its rows of the output
    for (int64_t s0 = 0; s0 < S; s0 += P) {
        const int64_t ns = std::min(P, S - s0);
        MCD_HIP(hipMemcpyAsync(d_params, params + (size_t)s0 * k, (size_t)ns * k * sizeof(double), hipMemcpyHostToDevice, slot.stream));
        MCD_HIP(mcd::launch_prepare_walkers(slot.stream, d_params, ns, k, cat->model, cat->free_centre, cat->precision, d_wpar));
        if (cat->timing) MCD_HIP(hipEventRecord(d.e0, slot.stream));
        MCD_HIP(mcd::launch_replicate(slot.stream, shape, sh.records, d_order, d_chunks, n_chunks, d_wpar, ns,
                                      cat->replicate_row0 + s0, seed, bg_mean, bg_sigma2, d_partials));
        if (cat->timing) MCD_HIP(hipEventRecord(d.e1, slot.stream));
        MCD_HIP(mcd::launch_replicate_reduce(slot.stream, d_partials, d_offsets, R, ns, d_out));
        MCD_HIP(hipMemcpyAsync(out + (size_t)s0 * out_row, d_out, (size_t)ns * out_row * sizeof(double), hipMemcpyDeviceToHost,
                               slot.stream));
        MCD_WAIT(cat->ctx, slot.stream, cat->spin_us, "mcd_replicate_check");
        if (cat->timing) {
            float ms = 0.f;
            MCD_HIP(hipEventElapsedTime(&ms, d.e0, d.e1));
            kernel_ms += ms;
        }
    }
    if (cat->timing) {
        cat->last_kernel_ms = kernel_ms;
        cat->timing_pending = false;
    }
    cat->last_chunks = n_chunks;
    cat->last_grid = mcd::main_grid(n_chunks, P);
    return MCD_OK;
}

}  // namespace

extern "C" {

int mcd_replicate_check(mcd_catalog* cat, int64_t n_samples, int32_t k, const double* params, uint64_t seed, int32_t n_ranges,
                        const int64_t* range_offsets, const int64_t* order, double bg_mean, double bg_sigma, double* out) {
    try {
    return replicate_check(cat, n_samples, k, params, seed, n_ranges, range_offsets, order, bg_mean, bg_sigma, out);
    } catch (...) { return on_exception("mcd_replicate_check"); }
}

int mcd_replicate_numbers(uint64_t seed, int64_t sample0, int64_t n_samples, int64_t star0, int64_t n_stars, double* g,
                          double* u) {
    try {
    if (sample0 < 0 || n_samples < 0 || star0 < 0 || n_stars < 0 || (!g && !u))
        return fail(MCD_ERR_INVALID, "mcd_replicate_numbers: bad arguments");
    for (int64_t s = 0; s < n_samples; ++s)
        for (int64_t i = 0; i < n_stars; ++i) {
            if (g) g[s * n_stars + i] = mcd::rep_normal(seed, sample0 + s, star0 + i);
            if (u) u[s * n_stars + i] = mcd::rep_uniform(seed, sample0 + s, star0 + i);
        }
    return MCD_OK;
    } catch (...) { return on_exception("mcd_replicate_numbers"); }
}

}  // extern "C"

// mcd_api_diag.hip -- C-ABI of the MI355X log-likelihood library (see include/mcd.h; mcd_host.h lists the host units): host
// driver of the chain convergence diagnostics (kernels: mcd_diag.hip; the arithmetic, and the loop that runs without a
// context, mcd_diag.h).
#include "mcd_host.h"
#include "mcd_diag.h"

using namespace mcd::host;

namespace {

struct DiagOut {
    double* tau;
    int64_t* window;
    int32_t* found;
    double *rhat, *mean, *var, *rho;
};

// what mcd_chain_diagnostics_info reports: the last call of this thread
thread_local int64_t g_tile_groups = 0, g_tiles = 0;
thread_local double g_kernel_ms = 0.0;

int check(const mcd_diag_desc* d, const double* chain, const DiagOut& o) {
    if (!d || !chain) return fail(MCD_ERR_INVALID, "mcd_chain_diagnostics: null descriptor or chain");
    if (!o.tau || !o.window || !o.found || !o.rhat || !o.mean || !o.var)
        return fail(MCD_ERR_INVALID, "mcd_chain_diagnostics: only rho may be NULL among the outputs");
    if (d->n_groups < 1 || d->n_walkers < 1 || d->n_dim < 1)
        return fail(MCD_ERR_INVALID, "mcd_chain_diagnostics: n_groups, n_walkers and n_dim must be >= 1");
    if (d->n_steps < 2) return fail(MCD_ERR_INVALID, "mcd_chain_diagnostics: n_steps must be >= 2");
    if (d->max_lag < 1 || d->max_lag > d->n_steps - 1)
        return fail(MCD_ERR_INVALID, "mcd_chain_diagnostics: max_lag = " + std::to_string(d->max_lag) + " is outside [1, n_steps - 1 = " +
                                         std::to_string(d->n_steps - 1) + "]");
    if (!(d->c > 0.0) || !std::isfinite(d->c)) return fail(MCD_ERR_INVALID, "mcd_chain_diagnostics: c must be > 0 and finite");
    if (d->scratch_mb < 0) return fail(MCD_ERR_INVALID, "mcd_chain_diagnostics: scratch_mb must be >= 0 (0: 1024)");
    // (sizes as int64 byte counts: every product below stays far inside the range for a chain that fits host memory)
    const long double cells = (long double)d->n_steps * d->n_groups * d->n_walkers * d->n_dim;
    if (cells > 1.0e17L) return fail(MCD_ERR_INVALID, "mcd_chain_diagnostics: the chain has more than 1e17 samples");
    return MCD_OK;
}

int on_host(const mcd_diag_desc* d, const double* chain, const DiagOut& o) {
    const int64_t ns = d->n_walkers * d->n_dim;
    std::vector<double> a((size_t)(d->max_lag + 1) * ns), mom((size_t)mcd::kDiagMoments * ns);
    mcd::diag_host_groups(chain, d->n_steps, d->n_groups, d->n_walkers, d->n_dim, d->max_lag, d->c, 0, d->n_groups, a.data(),
                          mom.data(), o.tau, o.window, o.found, o.rhat, o.mean, o.var, o.rho);
    g_tile_groups = d->n_groups;
    g_tiles = 1;
    return MCD_OK;
}

// Tiles of whole groups within the scratch budget: the tile's series to the device by one strided copy, four kernels, the
// tile's rows of every output back.  A group's numbers depend on its own series only: the plan changes no bit.
int on_device(mcd_ctx* ctx, const mcd_diag_desc* d, const double* chain, const DiagOut& o) {
    if (ctx->slots.empty()) return fail(MCD_ERR_INVALID, "mcd_chain_diagnostics: the context has no device");
    if (int rc = ctx_usable(ctx)) return rc;
    const int64_t T = d->n_steps, G = d->n_groups, W = d->n_walkers, L = d->max_lag;
    const int P = d->n_dim;
    const int64_t mb = d->scratch_mb > 0 ? d->scratch_mb : 1024;
    const int64_t tg = mcd::diag_tile_groups(T, G, W, P, L, mb * (int64_t)1048576);
    if (tg < 1)
        return fail(MCD_ERR_INVALID, "mcd_chain_diagnostics: scratch_mb = " + std::to_string(mb) + " cannot hold one group's series and lag sums (" +
                                         std::to_string(mcd::diag_group_bytes(T, W, P, L)) + " bytes)");
    const DeviceSlot& slot = ctx->slots[0];
    MCD_HIP(hipSetDevice(slot.device));
    const int64_t ns_max = tg * W * P, rows_max = tg * P, row_bytes = G * W * P * (int64_t)sizeof(double);
    DeviceScratch sc;
    double *d_x = nullptr, *d_a = nullptr, *d_mom = nullptr, *d_rho = nullptr, *d_f64 = nullptr;
    int64_t* d_window = nullptr;
    int32_t* d_found = nullptr;
    MCD_HIP(sc.malloc(&d_x, (size_t)T * ns_max * sizeof(double)));
    MCD_HIP(sc.malloc(&d_a, (size_t)(L + 1) * ns_max * sizeof(double)));
    MCD_HIP(sc.malloc(&d_mom, (size_t)mcd::kDiagMoments * ns_max * sizeof(double)));
    MCD_HIP(sc.malloc(&d_rho, (size_t)rows_max * (L + 1) * sizeof(double)));
    MCD_HIP(sc.malloc(&d_f64, (size_t)4 * rows_max * sizeof(double)));      // tau | rhat | mean | var
    MCD_HIP(sc.malloc(&d_window, (size_t)rows_max * sizeof(int64_t)));
    MCD_HIP(sc.malloc(&d_found, (size_t)rows_max * sizeof(int32_t)));
    MCD_HIP(sc.create_events());
    g_tile_groups = tg;
    for (int64_t g0 = 0; g0 < G; g0 += tg) {
        const int64_t ng = std::min(tg, G - g0), ns = ng * W * P, rows = ng * P;
        const size_t width = (size_t)ns * sizeof(double);
        if (ng == G)
            MCD_HIP(hipMemcpyAsync(d_x, chain, (size_t)T * width, hipMemcpyHostToDevice, slot.stream));
        else
            MCD_HIP(hipMemcpy2DAsync(d_x, width, chain + g0 * W * P, (size_t)row_bytes, width, (size_t)T, hipMemcpyHostToDevice,
                                     slot.stream));
        MCD_HIP(hipEventRecord(sc.e0, slot.stream));
        MCD_HIP(mcd::launch_diag(slot.stream, d_x, T, ng, W, P, L, d->c, d_a, d_mom, d_rho, d_f64, d_window, d_found,
                                 d_f64 + rows_max, d_f64 + 2 * rows_max, d_f64 + 3 * rows_max));
        MCD_HIP(hipEventRecord(sc.e1, slot.stream));
        double* const f64_out[4] = {o.tau, o.rhat, o.mean, o.var};
        for (int f = 0; f < 4; ++f)
            MCD_HIP(hipMemcpyAsync(f64_out[f] + g0 * P, d_f64 + f * rows_max, (size_t)rows * sizeof(double), hipMemcpyDeviceToHost,
                                   slot.stream));
        MCD_HIP(hipMemcpyAsync(o.window + g0 * P, d_window, (size_t)rows * sizeof(int64_t), hipMemcpyDeviceToHost, slot.stream));
        MCD_HIP(hipMemcpyAsync(o.found + g0 * P, d_found, (size_t)rows * sizeof(int32_t), hipMemcpyDeviceToHost, slot.stream));
        if (o.rho)
            MCD_HIP(hipMemcpyAsync(o.rho + g0 * P * (L + 1), d_rho, (size_t)rows * (L + 1) * sizeof(double), hipMemcpyDeviceToHost,
                                   slot.stream));
        // (the scratch is reused by the next tile: wait here, under the context's deadline)
        MCD_WAIT(ctx, slot.stream, 20000, "mcd_chain_diagnostics");
        float ms = 0.f;
        MCD_HIP(hipEventElapsedTime(&ms, sc.e0, sc.e1));
        g_kernel_ms += ms;
        ++g_tiles;
    }
    return MCD_OK;
}

}  // namespace

extern "C" {

int mcd_chain_diagnostics(mcd_ctx* ctx, const mcd_diag_desc* d, const double* chain, double* tau, int64_t* window,
                          int32_t* found, double* rhat, double* mean, double* var, double* rho) {
    try {
    g_tile_groups = g_tiles = 0;
    g_kernel_ms = 0.0;
    const DiagOut o{tau, window, found, rhat, mean, var, rho};
    if (int rc = check(d, chain, o)) return rc;
    return ctx ? on_device(ctx, d, chain, o) : on_host(d, chain, o);
    } catch (...) { return on_exception("mcd_chain_diagnostics"); }
}

int mcd_chain_diagnostics_info(int64_t* tile_groups, int64_t* n_tiles, double* kernel_ms) {
    if (tile_groups) *tile_groups = g_tile_groups;
    if (n_tiles) *n_tiles = g_tiles;
    if (kernel_ms) *kernel_ms = g_kernel_ms;
    return MCD_OK;
}

}  // extern "C"

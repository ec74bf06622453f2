// mcd_api_mmatch.hip -- C-ABI of the MI355X log-likelihood library (see include/mcd.h; mcd_host.h lists the host units):
// host driver of mcd_moment_match.  Stars run in lock-stepped groups of floor(65536 / S); rows, weights, moments and kernel
// tables of a group stay on the device for the whole call, every round is transform -> hold-out evaluation -> weights on
// the catalogue's stream, and only the per-star scalars (k^, the sums, two flags) come back for the decisions of
// mcd_mmatch.h (MmState).  Kernels: mcd_mmatch.hip and, for the evaluation, mcd_holdout.hip.
#include "mcd_host.h"
#include "mcd_holdout.h"
#include "mcd_mmatch.h"
#include "mcd_psis.h"

using namespace mcd::host;

namespace {

struct MmOutputs {
    double *elpd, *pareto_k, *n_eff, *k_before, *k_loop;
    int32_t *iterations, *accepted;
    double *A, *b;
};

// One group of g stars (stars: their catalogue indices).  res: [g] rows of the outputs, written by the caller on success.
struct MmResult {
    double elpd = 0.0, k = 0.0, n_eff = 0.0, k_before = 0.0, k_loop = 0.0;
    mcd::MmState st;
    std::vector<double> map;
};

int match_group(mcd_catalog* cat, const mcd_mmatch_desc* d, const PriorHost& ph, int64_t S, int64_t M, const double* d_draws,
                const int64_t* stars, int64_t g, double* kernel_ms, MmResult* res) {
    const mcd_stretch_desc& m = d->map;
    const int P = m.n_dim, K = m.k;
    const int nm = mcd::mm_map_doubles(P);
    Shard& sh = cat->shards[0];
    const DeviceSlot& slot = cat->ctx->slots[sh.slot];
    std::vector<int64_t> star_range;
    const std::vector<int64_t> ranges = mcd::mm_ranges(cat->n_stars, stars, g, star_range);
    HoldoutWork* wp = nullptr;
    if (int rc = holdout_device_plan(cat, ranges, g * S, &wp)) return rc;
    HoldoutWork& w = *wp;

    DeviceScratch sc;
    mcd::MmDevice dev;
    dev.P = P; dev.K = K; dev.fixed_ok = m.fixed_ok; dev.S = S; dev.M = M; dev.G = g;
    dev.draws = d_draws;
    // the descriptor's arrays in one block of doubles and one of int32
    const size_t n_dbl = (size_t)2 * K + (size_t)5 * P;
    std::vector<double> hd(n_dbl);
    std::vector<int32_t> hi32((size_t)K + P);
    for (int c = 0; c < K; ++c) { hd[c] = m.col_const[c]; hd[K + c] = m.col_factor[c]; hi32[c] = m.col_source[c]; }
    for (int c = 0; c < P; ++c) {
        hd[2 * K + c] = m.lo[c]; hd[2 * K + P + c] = m.hi[c];
        hd[2 * K + 2 * P + c] = ph.table.any() ? ph.loc[c] : 0.0;
        hd[2 * K + 3 * P + c] = ph.table.any() ? ph.scale[c] : 1.0;
        hd[2 * K + 4 * P + c] = ph.table.any() ? ph.c0[c] : 0.0;
        hi32[K + c] = ph.table.any() ? ph.kind[c] : 0;
    }
    double* d_dbl = nullptr;
    int32_t *d_i32 = nullptr, *d_ctrl = nullptr;
    int64_t* d_range = nullptr;
    double* d_inv = nullptr;
    MCD_HIP(sc.malloc(&d_dbl, n_dbl * 8));
    MCD_HIP(sc.malloc(&d_i32, hi32.size() * 4));
    MCD_HIP(sc.malloc(&d_ctrl, (size_t)4 * g * 4));                          // level [g], sel [g], flags [g][2]
    MCD_HIP(sc.malloc(&d_range, (size_t)g * 8));
    MCD_HIP(sc.malloc(&dev.rows, (size_t)2 * g * S * P * 8));
    MCD_HIP(sc.malloc(&dev.wts, (size_t)2 * g * S * 8));
    MCD_HIP(sc.malloc(&dev.li, (size_t)2 * g * S * 8));
    MCD_HIP(sc.malloc(&dev.stat, (size_t)2 * g * mcd::MS_FIELDS * 8));
    MCD_HIP(sc.malloc(&dev.maps, (size_t)2 * g * nm * 8));
    MCD_HIP(sc.malloc(&d_inv, (size_t)g * (nm + 1) * 8));                    // the inverse maps, then log|det A| [g]
    MCD_HIP(sc.malloc(&dev.mom, (size_t)g * mcd::mm_moment_doubles(P) * 8));
    MCD_HIP(sc.malloc(&dev.inside, (size_t)g * S * 4));
    MCD_HIP(sc.malloc(&dev.lnprior, (size_t)g * S * 8));
    MCD_HIP(sc.malloc(&dev.lp0, (size_t)g * S * 8));
    MCD_HIP(sc.malloc(&dev.lw, (size_t)g * S * 8));
    MCD_HIP(sc.malloc(&dev.num, (size_t)g * S * 8));
    MCD_HIP(sc.malloc(&dev.lpf, (size_t)g * S * 8));
    MCD_HIP(hipMemcpy(d_dbl, hd.data(), n_dbl * 8, hipMemcpyHostToDevice));
    MCD_HIP(hipMemcpy(d_i32, hi32.data(), hi32.size() * 4, hipMemcpyHostToDevice));
    MCD_HIP(hipMemcpy(d_range, star_range.data(), (size_t)g * 8, hipMemcpyHostToDevice));
    dev.col_const = d_dbl; dev.col_factor = d_dbl + K; dev.lo = d_dbl + 2 * K; dev.hi = dev.lo + P;
    dev.col_source = d_i32;
    if (ph.table.any()) {
        dev.prior.kind = d_i32 + K;
        dev.prior.loc = dev.hi + P; dev.prior.scale = dev.hi + 2 * P; dev.prior.c0 = dev.hi + 3 * P;
    }
    dev.level = d_ctrl; dev.sel = d_ctrl + g; dev.flags = d_ctrl + 2 * g;
    dev.inv = d_inv; dev.logdet = d_inv + (size_t)g * nm;
    dev.table = w.d_params; dev.out = w.d_out;

    std::vector<int32_t> ctrl((size_t)2 * g, 0), flags((size_t)2 * g, 0);
    std::vector<double> stat((size_t)2 * g * mcd::MS_FIELDS);
    int32_t* level = ctrl.data();
    int32_t* sel = ctrl.data() + g;
    // one round: every star's level of this launch -> the scalars of what it wrote (buffer 1 - sel)
    auto round = [&](bool moments) -> int {
        MCD_HIP(hipMemcpyAsync(d_ctrl, ctrl.data(), (size_t)2 * g * 4, hipMemcpyHostToDevice, slot.stream));
        if (moments) MCD_HIP(mcd::launch_mm_moments(slot.stream, dev));
        MCD_HIP(mcd::launch_mm_transform(slot.stream, dev));
        if (int rc = holdout_device_eval(cat, w, S, d_range)) return rc;
        MCD_HIP(mcd::launch_mm_weights(slot.stream, dev));
        MCD_HIP(hipMemcpyAsync(stat.data(), dev.stat, stat.size() * 8, hipMemcpyDeviceToHost, slot.stream));
        MCD_HIP(hipMemcpyAsync(flags.data(), dev.flags, flags.size() * 4, hipMemcpyDeviceToHost, slot.stream));
        MCD_WAIT(cat->ctx, slot.stream, cat->spin_us, "mcd_moment_match");
        if (cat->timing) {
            float ms = 0.f;
            MCD_HIP(hipEventElapsedTime(&ms, w.e0, w.e1));
            *kernel_ms += ms;
        }
        return MCD_OK;
    };
    auto stat_of = [&](int buf, int64_t e) { return stat.data() + ((size_t)buf * g + e) * mcd::MS_FIELDS; };

    // baseline
    for (int64_t e = 0; e < g; ++e) { level[e] = mcd::MM_BASE; sel[e] = 0; }
    if (int rc = round(false)) return rc;
    const int max_level = mcd::mm_max_level(d->cov, S, P);
    for (int64_t e = 0; e < g; ++e) {
        if (flags[2 * e + 1] != 0)
            return fail(MCD_ERR_NONFINITE, "mcd_moment_match: " + std::to_string(flags[2 * e + 1]) + " of the draws lie outside the prior");
        sel[e] = 1;
        const double k0 = stat_of(1, e)[mcd::MS_K];
        res[e].k_before = k0;
        mcd::mm_begin(res[e].st, k0, d->k_threshold, d->max_iters);
    }
    // the loop, all stars of the group in lock step
    for (;;) {
        bool any = false;
        for (int64_t e = 0; e < g; ++e) {
            level[e] = res[e].st.running ? res[e].st.level : (int32_t)mcd::MM_KEEP;
            any = any || res[e].st.running;
        }
        if (!any) break;
        if (int rc = round(true)) return rc;
        for (int64_t e = 0; e < g; ++e) {
            if (!res[e].st.running) continue;
            const bool usable = flags[2 * e] == 0 && flags[2 * e + 1] < S;
            if (mcd::mm_decide(res[e].st, stat_of(1 - sel[e], e)[mcd::MS_K], usable, d->k_threshold, d->max_iters, max_level))
                sel[e] = 1 - sel[e];
        }
    }
    // the total maps; what the loop left
    std::vector<double> maps((size_t)2 * g * nm);
    MCD_HIP(hipMemcpyAsync(maps.data(), dev.maps, maps.size() * 8, hipMemcpyDeviceToHost, slot.stream));
    MCD_HIP(hipMemcpyAsync(stat.data(), dev.stat, stat.size() * 8, hipMemcpyDeviceToHost, slot.stream));
    MCD_WAIT(cat->ctx, slot.stream, cat->spin_us, "mcd_moment_match");
    std::vector<int> final_buf((size_t)g);
    bool any_split = false;
    std::vector<double> inv((size_t)g * (nm + 1), 0.0), work((size_t)2 * P * P);
    for (int64_t e = 0; e < g; ++e) {
        MmResult& r = res[e];
        r.k_loop = r.st.k;
        final_buf[e] = sel[e];
        const double* mp = maps.data() + ((size_t)sel[e] * g + e) * nm;
        r.map.assign(mp, mp + nm);
        level[e] = mcd::MM_KEEP;
        const int n_acc = r.st.accepted[0] + r.st.accepted[1] + r.st.accepted[2];
        if (n_acc == 0) mcd::mm_identity(P, r.map.data(), r.map.data() + P * P);      // (the baseline's map, exactly)
        if (d->split && n_acc > 0 &&
            mcd::mm_inverse(P, mp, mp + P * P, inv.data() + (size_t)e * nm, inv.data() + (size_t)e * nm + P * P,
                            inv.data() + (size_t)g * nm + e, work.data())) {
            level[e] = mcd::MM_SPLIT_FWD;
            any_split = true;
        }
    }
    if (any_split) {
        MCD_HIP(hipMemcpyAsync(d_inv, inv.data(), inv.size() * 8, hipMemcpyHostToDevice, slot.stream));
        if (int rc = round(false)) return rc;
        for (int64_t e = 0; e < g; ++e)
            if (level[e] == mcd::MM_SPLIT_FWD) level[e] = mcd::MM_SPLIT_INV;
        if (int rc = round(false)) return rc;
        for (int64_t e = 0; e < g; ++e)
            if (level[e] == mcd::MM_SPLIT_INV) final_buf[e] = 1 - sel[e];
    }
    for (int64_t e = 0; e < g; ++e) {
        const double* st = stat_of(final_buf[e], e);
        res[e].elpd = st[mcd::MS_ELPD];
        res[e].k = st[mcd::MS_K];
        res[e].n_eff = d->r_eff * (st[mcd::MS_A1] * st[mcd::MS_A1]) / st[mcd::MS_A2];
    }
    return MCD_OK;
}

int moment_match(mcd_catalog* cat, const mcd_mmatch_desc* d, const mcd_prior_desc* prior, int64_t S, const double* draws,
                 int64_t n_match, const int64_t* stars, const MmOutputs& o) {
    const char* who = "mcd_moment_match";
    if (!cat || !d || !draws) return fail(MCD_ERR_INVALID, std::string(who) + ": null catalogue, descriptor or draws");
    if (int rc = ctx_usable(cat->ctx)) return rc;
    const mcd_stretch_desc& m = d->map;
    if (m.n_bins > 1 || cat->n_psets != 1) return fail(MCD_ERR_INVALID, std::string(who) + ": defined for un-binned catalogues only");
    if (cat->precision != MCD_F64) return fail(MCD_ERR_INVALID, std::string(who) + ": needs an MCD_F64 catalogue");
    if (cat->ctx->has_comm() || cat->shards.size() != 1)
        return fail(MCD_ERR_INVALID, std::string(who) + ": one device per process (no several devices, no communicator)");
    if (m.k != cat->k) return fail(MCD_ERR_INVALID, std::string(who) + ": descriptor has the wrong number of kernel columns");
    if (m.n_dim < 1 || m.n_dim > mcd::kMmMaxDim) return fail(MCD_ERR_INVALID, std::string(who) + ": 1 <= n_dim <= 12");
    if (!m.col_source || !m.col_const || !m.col_factor || !m.lo || !m.hi) return fail(MCD_ERR_INVALID, std::string(who) + ": null descriptor array");
    for (int c = 0; c < m.k; ++c)
        if (m.col_source[c] >= m.n_dim) return fail(MCD_ERR_INVALID, std::string(who) + ": col_source outside the free parameters");
    if (d->max_iters < 0) return fail(MCD_ERR_INVALID, std::string(who) + ": max_iters must be >= 0");
    if (!(d->r_eff > 0.0) || !std::isfinite(d->r_eff)) return fail(MCD_ERR_INVALID, std::string(who) + ": r_eff must be a finite positive number");
    if (S < 2 || S > mcd::kMmMaxRows) return fail(MCD_ERR_INVALID, std::string(who) + ": 2 <= n_samples <= " + std::to_string(mcd::kMmMaxRows));
    const int64_t M = mcd::psis_tail_len(S, d->r_eff);
    if (M < 5 || M > mcd::kPsisMaxTail || M >= S)
        return fail(MCD_ERR_INVALID, std::string(who) + ": the PSIS tail of " + std::to_string(S) + " samples has " + std::to_string(M) +
                                         " values (5 .. " + std::to_string(mcd::kPsisMaxTail) + " and fewer than the samples)");
    if (const char* why = mcd::mm_stars_error(n_match, stars, cat->n_stars)) return fail(MCD_ERR_INVALID, std::string(who) + ": " + why);
    PriorHost ph;
    if (int rc = prior_of(prior, m.n_dim, who, ph)) return rc;

    const int P = m.n_dim;
    const int64_t G = mcd::kMmMaxRows / S;
    Shard& sh = cat->shards[0];
    const DeviceSlot& slot = cat->ctx->slots[sh.slot];
    MCD_HIP(hipSetDevice(slot.device));
    MCD_WAIT(cat->ctx, slot.stream, cat->spin_us, "mcd_moment_match (previous evaluation)");
    DeviceScratch sc;
    double* d_draws = nullptr;
    MCD_HIP(sc.malloc(&d_draws, (size_t)S * P * 8));
    MCD_HIP(hipMemcpy(d_draws, draws, (size_t)S * P * 8, hipMemcpyHostToDevice));
    std::vector<MmResult> res((size_t)n_match);
    double kernel_ms = 0.0;
    for (int64_t e0 = 0; e0 < n_match; e0 += G) {
        const int64_t g = std::min(G, n_match - e0);
        if (int rc = match_group(cat, d, ph, S, M, d_draws, stars + e0, g, &kernel_ms, res.data() + e0)) return rc;
    }
    if (cat->timing) {
        cat->last_kernel_ms = kernel_ms;
        cat->timing_pending = false;
    }
    for (int64_t e = 0; e < n_match; ++e) {
        const MmResult& r = res[(size_t)e];
        if (o.elpd) o.elpd[e] = r.elpd;
        if (o.pareto_k) o.pareto_k[e] = r.k;
        if (o.n_eff) o.n_eff[e] = r.n_eff;
        if (o.k_before) o.k_before[e] = r.k_before;
        if (o.k_loop) o.k_loop[e] = r.k_loop;
        if (o.iterations) o.iterations[e] = r.st.iterations;
        if (o.accepted) std::memcpy(o.accepted + 3 * e, r.st.accepted, 3 * sizeof(int32_t));
        if (o.A) std::memcpy(o.A + (size_t)e * P * P, r.map.data(), (size_t)P * P * 8);
        if (o.b) std::memcpy(o.b + (size_t)e * P, r.map.data() + P * P, (size_t)P * 8);
    }
    return MCD_OK;
}

}  // namespace

extern "C" {

int mcd_moment_match(mcd_catalog* cat, const mcd_mmatch_desc* d, const mcd_prior_desc* prior, int64_t n_samples,
                     const double* draws, int64_t n_match, const int64_t* stars, double* elpd, double* pareto_k, double* n_eff,
                     double* k_before, double* k_loop, int32_t* iterations, int32_t* accepted, double* A, double* b) {
    try {
    return moment_match(cat, d, prior, n_samples, draws, n_match, stars,
                        MmOutputs{elpd, pareto_k, n_eff, k_before, k_loop, iterations, accepted, A, b});
    } catch (...) { return on_exception("mcd_moment_match"); }
}

}  // extern "C"

// mcd_api_de.hip -- C-ABI of the MI355X log-likelihood library (see include/mcd.h; mcd_host.h lists the host units):
// mcd_de_move / mcd_de_move_seeded, the differential-evolution move of mcd_de.h as a block resident on the device (kernels:
// mcd_de.hip) or driven from the host (mcd_de.h: de_block), mcd_de_numbers and mcd_de_info.
#include "mcd_host.h"
#include "mcd_prior.h"
#include "mcd_rng.h"
#include "mcd_de.h"

using namespace mcd::host;

namespace {

// the numbers of a block: the caller's arrays, or (seeded) what names them
struct DeNumbers {
    const int32_t* order = nullptr;
    const int32_t* pick_a = nullptr;
    const int32_t* pick_b = nullptr;
    const double* gamma = nullptr;
    const double* thr = nullptr;
    bool seeded = false;
    uint64_t seed = 0;
    int64_t step0 = 0;
    double gamma0 = 0.0, sigma = 0.0;
};

// ------------------------------------------------------------------------------------------------
// The block with the ensembles resident on the device: one chain of launches (step kernel, main kernel, reduction) per
// half step, enqueued ahead; the host waits once.  *done = false when the block has to be run host-driven: the
// configuration is not covered (anything but a float64 catalogue on one device in one process), or the device met
// something only the host loop handles (mcd::ChainStatus).  `pos`, `lnp`, `accepted` and the chain rows are then untouched.
int de_block_device(mcd_catalog* cat, const mcd_stretch_desc* d, int64_t n_steps, double* pos, double* lnp, const DeNumbers& num,
                    double* chain, double* lnprob_chain, int64_t* accepted, bool* done, const mcd::PriorTable& prior) {
    *done = false;
    mcd_ctx* ctx = cat->ctx;
    if (int urc = ctx_usable(ctx)) return urc;
    const int64_t B = cat->n_psets;
    if (!cat->device_chain || cat->shards.size() != 1 || ctx->n_ranks > 1 || ctx->force_collective || cat->precision != MCD_F64 ||
        n_steps < 1 || cat->timing || !d->fixed_ok)
        return MCD_OK;
    if (cat->de_backoff > 0) { --cat->de_backoff; return MCD_OK; }
    const int64_t W = d->n_walkers, half = W / 2;
    const int P = d->n_dim, K = d->k;
    Shard& sh = cat->shards[0];
    const DeviceSlot& slot = ctx->slots[sh.slot];
    MCD_HIP(hipSetDevice(slot.device));
    WorkSet* wp = nullptr;
    int rc = build_workset(cat, sh, half, &wp);
    if (rc != MCD_OK) return rc;
    WorkSet& w = *wp;
    // nothing of an earlier call may still use the work buffers or the arena
    MCD_WAIT(cat->ctx, slot.stream, cat->spin_us, "mcd_de_move (previous evaluation)");
    MCD_WAIT(cat->ctx, slot.stream2, cat->spin_us, "mcd_de_move (previous evaluation, second lane)");
    MCD_WAIT(cat->ctx, slot.comm_stream, cat->spin_us, "mcd_de_move (previous copies)");
    w.comm_pending[0] = w.comm_pending[1] = false;
    w.staged = false;                     // the walker constants are about to be overwritten on the device

    // ---- arena layout: [state, copied both ways | inputs, copied in | scratch | chain rows, copied out] ----
    size_t off = 0;
    auto take = [&](size_t bytes) { const size_t at = off; off += (bytes + 63) / 64 * 64; return at; };
    const size_t BW = (size_t)B * W, Bh = (size_t)B * half;
    const size_t o_pos = take(BW * P * 8), o_lnp = take(BW * 8), o_acc = take(BW * 8), o_meta = take(mcd::META_WORDS * 4);
    const size_t state_end = off;
    const size_t o_src = take((size_t)K * 4), o_const = take((size_t)K * 8), o_fac = take((size_t)K * 8);
    const size_t o_lo = take((size_t)P * 8), o_hi = take((size_t)P * 8);
    const bool with_prior = prior.any();
    const size_t o_pkind = take(with_prior ? (size_t)P * 4 : 0), o_ploc = take(with_prior ? (size_t)P * 8 : 0);
    const size_t o_pscale = take(with_prior ? (size_t)P * 8 : 0), o_pc0 = take(with_prior ? (size_t)P * 8 : 0);
    const size_t o_nok = take((size_t)2 * B * 4);                        // (zeroed with the inputs)
    const size_t fixed_end = off;
    // seeded blocks: a kernel writes the numbers where the upload would have put them (ensembles too large for it: the host
    // build of the same functions fills the pinned copy, uploaded as usual)
    const bool gen_device = num.seeded && mcd::chain_numbers_on_device(W);
    const size_t n_in = (size_t)n_steps;
    const size_t o_order = take(n_in * BW * 4), o_pa = take(n_in * BW * 4), o_pb = take(n_in * BW * 4);
    const size_t o_gamma = take(n_in * BW * 8), o_thr = take(n_in * BW * 8);
    const size_t input_end = off;
    const size_t o_prop = take(Bh * P * 8), o_ok = take(Bh), o_ranges = take((size_t)2 * B * mcd::kRangeDoubles * 8);
    const size_t o_pval = take(with_prior ? Bh * 8 : 0);
    const size_t o_chain = take(chain ? (size_t)n_steps * BW * P * 8 : 0);
    const size_t o_lnpc = take(lnprob_chain ? (size_t)n_steps * BW * 8 : 0);
    const size_t total = off;
    ChainArena& a = cat->chain;
    if (a.bytes < total) {
        // (a block too large for a device arena or for pinned host memory is no error: it runs host-driven, which needs neither)
        if (a.d) (void)hipFree(a.d);
        if (a.h) (void)hipHostFree(a.h);
        a = ChainArena();
        const size_t want = total + total / 2;
        if (hipMalloc((void**)&a.d, want) != hipSuccess) { (void)hipGetLastError(); a = ChainArena(); return MCD_OK; }
        if (hipHostMalloc((void**)&a.h, want, hipHostMallocDefault) != hipSuccess) {
            (void)hipGetLastError();
            (void)hipFree(a.d);
            a = ChainArena();
            return MCD_OK;
        }
        a.bytes = want;
    }
    std::memcpy(a.h + o_pos, pos, BW * P * 8);
    std::memcpy(a.h + o_lnp, lnp, BW * 8);
    if (accepted) std::memcpy(a.h + o_acc, accepted, BW * 8);
    else std::memset(a.h + o_acc, 0, BW * 8);
    std::memset(a.h + o_meta, 0, mcd::META_WORDS * 4);
    std::memcpy(a.h + o_src, d->col_source, (size_t)K * 4);
    std::memcpy(a.h + o_const, d->col_const, (size_t)K * 8);
    std::memcpy(a.h + o_fac, d->col_factor, (size_t)K * 8);
    std::memcpy(a.h + o_lo, d->lo, (size_t)P * 8);
    std::memcpy(a.h + o_hi, d->hi, (size_t)P * 8);
    if (with_prior) {
        std::memcpy(a.h + o_pkind, prior.kind, (size_t)P * 4);
        std::memcpy(a.h + o_ploc, prior.loc, (size_t)P * 8);
        std::memcpy(a.h + o_pscale, prior.scale, (size_t)P * 8);
        std::memcpy(a.h + o_pc0, prior.c0, (size_t)P * 8);
    }
    std::memset(a.h + o_nok, 0, (size_t)2 * B * 4);
    if (!gen_device) {
        if (num.seeded) {
            std::vector<uint64_t> sorter;
            for (int64_t i = 0; i < n_steps; ++i)
                mcd::de_numbers_of_step(num.seed, num.step0 + i, B, W, num.gamma0, num.sigma, (int32_t*)(a.h + o_order) + (size_t)i * BW,
                                        (int32_t*)(a.h + o_pa) + (size_t)i * BW, (int32_t*)(a.h + o_pb) + (size_t)i * BW,
                                        (double*)(a.h + o_gamma) + (size_t)i * BW, (double*)(a.h + o_thr) + (size_t)i * BW, sorter);
        } else {
            big_copy(a.h + o_order, num.order, n_in * BW * 4);
            big_copy(a.h + o_pa, num.pick_a, n_in * BW * 4);
            big_copy(a.h + o_pb, num.pick_b, n_in * BW * 4);
            big_copy(a.h + o_gamma, num.gamma, n_in * BW * 8);
            big_copy(a.h + o_thr, num.thr, n_in * BW * 8);
        }
    }

    // kernel family of this block: what the device's guard last asked for, else the verdict on the current positions
    int level = cat->de_hint;
    if (level < 0) {
        std::vector<double> table(BW * K);
        for (size_t j = 0; j < BW; ++j)
            for (int c = 0; c < K; ++c) {
                const int src = d->col_source[c];
                table[j * K + c] = src < 0 ? d->col_const[c]
                                           : (d->col_factor[c] == 1.0 ? pos[j * P + src] : pos[j * P + src] * d->col_factor[c]);
            }
        level = fast_level(cat, table.data(), (int64_t)BW);
    }

    mcd::DeDevice dd;
    mcd::StretchDevice& sd = dd.s;
    sd.n_bins = B;
    sd.n_walkers = W; sd.n_dim = P; sd.k = K; sd.fixed_ok = d->fixed_ok;
    sd.model = cat->model; sd.free_centre = cat->free_centre ? 1 : 0; sd.allow_fast = cat->allow_fast;
    sd.expected_level = level;
    sd.stats = cat->stats;                                              // (slices to the scalar part)
    sd.col_source = (const int32_t*)(a.d + o_src); sd.col_const = (const double*)(a.d + o_const);
    sd.col_factor = (const double*)(a.d + o_fac); sd.lo = (const double*)(a.d + o_lo); sd.hi = (const double*)(a.d + o_hi);
    sd.pos = (double*)(a.d + o_pos); sd.lnp = (double*)(a.d + o_lnp); sd.accepted = (long long*)(a.d + o_acc);
    sd.order = (const int32_t*)(a.d + o_order); sd.zz = (const double*)(a.d + o_gamma); sd.thr = (const double*)(a.d + o_thr);
    sd.pick = (const int32_t*)(a.d + o_pa);
    dd.pick_b = (const int32_t*)(a.d + o_pb);
    sd.chain = chain ? (double*)(a.d + o_chain) : nullptr;
    sd.lnprob_chain = lnprob_chain ? (double*)(a.d + o_lnpc) : nullptr;
    sd.proposal = (double*)(a.d + o_prop); sd.ok = (uint8_t*)(a.d + o_ok); sd.meta = (int32_t*)(a.d + o_meta);
    sd.n_ok = (int32_t*)(a.d + o_nok); sd.ranges = (double*)(a.d + o_ranges);
    sd.table = w.d_params; sd.wpar = (double*)w.d_wpar;
    if (with_prior) {
        sd.prior.kind = (const int32_t*)(a.d + o_pkind); sd.prior.loc = (const double*)(a.d + o_ploc);
        sd.prior.scale = (const double*)(a.d + o_pscale); sd.prior.c0 = (const double*)(a.d + o_pc0);
        sd.prior_val = (double*)(a.d + o_pval);
    }

    double* const out_buf = w.d_out;
    mcd::LaunchShape shape = main_launch_shape(cat, sh, w, level, false, out_buf, (int64_t)Bh);
    cat->last_narrow_bounded = 0;                      // (a resident chain keeps the narrow-range loop with its clamp)
    cat->last_series_chunks = 0;                       // (its tables are built on the device: no host count)
    cat->last_direct_chunks = 0;
    cat->last_exp_split = 0;
    cat->last_root_quad = 0;
    cat->last_block_step = 0;
    cat->last_quad_chunks = 0;
    const double* pset_const = fast_pset_const(cat, sh, level);
    const int64_t n_slots = mcd::partial_slots(shape, w.n_chunks, half);
    const int64_t max_slots = B == 1 ? n_slots : w.max_chunks_per_pset;

    MCD_HIP(hipMemcpyAsync(a.d, a.h, gen_device ? fixed_end : input_end, hipMemcpyHostToDevice, slot.stream));
    if (gen_device)
        MCD_HIP(mcd::launch_de_numbers(slot.stream, num.seed, num.step0, 0, n_steps, B, W, num.gamma0, num.sigma,
                                       (int32_t*)(a.d + o_order), (int32_t*)(a.d + o_pa), (int32_t*)(a.d + o_pb),
                                       (double*)(a.d + o_gamma), (double*)(a.d + o_thr)));
    double prev_tag = 0.0;
    int64_t acc_step = -1;
    int acc_h = 0;
    for (int64_t i = 0; i < n_steps; ++i)
        for (int h = 0; h < 2; ++h) {
            MCD_HIP(mcd::launch_de_step(slot.stream, dd, acc_step, acc_h, i, h, out_buf, prev_tag));
            prev_tag = (double)(++cat->launch_seq);
            shape.launch_tag = prev_tag;
            MCD_HIP(mcd::launch_loglike(slot.stream, shape, main_records(sh, w), w.d_chunks, w.n_chunks, w.d_wpar, w.d_partials, half));
            MCD_HIP(mcd::launch_reduce(slot.stream, w.d_partials, w.d_offsets, B, n_slots, max_slots, half, pset_const, out_buf));
            acc_step = i;
            acc_h = h;
        }
    MCD_HIP(mcd::launch_de_step(slot.stream, dd, acc_step, acc_h, -1, 0, out_buf, prev_tag));   // the last accept and verdict
    MCD_HIP(hipMemcpyAsync(a.h, a.d, state_end, hipMemcpyDeviceToHost, slot.stream));
    if (total > o_chain)
        MCD_HIP(hipMemcpyAsync(a.h + o_chain, a.d + o_chain, total - o_chain, hipMemcpyDeviceToHost, slot.stream));
    MCD_WAIT(cat->ctx, slot.stream, cat->spin_us, "mcd_de_move (resident block)");

    w.fast = level;
    cat->cur_walkers = half;
    cat->last_chunks = w.n_chunks;
    cat->last_grid = n_slots != w.n_chunks ? n_slots : mcd::main_grid(w.n_chunks, half);
    const int32_t* meta = (const int32_t*)(a.h + o_meta);
    if (meta[mcd::META_STATUS] != 0) {
        ++cat->de_discarded;
        cat->de_last_status = meta[mcd::META_STATUS];
        cat->de_hint = (meta[mcd::META_STATUS] & mcd::CHAIN_LEVEL) ? meta[mcd::META_LEVEL] : -1;
        cat->de_consecutive = std::min(cat->de_consecutive + 1, 7);
        cat->de_backoff = cat->de_consecutive > 1 ? ((int64_t)1 << (cat->de_consecutive - 1)) : 0;
        return MCD_OK;
    }
    cat->de_consecutive = 0;
    cat->de_hint = level;
    ++cat->de_device_blocks;
    std::memcpy(pos, a.h + o_pos, BW * P * 8);
    std::memcpy(lnp, a.h + o_lnp, BW * 8);
    if (accepted) std::memcpy(accepted, a.h + o_acc, BW * 8);
    if (chain) big_copy(chain, a.h + o_chain, (size_t)n_steps * BW * P * 8);
    if (lnprob_chain) big_copy(lnprob_chain, a.h + o_lnpc, (size_t)n_steps * BW * 8);
    *done = true;
    return MCD_OK;
}

// common part of mcd_de_move / mcd_de_move_seeded: argument checks, the resident block, else the host-driven one
int run_de(mcd_catalog* cat, const mcd_stretch_desc* d, const mcd_prior_desc* prior, int64_t n_steps, double* pos, double* lnp,
           const DeNumbers& num, double* chain, double* lnprob_chain, int64_t* accepted) {
    const std::string who = num.seeded ? "mcd_de_move_seeded" : "mcd_de_move";
    if (!cat || !d || !pos || !lnp) return fail(MCD_ERR_INVALID, who + ": null argument");
    if (!num.seeded && (!num.order || !num.pick_a || !num.pick_b || !num.gamma || !num.thr)) return fail(MCD_ERR_INVALID, who + ": null argument");
    const int64_t B = d->n_bins > 1 ? d->n_bins : 1;
    if (B != cat->n_psets)
        return fail(MCD_ERR_INVALID, who + ": desc->n_bins must equal the catalogue's number of parameter sets (radial bins)");
    if (d->k != cat->k) return fail(MCD_ERR_INVALID, who + ": descriptor has the wrong number of kernel columns");
    if (d->n_walkers < 4 || (d->n_walkers & 1) || d->n_dim <= 0 || n_steps < 0 || num.step0 < 0)
        return fail(MCD_ERR_INVALID, who + ": n_walkers must be even and >= 4 (two distinct partners in a half), n_dim positive, steps non-negative");
    if (num.seeded && !mcd::de_args_ok(d->n_walkers, num.gamma0, num.sigma))
        return fail(MCD_ERR_INVALID, who + ": gamma0 > 0 and sigma >= 0, both finite, and n_walkers <= 1048576 (the ordering keys hold the walker index in 20 bits)");
    if (!d->col_source || !d->col_const || !d->col_factor || !d->lo || !d->hi) return fail(MCD_ERR_INVALID, who + ": null descriptor array");
    for (int c = 0; c < d->k; ++c)
        if (d->col_source[c] >= d->n_dim) return fail(MCD_ERR_INVALID, who + ": col_source outside the free parameters");
    PriorHost ph;
    if (int prc = prior_of(prior, d->n_dim, who.c_str(), ph)) return prc;
    const int64_t W = d->n_walkers, half = W / 2;
    if (!num.seeded) {
        auto within = [](const int32_t* a, int64_t n, int64_t bound) {
            int32_t lo = 0, hi = 0;
            for (int64_t i = 0; i < n; ++i) { lo = a[i] < lo ? a[i] : lo; hi = a[i] > hi ? a[i] : hi; }
            return lo >= 0 && (int64_t)hi < bound;
        };
        if (!within(num.order, n_steps * B * W, W)) return fail(MCD_ERR_INVALID, "mcd_de_move: order holds an index outside 0..W-1");
        if (!within(num.pick_a, n_steps * B * W, half) || !within(num.pick_b, n_steps * B * W, half))
            return fail(MCD_ERR_INVALID, "mcd_de_move: pick_a / pick_b hold an index outside the half ensemble");
    }
    mcd::StretchDesc sd;
    sd.n_bins = B;
    sd.n_walkers = W; sd.n_dim = d->n_dim; sd.k = d->k; sd.col_source = d->col_source; sd.col_const = d->col_const;
    sd.col_factor = d->col_factor; sd.lo = d->lo; sd.hi = d->hi; sd.fixed_ok = d->fixed_ok;
    sd.prior = ph.table;
    bool done = false;
    const int dev_rc = de_block_device(cat, d, n_steps, pos, lnp, num, chain, lnprob_chain, accepted, &done, ph.table);
    if (dev_rc != MCD_OK) return dev_rc;
    if (done) return MCD_OK;
    ++cat->de_host_blocks;
    // host-driven block.  Seeded: the same numbers, from the same functions compiled for the host (mcd_de.h) -- one step at a
    // time, so that a block of any length needs the numbers of one step only
    int eval_rc = MCD_OK;
    auto eval = [&](const double* table, int64_t n, double* out) {
        eval_rc = mcd_loglike_batch(cat, n, d->k, table, out);
        return eval_rc;
    };
    int rc = mcd::STRETCH_OK;
    if (!num.seeded) {
        rc = mcd::de_block(sd, n_steps, pos, lnp, num.order, num.pick_a, num.pick_b, num.gamma, num.thr, chain, lnprob_chain,
                           accepted, eval);
    } else {
        std::vector<int32_t> g_order((size_t)B * W), g_pa((size_t)2 * B * half), g_pb((size_t)2 * B * half);
        std::vector<double> g_gamma((size_t)2 * B * half), g_thr((size_t)2 * B * half);
        std::vector<uint64_t> sorter;
        for (int64_t i = 0; i < n_steps && rc == mcd::STRETCH_OK; ++i) {
            mcd::de_numbers_of_step(num.seed, num.step0 + i, B, W, num.gamma0, num.sigma, g_order.data(), g_pa.data(), g_pb.data(),
                                    g_gamma.data(), g_thr.data(), sorter);
            rc = mcd::de_block(sd, 1, pos, lnp, g_order.data(), g_pa.data(), g_pb.data(), g_gamma.data(), g_thr.data(),
                               chain ? chain + (size_t)i * B * W * d->n_dim : nullptr,
                               lnprob_chain ? lnprob_chain + (size_t)i * B * W : nullptr, accepted, eval);
        }
    }
    if (rc == mcd::STRETCH_EVAL_FAILED) return eval_rc;                  // message already set by mcd_loglike_batch
    if (rc == mcd::STRETCH_NAN) return fail(MCD_ERR_NONFINITE, who + ": the log-probability returned NaN");
    if (rc != mcd::STRETCH_OK) return fail(MCD_ERR_INVALID, who + ": bad arguments");
    return MCD_OK;
}

}  // namespace

extern "C" {

int mcd_de_move(mcd_catalog* cat, const mcd_stretch_desc* d, const mcd_prior_desc* prior, int64_t n_steps, double* pos,
                double* lnp, const int32_t* order, const int32_t* pick_a, const int32_t* pick_b, const double* gamma,
                const double* thr, double* chain, double* lnprob_chain, int64_t* accepted) {
    try {
    DeNumbers num;
    num.order = order; num.pick_a = pick_a; num.pick_b = pick_b; num.gamma = gamma; num.thr = thr;
    return run_de(cat, d, prior, n_steps, pos, lnp, num, chain, lnprob_chain, accepted);
    } catch (...) { return on_exception("mcd_de_move"); }
}

int mcd_de_move_seeded(mcd_catalog* cat, const mcd_stretch_desc* d, const mcd_prior_desc* prior, double gamma0, double sigma,
                       int64_t n_steps, double* pos, double* lnp, uint64_t seed, int64_t step0, double* chain,
                       double* lnprob_chain, int64_t* accepted) {
    try {
    DeNumbers num;
    num.seeded = true; num.seed = seed; num.step0 = step0; num.gamma0 = gamma0; num.sigma = sigma;
    return run_de(cat, d, prior, n_steps, pos, lnp, num, chain, lnprob_chain, accepted);
    } catch (...) { return on_exception("mcd_de_move_seeded"); }
}

int mcd_de_numbers(uint64_t seed, int64_t step0, int64_t n_steps, int64_t n_bins, int64_t n_walkers, int32_t n_dim, double gamma0,
                   double sigma, int32_t* order, int32_t* pick_a, int32_t* pick_b, double* gamma, double* thr) {
    try {
    if (!order || !pick_a || !pick_b || !gamma || !thr || n_steps < 0 || step0 < 0 || n_dim <= 0 ||
        !mcd::de_args_ok(n_walkers, gamma0, sigma))
        return fail(MCD_ERR_INVALID, "mcd_de_numbers: bad arguments (n_walkers even, 4 .. 1048576; gamma0 > 0, sigma >= 0, finite)");
    const int64_t B = n_bins > 1 ? n_bins : 1, W = n_walkers, half = W / 2;
    std::vector<uint64_t> sorter;
    for (int64_t i = 0; i < n_steps; ++i) {
        const size_t at = (size_t)i * 2 * B * half;
        mcd::de_numbers_of_step(seed, step0 + i, B, W, gamma0, sigma, order + (size_t)i * B * W, pick_a + at, pick_b + at, gamma + at,
                                thr + at, sorter);
    }
    return MCD_OK;
    } catch (...) { return on_exception("mcd_de_numbers"); }
}

int mcd_de_info(const mcd_catalog* cat, int64_t* device_blocks, int64_t* host_blocks, int64_t* discarded_blocks,
                int32_t* last_discard_status) {
    if (!cat) return fail(MCD_ERR_INVALID, "null catalogue");
    if (device_blocks) *device_blocks = cat->de_device_blocks;
    if (host_blocks) *host_blocks = cat->de_host_blocks;
    if (discarded_blocks) *discarded_blocks = cat->de_discarded;
    if (last_discard_status) *last_discard_status = cat->de_last_status;
    return MCD_OK;
}

}  // extern "C"

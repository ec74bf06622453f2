// mcd_api_chain.hip -- C-ABI of the MI355X log-likelihood library (see include/mcd.h; mcd_host.h lists the host units):
// mcd_stretch_move / mcd_stretch_move_seeded as a block resident on the device (kernels: mcd_stretch.hip) or driven from
// the host (mcd_stretch.h), and mcd_chain_numbers; mcd_hmc_block in the same two forms (kernels: mcd_hmc.hip, algebra and
// host-driven loop: mcd_hmc.h), and mcd_hmc_numbers; the *_prior forms of the three blocks and mcd_prior_eval (mcd_prior.h).
#include "mcd_host.h"
#include "mcd_prior.h"
#include "mcd_rng.h"
#include "mcd_stretch.h"
#include "mcd_grad.h"
#include "mcd_hmc.h"

using namespace mcd::host;

MCD_HOST_BEGIN

// The structured priors of a call (PriorHost: mcd_host.h): mcd_prior_desc checked and its derived constants (mcd_prior.h:
// prior_derive, libm, once per call).  table.any() is false for a null descriptor and for one whose kinds are all flat: the
// call is then the prior-free one, bit for bit.
int prior_of(const mcd_prior_desc* p, int32_t n_dim, const char* who, PriorHost& out) {
    out.table = mcd::PriorTable();
    if (!p) return MCD_OK;
    if (p->n_dim != n_dim) return fail(MCD_ERR_INVALID, std::string(who) + ": the prior's n_dim differs from the descriptor's");
    if (n_dim < 1 || !p->kind || !p->p0 || !p->p1) return fail(MCD_ERR_INVALID, std::string(who) + ": null prior array");
    out.kind.assign(p->kind, p->kind + n_dim);
    out.loc.resize((size_t)n_dim); out.scale.resize((size_t)n_dim); out.c0.resize((size_t)n_dim);
    bool structured = false;
    if (!mcd::prior_derive(n_dim, p->kind, p->p0, p->p1, out.loc.data(), out.scale.data(), out.c0.data(), &structured))
        return fail(MCD_ERR_INVALID, std::string(who) + ": prior kinds are 0 (flat), 1 (normal: loc, scale > 0) or 2 (lognormal: mu, s > 0) with finite parameters");
    if (structured) {
        out.table.kind = out.kind.data(); out.table.loc = out.loc.data(); out.table.scale = out.scale.data(); out.table.c0 = out.c0.data();
    }
    return MCD_OK;
}

// user <-> pinned copies of tens of MB (a binned block: 40 MB of random numbers in, 70 MB of chain rows out) on four
// threads: one core moves ~10 GB/s, the copies would otherwise cost as much as the block's device time
void big_copy(void* dst, const void* src, size_t bytes) {
    constexpr size_t kSerial = (size_t)4 << 20;
    if (bytes < kSerial) { std::memcpy(dst, src, bytes); return; }
    constexpr int kMaxThreads = 16;
    static const int kThreads = [] {
        const char* e = std::getenv("MCD_COPY_THREADS");                  // tuning aid
        const int n = e ? std::atoi(e) : 4;
        return n < 1 ? 1 : (n > kMaxThreads ? kMaxThreads : n);
    }();
    std::thread workers[kMaxThreads - 1];
    const size_t part = (bytes / kThreads + 63) / 64 * 64;
    int started = 0;
    for (int t = 1; t < kThreads; ++t) {
        const size_t at = std::min(bytes, part * t), len = std::min(bytes, part * (t + 1)) - at;
        try {
            workers[t - 1] = std::thread([=] { if (len) std::memcpy((char*)dst + at, (const char*)src + at, len); });
            ++started;
        } catch (...) {                                        // no thread to be had: this share is copied here instead
            if (len) std::memcpy((char*)dst + at, (const char*)src + at, len);
        }
    }
    std::memcpy(dst, src, std::min(bytes, part));
    for (int t = 0; t < kThreads - 1; ++t)
        if (workers[t].joinable()) workers[t].join();
    (void)started;
}

MCD_HOST_END

namespace {

// ------------------------------------------------------------------------------------------------
// mcd_stretch_move with the ensemble resident on the device (mcd_stretch.hip).  Runs the whole block as one chain of
// launches and waits once.  *done = false when the block has to be run host-driven: the configuration is not covered, or
// the device met something only the host loop handles (mcd::ChainStatus).  `pos`, `lnp` and `accepted` are then
// untouched; the chain rows of a large block (cut into parts) may already hold rows of the discarded attempt, which the
// host-driven re-run overwrites (and which stay if that re-run fails).
// `seed` != nullptr: a seeded block (mcd_stretch_move_seeded) -- order / zz / thr / pick are null, a kernel generates the
// numbers of absolute steps step0 .. step0 + n_steps - 1 on the device (mcd_rng.h, mcd_stretch.hip: chain_numbers_kernel)
int stretch_block_device(mcd_catalog* cat, const mcd_stretch_desc* d, int64_t n_steps, double* pos, double* lnp,
                         const int32_t* order, const double* zz, const double* thr, const int32_t* pick, double* chain,
                         double* lnprob_chain, int64_t* accepted, bool* done, const mcd::PriorTable& prior,
                         const uint64_t* seed = nullptr, int64_t step0 = 0) {
    *done = false;
    mcd_ctx* ctx = cat->ctx;
    if (int urc = ctx_usable(ctx)) return urc;
    const int64_t B = cat->n_psets;                    // ensembles: one per parameter set (mcd_stretch_move checked n_bins)
    if (!cat->device_chain || cat->shards.size() != 1 || cat->precision != MCD_F64 || n_steps < 1 || cat->timing || !d->fixed_ok)
        return MCD_OK;
    if (B > 1 && cat->device_chain != 1) return MCD_OK;            // (the testing variants exist for one ensemble only)
    if (cat->chain_backoff > 0) { --cat->chain_backoff; return MCD_OK; }
    const int64_t W = d->n_walkers, half = W / 2;
    const int P = d->n_dim, K = d->k;
    bool small_ensemble = false;                                   // the step kernel that keeps the ensemble in LDS takes it
    {
        mcd::StretchDevice probe;
        probe.n_bins = B; probe.n_walkers = W; probe.n_dim = P; probe.k = K;
        probe.force_general = cat->device_chain == 2;
        if (!mcd::stretch_step_handles(probe)) return MCD_OK;
        small_ensemble = mcd::stretch_step_fuses(probe);
    }
    Shard& sh = cat->shards[0];
    const DeviceSlot& slot = ctx->slots[sh.slot];
    MCD_HIP(hipSetDevice(slot.device));
    WorkSet* wp = nullptr;
    int rc = build_workset(cat, sh, half, &wp);
    if (rc != MCD_OK) return rc;
    WorkSet& w = *wp;
    // nothing of an earlier call may still use the work buffers, the arena or the communicator
    MCD_WAIT(cat->ctx, slot.stream, cat->spin_us, "mcd_stretch_move (previous evaluation)");
    MCD_WAIT(cat->ctx, slot.stream2, cat->spin_us, "mcd_stretch_move (previous evaluation, second lane)");
    MCD_WAIT(cat->ctx, slot.comm_stream, cat->spin_us, "mcd_stretch_move (previous collective)");
    w.comm_pending[0] = w.comm_pending[1] = false;
    w.staged = false;                     // the walker constants are about to be overwritten on the device

    // ---- arena layout: [state, copied both ways | inputs, copied in | scratch | chain rows, copied out] ----
    // (every per-walker array carries the ensemble index in front: [B][W]..., random numbers [n_steps][..][B][..])
    size_t off = 0;
    auto take = [&](size_t bytes) { const size_t at = off; off += (bytes + 63) / 64 * 64; return at; };
    const size_t BW = (size_t)B * W, Bh = (size_t)B * half;
    const size_t o_pos = take(BW * P * 8), o_lnp = take(BW * 8), o_acc = take(BW * 8);
    const size_t o_meta = take(mcd::META_WORDS * 4), o_status = take(8);
    // deferred guard (one ensemble, the in-LDS step kernel; option "defer_guard"): every launch's table rows are kept and
    // judged together at the end of the block (mcd_stretch.hip: stretch_judge_kernel) -- unless the log would be large
    const size_t n_launches = (size_t)2 * n_steps;
    const bool defer = cat->defer_guard != 0 && B == 1 && small_ensemble && n_launches * half * K * 8 <= ((size_t)64 << 20);
    const size_t o_levels = take(defer ? n_launches * 4 : 0);
    const size_t state_end = off;
    const size_t o_src = take((size_t)K * 4), o_const = take((size_t)K * 8), o_fac = take((size_t)K * 8);
    const size_t o_lo = take((size_t)P * 8), o_hi = take((size_t)P * 8);
    const bool with_prior = prior.any();                        // (without: no bytes, the layout of a prior-free block)
    const size_t o_pkind = take(with_prior ? (size_t)P * 4 : 0), o_ploc = take(with_prior ? (size_t)P * 8 : 0);
    const size_t o_pscale = take(with_prior ? (size_t)P * 8 : 0), o_pc0 = take(with_prior ? (size_t)P * 8 : 0);
    const bool seeded = seed != nullptr;
    // seeded blocks: a kernel writes the numbers where the upload would have put them (ensembles too large for it: the host
    // build of the same functions fills the pinned copy, uploaded as usual)
    const bool gen_device = seeded && mcd::chain_numbers_on_device(W);
    const size_t n_in = (size_t)n_steps;
    const size_t o_order = take(n_in * BW * 4), o_zz = take(n_in * BW * 8);
    const size_t o_thr = take(n_in * BW * 8), o_pick = take(n_in * BW * 4);
    const size_t input_end = off;
    const size_t o_prop = take(Bh * P * 8), o_ok = take(Bh), o_nok = take((size_t)2 * B * 4), o_ranges = take((size_t)2 * B * mcd::kRangeDoubles * 8);
    const size_t o_pval = take(with_prior ? Bh * 8 : 0);
    const size_t o_nok_log = take(defer ? n_launches * 4 : 0), o_table_log = take(defer ? n_launches * half * K * 8 : 0);
    const size_t o_chain = take(chain ? (size_t)n_steps * BW * P * 8 : 0);
    const size_t o_lnpc = take(lnprob_chain ? (size_t)n_steps * BW * 8 : 0);
    const size_t total = off;
    ChainArena& a = cat->chain;
    if (a.bytes < total) {
        if (a.d) (void)hipFree(a.d);
        if (a.h) (void)hipHostFree(a.h);
        a = ChainArena();
        const size_t want = total + total / 2;
        // (a block too large for a device arena or for pinned host memory is no error on ONE device: it runs host-driven,
        // which needs neither; callers keep blocks of many ensembles short, analysis/binned.py.  In a multi-rank job the
        // choice between the resident and the host-driven sequence must be the same on every rank -- their collectives
        // differ in number and size -- so there a rank that cannot allocate reports the error instead)
        const bool must_agree = ctx->n_ranks > 1 || ctx->force_collective;
        if (hipMalloc((void**)&a.d, want) != hipSuccess) {
            (void)hipGetLastError();
            a = ChainArena();
            if (must_agree) return fail(MCD_ERR_NOMEM, "mcd_stretch_move: no device memory for the resident block of this rank (use shorter blocks)");
            return MCD_OK;
        }
        if (hipHostMalloc((void**)&a.h, want, hipHostMallocDefault) != hipSuccess) {
            (void)hipGetLastError();
            (void)hipFree(a.d);
            a = ChainArena();
            if (must_agree) return fail(MCD_ERR_NOMEM, "mcd_stretch_move: no pinned host memory for the resident block of this rank (use shorter blocks)");
            return MCD_OK;
        }
        a.bytes = want;
    }
    std::memcpy(a.h + o_pos, pos, BW * P * 8);
    std::memcpy(a.h + o_lnp, lnp, BW * 8);
    if (accepted) std::memcpy(a.h + o_acc, accepted, BW * 8);
    else std::memset(a.h + o_acc, 0, BW * 8);
    std::memset(a.h + o_meta, 0, mcd::META_WORDS * 4);
    std::memset(a.h + o_status, 0, 8);
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
    // Blocks that move tens of MB (binned catalogues: the random numbers of 64 steps of 55 x 512 walkers are 40 MB, their
    // chain rows 70 MB -- a third of the block's device time in copies) are cut into parts: the host copies and the PCIe
    // transfers of one part overlap the device work of another (copies on the second stream, joined by events).
    const size_t moved = (size_t)n_steps * BW * ((gen_device ? 0 : 24) + (chain ? (size_t)P * 8 : 0) + (lnprob_chain ? 8 : 0));
    size_t part_threshold = (size_t)16 << 20;
    if (const char* e = std::getenv("MCD_CHAIN_PART_BYTES")) part_threshold = (size_t)std::strtoull(e, nullptr, 10);   // testing aid
    // (what stays exposed is the first part's numbers going in and the last part's rows coming out: 1 / n_parts of the copies.
    // C5 shape, 64-step blocks: 233.8 us per step with 4 parts, 219.6 with 8, 216.7 with 16, 213.8 with 32)
    int64_t max_parts = 16;
    if (const char* e = std::getenv("MCD_CHAIN_PARTS")) max_parts = std::max<long long>(1, std::atoll(e));   // tuning aid
    const int64_t n_parts = moved >= part_threshold ? std::min<int64_t>(max_parts, n_steps) : 1;
    auto part_begin = [&](int64_t k) { return n_steps * k / n_parts; };
    auto copy_in = [&](int64_t i0, int64_t i1) {              // the random numbers of steps i0 .. i1: user -> pinned
        if (gen_device) return;
        const size_t at = (size_t)i0 * BW, n = (size_t)(i1 - i0) * BW;
        if (seeded) {
            std::vector<uint64_t> sorter;
            for (int64_t i = i0; i < i1; ++i)
                mcd::chain_numbers_of_step(*seed, step0 + i, B, W, P, (int32_t*)(a.h + o_order) + (size_t)i * BW,
                                           (double*)(a.h + o_zz) + (size_t)i * BW, (double*)(a.h + o_thr) + (size_t)i * BW,
                                           (int32_t*)(a.h + o_pick) + (size_t)i * BW, sorter);
            return;
        }
        big_copy(a.h + o_order + at * 4, order + at, n * 4);
        big_copy(a.h + o_zz + at * 8, zz + at, n * 8);
        big_copy(a.h + o_thr + at * 8, thr + at, n * 8);
        big_copy(a.h + o_pick + at * 4, pick + at, n * 4);
    };
    if (n_parts == 1) copy_in(0, n_steps);

    // kernel family of this block: what the device's guard last asked for, else the verdict on the current positions
    int level = cat->chain_hint;
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

    mcd::StretchDevice sd;
    sd.n_bins = B;
    sd.n_walkers = W; sd.n_dim = P; sd.k = K; sd.fixed_ok = d->fixed_ok;
    sd.model = cat->model; sd.free_centre = cat->free_centre ? 1 : 0; sd.allow_fast = cat->allow_fast;
    sd.expected_level = level;
    sd.force_general = cat->device_chain == 2;
    sd.stats = cat->stats;                                              // (slices to the scalar part)
    sd.col_source = (const int32_t*)(a.d + o_src); sd.col_const = (const double*)(a.d + o_const);
    sd.col_factor = (const double*)(a.d + o_fac); sd.lo = (const double*)(a.d + o_lo); sd.hi = (const double*)(a.d + o_hi);
    sd.pos = (double*)(a.d + o_pos); sd.lnp = (double*)(a.d + o_lnp); sd.accepted = (long long*)(a.d + o_acc);
    sd.order = (const int32_t*)(a.d + o_order); sd.zz = (const double*)(a.d + o_zz); sd.thr = (const double*)(a.d + o_thr);
    sd.pick = (const int32_t*)(a.d + o_pick);
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
    if (defer) {
        sd.defer_guard = 1;
        sd.table_log = (double*)(a.d + o_table_log); sd.n_ok_log = (int32_t*)(a.d + o_nok_log); sd.level_log = (int32_t*)(a.d + o_levels);
    }

    const bool coll = ctx->n_ranks > 1 || ctx->force_collective;
    double* const out_buf = w.d_out;
    mcd::LaunchShape shape = main_launch_shape(cat, sh, w, level, coll, out_buf, (int64_t)Bh);
    cat->last_narrow_bounded = 0;                      // (the resident chain keeps the narrow-range loop with its clamp)
    cat->last_series_chunks = 0;                       // (its tables are built on the device: no host count)
    cat->last_direct_chunks = 0;
    cat->last_exp_split = 0;                           // (... and the direct form without the split exponent offset)
    cat->last_root_quad = 0;
    cat->last_block_step = 0;
    cat->last_quad_chunks = 0;
    const double* pset_const = fast_pset_const(cat, sh, level);
    // launches with few partial sums per walker (balanced plans of small catalogues, radial bins of a few chunks): no
    // reduction kernel, the step kernel adds them up itself -- the same code in the same order (mcd_reduce.h), so the
    // chain keeps the bits of the host-driven loop.  Not with a collective: the all-reduce needs the sums in memory.
    const int64_t n_slots = mcd::partial_slots(shape, w.n_chunks, half);
    const int64_t max_slots = B == 1 ? n_slots : w.max_chunks_per_pset;
    const bool fused = cat->fused_reduce != 0 && !coll && max_slots <= mcd::kFusedReduceSlots && mcd::stretch_step_fuses(sd);
    sd.fused = fused ? 1 : 0;
    sd.partials = w.d_partials;
    sd.n_slots = n_slots;
    sd.slot_offsets = B == 1 ? nullptr : w.d_offsets;
    sd.pset_const = pset_const;
    cat->chain_last_fused = fused;
    double prev_tag = 0.0;
    int64_t acc_step = -1;
    int acc_h = 0;
#ifdef MCD_CHAIN_STAMPS
    static unsigned long long* d_stamps = nullptr;
    if (!d_stamps) MCD_HIP(hipMalloc((void**)&d_stamps, 8 * 8 * 4096));
    MCD_HIP(hipMemsetAsync(d_stamps, 0, 8 * 8 * 4096, slot.stream));
    sd.stamps = d_stamps;
#endif
    // launches of steps i0 .. i1; `mark` (may be null) is recorded right after the first step kernel, i.e. when the chain
    // rows of every step before i0 are final (the row of step i0 - 1 is written by that launch)
    auto enqueue_steps = [&](int64_t i0, int64_t i1, hipEvent_t mark) -> int {
        for (int64_t i = i0; i < i1; ++i)
            for (int h = 0; h < 2; ++h) {
#ifdef MCD_CHAIN_STAMPS
                sd.launch_index = i * 2 + h;
#endif
                MCD_HIP(mcd::launch_stretch_step(slot.stream, sd, acc_step, acc_h, i, h, out_buf, prev_tag));
                if (mark && i == i0 && h == 0) MCD_HIP(hipEventRecord(mark, slot.stream));
                prev_tag = coll ? 0.0 : (double)(++cat->launch_seq);
                shape.launch_tag = prev_tag;
                MCD_HIP(mcd::launch_loglike(slot.stream, shape, main_records(sh, w), w.d_chunks, w.n_chunks, w.d_wpar, w.d_partials, half));
                if (!fused)
                    MCD_HIP(mcd::launch_reduce(slot.stream, w.d_partials, w.d_offsets, B, n_slots, max_slots, half, pset_const,
                                               out_buf));
                if (coll) {
                    if (!ctx->multi_process) MCD_NCCL(g_rccl.GroupStart());
                    MCD_NCCL(g_rccl.AllReduce(out_buf, out_buf, Bh, ncclDouble, ncclSum, slot.comm, slot.stream));
                    if (!ctx->multi_process) MCD_NCCL(g_rccl.GroupEnd());
                }
                acc_step = i;
                acc_h = h;
            }
        return MCD_OK;
    };
    auto finish = [&]() -> int {                               // the last accept [+ the collective status word]
        MCD_HIP(mcd::launch_stretch_step(slot.stream, sd, acc_step, acc_h, -1, 0, out_buf, prev_tag));
        if (defer) MCD_HIP(mcd::launch_stretch_judge(slot.stream, sd, (int64_t)n_launches));
        if (coll) {
            // ranks hold different shares of the catalogue, so their guard verdicts may differ: all discard the block if one does
            double* status = (double*)(a.d + o_status);
            MCD_HIP(mcd::launch_stretch_status(slot.stream, sd.meta, status));
            if (!ctx->multi_process) MCD_NCCL(g_rccl.GroupStart());
            MCD_NCCL(g_rccl.AllReduce(status, status, 1, ncclDouble, ncclSum, slot.comm, slot.stream));
            if (!ctx->multi_process) MCD_NCCL(g_rccl.GroupEnd());
        }
        return MCD_OK;
    };
    // From the first launch on, the other ranks of a multi-rank job are committed to this block's sequence of
    // collectives: an error on this rank in the middle of it (a failed launch, a refused ncclAllReduce) cannot be undone
    // locally -- the peers would wait in an all-reduce this rank never enters.  The context is marked failed (the host
    // tells the peers: hostgroup.abort -> mcd_ctx_abort on their side; their deadline bounds the wait otherwise).
    struct MidBlockGuard {
        mcd_ctx* ctx; bool armed; bool ok;
        ~MidBlockGuard() {
            if (armed && !ok && !ctx->failed.load()) {
                const std::string cause = g_last_error;
                (void)ctx_fail(ctx, "mcd_stretch_move: this rank failed in the middle of a resident block (" + cause + ")");
            }
        }
    } mid_block{ctx, coll, false};
    bool rows_delivered = false;                               // chain rows already in the caller's arrays (parts)
    auto generate = [&](hipStream_t s, int64_t i0, int64_t i1) {   // seeded: the numbers of steps i0 .. i1, on the device
        return mcd::launch_chain_numbers(s, *seed, step0, i0, i1, B, W, P, (int32_t*)(a.d + o_order), (double*)(a.d + o_zz),
                                         (double*)(a.d + o_thr), (int32_t*)(a.d + o_pick));
    };
    if (n_parts == 1) {
        MCD_HIP(hipMemcpyAsync(a.d, a.h, gen_device ? o_order : input_end, hipMemcpyHostToDevice, slot.stream));
        if (gen_device) MCD_HIP(generate(slot.stream, 0, n_steps));
        rc = enqueue_steps(0, n_steps, nullptr);
        if (rc != MCD_OK) return rc;
        rc = finish();
        if (rc != MCD_OK) return rc;
        MCD_HIP(hipMemcpyAsync(a.h, a.d, state_end, hipMemcpyDeviceToHost, slot.stream));
        if (total > o_chain)
            MCD_HIP(hipMemcpyAsync(a.h + o_chain, a.d + o_chain, total - o_chain, hipMemcpyDeviceToHost, slot.stream));
        MCD_WAIT(cat->ctx, slot.stream, cat->spin_us, "mcd_stretch_move (resident block)");
    } else {
        // events: in[k] the numbers of part k are on the device; rows[k] the chain rows of part k are final; out[k] they
        // are in pinned memory
        while ((int64_t)cat->chain_events.size() < 3 * n_parts) {          // (events are kept for the catalogue's lifetime)
            hipEvent_t e;
            MCD_HIP(hipEventCreateWithFlags(&e, hipEventDisableTiming));
            cat->chain_events.push_back(e);
        }
        hipEvent_t* ev_in = cat->chain_events.data();
        hipEvent_t* ev_rows = ev_in + n_parts;
        hipEvent_t* ev_out = ev_rows + n_parts;
        auto rows_to_host = [&](int64_t k) -> int {            // D2H of part k's rows on the copy stream, behind rows[k]
            const size_t at = (size_t)part_begin(k) * BW, n = (size_t)(part_begin(k + 1) - part_begin(k)) * BW;
            MCD_HIP(hipStreamWaitEvent(slot.comm_stream, ev_rows[k], 0));
            if (chain) MCD_HIP(hipMemcpyAsync(a.h + o_chain + at * P * 8, a.d + o_chain + at * P * 8, n * P * 8, hipMemcpyDeviceToHost, slot.comm_stream));
            if (lnprob_chain) MCD_HIP(hipMemcpyAsync(a.h + o_lnpc + at * 8, a.d + o_lnpc + at * 8, n * 8, hipMemcpyDeviceToHost, slot.comm_stream));
            MCD_HIP(hipEventRecord(ev_out[k], slot.comm_stream));
            return MCD_OK;
        };
        auto rows_to_caller = [&](int64_t k) -> int {          // wait for out[k], pinned -> the caller's arrays
            const size_t at = (size_t)part_begin(k) * BW, n = (size_t)(part_begin(k + 1) - part_begin(k)) * BW;
            // (the event is the last thing on the copy stream at this point: wait for the stream, with the context's deadline)
            MCD_WAIT(cat->ctx, slot.comm_stream, cat->spin_us, "mcd_stretch_move (chain rows of a part)");
            if (chain) big_copy(chain + at * P, a.h + o_chain + at * P * 8, n * P * 8);
            if (lnprob_chain) big_copy(lnprob_chain + at, a.h + o_lnpc + at * 8, n * 8);
            return MCD_OK;
        };
        MCD_HIP(hipMemcpyAsync(a.d, a.h, o_order, hipMemcpyHostToDevice, slot.stream));   // state, column map, bounds
        for (int64_t k = 0; k < n_parts; ++k) {
            const int64_t i0 = part_begin(k), i1 = part_begin(k + 1);
            const size_t at = (size_t)i0 * BW, n = (size_t)(i1 - i0) * BW;
            if (gen_device) {
                MCD_HIP(generate(slot.comm_stream, i0, i1));
                MCD_HIP(hipEventRecord(ev_in[k], slot.comm_stream));
                MCD_HIP(hipStreamWaitEvent(slot.stream, ev_in[k], 0));
            } else {
                copy_in(i0, i1);
                MCD_HIP(hipMemcpyAsync(a.d + o_order + at * 4, a.h + o_order + at * 4, n * 4, hipMemcpyHostToDevice, slot.comm_stream));
                MCD_HIP(hipMemcpyAsync(a.d + o_zz + at * 8, a.h + o_zz + at * 8, n * 8, hipMemcpyHostToDevice, slot.comm_stream));
                MCD_HIP(hipMemcpyAsync(a.d + o_thr + at * 8, a.h + o_thr + at * 8, n * 8, hipMemcpyHostToDevice, slot.comm_stream));
                MCD_HIP(hipMemcpyAsync(a.d + o_pick + at * 4, a.h + o_pick + at * 4, n * 4, hipMemcpyHostToDevice, slot.comm_stream));
                MCD_HIP(hipEventRecord(ev_in[k], slot.comm_stream));
                MCD_HIP(hipStreamWaitEvent(slot.stream, ev_in[k], 0));
            }
            rc = enqueue_steps(i0, i1, k > 0 ? ev_rows[k - 1] : nullptr);
            if (rc != MCD_OK) return rc;
            if (k > 0) {
                rc = rows_to_host(k - 1);
                if (rc != MCD_OK) return rc;
                rc = rows_to_caller(k - 1);                     // (the device is busy with part k meanwhile)
                if (rc != MCD_OK) return rc;
            }
        }
        rc = finish();
        if (rc != MCD_OK) return rc;
        MCD_HIP(hipEventRecord(ev_rows[n_parts - 1], slot.stream));
        MCD_HIP(hipMemcpyAsync(a.h, a.d, state_end, hipMemcpyDeviceToHost, slot.stream));
        rc = rows_to_host(n_parts - 1);
        if (rc != MCD_OK) return rc;
        rc = rows_to_caller(n_parts - 1);
        if (rc != MCD_OK) return rc;
        MCD_WAIT(cat->ctx, slot.stream, cat->spin_us, "mcd_stretch_move (resident block, last part)");
        MCD_WAIT(cat->ctx, slot.comm_stream, cat->spin_us, "mcd_stretch_move (resident block, chain rows)");
        rows_delivered = true;   // (a discarded block leaves garbage there: the host-driven re-run overwrites every row)
    }
#ifdef MCD_CHAIN_STAMPS
    {
        const int64_t n = std::min<int64_t>(n_steps * 2, 4096);
        std::vector<unsigned long long> st((size_t)n * 8);
        MCD_HIP(hipMemcpy(st.data(), d_stamps, st.size() * 8, hipMemcpyDeviceToHost));
        double sum[8] = {0}, period = 0;
        int64_t cnt = 0;
        for (int64_t i = 2; i + 1 < n; ++i) {
            for (int k = 1; k < 8; ++k) sum[k] += (double)(st[i * 8 + k] - st[i * 8 + k - 1]);
            period += (double)(st[(i + 1) * 8] - st[i * 8]);
            ++cnt;
        }
        if (cnt > 0) {
            fprintf(stderr, "[chain stamps] period %.2f us; phases (us):", period / cnt / 100.0);
            for (int k = 1; k < 8; ++k) fprintf(stderr, " %d:%.2f", k, sum[k] / cnt / 100.0);
            fprintf(stderr, "\n");
        }
    }
#endif

    mid_block.ok = true;
    w.fast = level;
    cat->cur_walkers = half;
    cat->last_chunks = w.n_chunks;
    {
        const int64_t slots = mcd::partial_slots(shape, w.n_chunks, half);
        cat->last_grid = slots != w.n_chunks ? slots : mcd::main_grid(w.n_chunks, half);
    }
    const int32_t* meta = (const int32_t*)(a.h + o_meta);
    const bool discard = meta[mcd::META_STATUS] != 0 || (coll && *(const double*)(a.h + o_status) != 0.0);
    if (discard) {
        ++cat->chain_discarded;
        cat->chain_last_status = meta[mcd::META_STATUS];
        cat->chain_hint = (meta[mcd::META_STATUS] & mcd::CHAIN_LEVEL) ? meta[mcd::META_LEVEL] : -1;
        if (defer && (meta[mcd::META_STATUS] & mcd::CHAIN_LEVEL)) {      // the first launch whose verdict differed
            const int32_t* levels = (const int32_t*)(a.h + o_levels);
            cat->chain_hint = -1;
            for (size_t l = 0; l < n_launches; ++l)
                if (levels[l] >= 0 && levels[l] != level) { cat->chain_hint = levels[l]; break; }
        }
        // every rank of a job counts the same discards (the verdict above is collective), so the back-off stays in step
        cat->chain_consecutive = std::min(cat->chain_consecutive + 1, 7);
        cat->chain_backoff = cat->chain_consecutive > 1 ? ((int64_t)1 << (cat->chain_consecutive - 1)) : 0;
        return MCD_OK;
    }
    cat->chain_consecutive = 0;
    cat->chain_hint = level;
    ++cat->chain_device_blocks;
    std::memcpy(pos, a.h + o_pos, BW * P * 8);
    std::memcpy(lnp, a.h + o_lnp, BW * 8);
    if (accepted) std::memcpy(accepted, a.h + o_acc, BW * 8);
    if (chain && !rows_delivered) big_copy(chain, a.h + o_chain, (size_t)n_steps * BW * P * 8);
    if (lnprob_chain && !rows_delivered) big_copy(lnprob_chain, a.h + o_lnpc, (size_t)n_steps * BW * 8);
    *done = true;
    return MCD_OK;
}

// common part of mcd_stretch_move / mcd_stretch_move_seeded: argument checks, the resident block, else the host-driven one
int run_stretch(mcd_catalog* cat, const mcd_stretch_desc* d, int64_t n_steps, double* pos, double* lnp,
                const int32_t* order, const double* zz, const double* thr, const int32_t* pick, double* chain,
                double* lnprob_chain, int64_t* accepted, const uint64_t* seed, int64_t step0, const mcd_prior_desc* prior) {
    const char* who = seed ? "mcd_stretch_move_seeded" : "mcd_stretch_move";
    if (!cat || !d || !pos || !lnp) return fail(MCD_ERR_INVALID, std::string(who) + ": null argument");
    if (!seed && (!order || !zz || !thr || !pick)) return fail(MCD_ERR_INVALID, std::string(who) + ": null argument");
    if (seed && d->n_walkers > mcd::kSeededMaxWalkers)
        return fail(MCD_ERR_INVALID, std::string(who) + ": the generator's ordering keys hold the walker index in 20 bits (n_walkers <= 1048576)");
    const int64_t B = d->n_bins > 1 ? d->n_bins : 1;
    if (B != cat->n_psets)
        return fail(MCD_ERR_INVALID, std::string(who) + ": desc->n_bins must equal the catalogue's number of parameter sets (radial bins)");
    if (d->k != cat->k) return fail(MCD_ERR_INVALID, std::string(who) + ": descriptor has the wrong number of kernel columns");
    if (d->n_walkers <= 0 || (d->n_walkers & 1) || d->n_dim <= 0 || n_steps < 0 || step0 < 0)
        return fail(MCD_ERR_INVALID, std::string(who) + ": n_walkers must be positive and even, n_dim positive, steps non-negative");
    if (!d->col_source || !d->col_const || !d->col_factor || !d->lo || !d->hi) return fail(MCD_ERR_INVALID, std::string(who) + ": null descriptor array");
    for (int c = 0; c < d->k; ++c)
        if (d->col_source[c] >= d->n_dim) return fail(MCD_ERR_INVALID, std::string(who) + ": col_source outside the free parameters");
    PriorHost ph;
    if (int prc = prior_of(prior, d->n_dim, who, ph)) return prc;
    const int64_t W = d->n_walkers, half = W / 2;
    if (!seed) {
        // (range checks as min / max reductions: branch-free, vectorised -- a binned block holds millions of indices)
        auto within = [](const int32_t* a, int64_t n, int64_t bound) {
            int32_t lo = 0, hi = 0;
            for (int64_t i = 0; i < n; ++i) { lo = a[i] < lo ? a[i] : lo; hi = a[i] > hi ? a[i] : hi; }
            return lo >= 0 && (int64_t)hi < bound;
        };
        if (!within(order, n_steps * B * W, W)) return fail(MCD_ERR_INVALID, "mcd_stretch_move: order holds an index outside 0..W-1");
        if (!within(pick, n_steps * B * W, half)) return fail(MCD_ERR_INVALID, "mcd_stretch_move: pick holds an index outside the half ensemble");
    }
    mcd::StretchDesc sd;
    sd.n_bins = B;
    sd.n_walkers = W; sd.n_dim = d->n_dim; sd.k = d->k; sd.col_source = d->col_source; sd.col_const = d->col_const;
    sd.col_factor = d->col_factor; sd.lo = d->lo; sd.hi = d->hi; sd.fixed_ok = d->fixed_ok;
    sd.prior = ph.table;
    bool done = false;
    const int dev_rc = stretch_block_device(cat, d, n_steps, pos, lnp, order, zz, thr, pick, chain, lnprob_chain, accepted, &done,
                                            ph.table, seed, step0);
    if (dev_rc != MCD_OK) return dev_rc;
    if (done) return MCD_OK;
    ++cat->chain_host_blocks;
    // host-driven block.  Seeded: the same numbers, from the same functions compiled for the host (mcd_rng.h) -- one step at
    // a time, so that a block of any length needs the numbers of one step only
    std::vector<int32_t> g_order, g_pick;
    std::vector<double> g_zz, g_thr, g_keys;
    std::vector<uint64_t> sorter;
    int eval_rc = MCD_OK;
    auto eval = [&](const double* table, int64_t n, double* out) {
        eval_rc = mcd_loglike_batch(cat, n, d->k, table, out);
        return eval_rc;
    };
    int rc = mcd::STRETCH_OK;
    if (!seed) {
        rc = mcd::stretch_block(sd, n_steps, pos, lnp, order, zz, thr, pick, chain, lnprob_chain, accepted, eval);
    } else {
        g_order.resize((size_t)B * W); g_pick.resize((size_t)2 * B * half); g_zz.resize((size_t)2 * B * half); g_thr.resize((size_t)2 * B * half);
        for (int64_t i = 0; i < n_steps && rc == mcd::STRETCH_OK; ++i) {
            mcd::chain_numbers_of_step(*seed, step0 + i, B, W, d->n_dim, g_order.data(), g_zz.data(), g_thr.data(), g_pick.data(), sorter);
            rc = mcd::stretch_block(sd, 1, pos, lnp, g_order.data(), g_zz.data(), g_thr.data(), g_pick.data(),
                                    chain ? chain + (size_t)i * B * W * d->n_dim : nullptr,
                                    lnprob_chain ? lnprob_chain + (size_t)i * B * W : nullptr, accepted, eval);
        }
    }
    if (rc == mcd::STRETCH_EVAL_FAILED) return eval_rc;                  // message already set by mcd_loglike_batch
    if (rc == mcd::STRETCH_NAN) return fail(MCD_ERR_NONFINITE, std::string(who) + ": the log-probability returned NaN");
    if (rc != mcd::STRETCH_OK) return fail(MCD_ERR_INVALID, std::string(who) + ": bad arguments");
    return MCD_OK;
}

// ------------------------------------------------------------------------------------------------
// mcd_hmc_block resident on the device: the starting point is evaluated through mcd_loglike_grad_batch (which also
// stages the work set of W walkers and sizes its gradient scratch), then n_steps x n_leap gradient evaluations with the
// two kernels of mcd_hmc.hip between them run as ONE chain of launches on the shard's stream, and the host waits once
// under the context's deadline.  Nothing on the device needs the host: a divergent trajectory is a rejection.
// *done = false (nothing written) when the trajectory scratch cannot be had: the caller runs the block host-driven.
constexpr int64_t kHmcResidentMaxWalkers = 65536;              // what the trajectory scratch is sized for
constexpr size_t kHmcResidentMaxBytes = (size_t)512 << 20;     // ... and a block's chain rows with it

bool hmc_resident_covers(const mcd_catalog* cat, int64_t W, int P, int64_t n_steps) {
    if (!cat->device_chain || cat->shards.size() != 1 || cat->ctx->has_comm() || cat->timing || n_steps < 1) return false;
    if (W > kHmcResidentMaxWalkers) return false;
    return (size_t)n_steps * W * (P + 2) * 8 <= kHmcResidentMaxBytes;
}

int hmc_block_device(mcd_catalog* cat, const mcd::HmcShared& hs, int64_t W, int64_t n_steps, double* pos, double* lnp,
                     uint64_t seed, int64_t step0, double* chain, double* lnprob_chain, int64_t* accepted,
                     double* energy_error, bool* done) {
    *done = false;
    mcd_ctx* ctx = cat->ctx;
    const int P = hs.n_dim, K = hs.k;
    // ---- the starting point (host round trip, once per block): values, column derivatives, chain rule, checks
    std::vector<double> table((size_t)W * K), ll((size_t)W), gcols((size_t)W * K), grad((size_t)W * P), lnp0((size_t)W);
    for (int64_t w = 0; w < W; ++w) mcd::hmc_row(hs, pos + w * P, table.data() + w * K);
    int rc = mcd_loglike_grad_batch(cat, W, K, table.data(), ll.data(), gcols.data());
    if (rc != MCD_OK) return rc;
    if (mcd::hmc_start(hs, W, pos, ll.data(), gcols.data(), lnp0.data(), grad.data()) != mcd::HMC_OK)
        return fail(MCD_ERR_NONFINITE, "mcd_hmc_block: a walker starts outside the prior or with a non-finite log-likelihood or gradient");
    Shard& sh = cat->shards[0];
    const DeviceSlot& slot = ctx->slots[sh.slot];
    MCD_HIP(hipSetDevice(slot.device));
    const auto it = sh.work.find(W);
    if (it == sh.work.end() || !it->second.d_grad_out || !it->second.d_grad_partials)
        return fail(MCD_ERR_INVALID, "mcd_hmc_block: the gradient work set of this walker count is gone");
    WorkSet& w = it->second;

    // ---- arena: [state, both ways | column map, bounds, factor: in | trajectory scratch | rows of the block: out]
    size_t off = 0;
    auto take = [&](size_t bytes) { const size_t at = off; off += (bytes + 63) / 64 * 64; return at; };
    const size_t WP = (size_t)W * P;
    const size_t o_pos = take(WP * 8), o_lnp = take((size_t)W * 8), o_grad = take(WP * 8), o_acc = take((size_t)W * 8);
    const size_t state_end = off;
    const size_t o_src = take((size_t)K * 4), o_const = take((size_t)K * 8), o_fac = take((size_t)K * 8);
    const size_t o_lo = take((size_t)P * 8), o_hi = take((size_t)P * 8), o_chol = take((size_t)P * P * 8);
    const bool with_prior = hs.prior.any();
    const size_t o_pkind = take(with_prior ? (size_t)P * 4 : 0), o_ploc = take(with_prior ? (size_t)P * 8 : 0);
    const size_t o_pscale = take(with_prior ? (size_t)P * 8 : 0), o_pc0 = take(with_prior ? (size_t)P * 8 : 0);
    const size_t input_end = off;
    const size_t o_q = take(WP * 8), o_p = take(WP * 8), o_h0 = take((size_t)W * 8), o_eps = take((size_t)W * 8);
    const size_t o_alive = take((size_t)W * 4);
    const size_t o_rows = off;
    const size_t o_chain = take(chain ? (size_t)n_steps * WP * 8 : 0);
    const size_t o_lnpc = take(lnprob_chain ? (size_t)n_steps * W * 8 : 0);
    const size_t o_err = take(energy_error ? (size_t)n_steps * W * 8 : 0);
    const size_t total = off;
    ChainArena& a = cat->hmc;
    if (a.bytes < total) {
        if (a.d) (void)hipFree(a.d);
        if (a.h) (void)hipHostFree(a.h);
        a = ChainArena();
        const size_t want = total + total / 2;
        // (one device, no collective: a block too large for the scratch simply runs host-driven)
        if (hipMalloc((void**)&a.d, want) != hipSuccess) { (void)hipGetLastError(); a = ChainArena(); return MCD_OK; }
        if (hipHostMalloc((void**)&a.h, want, hipHostMallocDefault) != hipSuccess) {
            (void)hipGetLastError();
            (void)hipFree(a.d);
            a = ChainArena();
            return MCD_OK;
        }
        a.bytes = want;
    }
    std::memcpy(a.h + o_pos, pos, WP * 8);
    std::memcpy(a.h + o_lnp, lnp0.data(), (size_t)W * 8);
    std::memcpy(a.h + o_grad, grad.data(), WP * 8);
    std::memset(a.h + o_acc, 0, (size_t)W * 8);
    std::memcpy(a.h + o_src, hs.col_source, (size_t)K * 4);
    std::memcpy(a.h + o_const, hs.col_const, (size_t)K * 8);
    std::memcpy(a.h + o_fac, hs.col_factor, (size_t)K * 8);
    std::memcpy(a.h + o_lo, hs.lo, (size_t)P * 8);
    std::memcpy(a.h + o_hi, hs.hi, (size_t)P * 8);
    std::memcpy(a.h + o_chol, hs.chol, (size_t)P * P * 8);
    if (with_prior) {
        std::memcpy(a.h + o_pkind, hs.prior.kind, (size_t)P * 4);
        std::memcpy(a.h + o_ploc, hs.prior.loc, (size_t)P * 8);
        std::memcpy(a.h + o_pscale, hs.prior.scale, (size_t)P * 8);
        std::memcpy(a.h + o_pc0, hs.prior.c0, (size_t)P * 8);
    }

    mcd::HmcDevice hd;
    hd.s = hs;
    hd.s.col_source = (const int32_t*)(a.d + o_src); hd.s.col_const = (const double*)(a.d + o_const);
    hd.s.col_factor = (const double*)(a.d + o_fac); hd.s.lo = (const double*)(a.d + o_lo); hd.s.hi = (const double*)(a.d + o_hi);
    hd.s.chol = (const double*)(a.d + o_chol);
    if (with_prior) {
        hd.s.prior.kind = (const int32_t*)(a.d + o_pkind); hd.s.prior.loc = (const double*)(a.d + o_ploc);
        hd.s.prior.scale = (const double*)(a.d + o_pscale); hd.s.prior.c0 = (const double*)(a.d + o_pc0);
    }
    hd.n_walkers = W; hd.seed = seed;
    hd.pos = (double*)(a.d + o_pos); hd.lnp = (double*)(a.d + o_lnp); hd.grad = (double*)(a.d + o_grad);
    hd.accepted = (long long*)(a.d + o_acc);
    hd.q = (double*)(a.d + o_q); hd.p = (double*)(a.d + o_p); hd.h0 = (double*)(a.d + o_h0); hd.eps = (double*)(a.d + o_eps);
    hd.alive = (int32_t*)(a.d + o_alive);
    hd.chain = chain ? (double*)(a.d + o_chain) : nullptr;
    hd.lnprob_chain = lnprob_chain ? (double*)(a.d + o_lnpc) : nullptr;
    hd.energy_error = energy_error ? (double*)(a.d + o_err) : nullptr;
    hd.table = w.d_params;
    hd.fields = w.d_grad_out;
    hd.padded = mcd::padded_walkers(W);

    // (mcd_loglike_grad_batch has waited for the stream: nothing of an earlier call uses the work buffers)
    w.staged = false;                     // the parameter table and the walker constants are about to be overwritten
    const mcd::LaunchShape shape{cat->model, cat->free_centre, cat->precision, 0};
    MCD_HIP(hipMemcpyAsync(a.d, a.h, input_end, hipMemcpyHostToDevice, slot.stream));
    for (int64_t i = 0; i < n_steps; ++i) {
        MCD_HIP(mcd::launch_hmc_begin(slot.stream, hd, step0 + i));
        for (int leap = 1; leap <= hs.n_leap; ++leap) {
            MCD_HIP(mcd::launch_prepare_walkers(slot.stream, w.d_params, W, K, cat->model, cat->free_centre, cat->precision, w.d_wpar));
            MCD_HIP(mcd::launch_loglike_grad(slot.stream, shape, main_records(sh, w), w.d_chunks, w.n_chunks, w.d_params, w.d_wpar,
                                             w.d_grad_partials, W));
            MCD_HIP(mcd::launch_grad_reduce(slot.stream, shape, w.d_grad_partials, w.n_chunks, w.d_offsets, cat->n_psets,
                                            w.max_chunks_per_pset, W, w.d_grad_out));
            MCD_HIP(mcd::launch_hmc_leap(slot.stream, hd, step0 + i, i, leap));
        }
    }
    MCD_HIP(hipMemcpyAsync(a.h, a.d, state_end, hipMemcpyDeviceToHost, slot.stream));
    if (total > o_rows) MCD_HIP(hipMemcpyAsync(a.h + o_rows, a.d + o_rows, total - o_rows, hipMemcpyDeviceToHost, slot.stream));
    MCD_WAIT(cat->ctx, slot.stream, cat->spin_us, "mcd_hmc_block (resident block)");

    ++cat->hmc_device_blocks;
    std::memcpy(pos, a.h + o_pos, WP * 8);
    std::memcpy(lnp, a.h + o_lnp, (size_t)W * 8);
    if (accepted) {
        const int64_t* acc = (const int64_t*)(a.h + o_acc);
        for (int64_t x = 0; x < W; ++x) accepted[x] += acc[x];
    }
    if (chain) big_copy(chain, a.h + o_chain, (size_t)n_steps * WP * 8);
    if (lnprob_chain) std::memcpy(lnprob_chain, a.h + o_lnpc, (size_t)n_steps * W * 8);
    if (energy_error) std::memcpy(energy_error, a.h + o_err, (size_t)n_steps * W * 8);
    *done = true;
    return MCD_OK;
}

int run_hmc(mcd_catalog* cat, const mcd_hmc_desc* d, int64_t n_steps, double* pos, double* lnp, uint64_t seed, int64_t step0,
            double* chain, double* lnprob_chain, int64_t* accepted, double* energy_error, const mcd_prior_desc* prior) {
    if (!cat || !d || !pos || !lnp) return fail(MCD_ERR_INVALID, "mcd_hmc_block: null argument");
    if (int urc = ctx_usable(cat->ctx)) return urc;
    const mcd_stretch_desc& m = d->map;
    if (m.n_bins > 1 || cat->n_psets != 1)
        return fail(MCD_ERR_INVALID, "mcd_hmc_block: binned catalogues are not covered (lock-stepped ensembles have no HMC block)");
    if (cat->precision != MCD_F64) return fail(MCD_ERR_INVALID, "mcd_hmc_block: gradients need an MCD_F64 catalogue");
    if (m.k != cat->k) return fail(MCD_ERR_INVALID, "mcd_hmc_block: descriptor has the wrong number of kernel columns");
    if (m.n_walkers < 1 || m.n_dim < 1 || m.n_dim > mcd::kHmcMaxDim || n_steps < 0 || step0 < 0)
        return fail(MCD_ERR_INVALID, "mcd_hmc_block: n_walkers >= 1, 1 <= n_dim <= 12, steps non-negative");
    if (!m.col_source || !m.col_const || !m.col_factor || !m.lo || !m.hi || !d->chol) return fail(MCD_ERR_INVALID, "mcd_hmc_block: null descriptor array");
    for (int c = 0; c < m.k; ++c)
        if (m.col_source[c] >= m.n_dim) return fail(MCD_ERR_INVALID, "mcd_hmc_block: col_source outside the free parameters");
    mcd::HmcShared hs;
    hs.n_dim = m.n_dim; hs.k = m.k; hs.col_source = m.col_source; hs.col_const = m.col_const; hs.col_factor = m.col_factor;
    hs.lo = m.lo; hs.hi = m.hi; hs.chol = d->chol; hs.fixed_ok = m.fixed_ok; hs.n_leap = d->n_leap;
    hs.step_size = d->step_size; hs.jitter = d->jitter;
    hs.diagonal = mcd::hmc_is_diagonal(d->chol, m.n_dim) ? 1 : 0;
    PriorHost ph;
    if (int prc = prior_of(prior, m.n_dim, "mcd_hmc_block", ph)) return prc;
    hs.prior = ph.table;
    if (!mcd::hmc_args_ok(hs, m.n_walkers))
        return fail(MCD_ERR_INVALID, "mcd_hmc_block: step_size > 0, 0 <= jitter < 1, n_leap >= 1 and a finite lower-triangular chol with a positive diagonal");
    const int64_t W = m.n_walkers;
    if (hmc_resident_covers(cat, W, hs.n_dim, n_steps)) {
        bool done = false;
        const int rc = hmc_block_device(cat, hs, W, n_steps, pos, lnp, seed, step0, chain, lnprob_chain, accepted, energy_error, &done);
        if (rc != MCD_OK) return rc;
        if (done) return MCD_OK;
    }
    // host-driven block: the same loop (mcd_hmc.h) around mcd_loglike_grad_batch, whose all-reduce makes it work on
    // several devices and ranks
    ++cat->hmc_host_blocks;
    int eval_rc = MCD_OK;
    const int rc = mcd::hmc_block(hs, W, n_steps, pos, lnp, seed, step0, chain, lnprob_chain, accepted, energy_error,
                                  [&](const double* table, int64_t n, double* out, double* grad) {
                                      eval_rc = mcd_loglike_grad_batch(cat, n, m.k, table, out, grad);
                                      return eval_rc;
                                  });
    if (rc == mcd::HMC_EVAL_FAILED) return eval_rc;                      // message already set
    if (rc == mcd::HMC_NONFINITE)
        return fail(MCD_ERR_NONFINITE, "mcd_hmc_block: a walker starts outside the prior or with a non-finite log-likelihood or gradient");
    if (rc != mcd::HMC_OK) return fail(MCD_ERR_INVALID, "mcd_hmc_block: bad arguments");
    return MCD_OK;
}

}  // namespace

extern "C" {

int mcd_stretch_move(mcd_catalog* cat, const mcd_stretch_desc* d, int64_t n_steps, double* pos, double* lnp,
                     const int32_t* order, const double* zz, const double* thr, const int32_t* pick, double* chain,
                     double* lnprob_chain, int64_t* accepted) {
    try {
    return run_stretch(cat, d, n_steps, pos, lnp, order, zz, thr, pick, chain, lnprob_chain, accepted, nullptr, 0, nullptr);
    } catch (...) { return on_exception("mcd_stretch_move"); }
}

int mcd_stretch_move_prior(mcd_catalog* cat, const mcd_stretch_desc* d, int64_t n_steps, double* pos, double* lnp,
                           const int32_t* order, const double* zz, const double* thr, const int32_t* pick, double* chain,
                           double* lnprob_chain, int64_t* accepted, const mcd_prior_desc* prior) {
    try {
    return run_stretch(cat, d, n_steps, pos, lnp, order, zz, thr, pick, chain, lnprob_chain, accepted, nullptr, 0, prior);
    } catch (...) { return on_exception("mcd_stretch_move_prior"); }
}

int mcd_stretch_move_seeded(mcd_catalog* cat, const mcd_stretch_desc* d, int64_t n_steps, double* pos, double* lnp,
                            uint64_t seed, int64_t step0, double* chain, double* lnprob_chain, int64_t* accepted) {
    try {
    return run_stretch(cat, d, n_steps, pos, lnp, nullptr, nullptr, nullptr, nullptr, chain, lnprob_chain, accepted, &seed, step0,
                       nullptr);
    } catch (...) { return on_exception("mcd_stretch_move_seeded"); }
}

int mcd_stretch_move_seeded_prior(mcd_catalog* cat, const mcd_stretch_desc* d, int64_t n_steps, double* pos, double* lnp,
                                  uint64_t seed, int64_t step0, double* chain, double* lnprob_chain, int64_t* accepted,
                                  const mcd_prior_desc* prior) {
    try {
    return run_stretch(cat, d, n_steps, pos, lnp, nullptr, nullptr, nullptr, nullptr, chain, lnprob_chain, accepted, &seed, step0,
                       prior);
    } catch (...) { return on_exception("mcd_stretch_move_seeded_prior"); }
}

int mcd_prior_eval(const mcd_prior_desc* prior, int64_t n_rows, const double* x, double* value, double* grad) {
    try {
    if (!prior || n_rows < 0 || (n_rows > 0 && (!x || !value))) return fail(MCD_ERR_INVALID, "mcd_prior_eval: null argument");
    PriorHost ph;
    if (int prc = prior_of(prior, prior->n_dim, "mcd_prior_eval", ph)) return prc;
    const int P = prior->n_dim;
    for (int64_t r = 0; r < n_rows; ++r) {
        const double* row = x + r * P;
        double* g = grad ? grad + r * P : nullptr;
        if (g) for (int c = 0; c < P; ++c) g[c] = 0.0;
        if (!ph.table.any()) { value[r] = 0.0; continue; }
        if (!mcd::prior_row_inside(ph.table, P, row)) { value[r] = -INFINITY; continue; }
        value[r] = g ? mcd::prior_row_grad(ph.table, P, row, g) : mcd::prior_row(ph.table, P, row);
    }
    return MCD_OK;
    } catch (...) { return on_exception("mcd_prior_eval"); }
}

int mcd_chain_numbers(uint64_t seed, int64_t step0, int64_t n_steps, int64_t n_bins, int64_t n_walkers, int32_t n_dim,
                      int32_t* order, double* zz, double* thr, int32_t* pick) {
    try {
    if (!order || !zz || !thr || !pick || n_steps < 0 || step0 < 0 || n_walkers <= 0 || (n_walkers & 1) || n_dim <= 0)
        return fail(MCD_ERR_INVALID, "mcd_chain_numbers: bad arguments");
    if (n_walkers > mcd::kSeededMaxWalkers) return fail(MCD_ERR_INVALID, "mcd_chain_numbers: n_walkers <= 1048576");
    const int64_t B = n_bins > 1 ? n_bins : 1, W = n_walkers, half = W / 2;
    std::vector<uint64_t> sorter;
    for (int64_t i = 0; i < n_steps; ++i)
        mcd::chain_numbers_of_step(seed, step0 + i, B, W, n_dim, order + (size_t)i * B * W, zz + (size_t)i * 2 * B * half,
                                   thr + (size_t)i * 2 * B * half, pick + (size_t)i * 2 * B * half, sorter);
    return MCD_OK;
    } catch (...) { return on_exception("mcd_chain_numbers"); }
}

int mcd_hmc_block(mcd_catalog* cat, const mcd_hmc_desc* d, int64_t n_steps, double* pos, double* lnp, uint64_t seed,
                  int64_t step0, double* chain, double* lnprob_chain, int64_t* accepted, double* energy_error) {
    try {
    return run_hmc(cat, d, n_steps, pos, lnp, seed, step0, chain, lnprob_chain, accepted, energy_error, nullptr);
    } catch (...) { return on_exception("mcd_hmc_block"); }
}

int mcd_hmc_block_prior(mcd_catalog* cat, const mcd_hmc_desc* d, int64_t n_steps, double* pos, double* lnp, uint64_t seed,
                        int64_t step0, double* chain, double* lnprob_chain, int64_t* accepted, double* energy_error,
                        const mcd_prior_desc* prior) {
    try {
    return run_hmc(cat, d, n_steps, pos, lnp, seed, step0, chain, lnprob_chain, accepted, energy_error, prior);
    } catch (...) { return on_exception("mcd_hmc_block_prior"); }
}

int mcd_hmc_numbers(uint64_t seed, int64_t step0, int64_t n_steps, int64_t n_walkers, int32_t n_dim, double* z, double* thr,
                    double* eps_factor) {
    try {
    if (!z || !thr || !eps_factor || n_steps < 0 || step0 < 0 || n_walkers < 1 || n_dim < 1 || n_dim > mcd::kHmcMaxDim)
        return fail(MCD_ERR_INVALID, "mcd_hmc_numbers: bad arguments");
    for (int64_t i = 0; i < n_steps; ++i)
        for (int64_t w = 0; w < n_walkers; ++w) {
            for (int c = 0; c < n_dim; ++c) z[((size_t)i * n_walkers + w) * n_dim + c] = mcd::hmc_normal(seed, step0 + i, w, c);
            mcd::hmc_aux(seed, step0 + i, w, thr[(size_t)i * n_walkers + w], eps_factor[(size_t)i * n_walkers + w]);
        }
    return MCD_OK;
    } catch (...) { return on_exception("mcd_hmc_numbers"); }
}

int mcd_hmc_info(const mcd_catalog* cat, int64_t* device_blocks, int64_t* host_blocks) {
    if (!cat) return fail(MCD_ERR_INVALID, "null catalogue");
    if (device_blocks) *device_blocks = cat->hmc_device_blocks;
    if (host_blocks) *host_blocks = cat->hmc_host_blocks;
    return MCD_OK;
}

}  // extern "C"

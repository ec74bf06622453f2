// mcd_temper.h -- host+device: the per-walker algebra of parallel tempering (Swendsen & Wang 1986; Geyer 1991; Earl & Deem
// 2005) on the stretch move of mcd_stretch.h.  Written once and used by the device kernels (mcd_temper.hip), by the
// host-driven block (mcd_api_temper.hip: temper_block below around mcd_loglike_batch) and by the CPU harness
// tests/emul/temper_emul.cpp.  No HIP types; compiled with -ffp-contract=off everywhere, and every operation below is an
// IEEE +, -, * or comparison in a fixed order (the logarithms are mcd_rng.h's det_log), so that host and device produce
// the same bits.  The reference has one ensemble at one temperature (emcee's stretch move, analysis/runner.py:403-419).
//
// T ensembles ("rungs") of W walkers each sample prior(x) L(x)^beta_t on a ladder 1 = beta_0 > beta_1 > ... > beta_{T-1} >= 0.
// State per rung t and walker w: position [P], log-likelihood ll, log-prior lp (0.0 inside the box when the block has no
// structured prior) -- kept as ll and lp, never as their sum: the rungs weigh them differently.
//
// One step (absolute step index `step`) has three phases:
//   half steps h = 0, 1, in every rung at once: the stretch move of mcd_stretch.h with ensemble index b = t.  The split of
//             the ensemble, the stretch factor z, the threshold thr and the partner come from chain_draw(seed, step, h, t,
//             j, W/2, P) in the order chain_numbers_of_step produces for B = T.
//     propose   p = q - (q - s) z   (s: the walker that moves, q: its partner in the other half of ITS OWN rung)
//     inside    iff fixed_ok, lo <= p <= hi (inclusive; false for NaN) and every prior's support holds p (prior_row_inside)
//     row       the launch needs a valid row for every slot: a proposal outside the prior is "evaluated" at the walker's own
//               current position s and the result is ignored (the rule mcd_hmc.h uses for a rejected trajectory)
//     accept    iff inside, ll_new finite and
//                    thr < beta_t * (ll_new - ll_old)                          without structured priors
//                    thr < beta_t * (ll_new - ll_old) + (lp_new - lp_old)      with them
//               in exactly this order: the difference of the log-likelihoods, times beta_t, plus the difference of the
//               log-priors.  With beta = 1 and no prior that is the stretch move's `thr < ll_new - ll_old` bit for bit
//               (1.0 * x is exact).  A proposal outside the prior or with ll_new = +-inf is rejected at EVERY rung, beta = 0
//               included (0 * inf would be NaN, and a point of zero likelihood has no place on the ladder); a NaN ll_new of
//               a proposal inside the prior is an error (TEMPER_NAN, as STRETCH_NAN).  fixed_ok == 0 rejects everything.
//   swap phase, after half step 1: the adjacent pairs (t, t + 1) with t = step (mod 2), walker w of rung t with walker w of
//             rung t + 1 (the walkers of an ensemble are exchangeable and its split is reshuffled every step).  One
//             generator call per (step, t, w) with a key of its own:
//     accept    iff det_log(u) < (beta_t - beta_{t+1}) * (ll_{t+1} - ll_t)      (and fixed_ok)
//               the two walkers then exchange position, ll and lp.  Every (pair, walker) decision touches two walkers
//               nobody else touches in this phase: one parallel pass.  Proposed and accepted swaps are counted per pair.
//   rows      the step's chain rows are the state after the swap phase.
#pragma once

#include <cstdint>
#include <vector>

#include "mcd_prior.h"
#include "mcd_rng.h"

namespace mcd {

constexpr int kTemperMaxDim = 12;                            // P <= 12 free parameters, as mcd_hmc.h
constexpr uint64_t kTemperKey1 = 0x6d63645f746d70ull;        // "mcd_tmp": neither kChainKey1 nor kHmcKey1

MCD_HD bool temper_finite(double x) { return x - x == 0.0; }    // false for NaN and +-inf

// What a block shares between its walkers (pointers into host or device memory, by where the code runs).
struct TemperShared {
    int32_t n_dim = 0, k = 0;                  // P, K
    const int32_t* col_source = nullptr;       // [K]  as mcd_stretch_desc
    const double* col_const = nullptr;         // [K]
    const double* col_factor = nullptr;        // [K]
    const double* lo = nullptr;                // [P]
    const double* hi = nullptr;                // [P]
    int32_t fixed_ok = 1;
    int32_t n_temps = 0;                       // T
    int64_t n_walkers = 0;                     // W per rung (even)
    const double* betas = nullptr;             // [T]
    PriorTable prior;                          // structured priors of the free parameters, or none
};

// log(u) of the swap of walker w between rungs t and t + 1 in step `step`: word 0 of ONE generator call
MCD_HD double temper_swap_thr(uint64_t seed, int64_t step, int64_t t, int64_t w) {
    const Philox4x64 r = philox4x64_10((uint64_t)step, (uint64_t)t, (uint64_t)w, 0, seed, kTemperKey1);
    return det_log(uniform53(r.v[0]));
}

// is the pair (t, t + 1) exchanged in step `step`
MCD_HD bool temper_pair_active(int64_t step, int64_t t, int64_t n_temps) { return t + 1 < n_temps && ((t ^ step) & 1) == 0; }

// resolved kernel row of a position: mcd_stretch.h's rule, column by column
MCD_HD void temper_row(const TemperShared& s, const double* q, double* row) {
    for (int c = 0; c < s.k; ++c) {
        const int src = s.col_source[c];
        row[c] = src < 0 ? s.col_const[c] : (s.col_factor[c] == 1.0 ? q[src] : q[src] * s.col_factor[c]);
    }
}

// is x [P] inside the prior: the inclusive box and every prior's support
MCD_HD bool temper_inside(const TemperShared& s, const double* x) {
    bool good = true;
    for (int c = 0; c < s.n_dim; ++c) good = good && (x[c] >= s.lo[c]) && (x[c] <= s.hi[c]);      // false for NaN as well
    if (good && s.prior.any()) good = prior_row_inside(s.prior, s.n_dim, x);
    return good;
}

// log-prior of a position inside the prior: 0.0 without structured priors
MCD_HD double temper_lnprior(const TemperShared& s, const double* x) {
    return s.prior.any() ? prior_row(s.prior, s.n_dim, x) : 0.0;
}

// Proposal of the walker at `sp` with partner `q` and stretch factor z: p [P], the kernel row to evaluate [K] (the walker's
// own when the proposal is outside the prior) and the proposal's log-prior.  Returns whether the proposal is inside.
MCD_HD bool temper_propose(const TemperShared& s, const double* sp, const double* q, double z, double* p, double* row,
                           double* lp_new) {
    for (int c = 0; c < s.n_dim; ++c) p[c] = q[c] - (q[c] - sp[c]) * z;
    const bool good = s.fixed_ok != 0 && temper_inside(s, p);
    temper_row(s, good ? p : sp, row);
    *lp_new = good ? temper_lnprior(s, p) : 0.0;
    return good;
}

// 1 accept, 0 reject, -1 the log-likelihood of a proposal inside the prior is NaN (the operation order: head of this file)
MCD_HD int temper_accept(const TemperShared& s, double beta, double thr, bool inside, double ll_new, double lp_new,
                         double ll_old, double lp_old) {
    if (!inside) return 0;
    if (ll_new != ll_new) return -1;
    if (!temper_finite(ll_new)) return 0;
    double d = beta * (ll_new - ll_old);
    if (s.prior.any()) d = d + (lp_new - lp_old);
    return thr < d ? 1 : 0;
}

// the swap of one walker between rungs t and t + 1
MCD_HD bool temper_swap_accept(const TemperShared& s, int64_t t, double thr, double ll_t, double ll_t1) {
    return s.fixed_ok != 0 && thr < (s.betas[t] - s.betas[t + 1]) * (ll_t1 - ll_t);
}

// ---- host: one block of steps around a log-likelihood callable ------------------------------------------------------
enum TemperStatus : int { TEMPER_OK = 0, TEMPER_NAN = 1, TEMPER_EVAL_FAILED = 2, TEMPER_BAD_ARGS = 3, TEMPER_OUTSIDE = 4 };

// W even and >= 2, 1 <= T, betas[0] == 1, strictly decreasing within [0, 1], 1 <= P <= 12, 1 <= n_chain_temps <= T
inline bool temper_args_ok(const TemperShared& s, int32_t n_chain_temps) {
    if (s.n_walkers < 2 || (s.n_walkers & 1) || s.n_walkers > kSeededMaxWalkers) return false;
    if (s.n_temps < 1 || s.n_dim < 1 || s.n_dim > kTemperMaxDim || s.k < 1 || !s.betas) return false;
    if (n_chain_temps < 1 || n_chain_temps > s.n_temps) return false;
    if (!(s.betas[0] == 1.0)) return false;
    for (int t = 0; t < s.n_temps; ++t) {
        if (!(s.betas[t] >= 0.0) || !(s.betas[t] <= 1.0)) return false;                   // false for NaN as well
        if (t > 0 && !(s.betas[t] < s.betas[t - 1])) return false;
    }
    return true;
}

// The block's starting point: every walker inside the prior with a finite log-likelihood (else TEMPER_OUTSIDE; with
// fixed_ok == 0 nothing ever moves and nothing is checked).  lp [T][W] is WRITTEN: the log-prior of every start position.
inline int temper_start(const TemperShared& s, const double* pos, const double* ll, double* lp) {
    const int64_t n = (int64_t)s.n_temps * s.n_walkers;
    for (int64_t x = 0; x < n; ++x) {
        const bool ok = temper_inside(s, pos + x * s.n_dim) && temper_finite(ll[x]);
        if (!ok && s.fixed_ok) return TEMPER_OUTSIDE;
        lp[x] = ok ? temper_lnprior(s, pos + x * s.n_dim) : 0.0;
    }
    return TEMPER_OK;
}

// proposed swaps of pair t in steps step0 .. step0 + n_steps - 1: W per step of the pair's parity
inline int64_t temper_swaps_proposed(int64_t step0, int64_t n_steps, int64_t t, int64_t n_temps, int64_t W) {
    int64_t n = 0;
    for (int64_t i = 0; i < n_steps; ++i) n += temper_pair_active(step0 + i, t, n_temps) ? W : 0;
    return n;
}

// eval(table [T W/2][K], T W/2, out [T W/2]) -> 0 on success: the batched log-likelihood of one half step's rows, rung-major.
// pos [T][W][P] and ll [T][W] are updated in place and lp [T][W] is written (the log-prior of the start positions is
// computed here, whatever the array holds), all three only with final values and only when the block succeeds.
// chain [n_steps][n_chain_temps][W][P], lnlike_chain [n_steps][T][W], accepted [T][W], swap_proposed / swap_accepted [T-1]
// (all three incremented) may be null.
template <class Eval>
int temper_block(const TemperShared& s, int64_t n_steps, double* pos, double* ll, double* lp, uint64_t seed, int64_t step0,
                 int32_t n_chain_temps, double* chain, double* lnlike_chain, int64_t* accepted, int64_t* swap_proposed,
                 int64_t* swap_accepted, Eval&& eval) {
    if (!temper_args_ok(s, n_chain_temps) || n_steps < 0 || step0 < 0) return TEMPER_BAD_ARGS;
    const int64_t T = s.n_temps, W = s.n_walkers, half = W / 2, rows = T * half;
    const int P = s.n_dim, K = s.k;
    std::vector<double> cur(pos, pos + T * W * P), cll(ll, ll + T * W), clp((size_t)(T * W));
    if (temper_start(s, cur.data(), cll.data(), clp.data()) != TEMPER_OK) return TEMPER_OUTSIDE;
    std::vector<double> proposal((size_t)rows * P), table((size_t)rows * K), ll_new((size_t)rows), lp_new((size_t)rows);
    std::vector<uint8_t> ok((size_t)rows);
    std::vector<int32_t> order((size_t)(T * W)), pick((size_t)(2 * rows));
    std::vector<double> zz((size_t)(2 * rows)), thr((size_t)(2 * rows));
    std::vector<int64_t> acc((size_t)(T * W), 0), sw_acc((size_t)T, 0);
    std::vector<uint64_t> sorter;
    for (int64_t i = 0; i < n_steps; ++i) {
        const int64_t step = step0 + i;
        chain_numbers_of_step(seed, step, T, W, P, order.data(), zz.data(), thr.data(), pick.data(), sorter);
        for (int h = 0; h < 2; ++h) {
            for (int64_t t = 0; t < T; ++t) {
                const int32_t* first = order.data() + t * W + (h == 0 ? 0 : half);
                const int32_t* second = order.data() + t * W + (h == 0 ? half : 0);
                const double* ens = cur.data() + t * W * P;
                for (int64_t j = 0; j < half; ++j) {
                    const int64_t r = t * half + j, at = ((int64_t)h * T + t) * half + j;
                    ok[r] = temper_propose(s, ens + (int64_t)first[j] * P, ens + (int64_t)second[pick[at]] * P, zz[at],
                                           proposal.data() + r * P, table.data() + r * K, &lp_new[r]);
                }
            }
            if (eval(table.data(), rows, ll_new.data()) != 0) return TEMPER_EVAL_FAILED;
            for (int64_t t = 0; t < T; ++t) {
                const int32_t* first = order.data() + t * W + (h == 0 ? 0 : half);
                for (int64_t j = 0; j < half; ++j) {
                    const int64_t r = t * half + j, at = ((int64_t)h * T + t) * half + j, w = t * W + first[j];
                    const int a = temper_accept(s, s.betas[t], thr[at], ok[r] != 0, ll_new[r], lp_new[r], cll[w], clp[w]);
                    if (a < 0) return TEMPER_NAN;
                    if (a > 0) {
                        for (int c = 0; c < P; ++c) cur[w * P + c] = proposal[r * P + c];
                        cll[w] = ll_new[r];
                        clp[w] = lp_new[r];
                        acc[w] += 1;
                    }
                }
            }
        }
        for (int64_t t = 0; t + 1 < T; ++t) {
            if (!temper_pair_active(step, t, T)) continue;
            for (int64_t w = 0; w < W; ++w) {
                const int64_t a = t * W + w, b = (t + 1) * W + w;
                if (!temper_swap_accept(s, t, temper_swap_thr(seed, step, t, w), cll[a], cll[b])) continue;
                for (int c = 0; c < P; ++c) { const double x = cur[a * P + c]; cur[a * P + c] = cur[b * P + c]; cur[b * P + c] = x; }
                { const double x = cll[a]; cll[a] = cll[b]; cll[b] = x; }
                { const double x = clp[a]; clp[a] = clp[b]; clp[b] = x; }
                sw_acc[t] += 1;
            }
        }
        if (chain)
            for (int64_t x = 0; x < (int64_t)n_chain_temps * W * P; ++x) chain[i * n_chain_temps * W * P + x] = cur[x];
        if (lnlike_chain) for (int64_t x = 0; x < T * W; ++x) lnlike_chain[i * T * W + x] = cll[x];
    }
    // (the caller's state is written last, with final values only)
    for (int64_t x = 0; x < T * W * P; ++x) pos[x] = cur[x];
    for (int64_t x = 0; x < T * W; ++x) { ll[x] = cll[x]; lp[x] = clp[x]; }
    if (accepted) for (int64_t x = 0; x < T * W; ++x) accepted[x] += acc[x];
    for (int64_t t = 0; t + 1 < T; ++t) {
        if (swap_proposed) swap_proposed[t] += temper_swaps_proposed(step0, n_steps, t, T, W);
        if (swap_accepted) swap_accepted[t] += sw_acc[t];
    }
    return TEMPER_OK;
}

// ---- device: the resident block (mcd_temper.hip) -------------------------------------------------------------------
// Everything the two kernels need, by value in their argument block; every pointer is device memory.
struct TemperDevice {
    TemperShared s;
    uint64_t seed = 0;
    double* pos = nullptr;            // [T][W][P] current points, their log-likelihoods [T][W] and log-priors [T][W]
    double* ll = nullptr;
    double* lp = nullptr;
    long long* accepted = nullptr;    // [T][W] stretch-move accepts of this block
    long long* swap_accepted = nullptr;   // [T][W] accepted swaps of (pair t, walker w) in this block (row T - 1 stays 0)
    int32_t* status = nullptr;        // [1] set to 1 by a NaN log-likelihood of a proposal inside the prior
    const int32_t* order = nullptr;   // the block's stretch numbers as launch_chain_numbers writes them for B = T:
    const double* zz = nullptr;       // order [n_steps][T][W], zz / thr / pick [n_steps][2][T][W/2]
    const double* thr = nullptr;
    const int32_t* pick = nullptr;
    double* proposal = nullptr;       // [T W/2][P], and per row: inside the prior, the proposal's log-prior
    uint8_t* ok = nullptr;
    double* lp_new = nullptr;
    double* table = nullptr;          // [T W/2][K] the work set's parameter table (prepare_walkers reads it)
    const double* out = nullptr;      // [T W/2] reduced log-likelihoods of the rows
    double* chain = nullptr;          // [n_steps][n_chain_temps][W][P] or null
    double* lnlike_chain = nullptr;   // [n_steps][T][W] or null
    int32_t n_chain_temps = 1;
};

#if defined(__HIPCC__)
// acc_i / prop_i: index inside the block of the step whose half step acc_h is accepted / whose half step prop_h is
// proposed (-1: none); the accept runs first.  swap: the swap phase of absolute step `step`, rows of block index `row`.
hipError_t launch_temper_step(hipStream_t s, const TemperDevice& d, int64_t acc_i, int acc_h, int64_t prop_i, int prop_h);
hipError_t launch_temper_swap(hipStream_t s, const TemperDevice& d, int64_t step, int64_t row);
#endif

}  // namespace mcd

// mcd_de.h -- the differential-evolution move of the ensemble samplers (ter Braak 2006; with a jittered scale, Nelson et
// al. 2013), beside the stretch move of mcd_stretch.h: the same red / blue half steps, the same launch of W/2 rows per half
// step, the same kernels -- only the proposal and its acceptance rule differ.
//
// For half step h of step i, ensemble b, slot j (half = W/2, first / second the halves of the step's split, s = pos[first[j]]):
//   partners   a = min(floor(u0 half), half - 1), c = min(floor(u1 (half - 1)), half - 2), a' = c + (c >= a): two DISTINCT
//              slots of the complementary half, every ordered pair equally likely -- the proposal is symmetric
//   scale      g = gamma0 (1 + sigma n), n a standard normal (defaults of the samplers: gamma0 = 2.38 / sqrt(2 P), 1e-5)
//   proposal   p[c] = s[c] + (x_a[c] - x_a'[c]) * g: a subtraction, a multiplication, an addition (no contraction)
//   accept     iff thr < lnp_new - lnp_old, thr = det_log(u2): no (P - 1) log z term
//   split      walkers sorted by (upper 44 bits of a generator word, walker index), exactly as chain_draw's (mcd_rng.h)
//
// Random numbers: Philox4x64-10 under a key constant of its own (kDeKey1: never the stretch move's stream of the same seed),
// counter = (step, half step + 2 call, ensemble, slot).  Call 0 holds u0, u1, u2 and the ordering key; calls 1 .. hold the
// pairs of the normal's polar method (with det_log, as hmc_normal of mcd_hmc.h: no libm call decides a bit).  A chain is a
// function of (seed, step, half step, ensemble, slot) alone; any range of steps can be replayed on the host.
//
// The first part (de_draw and below) is host + device code; de_block is host only, shared by the C-ABI (mcd_api_de.hip) and
// the CPU test harness (tests/emul).
#pragma once

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <vector>

#include "mcd_prior.h"
#include "mcd_rng.h"
#include "mcd_stretch.h"   // StretchDesc, StretchStatus: the block's contract is the stretch block's

namespace mcd {

constexpr uint64_t kDeKey1 = 0x6d63645f64656dull;            // "mcd_dem": never the stretch move's stream (kChainKey1)
// Marsaglia's polar method accepts a pair with probability pi / 4; each generator call holds two pairs.  After kDeNormalCalls
// calls (32 pairs) the draw gives up and returns 0.0 (g = gamma0): probability 4.1e-22 per normal, and harmless if it ever did.
constexpr int kDeNormalCalls = 16;

struct DeDraw { double gamma, thr; int32_t pick_a, pick_b; uint64_t order_key; };

// the raw words of generator call `call` of (step, h, b, j): call 0 the draw's own, 1 .. the normal's pairs
MCD_HD Philox4x64 de_words(uint64_t seed, int64_t step, int h, int64_t b, int64_t j, int call) {
    return philox4x64_10((uint64_t)step, (uint64_t)(h + 2 * call), (uint64_t)b, (uint64_t)j, seed, kDeKey1);
}

// Standard normal of (seed, step, h, b, j): u, v = 2 uniform53 - 1, s = u^2 + v^2, accepted for 0 < s < 1,
// n = u sqrt(-2 log(s) / s).  `max_calls` is kDeNormalCalls everywhere but in the test that walks into the fallback;
// *pairs_used (may be null): pairs drawn.
MCD_HD double de_normal(uint64_t seed, int64_t step, int h, int64_t b, int64_t j, int max_calls = kDeNormalCalls,
                        int* pairs_used = nullptr) {
    int used = 0;
    for (int c = 0; c < max_calls; ++c) {
        const Philox4x64 r = de_words(seed, step, h, b, j, 1 + c);
        for (int q = 0; q < 2; ++q) {
            const double u = 2.0 * uniform53(r.v[2 * q]) - 1.0, v = 2.0 * uniform53(r.v[2 * q + 1]) - 1.0;
            const double s = u * u + v * v;
            ++used;
            if (s > 0.0 && s < 1.0) {
                if (pairs_used) *pairs_used = used;
                return u * sqrt_(-2.0 * det_log(s) / s);
            }
        }
    }
    if (pairs_used) *pairs_used = used;
    return 0.0;                                                // documented fallback, see kDeNormalCalls
}

// half >= 2.  order_key: (upper 44 bits) << 20 | walker, walker = h half + j -- chain_draw's.
MCD_HD DeDraw de_draw(uint64_t seed, int64_t step, int h, int64_t b, int64_t j, int64_t half, double gamma0, double sigma,
                      int max_calls = kDeNormalCalls) {
    const Philox4x64 r = de_words(seed, step, h, b, j, 0);
    DeDraw d;
    int64_t a = (int64_t)(uniform53(r.v[0]) * (double)half);
    a = a < half ? a : half - 1;
    int64_t c = (int64_t)(uniform53(r.v[1]) * (double)(half - 1));
    c = c < half - 1 ? c : half - 2;
    d.pick_a = (int32_t)a;
    d.pick_b = (int32_t)(c + (c >= a ? 1 : 0));
    d.thr = det_log(uniform53(r.v[2]));
    d.order_key = ((r.v[3] >> kOrderKeyShift) << kOrderKeyShift) | (uint64_t)((int64_t)h * half + j);
    const double n = de_normal(seed, step, h, b, j, max_calls);
    d.gamma = gamma0 * (1.0 + sigma * n);
    return d;
}

// What the entry points accept (include/mcd.h): W >= 4 and even (two distinct partners in a half), a finite gamma0 > 0, a
// finite sigma >= 0.
inline bool de_args_ok(int64_t n_walkers, double gamma0, double sigma) {
    return n_walkers >= 4 && !(n_walkers & 1) && n_walkers <= kSeededMaxWalkers && gamma0 > 0.0 && gamma0 - gamma0 == 0.0 &&
           sigma >= 0.0 && sigma - sigma == 0.0;
}

// Host: the numbers of ONE step in the layout mcd_de_move takes for a block of one step: order [B][W], pick_a / pick_b /
// gamma / thr [2][B][W/2].
inline void de_numbers_of_step(uint64_t seed, int64_t step, int64_t B, int64_t W, double gamma0, double sigma, int32_t* order,
                               int32_t* pick_a, int32_t* pick_b, double* gamma, double* thr, std::vector<uint64_t>& sorter) {
    const int64_t half = W / 2;
    sorter.resize((size_t)W);
    for (int64_t b = 0; b < B; ++b) {
        for (int h = 0; h < 2; ++h)
            for (int64_t j = 0; j < half; ++j) {
                const DeDraw dd = de_draw(seed, step, h, b, j, half, gamma0, sigma);
                const int64_t at = ((int64_t)h * B + b) * half + j;
                pick_a[at] = dd.pick_a; pick_b[at] = dd.pick_b; gamma[at] = dd.gamma; thr[at] = dd.thr;
                sorter[(size_t)(h * half + j)] = dd.order_key;
            }
        std::sort(sorter.begin(), sorter.end());                       // (distinct: the walker index is part of the key)
        for (int64_t x = 0; x < W; ++x) order[b * W + x] = (int32_t)(sorter[(size_t)x] & (((uint64_t)1 << kOrderKeyShift) - 1));
    }
}

// ---- host only: one block of steps around `eval`, written operation for operation like the NumPy loop of
// mcmc_dynamics_amd/sampler.py (_half_steps, move "de").  The contract is stretch_block's (mcd_stretch.h): box prior plus
// structured priors, fixed_ok, rows outside the prior take the first valid row's place in the launch and are masked
// afterwards, NaN gives STRETCH_NAN, B lock-stepped ensembles share every evaluation.  The numbers are the caller's:
// order [n][B][W], pick_a / pick_b / gamma / thr [n][2][B][W/2].
template <class Eval>
int de_block(const StretchDesc& d, int64_t n_steps, double* pos, double* lnp, const int32_t* order, const int32_t* pick_a,
             const int32_t* pick_b, const double* gamma, const double* thr, double* chain, double* lnprob_chain,
             int64_t* accepted, Eval&& eval) {
    const int64_t B = d.n_bins, W = d.n_walkers, half = W / 2;
    const int P = d.n_dim, K = d.k;
    if (B <= 0 || W < 4 || (W & 1) || P <= 0 || K <= 0) return STRETCH_BAD_ARGS;
    const int64_t rows = B * half;
    std::vector<double> proposal((size_t)rows * P), table((size_t)rows * K), ll((size_t)rows), new_lnp((size_t)rows);
    std::vector<uint8_t> ok((size_t)rows);
    for (int64_t i = 0; i < n_steps; ++i) {
        for (int h = 0; h < 2; ++h) {
            // proposal = s + (x_a - x_b) * g   (sampler.py: `s_pos + (xa - xb) * gamma[:, None]`)
            int64_t n_ok = 0, donor = -1;
            for (int64_t b = 0; b < B; ++b) {
                const int32_t* ord = order + (i * B + b) * W;
                const int32_t* first = ord + (h == 0 ? 0 : half);
                const int32_t* second = ord + (h == 0 ? half : 0);
                const int64_t at = ((i * 2 + h) * B + b) * half;
                const double* ens = pos + b * W * P;
                for (int64_t j = 0; j < half; ++j) {
                    const double* s = ens + (int64_t)first[j] * P;
                    const double* xa = ens + (int64_t)second[pick_a[at + j]] * P;
                    const double* xb = ens + (int64_t)second[pick_b[at + j]] * P;
                    const double g = gamma[at + j];
                    double* p = proposal.data() + (b * half + j) * P;
                    bool good = d.fixed_ok != 0;
                    for (int c = 0; c < P; ++c) {
                        p[c] = s[c] + (xa[c] - xb[c]) * g;
                        good = good && (p[c] >= d.lo[c]) && (p[c] <= d.hi[c]);        // false for NaN as well
                    }
                    if (d.prior.any()) good = good && prior_row_inside(d.prior, P, p);   // a log-normal coordinate <= 0
                    ok[b * half + j] = good;
                    if (good) { ++n_ok; if (donor < 0) donor = b * half + j; }
                }
            }
            if (n_ok > 0) {
                for (int64_t r = 0; r < rows; ++r) {
                    const double* p = proposal.data() + (ok[r] ? r : donor) * P;
                    double* row = table.data() + r * K;
                    for (int c = 0; c < K; ++c) {
                        const int src = d.col_source[c];
                        row[c] = src < 0 ? d.col_const[c] : (d.col_factor[c] == 1.0 ? p[src] : p[src] * d.col_factor[c]);
                    }
                }
                if (eval(table.data(), half, ll.data()) != 0) return STRETCH_EVAL_FAILED;
            }
            for (int64_t r = 0; r < rows; ++r) {
                new_lnp[r] = (n_ok > 0 && ok[r]) ? ll[r] : -INFINITY;
                if (d.prior.any() && n_ok > 0 && ok[r]) new_lnp[r] = ll[r] + prior_row(d.prior, P, proposal.data() + r * P);
                if (new_lnp[r] != new_lnp[r]) return STRETCH_NAN;                 // "Probability function returned NaN"
            }
            // accept iff thr < new_lnp - old_lnp   (thr = log(u): the proposal is symmetric)
            for (int64_t b = 0; b < B; ++b) {
                const int32_t* first = order + (i * B + b) * W + (h == 0 ? 0 : half);
                const double* t = thr + ((i * 2 + h) * B + b) * half;
                for (int64_t j = 0; j < half; ++j) {
                    const int64_t w = b * W + first[j], r = b * half + j;
                    if (t[j] < new_lnp[r] - lnp[w]) {
                        const double* p = proposal.data() + r * P;
                        for (int c = 0; c < P; ++c) pos[w * P + c] = p[c];
                        lnp[w] = new_lnp[r];
                        if (accepted) accepted[w] += 1;
                    }
                }
            }
        }
        if (chain) for (int64_t x = 0; x < B * W * P; ++x) chain[i * B * W * P + x] = pos[x];
        if (lnprob_chain) for (int64_t w = 0; w < B * W; ++w) lnprob_chain[i * B * W + w] = lnp[w];
    }
    return STRETCH_OK;
}

}  // namespace mcd

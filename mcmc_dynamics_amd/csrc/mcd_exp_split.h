// mcd_exp_split.h -- host side of the split exponent offset of the direct BGFIXED loops (option "exp_split"; the loop and
// its error budget: mcd_math.h: kExpSplitC, BgFixedAcc::add_gs).  Host only: everything here is evaluated in long double
// (x87 80-bit on the hosts this library is built for) and rounded once.  Shared with the CPU tests (tests/emul).
#pragma once

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <limits>
#include <vector>

#include "mcd_chunks.h"
#include "mcd_math.h"

namespace mcd {

constexpr long double kExpSplitInvStepL = 1.44269504088896340735992468100189214L * kExpTabSize;    // N / ln 2
constexpr long double kExpSplitStepL = 0.693147180559945309417232121458176568L / kExpTabSize;      // ln 2 / N
constexpr double kExpSplitMagic = 6755399441055744.0;                                              // 1.5 2^52

// One star's share of the split: nbp N / ln 2 = nbi + nbf with nbi = rint(..) (ties to even), so |nbf| <= 1/2.
//   M    = 1.5 2^52 + nbi - 5 N: an integer below 2^53 in magnitude, exact (|nbi| <= 3e6: nbp in [-2000, 60])
//   ompk = omp' = kappa omp,  kappa = (c / 32) e^{-nbf ln2/N} with c the DOUBLE kExpSplitC the kernel scales the root by
//   nbf  as a double (2^-54 of a table step off at most); kappa is formed from this rounded value, so that what the
//        chunk constant takes back is what the record put in
struct ExpSplitRecord {
    double M, ompk, nbf;
};
inline ExpSplitRecord exp_split_record(double nbp, double omp) {
    const long double t = (long double)nbp * kExpSplitInvStepL;
    const long double nbi = rintl(t);
    const double nbf = (double)(t - nbi);                                     // t - nbi is exact
    const long double kappa = ((long double)kExpSplitC / (1 << kExpSplitShift)) * expl(-(long double)nbf * kExpSplitStepL);
    ExpSplitRecord out;
    out.M = (double)((long double)kExpSplitMagic + (nbi - (long double)(kExpSplitShift * kExpTabSize)));
    out.ompk = (double)((long double)omp * kappa);
    out.nbf = nbf;
    return out;
}

// log kappa summed over `count` stars, with its sign turned: what a chunk adds to the sum of log y' to get the sum of log y
inline double exp_split_chunk_const(const double* nbf, int64_t count) {
    long double s = 0.0L;
    for (int64_t i = 0; i < count; ++i) s += (long double)nbf[i];
    return (double)(s * kExpSplitStepL - (long double)count * logl((long double)kExpSplitC / (1 << kExpSplitShift)));
}

// ---- the quadratic series root on 32-star bands (option "root_quad"; mcd_math.h: RootQuad) ----
// Block b of a verr-sorted array of n records is records 32 b .. 32 b + 31 in absolute positions, whatever the chunk plan;
// the last block also takes a remainder shorter than 32 (32 .. 63 stars), and an array shorter than 32 has no block.
constexpr int64_t kQuadBlock = 32;
inline int64_t quad_blocks(int64_t n) { return n / kQuadBlock; }
// the block of record i (n >= 32)
inline int64_t quad_block_of(int64_t i, int64_t n) { return std::min(i / kQuadBlock, quad_blocks(n) - 1); }
// Economisation of e^3 on the block whose verr^2 runs from e_lo to e_hi: e^3 = a2 e^2 + a1 e + a0 to within h^3 / 4 with
// m = (e_lo + e_hi) / 2, h = (e_hi - e_lo) / 2; each constant rounded ONCE from long double
struct QuadBlock {
    double a2, a1, a0, h;
};
inline QuadBlock quad_block(double e_lo, double e_hi) {
    const long double m = 0.5L * ((long double)e_lo + (long double)e_hi), h = 0.5L * ((long double)e_hi - (long double)e_lo);
    QuadBlock out;
    out.a2 = (double)(3.0L * m);
    out.a1 = (double)(0.75L * h * h - 3.0L * m * m);
    out.a0 = (double)(m * m * m - 0.75L * h * h * m);
    out.h = (double)h;
    return out;
}
// ... of block b of the sorted verr^2 column e2[0 .. n)
inline QuadBlock quad_block_consts(const double* e2, int64_t n, int64_t b) {
    const int64_t last = b == quad_blocks(n) - 1 ? n - 1 : kQuadBlock * b + kQuadBlock - 1;
    return quad_block(e2[kQuadBlock * b], e2[last]);
}
// The blocks' constants in the unused slots of the split array `split` of n records (verr^2 in slot 1): a2 and a1 in slots 6
// and 7 of the block's first record, a0 in slot 6 of its second.  They do not depend on the plan.
inline void quad_fill_records(double* split, int64_t n) {
    constexpr int ND = record_doubles(MODEL_BGFIXED, false), XB = geometry_doubles(MODEL_BGFIXED, false);
    for (int64_t b = 0; b < quad_blocks(n); ++b) {
        const int64_t first = kQuadBlock * b, last = b == quad_blocks(n) - 1 ? n - 1 : first + kQuadBlock - 1;
        const QuadBlock q = quad_block(split[first * ND + 1], split[last * ND + 1]);
        split[first * ND + XB + 2] = q.a2;
        split[first * ND + XB + 3] = q.a1;
        split[(first + 1) * ND + XB + 2] = q.a0;
    }
}
// H of a chunk: the largest h of any block that records begin .. begin + count - 1 touch; +inf where the chunk cannot take
// the quadratic form (no block, an empty chunk, a start that is no multiple of 8, a NaN in a block's ends)
inline double quad_chunk_width(const double* e2, int64_t n, int64_t begin, int64_t count) {
    const double inf = std::numeric_limits<double>::infinity();
    if (quad_blocks(n) <= 0 || count <= 0 || begin % 8 != 0) return inf;
    double H = 0.0;
    for (int64_t b = quad_block_of(begin, n); b <= quad_block_of(begin + count - 1, n); ++b) {
        const double h = quad_block_consts(e2, n, b).h;
        if (!(h >= 0.0)) return inf;
        H = std::max(H, h);
    }
    return H;
}

// the split array of `n` BGFIXED fixed-centre records (8 doubles each): [v, verr^2, cx, cy, M, omp', 0, 0] per star (the
// two spare slots of a block's first two records: quad_fill_records), and the stars' nbf
inline void exp_split_records(const double* rec, int64_t n, double* out, double* nbf) {
    constexpr int ND = record_doubles(MODEL_BGFIXED, false), XB = geometry_doubles(MODEL_BGFIXED, false);
    for (int64_t i = 0; i < n; ++i) {
        const double* r = rec + i * ND;
        double* o = out + i * ND;
        for (int j = 0; j < XB; ++j) o[j] = r[j];
        const ExpSplitRecord s = exp_split_record(r[XB + 3], r[XB + 2]);
        o[XB] = s.M;
        o[XB + 1] = s.ompk;
        o[XB + 2] = o[XB + 3] = 0.0;
        nbf[i] = s.nbf;
    }
    quad_fill_records(out, n);
}

// per chunk of `plan` (Chunk::begin counts from the shard's first record, as `nbf` and the sorted verr^2 column `e2` of the
// shard's n records do): two doubles, {sum of log kappa, H of quad_chunk_width}
inline std::vector<double> exp_split_chunk_consts(const ChunkPlan& plan, const double* nbf, const double* e2, int64_t n) {
    std::vector<double> out(2 * plan.chunks.size());
    for (size_t c = 0; c < plan.chunks.size(); ++c) {
        out[2 * c] = exp_split_chunk_const(nbf + plan.chunks[c].begin, plan.chunks[c].count);
        out[2 * c + 1] = quad_chunk_width(e2, n, plan.chunks[c].begin, plan.chunks[c].count);
    }
    return out;
}

}  // namespace mcd

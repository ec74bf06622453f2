// mcd_exp_split.h -- host side of the split exponent offset of the direct BGFIXED loops (option "exp_split"; the loop and
// its error budget: mcd_math.h: kExpSplitC, BgFixedAcc::add_gs).  Host only: everything here is evaluated in long double
// (x87 80-bit on the hosts this library is built for) and rounded once.  Shared with the CPU tests (tests/emul).
#pragma once

#include <cmath>
#include <cstdint>
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

// the split array of `n` BGFIXED fixed-centre records (8 doubles each): [v, verr^2, cx, cy, M, omp', 0, 0] per star, and the
// stars' nbf
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
}

// per chunk of `plan` (Chunk::begin counts from the shard's first record, as `nbf` does)
inline std::vector<double> exp_split_chunk_consts(const ChunkPlan& plan, const double* nbf) {
    std::vector<double> out(plan.chunks.size());
    for (size_t c = 0; c < plan.chunks.size(); ++c)
        out[c] = exp_split_chunk_const(nbf + plan.chunks[c].begin, plan.chunks[c].count);
    return out;
}

}  // namespace mcd

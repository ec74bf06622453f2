// CPU build of the moment-matching algebra (csrc/mcd_mmatch.h) for tests/test_mmatch_cpu.py: the expressions the device
// kernels and the host loop of mcd_moment_match compile.  Test infrastructure only.
#include <cstdint>
#include <cstring>
#include <vector>

#include "mcd_mmatch.h"

using namespace mcd;

extern "C" {

int emul_mm_moment_doubles(int P) { return mm_moment_doubles(P); }

void emul_mm_moments(int P, int64_t S, const double* rows, const double* w, double* mom) { mm_moments(P, S, rows, w, mom); }

// (At, bt) of `level` from the moments; returns 1 when the trial was made, 0 when it is skipped
int emul_mm_trial(int P, int level, const double* mom, double* At, double* bt) {
    std::vector<double> work((size_t)2 * P * P);
    return mm_trial(P, level, mom, At, bt, work.data()) ? 1 : 0;
}

int emul_mm_cholesky(int P, const double* a, double* l) { return mm_cholesky(P, a, l) ? 1 : 0; }

void emul_mm_compose(int P, const double* At, const double* bt, const double* A, const double* b, double* A2, double* b2) {
    mm_compose(P, At, bt, A, b, A2, b2);
}

void emul_mm_apply(int P, int64_t S, const double* A, const double* b, const double* x, double* y) {
    for (int64_t s = 0; s < S; ++s) mm_apply(P, A, b, x + s * P, y + s * P);
}

int emul_mm_inverse(int P, const double* A, const double* b, double* Ai, double* bi, double* lad) {
    std::vector<double> work((size_t)2 * P * P);
    return mm_inverse(P, A, b, Ai, bi, lad, work.data()) ? 1 : 0;
}

// inside [S] (0 / 1) and the trial's log weights: box and lognormal support, then mm_lw_trial
void emul_mm_rows_inside(int P, int64_t S, const double* lo, const double* hi, const int32_t* kind, int32_t fixed_ok,
                         const double* x, int32_t* inside) {
    PriorTable t;
    t.kind = kind;                                          // (only the kinds are read by the support test)
    for (int64_t s = 0; s < S; ++s) inside[s] = mm_row_inside(P, lo, hi, t, fixed_ok, x + s * P) ? 1 : 0;
}

void emul_mm_lw_trial(int64_t S, const int32_t* inside, const double* train, const double* lnprior, const double* lp0, double* lw) {
    for (int64_t s = 0; s < S; ++s) lw[s] = mm_lw_trial(inside[s] != 0, train[s], lnprior[s], lp0[s]);
}

void emul_mm_lw_split(int64_t S, const double* num, const double* lpf, const int32_t* inv_inside, const double* lp_inv,
                      double lad, double* lw) {
    for (int64_t s = 0; s < S; ++s) lw[s] = mm_lw_split(num[s], lpf[s], inv_inside[s] != 0, lp_inv[s], lad);
}

// The decision loop fed a script of trial results: k_trial [n], usable [n].  Returns the trials consumed; out: k,
// iterations, accepted[3], and levels [n] = the level each consumed trial was made at
int emul_mm_loop(double k0, double thr, int max_iters, int max_level, int n, const double* k_trial, const int32_t* usable,
                 double* k_out, int32_t* iterations, int32_t* accepted, int32_t* levels, int32_t* accepts) {
    MmState s;
    mm_begin(s, k0, thr, max_iters);
    int t = 0;
    while (s.running && t < n) {
        levels[t] = s.level;
        accepts[t] = mm_decide(s, k_trial[t], usable[t] != 0, thr, max_iters, max_level) ? 1 : 0;
        ++t;
    }
    *k_out = s.k;
    *iterations = s.iterations;
    std::memcpy(accepted, s.accepted, sizeof s.accepted);
    return s.running ? -t - 1 : t;
}

int emul_mm_max_level(int cov, int64_t S, int P) { return mm_max_level(cov, S, P); }

// ranges [<= 2 g + 2] and star_range [g]; returns the number of ranges
int64_t emul_mm_ranges(int64_t n_stars, const int64_t* stars, int64_t g, int64_t* ranges, int64_t* star_range) {
    std::vector<int64_t> sr;
    const std::vector<int64_t> r = mm_ranges(n_stars, stars, g, sr);
    std::memcpy(ranges, r.data(), r.size() * 8);
    std::memcpy(star_range, sr.data(), sr.size() * 8);
    return (int64_t)r.size() - 1;
}

const char* emul_mm_stars_error(int64_t n_match, const int64_t* stars, int64_t n_stars) {
    return mm_stars_error(n_match, stars, n_stars);
}

}  // extern "C"

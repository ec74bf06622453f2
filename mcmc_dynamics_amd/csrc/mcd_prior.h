// mcd_prior.h -- host+device: structured priors on the free parameters -- flat, normal, log-normal -- on top of the
// inclusive box of mcd_stretch_desc.  One text for the host-driven blocks (mcd_stretch.h, mcd_hmc.h), the device kernels
// (mcd_stretch.hip, mcd_hmc.hip), mcd_prior_eval and the CPU harness tests/emul/prior_emul.cpp.  No HIP types; compiled
// with -ffp-contract=off everywhere.  The reference has priors as `lnprior` expressions over scipy's norm / lognorm
// (parameter.py:64-74, 684-705), evaluated at the value rounded to six decimals; here the un-truncated log-density is
// evaluated at the full float64 value:
//
//   kind 0 flat        0
//   kind 1 normal      c0 - h,        h = 1/2 t^2,  t = (x - loc) / scale,        c0 = -log(scale) - 1/2 log(2 pi)
//   kind 2 lognormal   (c0 - l) - h,  l = det_log(x),  t = (l - mu) / s,          c0 = -log(s) - 1/2 log(2 pi)
//                      (scipy's lognorm(s, scale=exp(mu))); x <= 0 is OUTSIDE the prior, like a coordinate beyond the box
//
// `c0` is derived ONCE per call on the host with libm (prior_derive: in long double, rounded once -- near scale = 0.4 the
// two terms cancel and a float64 difference would carry the error of log(scale) itself) and handed to the host loop and to
// the device as an array: the device never calls log for it.  What runs per proposal is a fixed sequence of IEEE +, -, *,
// /, fma and det_log (mcd_rng.h: itself a fixed sequence for finite x > 0), so host and device produce the same bits.
// h is evaluated with the rounding errors of the difference, the quotient and the square carried along
// (prior_half_square: TwoSum, the division's exact remainder, the product's exact error): a plain (x - loc) * (1 / scale)
// squared carries SEVEN half-ulps of h where the value's error budget, 2^-52 (|c0| + |l| + h), has room for one (the other
// is the final subtraction's), and at |t| = 40 that is the whole error.  The prior of a row is the sum of its coordinates'
// terms in ascending coordinate order, starting from 0.0; flat coordinates add nothing.
#pragma once

#include <cmath>
#include <cstdint>

#include "mcd_rng.h"   // det_log, MCD_HD

namespace mcd {

enum PriorKind : int32_t { PRIOR_FLAT = 0, PRIOR_NORMAL = 1, PRIOR_LOGNORMAL = 2 };

// The table of one block: [P] arrays in host or device memory, by where the code runs.  kind == nullptr: no structured
// prior (every caller then runs the code it ran before priors existed).
struct PriorTable {
    const int32_t* kind = nullptr;
    const double* loc = nullptr;      // loc (normal) or mu (lognormal)
    const double* scale = nullptr;    // scale (normal) or s (lognormal)
    const double* c0 = nullptr;       // -log(scale or s) - 1/2 log(2 pi)
    MCD_HD bool any() const { return kind != nullptr; }
};

// host: (kind, p0, p1) -> (loc, scale, c0).  false (nothing usable written) for an unknown kind, a non-finite parameter or
// a scale <= 0.  *structured: whether any coordinate is not flat.
inline bool prior_derive(int n_dim, const int32_t* kind, const double* p0, const double* p1, double* loc, double* scale,
                         double* c0, bool* structured) {
    bool any = false;
    for (int c = 0; c < n_dim; ++c) {
        loc[c] = 0.0; scale[c] = 1.0; c0[c] = 0.0;
        if (kind[c] == PRIOR_FLAT) continue;
        if (kind[c] != PRIOR_NORMAL && kind[c] != PRIOR_LOGNORMAL) return false;
        if (!std::isfinite(p0[c]) || !std::isfinite(p1[c]) || !(p1[c] > 0.0)) return false;
        loc[c] = p0[c];
        scale[c] = p1[c];
        c0[c] = (double)(-std::log((long double)p1[c]) - 0.918938533204672741780329736406L);        // 1/2 log(2 pi)
        any = true;
    }
    if (structured) *structured = any;
    return true;
}

MCD_HD bool prior_finite(double x) { return x - x == 0.0; }     // false for NaN and +-inf

// is coordinate x inside the support of its prior (the box is checked by the caller)
MCD_HD bool prior_inside(int32_t kind, double x) { return kind != PRIOR_LOGNORMAL || x > 0.0; }

// h = 1/2 ((a - b) / scale)^2 to one rounding, and t = (a - b) / scale for the derivative:
//   a - b = d + e exactly (TwoSum), d = q scale + r exactly (fma), so t = q + (r + e) / scale =: q + lo with |lo| <= ulp(q),
//   q^2 = p + pe exactly (fma), t^2 = p + (pe + 2 q lo) up to lo^2.
// Where q^2 overflows (or anything is not finite) the corrections are skipped: the result is +inf or NaN as it stands.
MCD_HD double prior_half_square(double a, double b, double scale, double& t) {
    const double d = a - b;
    const double q = d / scale, p = q * q;
    t = q;
    if (!prior_finite(p)) return 0.5 * p;
    const double bb = d - a;
    const double e = (a - (d - bb)) + (-b - bb);
    const double r = fma_(-q, scale, d);
    const double lo = (r + e) / scale;
    const double pe = fma_(q, q, -p);
    t = q + lo;
    return 0.5 * (p + (pe + (2.0 * q) * lo));
}

// one coordinate's term (kind != flat, x inside the support) and its derivative:  normal -t / scale,
// lognormal -(1 + t / s) / x
MCD_HD double prior_term_grad(int32_t kind, double loc, double scale, double c0, double x, double& dx) {
    double t;
    if (kind == PRIOR_NORMAL) {
        const double h = prior_half_square(x, loc, scale, t);
        dx = -(t / scale);
        return c0 - h;
    }
    const double l = det_log(x);
    const double h = prior_half_square(l, loc, scale, t);
    dx = -((1.0 + t / scale) / x);
    return (c0 - l) - h;
}

MCD_HD double prior_term(int32_t kind, double loc, double scale, double c0, double x) {
    double t;
    if (kind == PRIOR_NORMAL) return c0 - prior_half_square(x, loc, scale, t);
    const double l = det_log(x);
    return (c0 - l) - prior_half_square(l, loc, scale, t);
}

// a row of P coordinates: inside the support of every prior?
MCD_HD bool prior_row_inside(const PriorTable& t, int P, const double* x) {
    bool ok = true;
    for (int c = 0; c < P; ++c) ok = ok && prior_inside(t.kind[c], x[c]);
    return ok;
}

// ... its log-prior (the row is inside)
MCD_HD double prior_row(const PriorTable& t, int P, const double* x) {
    double sum = 0.0;
    for (int c = 0; c < P; ++c)
        if (t.kind[c] != PRIOR_FLAT) sum += prior_term(t.kind[c], t.loc[c], t.scale[c], t.c0[c], x[c]);
    return sum;
}

// ... and with the derivatives ADDED to g [P]
MCD_HD double prior_row_grad(const PriorTable& t, int P, const double* x, double* g) {
    double sum = 0.0;
    for (int c = 0; c < P; ++c)
        if (t.kind[c] != PRIOR_FLAT) {
            double dx;
            sum += prior_term_grad(t.kind[c], t.loc[c], t.scale[c], t.c0[c], x[c], dx);
            g[c] += dx;
        }
    return sum;
}

}  // namespace mcd

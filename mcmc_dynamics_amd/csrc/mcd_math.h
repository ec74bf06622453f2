// mcd_math.h -- per-term arithmetic of the log-likelihood kernels.
//
// Written once as host+device inline code so that the exact expression trees the gfx950 kernels
// execute can also be compiled for the CPU by tests/emul (test infrastructure only; the product
// never runs this on the CPU).
//
// Reference formulas (skamann/mcmc-dynamics):
//   v_los  = v_sys + v_max sin(theta - theta_0)                      analysis/constant.py:107-111
//          = v_sys + v_maxx sin(theta) - v_maxy cos(theta)
//   norm   = verr^2 + sigma^2 ; exponent = -1/2 (v - v_los)^2 / norm  analysis/runner.py:261-262
//   no background : lnL = -1/2 sum log(2 pi norm) + sum exponent      analysis/runner.py:269-271
//   background    : per-star log-sum-exp mixture                      analysis/runner.py:280-286
//   GB            : per-walker Gaussian background + density prior    analysis/constant.py:326-364
#pragma once

#include <cmath>
#include <cstdint>
#include <cstring>
#include <type_traits>

#include "mcd_exp_table.h"

#if defined(__HIPCC__)
#define MCD_HD __host__ __device__ __forceinline__
#else
#define MCD_HD inline
#endif
// Star records are read through the CONSTANT address space on the device: a wave-uniform load from it is a scalar load
// (s_load_dwordxN) by construction.  From the global address space the compiler emits scalar loads only while it can
// prove that nothing in the kernel may have written the memory; an inline asm that takes the record pointer (the
// software prefetch below) ends that proof and the record reads silently become per-lane global_load instructions.
#if defined(__HIP_DEVICE_COMPILE__)
#define MCD_CONST_AS __attribute__((address_space(4)))
#else
#define MCD_CONST_AS
#endif
namespace mcd { template <class T> using RecPtr = const T MCD_CONST_AS*; }

// An empty volatile asm keeps the compiler from turning a small wave-uniform `if` into per-lane selects (v_cndmask on
// every iteration): the block stays behind a scalar branch.
#if defined(__HIP_DEVICE_COMPILE__)
#define MCD_KEEP_BRANCH() asm volatile("")
#else
#define MCD_KEEP_BRANCH() ((void)0)
#endif
// bands between a block step of the bounded quadratic loop and the band whose records it prefetches (chunk_bgfixed_fast;
// -D for A/B builds, csrc/Makefile: variant)
#ifndef MCD_BLOCK_STEP_AHEAD
#define MCD_BLOCK_STEP_AHEAD 1
#endif

namespace mcd {

constexpr double kLn2 = 0.693147180559945309417232121458;
constexpr double kLn2Pi = 1.837877066409345483560659472811;   // log(2 pi)
constexpr double kHalfLn2Pi = 0.918938533204672741780329736406;

// Derived per-walker constants (one row of KD doubles per (parameter set, walker)), produced by the
// walker-prep kernel from the resolved parameter table.
enum WalkerSlot : int {
    W_VSYS = 0, W_S2 = 1, W_VX = 2, W_VY = 3,       // v_sys, sigma_max^2, v_maxx, v_maxy
    W_SAC = 4, W_CAC = 5, W_SDC = 6, W_CDC = 7,     // sin/cos(ra_center), sin/cos(dec_center)
    W_VB = 8, W_SB2 = 9, W_FB = 10,                 // v_back, sigma_back^2, f_back
    W_A2 = 11, W_S2A = 12, W_RP2 = 13, W_2RP = 14,  // profile models: a^2, sigma_max^2 a, r_peak^2, 2 r_peak (arcsec)
    W_VXC = 15, W_VYC = 16, W_RC2 = 17, W_2RC = 18, // double models: v_maxx_c, v_maxy_c, rho_2^2, 2 rho_2 (rho_2 = ratio r_peak)
    W_ES2 = 19,                                     // error-scale models: err_scale^2; 0 for every other model
    KD = 20                                         // (a row stays a whole number of 32-byte segments)
};

// Likelihood variants.  Cluster part: CONST (analysis/constant.py) or PROFILE (analysis/model.py:93-180);
// background part: none, fixed per-star lnL + pmember (runner.py:272-286), per-walker Gaussian + density prior
// (constant.py:326-364, model.py:391-456), fixed per-star lnL + density prior with per-walker f_back (model.py:565-623).
enum Model : int {
    MODEL_CONST = 0, MODEL_BGFIXED = 1, MODEL_BGGAUSS = 2,
    MODEL_PROFILE = 3, MODEL_PROFILE_BGGAUSS = 4, MODEL_PROFILE_BGDENS = 5,
    MODEL_PROFILE_BGFIXED = 6,         // ModelFit(background=...): profile cluster part + the pmember mixture of runner.py:272-286
    // DoubleModelFit / DoubleModelFitGB: two Lynden-Bell components on one Plummer dispersion profile (star_d_n), without
    // background / with the per-walker Gaussian background and density prior of MODEL_PROFILE_BGGAUSS.  float64 only, no
    // narrow-range (level 2) variant.
    MODEL_DOUBLE = 7, MODEL_DOUBLE_BGGAUSS = 8,
    // ConstantFitES / ModelFitES: MODEL_CONST / MODEL_PROFILE with a fitted velocity-error scale, one per walker:
    //   variance = err_scale^2 verr^2 + sigma_los^2,  v_los unchanged  (star_d_n).
    // No background, float64 only, no narrow-range (level 2) variant.  Records are the base models'.
    // (id 9 stays unassigned: mcd_catalog_create has always answered it with "unknown model", and callers rely on that)
    MODEL_CONST_ESCALE = 10, MODEL_PROFILE_ESCALE = 11
};
constexpr int kNumModels = 7;           // the models of the reference's running classes: what dispatch_model lists
constexpr int kNumAllModels = 9;        // ... and the double Lynden-Bell models: what dispatch_any_model lists (mcd_dispatch.h)
constexpr int kNumLaunchModels = 12;    // one past the largest id dispatch_launch_model lists (the error-scale models; not 9)
enum Background : int { BG_NONE = 0, BG_FIXED = 1, BG_GAUSS = 2, BG_FIXED_DENSITY = 3 };

MCD_HD constexpr bool is_escale(int model) { return model == MODEL_CONST_ESCALE || model == MODEL_PROFILE_ESCALE; }
// the ids a catalogue can have: what dispatch_launch_model reaches
MCD_HD constexpr bool is_launch_model(int model) { return (model >= 0 && model < kNumAllModels) || is_escale(model); }
// the model an error-scale model is at err_scale = 1 (records, chunk functions, launch costs); every other model itself
MCD_HD constexpr int base_model(int model) {
    return model == MODEL_CONST_ESCALE ? (int)MODEL_CONST : model == MODEL_PROFILE_ESCALE ? (int)MODEL_PROFILE : model;
}
MCD_HD constexpr bool is_profile(int model) { return (model >= MODEL_PROFILE && model < kNumAllModels) || model == MODEL_PROFILE_ESCALE; }
MCD_HD constexpr bool is_double(int model) { return model == MODEL_DOUBLE || model == MODEL_DOUBLE_BGGAUSS; }
// kernel columns of the cluster part in front of the centre columns (mcd_prep.h has the order); err_scale is the last of them
MCD_HD constexpr int cluster_columns(int model) {
    return (is_double(model) ? 9 : is_profile(model) ? 6 : 4) + (is_escale(model) ? 1 : 0);
}
MCD_HD constexpr int bg_kind(int model) {
    return (model == MODEL_CONST || model == MODEL_PROFILE || model == MODEL_DOUBLE || is_escale(model)) ? BG_NONE
           : (model == MODEL_BGFIXED || model == MODEL_PROFILE_BGFIXED) ? BG_FIXED
           : (model == MODEL_PROFILE_BGDENS) ? BG_FIXED_DENSITY : BG_GAUSS;
}

// Star record slots (doubles).
//   CONST,   fixed centre: v, e2, sin(theta), cos(theta)                     (4)
//   PROFILE, fixed centre: v, e2, dx, dy [arcsec], r^2 [arcsec^2], pad       (6)
//   free centre (both)   : v, e2, sin(ra), cos(ra), sin(dec), cos(dec)       (6)
// extras: BG_FIXED -> lnL_bg, pmember, 1 - pmember, -(lnL_bg + 1/2 log 2pi)   (4)
//         BG_GAUSS -> density, pad                                            (2)
//         BG_FIXED_DENSITY -> lnL_bg, -(lnL_bg + 1/2 log 2pi), density, pad   (4)
MCD_HD constexpr int geometry_doubles(int model, bool free_centre) {
    return (free_centre || is_profile(model)) ? 6 : 4;
}
MCD_HD constexpr int record_doubles(int model, bool free_centre) {
    return geometry_doubles(model, free_centre) +
           (bg_kind(model) == BG_NONE ? 0 : (bg_kind(model) == BG_GAUSS ? 2 : 4));
}

constexpr double kArcsecPerRad = 206264.80624709635516;   // 10800 / pi arcmin x 60: r0 of calc_xy_offset.py:11 in arcsec

// ---------------------------------------------------------------------------------------------
// Host/device shims, once each: the builtin (or HIP's overload) in the device pass, libm in the host pass (tests/emul).
#if defined(__HIP_DEVICE_COMPILE__)
#define MCD_ON_DEVICE(device_expr, host_expr) (device_expr)
#else
#define MCD_ON_DEVICE(device_expr, host_expr) (host_expr)
#endif
template <class T> MCD_HD T fma_(T a, T b, T c) { return MCD_ON_DEVICE(__builtin_fma(a, b, c), std::fma(a, b, c)); }
MCD_HD float fma_(float a, float b, float c) { return MCD_ON_DEVICE(__builtin_fmaf(a, b, c), std::fmaf(a, b, c)); }
template <class T> MCD_HD T sqrt_(T x) { return MCD_ON_DEVICE(sqrt(x), std::sqrt(x)); }
template <class T> MCD_HD T log_(T x) { return MCD_ON_DEVICE(log(x), std::log(x)); }
template <class T> MCD_HD T exp_(T x) { return MCD_ON_DEVICE(exp(x), std::exp(x)); }
MCD_HD double frexp_(double x, int* e) { return MCD_ON_DEVICE(__builtin_frexp(x, e), std::frexp(x, e)); }
MCD_HD float frexp_(float x, int* e) { return MCD_ON_DEVICE(__builtin_frexpf(x, e), std::frexp(x, e)); }
MCD_HD double ldexp_(double x, int k) { return MCD_ON_DEVICE(__builtin_ldexp(x, k), std::ldexp(x, k)); }
MCD_HD double fmin_(double a, double b) { return MCD_ON_DEVICE(__builtin_fmin(a, b), std::fmin(a, b)); }     // v_min_f64
MCD_HD double fmax_(double a, double b) { return MCD_ON_DEVICE(__builtin_fmax(a, b), std::fmax(a, b)); }     // v_max_f64
MCD_HD double fabs_(double a) { return MCD_ON_DEVICE(__builtin_fabs(a), std::fabs(a)); }         // source modifier, no instruction
template <class T> MCD_HD T max_(T a, T b) { return a > b ? a : b; }
// the hardware estimates; measured max rel. error on gfx950 (tools/rsq_probe.hip): v_rsq_f64 2^-24.2, v_rcp_f64 2^-24.4
MCD_HD double rsq_(double x) { return MCD_ON_DEVICE(__builtin_amdgcn_rsq(x), 1.0 / std::sqrt(x)); }
MCD_HD double rcp_(double x) { return MCD_ON_DEVICE(__builtin_amdgcn_rcp(x), 1.0 / x); }
MCD_HD float rsqf_(float x) { return MCD_ON_DEVICE(__builtin_amdgcn_rsqf(x), 1.0f / std::sqrt(x)); }
// v_exp_f32; arguments below -126 / ln 2 flush to 0
MCD_HD float expf_(float x) { return MCD_ON_DEVICE(__builtin_amdgcn_exp2f(x * 1.44269504088896340736f), std::exp(x)); }
#undef MCD_ON_DEVICE          // textual selection: the other arm is never parsed -- for the one-line shims above only

// n^(-1/2): v_rsq_f64 and one third-order step: with e = 1 - n y^2 (|e| <= 2^-23.2),  n^-1/2 = y (1 + e/2 + 3 e^2/8 + O(e^3)),
// remaining error 5/16 e^3 < 2^-71: full f64 after the final rounding.  5 instructions.
MCD_HD double rsqrt_nr(double n) {
    const double y = rsq_(n);
    const double e = fma_(-(n * y), y, 1.0);
    const double t = fma_(0.375, e, 0.5);
    return fma_(y, t * e, y);
}

// 1/x = y (1 + e + e^2 + O(e^3)),  y from v_rcp_f64,  e = 1 - x y
MCD_HD double rcp_nr(double x) {
    const double y = rcp_(x);
    const double e = fma_(-x, y, 1.0);
    return fma_(y, fma_(e, e, e), y);
}

// Free centre: tangent-plane offsets of calc_xy_offset.py:30-31 (in units of r0) from per-star products prepared at
// upload, A = cos(dec) sin(ra), B = cos(dec) cos(ra), sd = sin(dec), and the walker's sin/cos of the centre:
//   x = -cos(dec) sin(ra - ra_c)                         = B sin(ra_c) - A cos(ra_c)
//   y = sin(dec) cos(dec_c) - cos(dec) sin(dec_c) cos(ra - ra_c) = sd cos(dec_c) - sin(dec_c) (B cos(ra_c) + A sin(ra_c))
// Six operations, no per-term trigonometry.
template <class T>
MCD_HD void free_centre_xy(T A, T B, T sd, T sac, T cac, T sdc, T cdc, T& x, T& y) {
    x = fma_(B, sac, -(A * cac));
    const T t = fma_(B, cac, A * sac);
    y = fma_(sd, cdc, -(sdc * t));
}

// v - v_los for the constant-rotation models with a free centre (constant.py:106-111):
//   v_los = v_sys + v_maxx sin(theta) - v_maxy cos(theta),  sin(theta) = y / r, cos(theta) = x / r
//         = v_sys + (v_maxx y - v_maxy x) / r,
// one reciprocal square root and no separate sin/cos.  r == 0 follows numpy's arctan2(+0, -+0) = pi / 0: sin = 0, cos = -+1.
template <bool FASTMATH, class T>
MCD_HD T free_centre_residual(T A, T B, T sd, T sac, T cac, T sdc, T cdc, T vx, T vy, T v_minus_vsys) {
    T x, y;
    free_centre_xy(A, B, sd, sac, cac, sdc, cdc, x, y);
    const T r2 = fma_(x, x, y * y);
    T inv;
    if constexpr (FASTMATH && sizeof(T) == 8) {
        inv = (T)rsqrt_nr((double)r2);            // offsets are O(1e-9 .. 1) rad: r2 is a normal number (or exactly 0)
    } else {
        inv = T(1) / sqrt_(r2);
    }
    const T cross = fma_(vx, y, -(vy * x));
    const T general = fma_(-cross, inv, v_minus_vsys);
    const T on_centre = fma_(vy, std::signbit(x) ? T(-1) : T(1), v_minus_vsys);
    return r2 > T(0) ? general : on_centre;
}

// a * b + c with the addend c known to be wave-uniform (a star-record value held in an SGPR pair).  hipcc would
// otherwise copy c into VGPRs to use the two-address v_fmac_f64 (2 extra v_mov_b32 per use); the three-address
// VOP3 form takes the SGPR pair directly.
MCD_HD double fma_sgpr_addend(double a, double b, double c) {
#if defined(__HIP_DEVICE_COMPILE__)
    double r;
    asm("v_fma_f64 %0, %1, %2, %3" : "=v"(r) : "v"(a), "v"(b), "s"(c));
    return r;
#else
    return std::fma(a, b, c);
#endif
}

// -(a * b) + c, same SGPR-addend form (the negation is a source modifier)
MCD_HD double fnma_sgpr_addend(double a, double b, double c) {
#if defined(__HIP_DEVICE_COMPILE__)
    double r;
    asm("v_fma_f64 %0, -%1, %2, %3" : "=v"(r) : "v"(a), "v"(b), "s"(c));
    return r;
#else
    return std::fma(-a, b, c);
#endif
}

// max(x, lo) for an x that is already an arithmetic result (never a signalling NaN): the plain v_max_f64.  The
// builtin fmax after an inline-asm producer makes hipcc insert a canonicalising v_max_f64 x, x, x first.
MCD_HD double fmax_raw(double x, double lo) {
#if defined(__HIP_DEVICE_COMPILE__)
    double r;
    asm("v_max_f64 %0, %1, %2" : "=v"(r) : "v"(x), "s"(lo));
    return r;
#else
    return std::fmax(x, lo);
#endif
}

// log(m) for the mantissa of a rescaled product, m in [1/2, 1): m' = m or 2m in [sqrt(1/2), sqrt(2)), f = (m' - 1) / (m' + 1),
// log m' = 2 f (1 + s/3 + ... + s^10/21), s = f^2 <= 0.0295 (remainder < 1e-18) -- one division and eleven fused
// multiply-adds instead of libm's double-double logarithm (~100 vector instructions, once per wave and product: 7 % of a
// wave's work at 100 stars per chunk).  The absolute error, ~1e-16, sits far below one ulp of what it is added to
// (exponent x ln 2).  Anything else (0 from an underflowed product, inf, NaN) takes libm's log and its special cases.
MCD_HD double log_unit(double m) {
    if (!(m >= 0.5 && m < 1.0)) return log_(m);
    const bool low = m < 0.70710678118654752440;
    const double mm = low ? m + m : m;
    const double f = (mm - 1.0) / (mm + 1.0), s = f * f;
    double t = 1.0 / 21.0;
    t = fma_(t, s, 1.0 / 19.0);
    t = fma_(t, s, 1.0 / 17.0);
    t = fma_(t, s, 1.0 / 15.0);
    t = fma_(t, s, 1.0 / 13.0);
    t = fma_(t, s, 1.0 / 11.0);
    t = fma_(t, s, 1.0 / 9.0);
    t = fma_(t, s, 1.0 / 7.0);
    t = fma_(t, s, 1.0 / 5.0);
    t = fma_(t, s, 1.0 / 3.0);
    t = fma_(t, s, 1.0);
    return fma_(low ? -1.0 : 0.0, 0.693147180559945309417232121458, (f + f) * t);
}

// ---------------------------------------------------------------------------------------------
// sum of logs as the log of a running product with explicit exponent tracking:
//   sum_i log(x_i) = log(prod_i m_i) + ln2 * sum_i e_i .
// One multiply per factor instead of one log per factor; the product's relative error grows by
// 2^-53 per multiply, i.e. the absolute error of the log sum is <= 1.1e-16 per term -- tighter than
// summing individually rounded logs.
struct LogProduct {
    double p;
    int64_t e;     // exponent carried over from finished groups
    int e32;       // exponent of the current group (folded into e by rescale(); |e32| stays far below 2^31)
    MCD_HD void init() { p = 1.0; e = 0; e32 = 0; }
    MCD_HD void mul(double x) { p *= x; }            // caller keeps |log2 p| < ~1000 between rescales
    MCD_HD void rescale() {
        int ex;
        p = frexp_(p, &ex);
        e += (int64_t)(e32 + ex);
        e32 = 0;
    }
    // narrow-range products: the group exponent stays in the 32-bit counter (|ex| <= 1000 per group of up to 8 factors,
    // chunks hold <= 2^20 stars: mcd_chunks.h kMaxChunkLen), folded into e by value()
    MCD_HD void rescale_narrow() {
        int ex;
        p = frexp_(p, &ex);
        e32 += ex;
    }
    MCD_HD void mul_any(double x) {                  // any positive finite x: split first
        int ex;
        p *= frexp_(x, &ex);
        e32 += ex;
    }
    // as mul_any for x >= 0, additionally keeping the smallest BIASED exponent field seen (one v_min_i32): a field
    // below kTrackFloor (x < 2^-1000, which includes denormals and an exact 0) marks the regime where the reference's
    // log-sum-exp works on denormal numbers (see BgFixedAcc::denormal).  The exponent comes from the bit field (one
    // shift) instead of v_frexp_exp; for a denormal or zero x it is off, but those batches are re-evaluated anyway.
    static constexpr int kTrackInit = 2047, kTrackFloor = 23;      // 23 - 1023 = -1000
    MCD_HD void mul_any_track(double x, int& emin) {
        uint64_t bits;
        std::memcpy(&bits, &x, sizeof bits);
        const int bx = (int)(bits >> 52);                            // sign bit is 0
#if defined(__HIP_DEVICE_COMPILE__)
        double m = __builtin_amdgcn_frexp_mant(x);
#else
        int unused;
        double m = std::frexp(x, &unused);
#endif
        p *= m;
        e32 += bx - 1022;
        emin = bx < emin ? bx : emin;
    }
    MCD_HD double value() {
        rescale();
        return fma_((double)e, kLn2, log_unit(p));
    }
};

// ---------------------------------------------------------------------------------------------
// MODEL_CONST, fast path: G stars of one walker reduced to ONE division and ONE product factor.
//   sum_j q_j / n_j = NUM / DEN,  DEN = prod_j n_j,  built as a balanced tree of (num, den) pairs:
//   (a, m) (+) (b, n) = (a n + b m, m n).
// Valid while DEN and NUM stay in range: host guards 2^-60 <= n <= 2^60 and q < 2^120 for G = 8.
template <class T> struct Frac { T num, den; };
template <class T> MCD_HD Frac<T> frac_leaf2(T q0, T n0, T q1, T n1) {
    Frac<T> f;
    f.den = n0 * n1;
    f.num = fma_(q1, n0, q0 * n1);
    return f;
}
template <class T> MCD_HD Frac<T> frac_join(Frac<T> a, Frac<T> b) {
    Frac<T> f;
    f.den = a.den * b.den;
    f.num = fma_(b.num, a.den, a.num * b.den);
    return f;
}
template <class T> MCD_HD Frac<T> frac_tree4(const T* qq, const T* nn) {
    return frac_join(frac_leaf2(qq[0], nn[0], qq[1], nn[1]), frac_leaf2(qq[2], nn[2], qq[3], nn[3]));
}
template <class T> MCD_HD Frac<T> frac_tree8(const T* qq, const T* nn) {
    return frac_join(frac_tree4(qq, nn), frac_tree4(qq + 4, nn + 4));
}

struct ConstAcc {          // accumulators of one walker over one chunk (MODEL_CONST)
    double q;              // sum (v - v_los)^2 / norm
    LogProduct l;          // sum log(norm)
    MCD_HD void init() { q = 0.0; l.init(); }
    MCD_HD void add8(const double* qq, const double* nn) {
        const Frac<double> f = frac_tree8(qq, nn);
        // DEN is a normal number far from the range limits (host guard), so the IEEE division's scaling and
        // fix-up instructions are not needed: reciprocal (v_rcp_f64 + one residual step, < 1 ulp) times NUM.
        q += f.num * rcp_nr(f.den);
        l.mul(f.den);
        l.rescale();
    }
    // 16 stars: one more level of the tree, still ONE reciprocal (DEN = prod of 16 norms needs |log2 norm| <= 50)
    MCD_HD void add16(const double* qq, const double* nn) {
        const Frac<double> f = frac_join(frac_tree8(qq, nn), frac_tree8(qq + 8, nn + 8));
        q += f.num * rcp_nr(f.den);
        l.mul(f.den);
        l.rescale();
    }
    MCD_HD void add1(double q1, double n1) {
        q += q1 / n1;
        l.mul_any(n1);
    }
    // lnL contribution of `count` stars: -1/2 (count log 2pi + sum log n + sum q/n)
    MCD_HD double finish(int64_t count) { return -0.5 * (fma_((double)count, kLn2Pi, l.value()) + q); }
};

// MODEL_PROFILE, narrow-range variant (guard level 2, mcd_guard.h: level_verdict): the Lynden-Bell residual
//   d = dv - K c / m,   dv = v - v_sys,  c = v_maxx dy - v_maxy dx,  K = 2 r_peak,  m = r_peak^2 + r^2        (model.py:124-127)
// needs the reciprocal of m in the general fast form (v_rcp_f64 + a residual step: ~5 issue slots per term).  Here the
// division is left to the fraction tree:  d^2 / n = (dv m - K c)^2 / (m^2 n), i.e. the tree runs on
// (q', n') = ((dv m - K c)^2, m^2 n) -- two more multiplications instead of the reciprocal -- and since the tree's
// denominator is now prod m_i^2 n_i, the log term needs  sum log n_i = log prod n'_i - 2 log prod m_i: a second running
// product (one multiplication per term, one rescale and one log per 8 terms / per chunk).  Ranges (level_verdict): m <=
// 2^34 arcsec^2, 2^-30 <= n <= 2^30, |dv| <= 2^30: the 8-star denominator stays within 2^+-784, the numerator below 2^820.
struct ProfileNarrowAcc {
    double q;
    LogProduct l;          // prod m_i^2 n_i
    LogProduct lm;         // prod m_i
    MCD_HD void init() { q = 0.0; l.init(); lm.init(); }
    MCD_HD void add8(const double* qq, const double* nn, double m_prod) {
        const Frac<double> f = frac_tree8(qq, nn);
        q += f.num * rcp_nr(f.den);
        l.mul(f.den);
        l.rescale();
        lm.mul(m_prod);
        lm.rescale();
    }
    MCD_HD void add1(double q1, double n1, double m1) {
        q += q1 / n1;
        l.mul_any(n1);
        lm.mul_any(m1);
    }
    MCD_HD double finish(int64_t count) {
        const double sum_log_n = l.value() - 2.0 * lm.value();
        return -0.5 * (fma_((double)count, kLn2Pi, sum_log_n) + q);
    }
};

// float32 counterpart (MCD_F32 / MCD_F32_ACC64): groups of 4 stars so that DEN <= 2^60 and NUM <= 2^77 stay inside the
// f32 range under the host guard 2^-15 <= n <= 2^15, q <= 2^30.  The quotient sum accumulates in A (float or double).
template <class A>
struct ConstAccF {
    A q;
    float p;
    int e;
    MCD_HD void init() { q = 0; p = 1.0f; e = 0; }
    MCD_HD void fold(float x) {
        int ex;
        p = frexp_(p * x, &ex);
        e += ex;
    }
    MCD_HD void add4(const float* qq, const float* nn) {
        const Frac<float> f = frac_tree4(qq, nn);
#if defined(__HIP_DEVICE_COMPILE__)
        q += (A)(f.num * __builtin_amdgcn_rcpf(f.den));     // v_rcp_f32: 1 ulp
#else
        q += (A)(f.num / f.den);
#endif
        fold(f.den);
    }
    MCD_HD void add1(float q1, float n1) {
        q += (A)(q1 / n1);
        fold(n1);
    }
    MCD_HD double finish(int64_t count) {
        const double lg = fma_((double)e, kLn2, log_((double)p));
        return -0.5 * (fma_((double)count, kLn2Pi, lg) + (double)q);
    }
};

// ---------------------------------------------------------------------------------------------
// Plain per-term forms (robust path and mixtures): one log / exp per term as written in the reference.
// lnL_member of runner.py:280 / lnlike_cluster of constant.py:362
template <class T>
MCD_HD T gauss_lnl(T d, T n) {
    return T(-0.5) * (log_(n) + T(kLn2Pi) + d * d / n);
}

// per-star mixture of runner.py:282-284 / constant.py:320-323
template <class T>
MCD_HD T mixture_lnl(T m, T b, T p) {
    T mx = max_(m, b);
    return mx + log_(p * exp_(m - mx) + (T(1) - p) * exp_(b - mx));
}

// ---------------------------------------------------------------------------------------------
// Fast mixture paths (f64): no log, no divide per term.
//   exp(-1/2 d^2/n) / sqrt(n)  is formed from g = n^(-1/2)  (v_rsq_f64 + one third-order Newton step)
//   and one exp whose argument is <= 0 or exponent-clamped; the per-star mixture value y_i > 0 is
//   folded into a LogProduct:  sum_i log y_i = log prod_i y_i.

// 2 m^(-1/2) from v_rsq_f64 and ONE Newton step in its three-instruction form,  y (3 - m y^2) = 2 y (1 + e/2),
// e = 1 - m y^2 (|e| <= 2^-23.2):  m^-1/2 = y (1 + e/2 + 3 e^2/8 + ...), so the result is low by 3/8 e^2 <= 4.1e-15
// relative (1.4e-15 on average) plus three roundings.  Used by the narrow-range mixture variants only, where a term's
// log-likelihood responds to that factor with a sensitivity <= |1 - d^2/n|: over N stars the sum moves by <= 4e-15 N,
// i.e. 1e-15 of |lnL| -- inside the rounding error of the reference's own float64 summation.  The factor 2 is free:
// callers scale the variance they pass (m = 8 n gives (2 n)^-1/2).  Two instructions fewer than rsqrt_nr.
MCD_HD double rsqrt2_newton(double m) {
    const double y = rsq_(m);
    const double s = fma_(-m, y * y, 3.0);
    return y * s;
}

// e^u = 2^e T[j] e^r with k = rint(u N / ln 2) = N e + j, |r| <= ln 2 / 2N, T[j] = 2^(j/N) (mcd_exp_table.h,
// correctly rounded).  N = 1024 (default build): degree-3 polynomial 1 + r + c2 r^2 + c3 r^3 with the even part of its
// error levelled by c2 (tools/gen_exp_table.py), max error 9.4e-17, i.e. below half an ulp -- one FMA per term fewer than
// N = 256 with the degree-4 Taylor polynomial (remainder 3.8e-17; -DMCD_EXP_TAB_BITS=8), for one more integer
// instruction (the 8-bit index is a byte select, the 10-bit one an and + shift).
// Returns the mantissa part T[j] e^r in [1, 2) and e.  `tab` points to the table: LDS on the device (each workgroup
// copies it there; the per-lane lookup is a ds_read_b64, off the VALU), a static array on the host.
// k comes out of the low word of u * (N / ln 2) + 1.5 * 2^52 (round-to-nearest-even), so no v_rndne / v_cvt.
// Requires |u| < 1.4e6 (k inside int32; callers clamp or are bounded by the host guard, mcd_guard.h).
// x with the integer v added to the high word of its bit pattern (v << 20 scales a normal x by 2^v; one v_add_u32)
MCD_HD double add_hi_word(double x, int32_t v) {
    uint32_t w[2];                                    // little-endian: w[1] is the high word (sign, exponent, top of mantissa)
    std::memcpy(w, &x, sizeof w);
    w[1] += (uint32_t)v;                              // a 32-bit add: a 64-bit one would be a v_lshl_add_u64
    std::memcpy(&x, w, sizeof x);
    return x;
}

// Exponent-biased table (the narrow-range BGFIXED kernels, mcd_kernels.hip): entry j holds T[j] with j << (20 - B)
// subtracted from the high word of its bit pattern (B = kExpTabBits; j << (20 - B) < 2^20, so the entry stays a
// positive normal number).  Since k = 2^B e + j, adding k << (20 - B) to the entry's high word gives back T[j] with e
// added to its exponent field: the table address (k & (N - 1)) * 8 and that ONE v_lshl_add_u32 replace k >> B and
// v_ldexp_f64 (exp_tab_scaled).  The general form reads the same table and restores T[j] exactly (exp_tab<.., true>).
constexpr int kExpTabHiShift = 20 - kExpTabBits;
MCD_HD double exp_tab_bias(double t, int j) { return add_hi_word(t, -(j << kExpTabHiShift)); }

// k of exp_tab and its reduced argument: k comes out of the low word of u * (N / ln 2) + 1.5 * 2^52 (round-to-nearest-even)
// TWO_STEP = false, the one-constant reduction: ln 2 / N rounded to f64 is off by < 2^-53 of itself, so r is off by
// < 1.1e-16 |k| ln 2 / N, i.e. a relative error of 8e-17 |u| in e^u -- for callers whose |u| is small wherever e^u matters
template <bool TWO_STEP>
MCD_HD double exp_tab_reduce(double u, int& k) {
    constexpr double kMagic = 6755399441055744.0;            // 1.5 * 2^52
    const double shifted = fma_(u, kExpTabInvStep, kMagic);
    const double kf = shifted - kMagic;
    uint64_t bits;
    std::memcpy(&bits, &shifted, sizeof bits);
    k = (int)(uint32_t)bits;
    if constexpr (TWO_STEP) {
        const double r = fma_(-kf, kExpTabStepHi, u);
        return fma_(-kf, kExpTabStepLo, r);
    } else {
        return fma_(-kf, kExpTabStepHi + kExpTabStepLo, u);
    }
}
// e^r on the reduced argument, |r| <= ln 2 / 2N (degree and coefficients: mcd_exp_table.h)
MCD_HD double exp_poly(double r) {
    double p;
    if constexpr (kExpPolyDegree == 4) p = fma_(fma_(r, kExpPolyC4, kExpPolyC3), r, kExpPolyC2);
    else p = fma_(r, kExpPolyC3, kExpPolyC2);
    p = fma_(p, r, 1.0);
    return fma_(p, r, 1.0);
}

template <bool TWO_STEP = true, bool BIASED = false>
MCD_HD double exp_tab(double u, int& e_out, const double* __restrict__ tab) {
    int k;
    const double p = exp_poly(exp_tab_reduce<TWO_STEP>(u, k));
    e_out = k >> kExpTabBits;
    const int j = k & (kExpTabSize - 1);
    // the exponent-biased table: T[j] restored exactly (one integer instruction)
    if constexpr (BIASED) return add_hi_word(tab[j], j << kExpTabHiShift) * p;
    else return tab[j] * p;
}

// e^u = (T[j] 2^e) e^r from the exponent-biased table, with no v_ldexp_f64 and no k >> B: the integer part e is added
// straight into the high word of the table entry (see exp_tab_bias).  k is first raised to kExpTabKMin = -1021 N, so that
// T[j] 2^e e^r stays a normal number (T[j] e^r >= 1 - 2^-11); wherever k >= kExpTabKMin the result is then bit-identical
// to ldexp(exp_tab(u), e) (scaling by a power of two commutes with the rounding of the product while nothing is
// subnormal).  Where the clamp acts the result is some value < 2^-1019 instead of e^u < 2^-1019:
// callers add it, scaled by at most 2^31, to a number >= 2^-53 (BgFixedAcc::add<.., NARROW>), which absorbs both exactly.
// Requires -1.4e6 < u < 700 (k inside int32 and k << (20 - B) without overflow).
// CLAMP = false (the bounded narrow-range loop, mcd_guard.h: bounded_rescale): the host guarantees u >= -700, so that
// k >= -1034127 > kExpTabKMin and the v_max_i32 is a no-op -- dropped, same bits.
constexpr int kExpTabKMin = -1021 * kExpTabSize;
// x, opaque to the optimiser (no instruction): a constant passed through it is held in a VGPR across the loop instead
// of being re-materialised in the loop body (a v_mov_b64 per iteration in the bounded loop)
MCD_HD double vgpr_constant(double x) {
#if defined(__HIP_DEVICE_COMPILE__)
    asm("" : "+v"(x));
#endif
    return x;
}
// x, opaque to the optimiser AND tied to its place in the program (a volatile asm, no instruction): what is computed
// from it is neither shared with an equal computation elsewhere nor moved out of the branch it stands in
MCD_HD double vgpr_pinned(double x) {
#if defined(__HIP_DEVICE_COMPILE__)
    asm volatile("" : "+v"(x));
#endif
    return x;
}
template <bool TWO_STEP = false, bool CLAMP = true>
MCD_HD double exp_tab_scaled(double u, const double* __restrict__ tab) {
    int k;
    const double p = exp_poly(exp_tab_reduce<TWO_STEP>(u, k));
    if constexpr (CLAMP) k = k > kExpTabKMin ? k : kExpTabKMin;      // v_max_i32
    const double t = tab[k & (kExpTabSize - 1)];
    const int32_t kh = (int32_t)((uint32_t)k << kExpTabHiShift);
#if defined(__HIP_DEVICE_COMPILE__)
    if constexpr (!CLAMP) {
        // the same add on a two-word vector: through add_hi_word's byte copies the compiler splits it into five
        // byte-mask operations once no v_max_i32 stands between k and the add
        typedef uint32_t word2 __attribute__((ext_vector_type(2)));
        word2 w = __builtin_bit_cast(word2, t);
        w.y += (uint32_t)kh;
        return __builtin_bit_cast(double, w) * p;
    }
#endif
    return add_hi_word(t, kh) * p;
}

// Rotate-free reciprocal root of the level-2 BGFIXED fixed-centre loops on a verr-sorted record array.
//   g_i = (2 (e_i + s2))^(-1/2),  e_i = verr_i^2 (record, wave-uniform),  s2 = sigma^2 (per lane, constant over a chunk).
// On a chunk whose e_i all lie within a narrow band around a centre eb (sorted array: the midpoint of its first and last
// record), with m0 = 8 (eb + s2), delta = e_i - eb, t = 8 delta / m0 and G0 = 2 m0^(-1/2):
//   g = G0 (1 - t/2 + 3 t^2/8 - 5 t^3/16) + R,  |R| <= 35/128 t^4 G0  (<= 6.1e-17 relative for |t| <= 2^-13),
// i.e. a cubic in delta with four per-lane coefficients set up once per chunk: one subtraction and three fused
// multiply-adds per term instead of the variance, v_rsq_f64 and the Newton step (8 issue slots).  Error: the rounding of
// b0 and of the last FMA (2^-53 each) plus the truncation, < 2.9e-16 relative -- the one-step Newton form it replaces is low by up to
// 4.1e-15.  The rounding error of m0 itself (an exact two-sum) is folded into b0.
// What both forms of the series (RootSeries, RootDirect) start from at a chunk's centre eb for a lane's s2 -- one place, so
// that the two stay in step
struct RootCentre {
    double p, m0, inv, G0, q, corr;
    MCD_HD void setup(double eb, double s2) {
        p = 8.0 * eb;
        const double s2x = 8.0 * s2;                               // exact, both
        m0 = p + s2x;
        const double bb = m0 - p;
        const double err = (p - (m0 - bb)) + (s2x - bb);          // m0 + err = p + s2x exactly
        inv = rcp_nr(m0);
        // 2 (m0 + err)^(-1/2) = G0 (1 + corr) to second order: y is within an ulp of m0^(-1/2), its residual 1 - m0 y^2
        // comes out exactly (h + eh = m0 y without rounding); callers let both first-order corrections enter through ONE
        // last FMA, fma(G0, corr [+ ...], G0), which then carries one rounding
        const double y = rsqrt_nr(m0);
        const double h = m0 * y;
        const double eh = fma_(m0, y, -h);
        const double res = fma_(-h, y, 1.0) - eh * y;
        G0 = 2.0 * y;
        q = 8.0 * inv;                                             // t = q delta
        corr = 0.5 * (res - err * inv);
    }
};

struct RootSeries {
    static constexpr double kMaxT = 0x1p-13;
    double eb, b0, b1, b2, b3;
    // coefficients about the centre eb for this lane's s2; false when s2 puts a band of half-width `half` outside |t| <= 2^-13
    MCD_HD bool setup(double eb_, double half, double s2) {
        eb = eb_;
        RootCentre c;
        c.setup(eb, s2);
        const double m0 = c.m0, G0 = c.G0, q = c.q;
        b0 = fma_(G0, c.corr, G0);                                 // ONE rounding (RootCentre)
        b1 = -0.5 * (G0 * q);
        b2 = -0.75 * (b1 * q);
        b3 = (-5.0 / 6.0) * (b2 * q);
        return half >= 0.0 && 8.0 * half <= kMaxT * m0;            // (false for NaN)
    }
    // the chunk's records run from e_first to e_last (ascending)
    MCD_HD bool setup_chunk(double e_first, double e_last, double s2) {
        return setup(0.5 * e_first + 0.5 * e_last, 0.5 * (e_last - e_first), s2);
    }
    MCD_HD double g(double e) const {
        const double delta = e - eb;
        return fma_(fma_(fma_(b3, delta, b2), delta, b1), delta, b0);
    }
};

// a * s + c with the factor s known to be wave-uniform (a star-record value held in an SGPR pair): the three-address
// form with the SGPR pair as its one scalar operand, whatever the register allocator would have preferred
MCD_HD double fma_sgpr_factor(double a, double s, double c) {
#if defined(__HIP_DEVICE_COMPILE__)
    double r;
    asm("v_fma_f64 %0, %1, %2, %3" : "=v"(r) : "v"(a), "s"(s), "v"(c));
    return r;
#else
    return std::fma(a, s, c);
#endif
}

// The same cubic as RootSeries::g written in e itself: g = c0 + e (c1 + e (c2 + e c3)).  delta = e - eb is
// wave-uniform (record value and chunk centre), yet gfx950 has no scalar f64 add, so RootSeries::g pays the subtraction
// on the vector pipe once per term; here the coefficients are re-centred to 0 once per chunk and the three FMAs take the
// record value as their SGPR operand: one f64 instruction per term fewer.  With G = 2 (8 (eb + s2))^(-1/2), q = 1 / (eb + s2)
// and rho = q eb (the weight of the centre in the variance) the Taylor cubic about eb, expanded about 0, is
//   c0 =  G     (1   + rho/2   + 3 rho^2/8 + 5 rho^3/16)        c2 =  G q^2 (3/8 + 15 rho/16)
//   c1 = -G q   (1/2 + 3 rho/4 + 15 rho^2/16)                   c3 = -G q^3  5/16
// The price is conditioning: the terms no longer shrink with |t| <= 2^-13 but with x = q e <= rho + 2^-13, and c0's
// rounding is not damped, so the form is admitted for rho <= kRhoMax = 1/8 only (direct_ok; a wave-wide vote like the
// series').  Worst-case relative error against (2 (e + s2))^(-1/2) for |t| <= 2^-13 and rho <= 1/8, in units of
// u = 2^-53 = 1.11e-16 and relative to G (g / G lies within 1 +- 2^-14):
//   last FMA                                                                                   1.00
//   c0: ONE rounding of the value, |c0| <= 1.0690 G.  It is built as b0 is, G0 + G0 A in one FMA, where
//       A = (res - err inv) / 2 + P takes up G0's own error exactly (RootSeries::setup) and P = rho/2 + 3 rho^2/8 +
//       5 rho^3/16 <= 0.0690 carries rho's error (inv 1.5, m0 against m0 + err 1, the product 1: 3.5, times
//       rho P'/P <= 1.2) and three Horner roundings, 7.2 in all, plus the rounding of the sum: 0.0690 x 8.2 = 0.57    1.64
//   c1 e: |c1 e| <= x (1/2 + 3 rho/4 + 15 rho^2/16) G <= 0.0762 G.  c1: G0 2 (y 1.5, m0 0.5), q 2.5, G0 q 1, the bracket
//       2.7 (rho's 3.5 x 0.2, two roundings), the product 1: 9.2; the FMA that forms c1 + e (..) 1: 0.0762 x 10.2      0.78
//   c2 e^2: <= x^2 (3/8 + 15 rho/16) G <= 0.0077 G, coefficient and FMA <= 15: 0.0077 x 15                            0.12
//   c3 e^3: <= 5/16 x^3 G <= 0.00062 G, coefficient <= 12                                                             0.01
//   truncation 35/128 t^4 = 6.1e-17                                                                                   0.55
// 4.10 u (1 + 2^-14) = 4.6e-16 = kErrorBound (the issue's ceiling: 5e-16, an eighth of what the one-step Newton form is
// low by).  A bound, not an estimate: the roundings do not line up, and over 4e5 samples the largest error met is
// 2.9e-16, against 2.7e-16 for the delta form on the same inputs (tests/test_root_direct_cpu.py).
struct RootDirect {
    static constexpr double kRhoMax = 0.125;
    static constexpr double kErrorBound = 4.6e-16;
    double c0, c1, c2, c3;
    // rho = eb / (eb + s2) <= 1/8, without a division (false for NaN)
    static MCD_HD bool direct_ok(double eb, double s2) { return (1.0 / kRhoMax - 1.0) * eb <= s2; }
    // coefficients for this lane's s2 on the chunk with centre eb (the eb of RootSeries::setup)
    MCD_HD void setup(double eb, double s2) {
        RootCentre c;
        c.setup(eb, s2);
        const double G0 = c.G0, q = c.q;
        const double rho = c.p * c.inv;
        const double P = rho * fma_(rho, fma_(rho, 0.3125, 0.375), 0.5);
        c0 = fma_(G0, c.corr + P, G0);
        const double gq = G0 * q;
        c1 = -gq * fma_(rho, fma_(rho, 0.9375, 0.75), 0.5);
        const double gq2 = gq * q;
        c2 = gq2 * fma_(rho, 0.9375, 0.375);
        c3 = -0.3125 * (gq2 * q);
    }
    // e: the record's verr^2 (wave-uniform, an SGPR pair on the device)
    MCD_HD double g_direct(double e) const {
        return fma_sgpr_factor(fma_sgpr_factor(fma_sgpr_factor(c3, e, c2), e, c1), e, c0);
    }
};

// Split exponent offset of the direct loops (option "exp_split").  The record's nbp enters k = rint(u N / ln 2)
// additively and is the same for every walker, so the record preparation converts it into table steps once per star
// (mcd_exp_split.h: exp_split_record): nbp N / ln 2 = nbi + nbf, nbi an integer, |nbf| <= 1/2.  With the root scaled by
// c = sqrt(N / ln 2) (gs = c g: the scale sits in RootDirect's four per-chunk coefficients) and dgs = d gs,
//   shifted = fma(-dgs, dgs, M)     M = 1.5 2^52 + nbi - 5 N, an exact double from the record; k = low word of shifted
//   w       = shifted - M           exact, an integer
//   rv      = fma(-dgs, dgs, -w)    the reduced argument in table steps, |rv| <= 1/2, ONE rounding
// replace the parent's four instructions (u, shifted, kf, r).  e^u = 2^((w + nbi) / N) e^{rv ln2/N} e^{nbf ln2/N}: the
// polynomial runs in rv with its coefficients scaled by powers of ln 2 / N, the table supplies 2^(k / N) = 2^-5 2^((w + nbi) / N),
// and the walker-independent factor e^{nbf ln2/N} goes into the record's omp' = kappa (1 - p),
// kappa = (c / 32) e^{-nbf ln2/N} in 1.2011 (1 +- 3.4e-4), so that y' = fma(gs, es, omp') = kappa y.  Sum log kappa of a chunk is a constant
// of the plan, which the wave adds once per chunk (exp_split_chunk_const).  The 2^-5 keeps c = 38.4 out of the rescale
// headroom (mcd_guard.h: exp_split_admitted).
// Error of y' / kappa against (1 - p) + g e^u, in units of 2^-53 of the cluster term g e^u (the parent's direct form in
// brackets), on top of RootDirect's own budget for g, which both forms share:
//   scaled coefficients: the scale enters through G0 and its rounding error through c0's last FMA
//       (RootDirectSplit), so gs carries the roundings g does                                                   0     [0]
//   c as a double is off by delta = c^2 ln2/N - 1 = 4.9e-17 relative: a factor e^{-dg^2 delta}           0.44 dg^2  [0]
//   reduced argument: rv has ONE rounding, at most 2^-54 of a table step, times ln 2 / N                      4e-4  [0.72 |u|:
//       the parent's one-constant reduction is off by 8e-17 |u|]
//   rounding of dgs = d gs, doubled by the square and carried into the exponent                         2.0 dg^2  [the same]
//   polynomial: coefficients scaled at compile time (C2 s^2, C3 s^3, s: each within 2^-52 of a term <= 3.4e-4,
//       negligible), its last FMA                                                                              1.00  [1.00]
//   table entry, the product T[j] p, the last FMA of y                                                         2.50  [2.50]
//   record: omp' = kappa (1 - p) rounded ONCE from long double (1/2 ulp of the (1 - p) term); M is exact;
//       nbf is held as a double, 2^-54 of a table step off at most (4e-20 relative)                           0.50  [0]
// i.e. half an ulp more than the parent where |u| is small and less where |u| > 1.  Measured over 4.5e5 (star, walker) terms
// of a C3 catalogue through this code: largest relative error 8.6e-16 against the parent's 9.0e-16, both set by the root's
// error amplified by 1 + 2 dg^2 (tests/test_exp_split_cpu.py).
static_assert(kExpTabBits == 10 || kExpTabBits == 8, "kExpSplitC is written for N = 1024 (and halved exactly for N = 256)");
constexpr double kExpSplitC = 0x1.337cc2183b050p+5 / (kExpTabBits == 10 ? 1.0 : 2.0);   // sqrt(1024 / ln 2) = 38.4359170811663934...
constexpr int kExpSplitShift = 5;                                         // es comes out smaller by 2^-5
constexpr double kExpSplitS1 = kExpTabStepHi + kExpTabStepLo;             // ln 2 / N
constexpr double kExpSplitS2 = kExpPolyC2 * kExpSplitS1 * kExpSplitS1;
constexpr double kExpSplitS3 = kExpPolyC3 * kExpSplitS1 * kExpSplitS1 * kExpSplitS1;
constexpr double kExpSplitS4 = kExpPolyC4 * kExpSplitS1 * kExpSplitS1 * kExpSplitS1 * kExpSplitS1;
// k and the reduced argument rv (in table steps) of the split form for dgs = d gs and the record's M (wave-uniform)
MCD_HD double exp_split_reduce(double dgs, double M, int& k) {
    const double shifted = fnma_sgpr_addend(dgs, dgs, M);
    const double w = shifted - M;
    uint64_t bits;
    std::memcpy(&bits, &shifted, sizeof bits);
    k = (int)(uint32_t)bits;
    return fma_(-dgs, dgs, -w);
}
// e^{rv ln2/N}, |rv| <= 1/2: exp_poly with its coefficients scaled; s1 = kExpSplitS1, held in an SGPR pair on the device
MCD_HD double exp_poly_steps(double rv, double s1) {
    double p;
    if constexpr (kExpPolyDegree == 4) p = fma_(fma_(rv, kExpSplitS4, kExpSplitS3), rv, kExpSplitS2);
    else p = fma_(rv, kExpSplitS3, kExpSplitS2);
    p = fma_sgpr_addend(p, rv, s1);                            // (three-address: a VGPR addend is copied for a v_fmac_f64)
    return fma_(p, rv, 1.0);
}

// RootDirect with its coefficients scaled by `scale` (c): g_direct returns gs = c g.  The scale enters through G0, so every
// coefficient is rounded as often as RootDirect's: G0s = fl(c G0) is off by eg = c G0 - G0s, which comes out exactly and
// joins G0's own error in the one last FMA of c0 (eg / G0s to first order, with 1 / G0 = m0 G0 / 4 since G0^2 = 4 / m0)
struct RootDirectSplit : RootDirect {
    // c1, c2, c3 and what c0's one last FMA is made of: c0 = fma(G0s, A, G0s); returns q
    MCD_HD double setup_parts(double eb, double s2, double scale, double& G0s, double& A) {
        RootCentre c;
        c.setup(eb, s2);
        const double q = c.q;
        G0s = c.G0 * scale;
        const double eg = fma_(c.G0, scale, -G0s);
        const double rho = c.p * c.inv;
        const double P = rho * fma_(rho, fma_(rho, 0.3125, 0.375), 0.5);
        A = (c.corr + P) + eg * ((0.25 / scale) * (c.m0 * c.G0));
        const double gq = G0s * q;
        c1 = -gq * fma_(rho, fma_(rho, 0.9375, 0.75), 0.5);
        const double gq2 = gq * q;
        c2 = gq2 * fma_(rho, 0.9375, 0.375);
        c3 = -0.3125 * (gq2 * q);
        return q;
    }
    MCD_HD void setup_scaled(double eb, double s2, double scale) {
        double G0s, A;
        setup_parts(eb, s2, scale, G0s, A);
        c0 = fma_(G0s, A, G0s);
    }
};

// The cubic of RootDirectSplit economised to a quadratic on a 32-star band of the verr-sorted array (option "root_quad",
// DESIGN 3.2).  Block b of a shard's sorted record array is records 32 b .. 32 b + 31 (the last block also takes a remainder
// shorter than 32), whatever the chunk plan.  With e_lo, e_hi its first and last verr^2, m = (e_lo + e_hi) / 2 and
// h = (e_hi - e_lo) / 2, on [m - h, m + h]
//   (e - m)^3 = 3/4 h^2 (e - m) + R,  |R| <= h^3 / 4      (Chebyshev: 4 x^3 - 3 x = T3(x), x = (e - m) / h)
// hence e^3 = a2 e^2 + a1 e + a0 + R with a2 = 3 m, a1 = 3/4 h^2 - 3 m^2, a0 = m^3 - 3/4 h^2 m: constants of the catalogue,
// which the record preparation evaluates in long double and leaves in the unused slots of the block's first two split
// records (mcd_exp_split.h: quad_block_consts).  The lanes fold them into their coefficients once per block,
//   q2 = fma(c3, a2, c2)    q1 = fma(c3, a1, c1)    q0 = fma(G0s, fma(k3, a0, A), G0s)     (c3 = G0s k3, k3 = -5/16 q^3)
// and the root is gs = fma(fma(q2, e, q1), e, q0): two FMAs per term instead of three, three FMAs and two more per 32 terms.
// q0 is built the way c0 is -- A is the bracket of c0's one last FMA, which takes k3 a0 in -- so it carries c0's ONE rounding.
// A chunk takes this form only where the direct vote has passed (and the launch runs the split offset) and, in every lane,
//   H <= kMaxT (eb + s2),  kMaxT = 2^-17.5,  H the largest h of any block the chunk touches (a constant of the plan),
// a third wave-wide vote with the eb of the coefficients (quad_ok).
// Worst-case relative error against (2 (e + s2))^(-1/2), in units of u = 2^-53 relative to G, by the table above RootDirect
// (x = q e <= 1/8 + 2^-13):
//   last FMA                                                                                                       1.00
//   q0: c0's ONE rounding and its bracket (1.64); k3 a0 <= 5/16 x^3 = 6.2e-4 joins the bracket, coefficient <= 12  1.65
//   q1 e: |q1 e| <= |c1 e| + |c3 a1 e| <= (0.0762 + 3 x 6.2e-4) G = 0.0781 G; c1 9.2, the rounding of q1 1, the FMA that
//       forms q1 + e q2 1: 0.0781 x 11.2                                                                           0.88
//   q2 e^2: <= (0.0077 + 3 x 6.2e-4) G = 0.0096 G; c2 <= 14, the rounding of q2 1: 0.0096 x 15                       0.15
//   c3 in q2, q1 (coefficient <= 12, on 3 x 6.2e-4 twice)                                                          0.05
//   the a's, each rounded ONCE from long double: |c3 ai e^i| <= 3 x 6.2e-4 G (a2 e^2 and a1 e are three times e^3 each,
//       a0 once), so their half ulps cost 7 x 6.2e-4 / 2                                                           0.01
//   economisation |c3| h^3 / 4 = (5/64) (h q)^3 G, h q <= 2^-17.5                                                  0.111
//   truncation of the cubic, 35/128 t^4                                                                            0.55
// 4.40 u (1 + 2^-14) = 4.9e-16 = kErrorBound (the ceiling for this form: 5.9e-16).  Measured: tests/test_root_quad_cpu.py.
struct RootQuadCentre : RootDirectSplit {
    double G0s, A, k3;
    // RootDirectSplit's c1 .. c3 (bit for bit) and, in place of c0, what q0 is built from
    MCD_HD void setup_quad(double eb, double s2, double scale) {
        const double q = setup_parts(eb, s2, scale, G0s, A);
        k3 = -0.3125 * ((q * q) * q);
    }
};
struct RootQuad {
    static constexpr double kMaxT = 0x1.6a09e667f3bcdp-18;          // 2^-17.5
    static constexpr double kErrorBound = 4.9e-16;
    double q0, q1, q2;
    // H <= 2^-17.5 (eb + s2), without a division (false for NaN; true for H = 0, a block of equal verr)
    static MCD_HD bool quad_ok(double H, double eb, double s2) { return H <= kMaxT * (eb + s2); }
    // a2, a1, a0: the block's constants from its first two split records (wave-uniform, SGPR pairs on the device)
    MCD_HD void fold(const RootQuadCentre& c, double a2, double a1, double a0) {
        q2 = fma_sgpr_factor(c.c3, a2, c.c2);
        q1 = fma_sgpr_factor(c.c3, a1, c.c1);
        q0 = fma_(c.G0s, fma_sgpr_factor(c.k3, a0, c.A), c.G0s);
    }
    MCD_HD double g_quad(double e) const { return fma_sgpr_factor(fma_sgpr_factor(q2, e, q1), e, q0); }
};
// What a chunk needs to run the quadratic form (the main kernel fills it from the chunk's first record index and the
// length of the record array; default: never)
#if defined(__HIP_DEVICE_COMPILE__)
typedef __attribute__((address_space(3))) double* QuadParkPtr;      // (LDS as such: ds_read / ds_write, a 32-bit address)
#else
typedef double* QuadParkPtr;
#endif
struct QuadArgs {
    bool on = false;          // the third vote is held (option "root_quad", chunk start a multiple of 8, at least one block)
    int back = 0;             // records from the first record of the chunk's first block to the chunk's first record
    int to_boundary = 32;     // stars from the chunk's first record to the next multiple of 32
    int folds = 0;            // of the block boundaries ahead, those that start a block (the last block has no end)
    QuadParkPtr park = nullptr;   // device: 5 x `stride` doubles of LDS, one column per thread of the workgroup, for what
    int stride = 0;               // only the fold reads; park points at the wave's 64 columns (wave-uniform)
};
// ... for the chunk that starts at record `begin` of an array of n_records.  Blocks of 32 records in absolute positions; the
// last one also takes the remainder, so a chunk that starts beyond the last block's first 32 records still belongs to it.
MCD_HD QuadArgs quad_args(int64_t begin, int64_t n_records, bool enabled) {
    QuadArgs q;
    const int64_t n_blocks = n_records >> 5, b = begin >> 5;
    const int64_t b0 = b < n_blocks ? b : n_blocks - 1;
    q.on = enabled && n_blocks > 0 && (begin & 7) == 0;
    q.back = (int)(begin - 32 * b0);
    q.to_boundary = 32 - (int)(begin & 31);
    q.folds = b < n_blocks ? (int)(n_blocks - 1 - b) : 0;
    return q;
}

// true when `ok` holds in every active lane of the wave (one s_cmp on the ballot: callers branch on the scalar unit);
// host build: the caller has combined the lanes (tests/emul)
MCD_HD bool wave_all(bool ok) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_amdgcn_ballot_w64(!ok) == 0;
#else
    return ok;
#endif
}

// x == +-0 tested on the bit pattern: for a wave-uniform x (SGPR pair) this stays on the scalar unit.
MCD_HD bool is_zero_bits(double x) {
    uint64_t b;
    __builtin_memcpy(&b, &x, sizeof b);
    return (b << 1) == 0;
}

// MODEL_BGFIXED: lnL_i = b_i + log((1 - p_i) + p_i t_i),  t_i = exp(m_i - b_i) = g exp(-1/2 q g^2 - b'_i),
// b'_i = b_i + 1/2 log 2pi  (the record carries nbp = -b'_i + log p_i).  Same value as runner.py:280-286.
// BG_FIXED_DENSITY (model.py:565-623) is the same with p -> rho_i, (1 - p) -> f_back and an extra -log(rho_i + f_back).
struct BgFixedAcc {
    LogProduct l;          // sum log y_i   (sum b_i is walker-independent: added once per parameter set by the reduce kernel)
    LogProduct lden;       // BG_FIXED_DENSITY: sum log(rho_i + f)
    int emin;              // smallest biased exponent of any mixture value y_i (see denormal())
    MCD_HD void init() { l.init(); lden.init(); emin = LogProduct::kTrackInit; }
    // True when some y_i fell below 2^-1000.  Since 1 - p >= 2^-53 unless p == 1 exactly, that only happens for a star
    // with pmember == 1 (or a walker with f_back == 0) whose cluster term is e^-693 or less: there the reference's
    // log-sum-exp (runner.py:282-284) works on DENORMAL numbers and its result carries their rounding noise
    // (1e-7 .. 1e-2 absolute).  The library then re-evaluates the batch with the plain kernels, which execute the
    // reference's expression literally, so that fast and plain results never differ by more than rounding.
    // An exact y_i == 0 is flagged too: the reference applies its prefactors inside the exponent (e^{m - M}), this path
    // outside (g e^u), so the two underflow at slightly different outliers (found by tools/fuzz_gpu.py).
    MCD_HD bool denormal() const { return emin < LogProduct::kTrackFloor; }
    template <bool NARROW = false>
    MCD_HD void add_density(double d, double n, double rho, double f, double nbp, const double* __restrict__ exptab) {
        add<false, false, NARROW>(d, n, f, nbp, exptab);        // f_back is a per-walker (VGPR) value here
        lden.mul(rho + f);
    }
    // HALVED: the caller passes 2 n instead of n and the table sqrt(2) 2^(j/256) (MCD_EXP_TABLE_SQRT2_VALUES):
    //   gh = (2 n)^(-1/2) = g / sqrt(2),  -(d gh)^2 = -1/2 d^2 g^2,  p gh (sqrt(2) T[j]) e^r = p g T[j] e^r,
    // which drops the multiplication by -1/2 (2 n = 2 verr^2 + 2 sigma^2 is formed by one FMA, like n by one add).
    // NARROW (chosen per call by the host guard, mcd_guard.h: fast_level): every y_i is known to lie in [2^-53, 2^120]
    // -- pmember < 1 everywhere, so y >= 1 - p >= 2^-53; lnL_bg >= -60 and norm >= 2^-60, so y <= 1 + 2^30 e^{60} --
    // hence eight raw factors can be multiplied between two rescales without the per-star mantissa/exponent split,
    // without the k > 1000 exponent carry and without the denormal-regime tracking; g comes from the one-step Newton
    // form (rsqrt2_newton).
    // TAB_BIASED: `exptab` is the exponent-biased table (exp_tab_bias); NARROW then inserts the exponent with one integer
    // instruction instead of v_ldexp_f64 (exp_tab_scaled: same y bit for bit), the general form restores the entries.
    // CLAMP = false: the bounded sub-variant (u >= -700 by the host guard: exp_tab_scaled without its clamp).
    template <bool UNIFORM_OMP = true, bool HALVED = false, bool NARROW = false, bool TAB_BIASED = false, bool CLAMP = true>
    // The prior weight p of the cluster component is folded into the exponent by the record preparation:
    // nbp = -(b + 1/2 log 2pi) + log p (floored at -2000, where e^u is an exact 0: p == 0 gives y = 1 - p = 1), so
    // y = (1 - p) + g e^{u} with u = -1/2 d^2 g^2 + nbp needs no multiplication by p.
    MCD_HD void add(double d, double n, double omp, double nbp, const double* __restrict__ exptab) {
        // NARROW + HALVED: the caller passes 8 n and the one-step Newton form returns 2 (8 n)^-1/2 = (2 n)^-1/2
        const double g = (NARROW && HALVED) ? rsqrt2_newton(n) : rsqrt_nr(n);
        add_g<UNIFORM_OMP, HALVED, NARROW, TAB_BIASED, CLAMP>(d, g, omp, nbp, exptab);
    }
    // the same with the reciprocal root g given (HALVED: (2 n)^-1/2; the series loops, RootSeries::g)
    template <bool UNIFORM_OMP = true, bool HALVED = false, bool NARROW = false, bool TAB_BIASED = false, bool CLAMP = true>
    MCD_HD void add_g(double d, double g, double omp, double nbp, const double* __restrict__ exptab) {
        const double dg = d * g;
        // u <= 1e5 by the host guard (|lnL_bg| <= 1e5); below -1100 e^u is an exact 0 in f64 (as in the reference),
        // and the clamp keeps u N / ln 2 inside the int range of exp_tab.
        // (NARROW: the guard bounds |v - v_los|^2 / norm by 2e6 and the record floors nbp at -2000, so u > -1.1e6 needs no clamp)
        const double u0 = HALVED ? fnma_sgpr_addend(dg, dg, nbp) : fma_sgpr_addend(-0.5 * dg, dg, nbp);
        const double u = NARROW ? u0 : fmax_raw(u0, -1100.0);
        if constexpr (NARROW && TAB_BIASED) {
            // u < 60 (nbp <= -lnL_bg <= 60) and y >= 1 - p >= 2^-53 > 2^31 2^-1019: exp_tab_scaled's conditions hold
            const double es = exp_tab_scaled<false, CLAMP>(u, exptab);
            const double y = UNIFORM_OMP ? fma_sgpr_addend(g, es, omp) : fma_(g, es, omp);
            l.mul(y);
            return;
        }
        int k;
        const double er = exp_tab<!NARROW, TAB_BIASED>(u, k, exptab);
        if constexpr (NARROW) {
            const double y = UNIFORM_OMP ? fma_sgpr_addend(g, ldexp_(er, k), omp) : fma_(g, ldexp_(er, k), omp);
            l.mul(y);
            return;
        }
        // y = (1 - p) + g e^r 2^k.  k > 1000 (cluster likelihood e^693 times the background's) is carried in the
        // integer part of the product: there the (1 - p) term is below 2^-900 of y and drops out exactly as in f64.
        // k < -1074 underflows inside ldexp; with p == 1 exactly that gives y = 0 and lnL = -inf, which is also what
        // the reference returns there (runner.py:283: log(1 * exp(m - b) + 0) with exp underflowing).
        const int kc = k > 1000 ? 1000 : k;
        const double y = UNIFORM_OMP ? fma_sgpr_addend(g, ldexp_(er, kc), omp) : fma_(g, ldexp_(er, kc), omp);
        l.mul_any_track(y, emin);
        l.e32 += k - kc;
    }
    // The narrow-range term with the split exponent offset (see kExpSplitC): gs = c g, M and ompk = omp' from the split
    // record (wave-uniform), s1 = kExpSplitS1.  Multiplies the product by y' = kappa y.
    template <bool TAB_BIASED = false, bool CLAMP = true>
    MCD_HD void add_gs(double d, double gs, double M, double ompk, double s1, const double* __restrict__ exptab) {
        int k;
        const double p = exp_poly_steps(exp_split_reduce(d * gs, M, k), s1);
        if constexpr (CLAMP) k = k > kExpTabKMin ? k : kExpTabKMin;      // v_max_i32
        double es;
        if constexpr (TAB_BIASED) {
            const double t = exptab[k & (kExpTabSize - 1)];
            const int32_t kh = (int32_t)((uint32_t)k << kExpTabHiShift);
#if defined(__HIP_DEVICE_COMPILE__)
            // (the add on a two-word vector, as exp_tab_scaled<.., false>: here the compiler splits add_hi_word's byte copies
            // into byte-mask operations with the clamp in place too)
            typedef uint32_t word2 __attribute__((ext_vector_type(2)));
            word2 tw = __builtin_bit_cast(word2, t);
            tw.y += (uint32_t)kh;
            es = __builtin_bit_cast(double, tw) * p;
#else
            es = add_hi_word(t, kh) * p;
#endif
        } else {
            es = ldexp_(exptab[k & (kExpTabSize - 1)] * p, k >> kExpTabBits);
        }
        l.mul(fma_sgpr_addend(gs, es, ompk));
    }
    MCD_HD void rescale() { l.rescale(); }
    MCD_HD void rescale_density() { l.rescale(); lden.rescale(); }
    MCD_HD void rescale_narrow() { l.rescale_narrow(); }
    MCD_HD void rescale_density_narrow() { l.rescale_narrow(); lden.rescale_narrow(); }
    MCD_HD double finish() { return l.value(); }
    MCD_HD double finish_density() { return l.value() - lden.value(); }
};

// MODEL_BGGAUSS (constant.py:320-364):
//   lnL_i = log( mu_i C_i + (1 - mu_i) B_i ),  mu_i = rho_i / (rho_i + f)
//         = -1/2 log 2pi - log(rho_i + f) - 1/2 min(w, wb) + log y_i
//   y_i   = rho g + f gb e^{-delta}   (w <= wb)   or   rho g e^{-delta} + f gb   (w > wb),  delta = |wb - w| / 2
//   with g = n^-1/2, w = d^2 g^2 (cluster) and gb, wb (background).  One exp with a non-positive argument.
struct BgGaussAcc {
    double sum_min;        // sum min(w, wb)   (HALVED: sum of min(w, wb) / 2)
    LogProduct ly;         // sum log y_i      (HALVED: y_i / sqrt(2))
    LogProduct lden;       // sum log(rho_i + f)
    int emin;              // as BgFixedAcc::emin: y_i < 2^-1000 needs the undamped component to be exactly zero
    MCD_HD void init() { sum_min = 0.0; ly.init(); lden.init(); emin = LogProduct::kTrackInit; }
    MCD_HD bool denormal() const { return emin < LogProduct::kTrackFloor; }
    // HALVED: the caller passes 2 n and 2 nb: gh = g / sqrt(2), (d gh)^2 = w / 2, so that the exponent argument
    //   -|wb/2 - w/2| = -delta needs no multiplication by -1/2; y comes out divided by sqrt(2) and min(w, wb) halved,
    //   both undone by constants in finish().
    // NARROW (host guard, mcd_guard.h: fast_level): density and f_back in [2^-20, 2^20], norms in [2^-60, 2^60], so
    //   y >= the undamped term >= 2^-51 and y <= 2^52 -- eight raw factors between rescales, no mantissa/exponent split,
    //   no denormal tracking; |d|^2 <= 2e6 norm, so the exponent argument needs no clamp; one-constant range reduction.
    template <bool HALVED = false, bool NARROW = false>
    MCD_HD void add(double d, double n, double db, double nb, double rho, double f, const double* __restrict__ exptab) {
        // NARROW + HALVED: the caller passes 8 n and 8 nb (one-step Newton form, see BgFixedAcc::add)
        const double g = (NARROW && HALVED) ? rsqrt2_newton(n) : rsqrt_nr(n);
        const double gb = (NARROW && HALVED) ? rsqrt2_newton(nb) : rsqrt_nr(nb);
        const double dg = d * g, dbg = db * gb;
        const double w = dg * dg, wb = dbg * dbg;
        const double t = wb - w;
        const bool cluster_big = t >= 0.0;                 // w <= wb: the cluster exponent is the larger one
        const double u0 = HALVED ? -fabs_(t) : -0.5 * fabs_(t);
        int k;                                            // e^-1100 == 0 in f64; the clamp keeps k inside int range
        const double er = exp_tab<!NARROW>(NARROW ? u0 : fmax_(u0, -1100.0), k, exptab);
        const double e = ldexp_(er, k);                    // k <= 0: underflows to 0 inside ldexp
        const double a = rho * g, b = f * gb;
        // if the undamped component is exactly zero (f_back = 0 or density = 0) and e^{-delta} underflows, y = 0 and
        // lnL = -inf -- the same as the reference's log-sum-exp about the larger exponent (constant.py:320-323).
        const double y = cluster_big ? fma_(b, e, a) : fma_(a, e, b);
        if constexpr (NARROW) ly.mul(y);
        else ly.mul_any_track(y, emin);
        lden.mul(rho + f);
        sum_min += fmin_(w, wb);
    }
    MCD_HD void rescale() { ly.rescale(); lden.rescale(); }
    MCD_HD void rescale_narrow() { ly.rescale_narrow(); lden.rescale_narrow(); }
    template <bool HALVED = false>
    MCD_HD double finish(int64_t count) {
        // HALVED: log y = log(y / sqrt 2) + 1/2 log 2 per star, and sum_min already carries its factor 1/2
        const double per_star = HALVED ? kHalfLn2Pi - 0.5 * kLn2 : kHalfLn2Pi;
        return fma_(-(double)count, per_star, HALVED ? -sum_min : -0.5 * sum_min) + (ly.value() - lden.value());
    }
};

// ---------------------------------------------------------------------------------------------
// float32 fast mixtures (MCD_F32 / MCD_F32_ACC64): the same formulations with v_rsq_f32 / v_exp_f32 (1 ulp each, no
// Newton step, no table) and the running products in A = float or double.  Valid under the f32 conditions of
// mcd_guard.h (fast_guard): every mixture value y lies in [2^-27, 2^31], so four factors fit between two rescales.
template <class A>
struct LogProductF {                 // sum of logs as log of a product, mantissa in A, exponent in an int
    A p;
    int e;
    MCD_HD void init() { p = 1; e = 0; }
    MCD_HD void mul(float x) { p *= (A)x; }
    MCD_HD void rescale() {
        int ex;
        p = frexp_(p, &ex);
        e += ex;
    }
    MCD_HD double value() {
        rescale();
        return fma_((double)e, kLn2, log_unit((double)p));
    }
};
// BG_FIXED / BG_FIXED_DENSITY:  y = w0 + g exp(nbp - 1/2 d^2 g^2),  w0 = 1 - p (record) or f_back (walker)
template <class A>
struct BgFixedAccF {
    LogProductF<A> l, lden;
    MCD_HD void init() { l.init(); lden.init(); }
    MCD_HD void add(float d, float n, float w0, float nbp) {
        const float g = rsqf_(n);
        const float dg = d * g;
        l.mul(fma_(g, expf_(fma_(-0.5f * dg, dg, nbp)), w0));
    }
    MCD_HD void add_density(float d, float n, float rho, float f, float nbp) {
        add(d, n, f, nbp);
        lden.mul(rho + f);
    }
    MCD_HD void rescale() { l.rescale(); }
    MCD_HD void rescale_density() { l.rescale(); lden.rescale(); }
    MCD_HD double finish() { return l.value(); }
    MCD_HD double finish_density() { return l.value() - lden.value(); }
    MCD_HD A value_for_anchor() const { return l.p; }
};
// BG_GAUSS:  y = rho g + f gb e^{-delta} (or mirrored), as BgGaussAcc
template <class A>
struct BgGaussAccF {
    A sum_min;
    LogProductF<A> ly, lden;
    MCD_HD void init() { sum_min = 0; ly.init(); lden.init(); }
    MCD_HD void add(float d, float n, float db, float nb, float rho, float f) {
        const float g = rsqf_(n), gb = rsqf_(nb);
        const float dg = d * g, dbg = db * gb;
        const float w = dg * dg, wb = dbg * dbg;
        const float t = wb - w;
        const float e = expf_(-0.5f * (t < 0.0f ? -t : t));
        const float a = rho * g, b = f * gb;
        ly.mul(t >= 0.0f ? fma_(b, e, a) : fma_(a, e, b));
        lden.mul(rho + f);
        sum_min += (A)(w < wb ? w : wb);
    }
    MCD_HD void rescale() { ly.rescale(); lden.rescale(); }
    MCD_HD double finish(int64_t count) {
        return fma_(-(double)count, kHalfLn2Pi, -0.5 * (double)sum_min) + (ly.value() - lden.value());
    }
    MCD_HD A value_for_anchor() const { return ly.p; }
};

// ---------------------------------------------------------------------------------------------
// background.SingleStars (single_stars.py:42-77): one test star against a slice of the comparison stars.
//   e_j = -(c_j - v)^2 h,  h = 1 / (2 (verr^2 + sigma_int^2));   slice result: nearest distance + sum_j exp(e_j - e_max)
// Two passes over the slice: the nearest comparison star gives the largest exponent exactly, every term of the
// second pass then has a non-positive exponent and the nearest star contributes exactly 1.
struct KdeLane {
    double v, h, d2min, sum;
    MCD_HD void init(double v_, double verr, double sigma_int2) {
        v = v_;
        h = 0.5 / fma_(verr, verr, sigma_int2);
    }
    MCD_HD void nearest(double c, double& dmin) const { dmin = fmin_(dmin, fabs_(c - v)); }
    MCD_HD void begin_sum(double dmin) { d2min = dmin * dmin; sum = 0.0; }
    MCD_HD void add(double c, const double* __restrict__ exptab) {
        const double d = c - v;
        // exp(u) == 0 in f64 below u = -745.2; the clamp keeps k inside int range for far outliers
        const double u = fmax_(fma_(-d, d, d2min) * h, -800.0);
        int k;
        // one-constant range reduction: relative error 8e-17 |u| in a term that is e^u <= 1 of a sum >= 1
        const double er = exp_tab<false>(u, k, exptab);
        sum += ldexp_(er, k);
    }
};

// ---------------------------------------------------------------------------------------------
// Software prefetch of the star records the NEXT loop iteration reads, through the VECTOR memory path: lane l < LINES
// loads one word of the l-th 64-byte line, which pulls the lines into L2; the scalar loads of the next iteration then
// find them there.  (A scalar-load prefetch was tried first: the scalar cache serves a wave's requests in order, so the
// iteration's own loads queued behind the prefetch misses -- 7 - 18 % slower, gpurun_out/ab_prefetch.txt.)  The loaded
// word is kept alive until retire(), so the compiler's own s_waitcnt vmcnt covers it.  Reads up to 1.5 KiB past the
// chunk: the record array is allocated with that slack.  Measured on C3 (gpurun_out/ab_prefetch*.txt): 256 walkers
// 202.7 -> 200.1 us, 128 walkers 117.2 -> 107.4 us, 64 walkers 89.5 -> 61.5 us; with 256 walkers three of a chunk's four
// waves find their records fetched by the first, with fewer walkers every wave waits for memory on its own (VALUBusy
// 85 % / 67 % without the prefetch, tools/sq_w128.sh).
template <int BYTES, bool ON>
struct RecordPrefetch {
    static constexpr int kLines = (BYTES + 63) / 64 > 8 ? 8 : (BYTES + 63) / 64;
    uint32_t t;
    // ON is a template parameter of the kernel, not a launch parameter: even switched off at run time the lane index,
    // the predicate and the asm of retire() cost the tight CONST loops 6 - 16 % (C5: 190 us against 164 us compiled
    // out).  Which launches get the prefetching instantiation: mcd_api_catalog.hip, wants_prefetch().
    template <class P>
    MCD_HD void issue(P next) {
#if defined(__HIP_DEVICE_COMPILE__)
        if constexpr (ON) {
            const unsigned lane = __builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u));
            typedef const uint32_t __attribute__((address_space(1)))* global_word_ptr;
            t = 0;
            if (lane < (unsigned)kLines) t = *(global_word_ptr)((uint64_t)next + lane * 64u);
            return;
        }
#endif
        (void)next;
        t = 0;
    }
    MCD_HD void retire(double anchor) {
#if defined(__HIP_DEVICE_COMPILE__)
        if constexpr (ON) asm volatile("" :: "v"(t), "v"(anchor));
#endif
        (void)anchor;
    }
};

// ---------------------------------------------------------------------------------------------
// One chunk of stars for one walker.  On the GPU `r` is wave-uniform (lane = walker), so every record
// read below is a scalar load and the record values are SGPR operands of the vector ops.
template <class T> struct WalkerConsts {
    T vsys, s2, vx, vy, sac, cac, sdc, cdc, vb, sb2, fb, a2, s2a, rp2, rp_2;
    T vxc, vyc, rc2, rc_2;                            // double models only: dead loads for every other MODEL
    T es2;                                            // error-scale models only: likewise
    template <class P>
    MCD_HD void load(const P* __restrict__ p) {
        vsys = p[W_VSYS]; s2 = p[W_S2]; vx = p[W_VX]; vy = p[W_VY];
        sac = p[W_SAC]; cac = p[W_CAC]; sdc = p[W_SDC]; cdc = p[W_CDC];
        vb = p[W_VB]; sb2 = p[W_SB2]; fb = p[W_FB];
        a2 = p[W_A2]; s2a = p[W_S2A]; rp2 = p[W_RP2]; rp_2 = p[W_2RP];
        vxc = p[W_VXC]; vyc = p[W_VYC]; rc2 = p[W_RC2]; rc_2 = p[W_2RC];
        es2 = p[W_ES2];
    }
};

// Residual d = v - v_los and variance n = verr^2 + sigma_los^2 of one star for one walker.
//   CONST   (constant.py:52-111): v_los = v_sys + v_maxx sin(theta) - v_maxy cos(theta), sigma_los = sigma_max
//   PROFILE (model.py:93-180):    v_los = v_sys + 2 r_peak (v_maxx dy - v_maxy dx) / (r_peak^2 + r^2)
//                                 sigma_los^2 = sigma_max^2 a / sqrt(a^2 + r^2)           (all lengths in arcsec)
//   DOUBLE:  a second Lynden-Bell component with its own amplitudes and the peak radius rho_2 = r_peak_ratio r_peak on the
//            same dispersion profile.  With m_k = rho_k^2 + r^2, K_k = 2 rho_k, cross_k = v_maxx_k dy - v_maxy_k dx the two
//            quotients share ONE reciprocal:
//                d = (v - v_sys) - (K_1 cross_1 m_2 + K_2 cross_2 m_1) rcp(m_1 m_2),
//            i.e. two crosses, the product m_1 m_2 and four multiply-adds more than PROFILE and no second reciprocal
//            sequence.  The guard's general domain (lengths within 2^-100 .. 2^100, mcd_guard.h) keeps m_1 m_2 within
//            2^+-402.  With both second amplitudes 0 the value is PROFILE's up to the rounding of the shared reciprocal.
//   ESCALE:  the base model's d; the variance is err_scale^2 verr^2 + sigma_los^2 with es2 = err_scale^2 of the walker row:
//            CONST    n = fma(es2, verr^2, sigma_max^2)                       one fma in place of the add (fast forms;
//                                                                              the plain form multiplies, then adds)
//            PROFILE  n = fma(sigma_max^2 a, t, es2 verr^2)                   one multiply more than PROFILE
//            At es2 == 1 both are their base models' expressions bit for bit (1 x is exact), in every form.
// NEWTON1 (narrow-range variants of the profile mixtures, f64): the Plummer root from ONE Newton step in its
// three-instruction form (rsqrt2_newton: low by <= 4.1e-15 relative, see there), two instructions fewer than rsqrt_nr.
template <int MODEL, class T, bool FREE, bool FASTMATH = false, bool NEWTON1 = false>
MCD_HD void star_d_n(RecPtr<T> r, const WalkerConsts<T>& w, T& d, T& n) {
    if constexpr (!is_profile(MODEL)) {
        if (FREE) d = free_centre_residual<FASTMATH>(r[2], r[3], r[4], w.sac, w.cac, w.sdc, w.cdc, w.vx, w.vy, r[0] - w.vsys);
        else d = fma_(-w.vx, r[2], fma_(w.vy, r[3], r[0] - w.vsys));
        // (plain form: multiply, then add -- with the fma the plain CONST kernel with a fixed centre takes 134 VGPRs, with
        // the two operations 102; both are r[1] + w.s2 bit for bit at es2 == 1)
        if constexpr (is_escale(MODEL)) n = FASTMATH ? fma_(w.es2, r[1], w.s2) : w.es2 * r[1] + w.s2;
        else n = r[1] + w.s2;
    } else {
        T dx, dy, r2;
        if (FREE) {
            T x, y;
            free_centre_xy(r[2], r[3], r[4], w.sac, w.cac, w.sdc, w.cdc, x, y);
            dx = T(kArcsecPerRad) * x;
            dy = T(kArcsecPerRad) * y;
            r2 = fma_(dx, dx, dy * dy);
        } else { dx = r[2]; dy = r[3]; r2 = r[4]; }
        T t, inv;
        if constexpr (is_double(MODEL)) {
            // (NEWTON1 changes nothing here: the double models have no narrow-range variant, level_verdict never returns 2
            // for them and no launcher instantiates one)
            const T m1 = w.rp2 + r2, m2 = w.rc2 + r2, mm = m1 * m2;
            if constexpr (FASTMATH && sizeof(T) == 8) {
                t = (T)rsqrt_nr((double)(w.a2 + r2));
                inv = (T)rcp_nr((double)mm);
            } else {
                t = T(1) / sqrt_(w.a2 + r2);
                inv = T(1) / mm;
            }
            const T cross1 = fma_(w.vx, dy, -(w.vy * dx));
            const T cross2 = fma_(w.vxc, dy, -(w.vyc * dx));
            const T num = fma_(w.rp_2 * cross1, m2, (w.rc_2 * cross2) * m1);
            d = fma_(-num, inv, r[0] - w.vsys);
            n = fma_(w.s2a, t, r[1]);
            return;
        }
        if constexpr (FASTMATH && NEWTON1 && sizeof(T) == 8) {
            // rsqrt2_newton returns 2 (a^2 + r^2)^-1/2: the factor goes into sigma_max^2 a / 2 (loop-invariant)
            const T cross = fma_(w.vx, dy, -(w.vy * dx));
            inv = (T)rcp_nr((double)(w.rp2 + r2));
            d = fma_(-(w.rp_2 * inv), cross, r[0] - w.vsys);
            n = fma_(T(0.5) * w.s2a, (T)rsqrt2_newton((double)(w.a2 + r2)), r[1]);
            return;
        } else if constexpr (FASTMATH && sizeof(T) == 8) {
            t = (T)rsqrt_nr((double)(w.a2 + r2));
            inv = (T)rcp_nr((double)(w.rp2 + r2));
        } else {
            t = T(1) / sqrt_(w.a2 + r2);
            inv = T(1) / (w.rp2 + r2);
        }
        const T cross = fma_(w.vx, dy, -(w.vy * dx));
        d = fma_(-(w.rp_2 * inv), cross, r[0] - w.vsys);
        if constexpr (is_escale(MODEL)) n = fma_(w.s2a, t, w.es2 * r[1]);
        else n = fma_(w.s2a, t, r[1]);
    }
}

// `denormal` is set when a fast mixture path met the denormal regime described at BgFixedAcc::denormal().
// `exptab`: the 2^(j/256) table of exp_tab (read by the fast mixture paths only; may be null otherwise);
// for MODEL_BGFIXED it is the sqrt(2)-scaled table (exp_table_is_sqrt2_scaled).
MCD_HD constexpr bool exp_table_is_sqrt2_scaled(int model) { return model == MODEL_BGFIXED; }

// ---------------------------------------------------------------------------------------------
// One function per family of chunk_loglike (below).  The group loops (RecordPrefetch issue, body, retire, rescale) are
// written out in each: behind a shared loop helper that takes the body as a lambda hipcc emits other vector code.

// plain path without background: one log and one division per term (runner.py:269-270 keeps two sums as well)
template <int MODEL, bool FREE, class T, class A>
MCD_HD double chunk_plain(RecPtr<T> r, int count, const WalkerConsts<T>& w) {
    constexpr int ND = record_doubles(MODEL, FREE);
    A sum_log = 0, sum_q = 0;
#pragma unroll 4
    for (int j = 0; j < count; ++j, r += ND) {
        T d, n;
        star_d_n<MODEL, T, FREE>(r, w, d, n);
        sum_log += (A)log_(n);
        sum_q += (A)(d * d / n);
    }
    return -0.5 * ((double)count * kLn2Pi + (double)sum_log + (double)sum_q);
}

// plain mixtures: the reference's expressions term by term
template <int MODEL, bool FREE, class T, class A>
MCD_HD double chunk_plain_mixture(RecPtr<T> r, int count, const WalkerConsts<T>& w) {
    constexpr int ND = record_doubles(MODEL, FREE);
    constexpr int XB = geometry_doubles(MODEL, FREE);      // first background slot of a record
    constexpr int BG = bg_kind(MODEL);
    A sum = 0;
#pragma unroll 2
    for (int j = 0; j < count; ++j, r += ND) {
        T d, n;
        star_d_n<MODEL, T, FREE>(r, w, d, n);
        const T m = gauss_lnl(d, n);
        T b, p;
        if (BG == BG_FIXED) {
            b = r[XB];
            p = r[XB + 1];
        } else if (BG == BG_FIXED_DENSITY) {
            b = r[XB];
            const T rho = r[XB + 2];
            p = rho / (rho + w.fb);                          // model.py:588
        } else {
            const T nb = r[1] + w.sb2;                       // constant.py:333, model.py:423
            const T db = r[0] - w.vb;
            b = gauss_lnl(db, nb);                           // constant.py:334-336
            const T rho = r[XB];
            p = rho / (rho + w.fb);                          // constant.py:339, model.py:429
        }
        sum += (A)mixture_lnl(m, b, p);                      // runner.py:282-284, constant.py:320-323
    }
    return (double)sum;
}

// float32 fast mixtures: four stars (one scalar record batch) per rescale; A = float or double
template <int MODEL, bool FREE, class A, bool PF>
MCD_HD double chunk_mixture_f32(RecPtr<float> r, int count, const WalkerConsts<float>& w) {
    constexpr int ND = record_doubles(MODEL, FREE);
    constexpr int XB = geometry_doubles(MODEL, FREE);
    constexpr int BG = bg_kind(MODEL);
    auto run4 = [&](auto& acc, auto&& one, auto&& rescale) {
        const int n4 = count >> 2;
        for (int g = 0; g < n4; ++g, r += 4 * ND) {
            RecordPrefetch<4 * ND * 4, PF> pf;
            pf.issue(r + 4 * ND);
#pragma unroll
            for (int j = 0; j < 4; ++j) one(r + j * ND);
            rescale();
            pf.retire((double)acc.value_for_anchor());
        }
        for (int j = n4 * 4; j < count; ++j, r += ND) { one(r); rescale(); }
    };
    if constexpr (BG == BG_GAUSS) {
        BgGaussAccF<A> acc;
        acc.init();
        run4(acc, [&](RecPtr<float> rr) {
            float d, n;
            star_d_n<MODEL, float, FREE, true>(rr, w, d, n);
            acc.add(d, n, rr[0] - w.vb, rr[1] + w.sb2, rr[XB], w.fb);
        }, [&]() { acc.rescale(); });
        return acc.finish(count);
    } else if constexpr (BG == BG_FIXED) {
        BgFixedAccF<A> acc;
        acc.init();
        run4(acc, [&](RecPtr<float> rr) {
            float d, n;
            star_d_n<MODEL, float, FREE, true>(rr, w, d, n);
            acc.add(d, n, rr[XB + 2], rr[XB + 3]);
        }, [&]() { acc.rescale(); });
        return acc.finish();
    } else {
        BgFixedAccF<A> acc;
        acc.init();
        run4(acc, [&](RecPtr<float> rr) {
            float d, n;
            star_d_n<MODEL, float, FREE, true>(rr, w, d, n);
            acc.add_density(d, n, rr[XB + 2], w.fb, rr[XB + 1]);
        }, [&]() { acc.rescale_density(); });
        return acc.finish_density();
    }
}

// f32 fraction tree over 4 stars + f32 log-product.  One iteration covers 16 stars (four trees) so that four
// 64-byte scalar record loads are in flight per wave: a 4-star iteration is only ~40 ns of VALU work, far
// less than one load latency even with 8 waves per SIMD.
template <int MODEL, bool FREE, class A, bool PF>
MCD_HD double chunk_const_f32(RecPtr<float> r, int count, const WalkerConsts<float>& w) {
    constexpr int ND = record_doubles(MODEL, FREE);
    ConstAccF<A> acc;
    acc.init();
    // MODEL_CONST with a fixed centre has registers to spare for a 16-star tree (one reciprocal per 16 stars); the
    // other instantiations keep 8-star trees (a 16-star tree there costs occupancy)
    constexpr bool TREE16 = base_model(MODEL) == MODEL_CONST && !FREE;
    const int n16 = TREE16 ? count >> 4 : 0;
    for (int g = 0; g < n16; ++g, r += 16 * ND) {
        RecordPrefetch<16 * ND * 4, PF> pf;
        pf.issue(r + 16 * ND);
        float qq[16], nn[16];
#pragma unroll
        for (int j = 0; j < 16; ++j) {
            float d;
            star_d_n<MODEL, float, FREE, true>(r + j * ND, w, d, nn[j]);
            qq[j] = d * d;
        }
#pragma unroll
        for (int t = 0; t < 4; ++t) acc.add4(qq + 4 * t, nn + 4 * t);
        pf.retire((double)acc.p);
    }
    const int done = n16 << 4;
    const int n4 = (count - done) >> 2;
    for (int g = 0; g < n4; ++g, r += 4 * ND) {
        float qq[4], nn[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            float d;
            star_d_n<MODEL, float, FREE, true>(r + j * ND, w, d, nn[j]);
            qq[j] = d * d;
        }
        acc.add4(qq, nn);
    }
    for (int j = done + n4 * 4; j < count; ++j, r += ND) {
        float d, n;
        star_d_n<MODEL, float, FREE, true>(r, w, d, n);
        acc.add1(d * d, n);
    }
    return acc.finish(count);
}

// narrow-range profile variant (ProfileNarrowAcc): no reciprocal per term, one-step Newton root for the Plummer
// dispersion (rsqrt2_newton returns 2 (a^2 + r^2)^-1/2: the factor goes into sigma_max^2 a / 2)
template <bool PF>
MCD_HD double chunk_profile_narrow(RecPtr<double> r, int count, const WalkerConsts<double>& w) {
    constexpr int ND = record_doubles(MODEL_PROFILE, false);
    ProfileNarrowAcc acc;
    acc.init();
    const double hs2a = 0.5 * w.s2a;
    auto one = [&](RecPtr<double> rr, double& q1, double& n1, double& m1) {
        m1 = w.rp2 + rr[4];
        const double t2 = rsqrt2_newton(w.a2 + rr[4]);
        const double n = fma_(hs2a, t2, rr[1]);
        const double cross = fma_(w.vx, rr[3], -(w.vy * rr[2]));
        const double nd = fma_(rr[0] - w.vsys, m1, -(w.rp_2 * cross));
        q1 = nd * nd;
        n1 = (m1 * m1) * n;
    };
    const int n8 = count >> 3;
    for (int g = 0; g < n8; ++g, r += 8 * ND) {
        RecordPrefetch<8 * ND * 8, PF> pf;
        pf.issue(r + 8 * ND);
        double qq[8], nn[8], mm[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) one(r + j * ND, qq[j], nn[j], mm[j]);
        const double m_prod = ((mm[0] * mm[1]) * (mm[2] * mm[3])) * ((mm[4] * mm[5]) * (mm[6] * mm[7]));
        acc.add8(qq, nn, m_prod);
        pf.retire(acc.q);
    }
    for (int j = count & ~7; j < count; ++j, r += ND) {
        double q1, n1, m1;
        one(r, q1, n1, m1);
        acc.add1(q1, n1, m1);
    }
    return acc.finish(count);
}

// fraction-tree + log-product path (f64): 8 stars -> one division, one product factor
template <int MODEL, bool FREE, bool PF>
MCD_HD double chunk_const_fast(RecPtr<double> r, int count, const WalkerConsts<double>& w) {
    constexpr int ND = record_doubles(MODEL, FREE);
    ConstAcc acc;
    acc.init();
    // MODEL_CONST with a fixed centre has registers to spare for a 16-star tree (one reciprocal per 16 stars); the
    // other instantiations keep 8-star trees (a 16-star tree there costs occupancy)
    constexpr bool TREE16 = base_model(MODEL) == MODEL_CONST && !FREE;
    const int n16 = TREE16 ? count >> 4 : 0;
    for (int g = 0; g < n16; ++g, r += 16 * ND) {
        RecordPrefetch<16 * ND * 8, PF> pf;
        pf.issue(r + 16 * ND);
        double qq[16], nn[16];
#pragma unroll
        for (int j = 0; j < 16; ++j) {
            double d;
            star_d_n<MODEL, double, FREE, true>(r + j * ND, w, d, nn[j]);
            qq[j] = d * d;
        }
        acc.add16(qq, nn);
        pf.retire(acc.q);
    }
    const int n8 = TREE16 ? (count >> 3) & 1 : count >> 3;
    for (int g = 0; g < n8; ++g, r += 8 * ND) {
        RecordPrefetch<8 * ND * 8, PF> pf;
        pf.issue(r + 8 * ND);
        double qq[8], nn[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            double d;
            star_d_n<MODEL, double, FREE, true>(r + j * ND, w, d, nn[j]);
            qq[j] = d * d;
        }
        acc.add8(qq, nn);
        pf.retire(acc.q);
    }
    for (int j = count & ~7; j < count; ++j, r += ND) {
        double d, n;
        star_d_n<MODEL, double, FREE, true>(r, w, d, n);
        acc.add1(d * d, n);
    }
    return acc.finish(count);
}

// BG_FIXED, f64 fast forms.  MODEL_BGFIXED has norm = verr^2 + sigma^2 (constant.py:52-74): the accumulator takes 2 norm
// (HALVED form; 8 norm for the narrow-range variant's one-step Newton reciprocal root) and `exptab` is then the
// sqrt(2)-scaled table; star_d_n's own norm is dead code there.
template <int MODEL, bool FREE, int FAST, bool PF, bool TAB_BIASED, bool BOUNDED, bool BLOCK = false>
MCD_HD double chunk_bgfixed_fast(RecPtr<double> r, int count, const WalkerConsts<double>& w, bool& denormal,
                                 const double* __restrict__ exptab, int rescale_iters, bool series, bool direct,
                                 RecPtr<double> r_split, const double* __restrict__ split_const, const QuadArgs& quad) {
    constexpr int ND = record_doubles(MODEL, FREE);
    constexpr int XB = geometry_doubles(MODEL, FREE);
    constexpr bool HALVED = MODEL == MODEL_BGFIXED;
    constexpr bool NARROW = FAST == 2 && MODEL == MODEL_BGFIXED;
    constexpr double kScale = NARROW ? 8.0 : 2.0;
    const double s2x = kScale * w.s2;
    const double scale = BOUNDED ? vgpr_constant(kScale) : kScale;
    BgFixedAcc acc;
    acc.init();
    // SERIES (std::false_type / std::true_type / a RootDirect): the reciprocal root from the chunk's RootSeries (or from
    // the RootDirect passed along, the same cubic in verr^2 itself) instead of v_rsq_f64 and the Newton step; everything
    // after g is the same code
    RootSeries sr;
    auto one = [&](RecPtr<double> rr, auto SERIES, double sc) {
        double d, n;
        star_d_n<MODEL, double, FREE, true>(rr, w, d, n);
        if constexpr (std::is_same<decltype(SERIES), const RootQuad*>::value) {
            // the split loop with the block's quadratic in place of the chunk's cubic
            acc.add_gs<TAB_BIASED, !BOUNDED>(d, SERIES->g_quad(rr[1]), rr[XB], rr[XB + 1], sc, exptab);
        } else if constexpr (std::is_same<decltype(SERIES), RootDirectSplit>::value) {
            // the split record [v, verr^2, cx, cy, M, omp', 0, 0]; sc: kExpSplitS1 here
            acc.add_gs<TAB_BIASED, !BOUNDED>(d, SERIES.g_direct(rr[1]), rr[XB], rr[XB + 1], sc, exptab);
        } else if constexpr (std::is_same<decltype(SERIES), RootDirect>::value) {
            acc.add_g<true, HALVED, NARROW, TAB_BIASED, !BOUNDED>(d, SERIES.g_direct(rr[1]), rr[XB + 2], rr[XB + 3], exptab);
        } else if constexpr (decltype(SERIES)::value) {
            acc.add_g<true, HALVED, NARROW, TAB_BIASED, !BOUNDED>(d, sr.g(rr[1]), rr[XB + 2], rr[XB + 3], exptab);
        } else {
            if constexpr (HALVED) n = fma_(sc, rr[1], s2x);
            acc.add<true, HALVED, NARROW, TAB_BIASED, !BOUNDED>(d, n, rr[XB + 2], rr[XB + 3], exptab);
        }
    };
    const int n4 = count >> 2;
    static_assert(!BOUNDED || (NARROW && PF && TAB_BIASED && !FREE), "the bounded loop is the prefetching BGFIXED one");
    static_assert(!BLOCK || BOUNDED, "the block step belongs to the bounded loop");
    auto four = [&](RecPtr<double> r4, auto SERIES) {
        if constexpr (std::is_same<decltype(SERIES), RootDirectSplit>::value || std::is_same<decltype(SERIES), const RootQuad*>::value) {
            // (the linear coefficient of the scaled polynomial in place of the rsq loops' variance scale)
#pragma unroll
            for (int j = 0; j < 4; ++j) one(r4 + j * ND, SERIES, kExpSplitS1);
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j) one(r4 + j * ND, SERIES, scale);
        }
    };
    // The quadratic form (RootQuad): its coefficients change where the absolute record index reaches a multiple of 32 that
    // starts a block.  A scalar countdown in stars, tested where an 8-star iteration, a 4-star group or a single star
    // starts (chunk starts are multiples of 8, so a boundary never falls inside one); the fold is a block outside the loop
    // body, as the bounded rescale is.  `fold_at`: set by the quadratic copy below.
    RootQuad sq;
    RootQuadCentre qc;
    int to_boundary = quad.to_boundary, folds = quad.folds;
    auto fold_at = [&](RecPtr<double> rb) {
        RootQuadCentre c;
        c.c3 = qc.c3;
#if defined(__HIP_DEVICE_COMPILE__)
        // (volatile: re-read here, five ds_read_b64 per 32 terms, instead of five register pairs across the loop; the
        // thread's column is worked out here too, behind an empty volatile asm, so that no address stays in a register)
        int column;                                                    // the lane
        asm volatile("v_mbcnt_lo_u32_b32 %0, -1, 0\n\tv_mbcnt_hi_u32_b32 %0, -1, %0" : "=v"(column));
        const volatile __attribute__((address_space(3))) double* park = quad.park + column;
        c.c1 = park[0];
        c.c2 = park[quad.stride];
        c.G0s = park[2 * quad.stride];
        c.A = park[3 * quad.stride];
        c.k3 = park[4 * quad.stride];
#else
        c.c1 = qc.c1; c.c2 = qc.c2; c.G0s = qc.G0s; c.A = qc.A; c.k3 = qc.k3;
#endif
        sq.fold(c, rb[XB + 2], rb[XB + 3], rb[ND + XB + 2]);
    };
    auto boundary = [&](RecPtr<double> rb, int step) {
        if (to_boundary == 0) {
            to_boundary = 32;
            MCD_KEEP_BRANCH();
            if (folds > 0) { --folds; fold_at(rb); }
        }
        to_boundary -= step;
    };
    auto run = [&](auto SERIES) {
        constexpr bool QUAD = std::is_same<decltype(SERIES), const RootQuad*>::value;
        if constexpr (BOUNDED && BLOCK && QUAD) {
            // Block step (option "block_step"): the bounded quadratic loop with ONE block outside the loop body, taken
            // where the absolute record index reaches a multiple of 32.  It holds the fold (where a block starts there),
            // the rescale and the prefetch of a whole block, so the loop body is the per-term arithmetic alone.
            //   Rescale: at most 32 raw factors lie between two rescales here (the stars up to the chunk's first boundary,
            //   then whole blocks; a boundary inside the array's last block, which starts no block, rescales all the
            //   same).  The launch admits this loop only where 56 fit (mcd_guard.h: block_step_admitted).  Rescaling
            //   multiplies by a power of two: the bits of the loop below, whose rescales count from the chunk's start.
            //   Prefetch: one vector load whose lane l < 32 touches the 64-byte record l of the band BEHIND the one that
            //   starts here (MCD_BLOCK_STEP_AHEAD = 1; two bands ahead and 16 lanes on 128-byte lines measured the same at 256
            //   walkers and worse at 128, profiles/r14_c3_ab.txt), clamped to the chunk's own records -- the lanes are
            //   switched off through the exec mask, from scalar arithmetic -- so it addresses nothing outside the array.
            //   The chunk's records up to there, at most 64, are touched once in front of the loop.  The touched word is
            //   dead: it is retired in the NEXT block step (and behind the loop), where the wait has long been served.
            //   A band is touched 32 stars before it is read instead of 8: the launch takes this loop only where that
            //   much more in flight still fits the L2 (mcd_internal.h: block_step_fits_l2).
            //   `col`: the lane's column in the parked planes as an LDS address, kept in one VGPR across the loop; shifted
            //   by three it is the lane's record in the prefetch, less what `line0` takes off the scalar base.
            uint32_t touched = 0;
#if defined(__HIP_DEVICE_COMPILE__)
            uint32_t col = (uint32_t)(uintptr_t)quad.park +
                           8u * __builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u));
            asm volatile("" : "+v"(col));
            const uint64_t line0 = (uint64_t)(uint32_t)(uintptr_t)quad.park << 3;
#endif
            auto touch = [&](RecPtr<double> at, int records, int max_lines) {
#if defined(__HIP_DEVICE_COMPILE__)
                // (the lanes' mask by a select, not a clamp: hipcc takes a two-sided clamp of a wave-uniform int to v_med3_i32)
                const int lines = records > max_lines ? max_lines : records;
                const uint64_t lanes = lines > 0 ? (lines < 64 ? ~(~0ull << lines) : ~0ull) : 0;
                typedef const uint32_t __attribute__((address_space(1)))* global_word_ptr;
                asm volatile("" :: "v"(touched));
                // (the scalar base and the shift behind volatile asm: left in sight, the address becomes an induction
                // variable of the loop, a 64-bit vector add per iteration and a register pair across it)
                uint64_t base = (uint64_t)at - line0;
                asm volatile("" : "+s"(base));
                uint32_t line;
                asm volatile("v_lshlrev_b32 %0, 3, %1" : "=v"(line) : "v"(col));
                if (__builtin_amdgcn_inverse_ballot_w64(lanes)) touched = *(global_word_ptr)(base + (uint64_t)line);
#else
                (void)at; (void)records; (void)max_lines; (void)touched;
#endif
            };
            const int n8 = count >> 3;
            constexpr int kAhead = 32 * MCD_BLOCK_STEP_AHEAD;             // stars between a block step and the band it touches
            static_assert(ND * 8 == 64 && 32 + kAhead <= 64, "one lane per 64-byte record, a chunk's first bands in one load");
            touch(r, count < to_boundary + kAhead ? count : to_boundary + kAhead, 64);
            for (int g = 0; g < n8; ++g, r += 8 * ND) {
                if (to_boundary == 0) {
                    to_boundary = 32;
                    MCD_KEEP_BRANCH();
                    if (folds > 0) {
                        --folds;
#if defined(__HIP_DEVICE_COMPILE__)
                        RootQuadCentre c;
                        c.c3 = qc.c3;
                        const volatile __attribute__((address_space(3))) double* park =
                            (const volatile __attribute__((address_space(3))) double*)col;
                        c.c1 = park[0];
                        c.c2 = park[quad.stride];
                        c.G0s = park[2 * quad.stride];
                        c.A = park[3 * quad.stride];
                        c.k3 = park[4 * quad.stride];
                        sq.fold(c, r[XB + 2], r[XB + 3], r[ND + XB + 2]);
#else
                        fold_at(r);
#endif
                    }
                    acc.rescale_narrow();
                    touch(r + kAhead * ND, count - 8 * g - kAhead, 32);
                }
                to_boundary -= 8;
                four(r, SERIES);
                four(r + 4 * ND, SERIES);
            }
#if defined(__HIP_DEVICE_COMPILE__)
            asm volatile("" :: "v"(touched));
#endif
            acc.rescale_narrow();
            if (n4 & 1) {
                boundary(r, 4);
                four(r, SERIES);
                r += 4 * ND;
                acc.rescale_narrow();
            }
        } else if constexpr (BOUNDED) {
            // bounded sub-variant: every mixture value lies in [y_lo, y_hi] with R log2(y_hi) <= 1000 and
            // 1 + R (-log2 y_lo) <= 1000 (mcd_guard.h: bounded_rescale), so R = 8 rescale_iters raw factors fit between
            // two rescales.  A scalar countdown sends every rescale_iters-th iteration to the rescale, a block outside
            // the loop body (4 VALU instructions per R terms instead of 3 per 8; a nested loop costs a v_mov_b64 per
            // iteration).  Rescaling multiplies by a power of two, which commutes with the rounding of every product
            // while nothing overflows or goes subnormal: the same bits as the loop below.
            int until = rescale_iters;
            for (int g = 0; g < (count >> 3); ++g, r += 8 * ND) {
                if constexpr (QUAD) boundary(r, 8);
                RecordPrefetch<8 * ND * 8, PF> pf;
                pf.issue(r + 8 * ND);
                four(r, SERIES);
                four(r + 4 * ND, SERIES);
                pf.retire(acc.l.p);
                if (--until == 0) { until = rescale_iters; MCD_KEEP_BRANCH(); acc.rescale_narrow(); }
            }
            acc.rescale_narrow();
            if (n4 & 1) {
                if constexpr (QUAD) boundary(r, 4);
                four(r, SERIES);
                r += 4 * ND;
                acc.rescale_narrow();
            }
        } else if constexpr (NARROW && PF) {
            // eight raw factors per rescale in one 8-star iteration (two scalar record-load batches): the prefetch's
            // address and exec-mask instructions and the loop branch are paid once per eight terms, and the rescale needs
            // no branch and no register copy -- 23.6 VALU instructions per term instead of 24.0.  Same
            // products and rescale points as the 4-star loop below.  (Without the prefetch hipcc hoists the second
            // group's record loads and takes 76 VGPRs, i.e. 6 waves per SIMD: that instantiation keeps 4-star groups.)
            for (int g = 0; g < (count >> 3); ++g, r += 8 * ND) {
                if constexpr (QUAD) boundary(r, 8);
                RecordPrefetch<8 * ND * 8, PF> pf;
                pf.issue(r + 8 * ND);
                four(r, SERIES);
                four(r + 4 * ND, SERIES);
                pf.retire(acc.l.p);
                acc.rescale_narrow();
            }
            if (n4 & 1) {
                if constexpr (QUAD) boundary(r, 4);
                four(r, SERIES);
                r += 4 * ND;
                acc.rescale_narrow();
            }
        } else if constexpr (NARROW) {
            // eight raw factors per rescale: every second 4-star group (one scalar record-load batch each)
            for (int g = 0; g < n4; ++g, r += 4 * ND) {
                if constexpr (QUAD) boundary(r, 4);
                four(r, SERIES);
                if (g & 1) { MCD_KEEP_BRANCH(); acc.rescale_narrow(); }    // wave-uniform: a scalar branch, not a select
            }
            if (n4 & 1) acc.rescale_narrow();
        } else {
            for (int g = 0; g < n4; ++g, r += 4 * ND) {
                RecordPrefetch<4 * ND * 8, PF> pf;
                pf.issue(r + 4 * ND);
                four(r, SERIES);
                pf.retire(acc.l.p);
                acc.rescale();
            }
        }
        for (int j = n4 * 4; j < count; ++j, r += ND) {
            if constexpr (QUAD) boundary(r, 1);
            one(r, SERIES, (std::is_same<decltype(SERIES), RootDirectSplit>::value || QUAD) ? kExpSplitS1 : kScale);
            acc.rescale();
        }
    };
    // The series form where every lane's sigma^2 keeps the chunk's verr^2 band inside |t| <= 2^-13 (RootSeries): the
    // verdict depends on the chunk's first and last record and the wave's walkers alone, so the 4-star, the 8-star and
    // the bounded loop decide alike and stay bitwise equal to each other.  `series`: the records are sorted by verr
    // (host: LaunchShape::root_series).  A second vote, on the weight of the chunk's centre in every lane's variance
    // (RootDirect::direct_ok), sends a series chunk to the direct form of the cubic: it too depends on the end records and
    // the walkers alone.  `direct`: the second vote is held (option "root_direct"); without it every series chunk keeps
    // the delta form.
    constexpr bool kCanSeries = NARROW && MODEL == MODEL_BGFIXED && !FREE;
    // `r_split` (a launch with the split exponent offset, option "exp_split"): the chunk's records in the split array, which
    // a direct chunk then reads INSTEAD of `r` -- the vote's two records included (the same verr^2 in both arrays), so that
    // such a chunk touches one array only
    // A third vote (option "root_quad"), on the widest 32-star block the chunk touches against every lane's variance
    // (RootQuad::quad_ok; split_const[1], a constant of the plan), sends a direct chunk of such a launch to the quadratic form.
    bool use_series = false, use_direct = false, use_quad = false;
    const bool split = kCanSeries && r_split != nullptr;
    if constexpr (kCanSeries) {
        if (series && count > 0) {
            RootSeries vote;                                         // (its verdict and centre only: the rest is dead code)
            const RecPtr<double> rv = split ? r_split : r;
            const bool ok = vote.setup_chunk(rv[1], rv[(int64_t)(count - 1) * ND + 1], w.s2);
            use_series = wave_all(ok);
            if (use_series && direct) use_direct = wave_all(RootDirect::direct_ok(vote.eb, w.s2));
            // (on 8 H, 8 eb and s2x = 8 s2, which the loops keep anyway: the verdict of quad_ok(H, eb, s2), since scaling by
            // a power of two rounds nothing -- the range guard keeps all three far from the ends of the exponent range)
            if (use_direct && split && quad.on)
                use_quad = wave_all(RootQuad::quad_ok(kScale * split_const[1], kScale * vote.eb, s2x));
        }
    }
    if constexpr (kCanSeries) {
        // The three copies follow one another in the kernel, each behind its own test, and whatever a later copy takes
        // over from here stays in registers across the earlier ones: a series copy therefore forms its coefficients
        // itself, from the end records and from s2x (which the rsq loops keep anyway), behind vgpr_pinned so that
        // nothing of it is shared with the vote or moves out of the copy's own branch -- the same values as the
        // vote's, bit for bit, BECAUSE s2x = 8 s2 and (1/8) s2x are exact: scaling by a power of two rounds nothing as
        // long as 8 s2 is finite (and the way back lands on s2, which is representable, subnormal or not); the range
        // guard admits no fast mixture kernel for a variance beyond 2^200 (mcd_guard.h: guard_verdict).
        if (use_quad) {
            r = r_split;
            const double e_first = vgpr_pinned(r[1]), e_last = vgpr_pinned(r[(int64_t)(count - 1) * ND + 1]);
            // (s2 itself, which the kernel keeps for its general form anyway -- the same bits as (1/8) s2x, see above -- so
            // that s2x need not stay in registers across the split copy for this one)
            qc.setup_quad(0.5 * e_first + 0.5 * e_last, vgpr_pinned((1.0 / kScale) * s2x), kExpSplitC);
#if defined(__HIP_DEVICE_COMPILE__)
            {
                const QuadParkPtr park = quad.park + (int)__builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u));
                park[0] = qc.c1;
                park[quad.stride] = qc.c2;
                park[2 * quad.stride] = qc.G0s;
                park[3 * quad.stride] = qc.A;
                park[4 * quad.stride] = qc.k3;
            }
#endif
            fold_at(r - (int64_t)quad.back * ND);                   // the block the chunk starts in (or on)
            run((const RootQuad*)&sq);
            const double result = acc.finish() + *split_const;      // (the split loop's constant: the same kappa)
            denormal = acc.denormal();
            return result;
        } else if (use_direct && split) {
            r = r_split;
            const double e_first = vgpr_pinned(r[1]), e_last = vgpr_pinned(r[(int64_t)(count - 1) * ND + 1]);
            RootDirectSplit sd;
            sd.setup_scaled(0.5 * e_first + 0.5 * e_last, vgpr_pinned((1.0 / kScale) * s2x), kExpSplitC);
            run(sd);
            // sum of log kappa over the chunk's stars, a constant of the plan (mcd_exp_split.h: exp_split_chunk_const): read
            // on this branch only, so it can never reach a chunk that ran another loop
            const double result = acc.finish() + *split_const;
            denormal = acc.denormal();
            return result;
        } else if (use_direct) {
            const double e_first = vgpr_pinned(r[1]), e_last = vgpr_pinned(r[(int64_t)(count - 1) * ND + 1]);
            RootDirect sd;
            sd.setup(0.5 * e_first + 0.5 * e_last, vgpr_pinned((1.0 / kScale) * s2x));
            run(sd);
        } else if (use_series) {
            const double e_first = vgpr_pinned(r[1]), e_last = vgpr_pinned(r[(int64_t)(count - 1) * ND + 1]);
            sr.setup_chunk(e_first, e_last, vgpr_pinned((1.0 / kScale) * s2x));
            run(std::true_type());
        }
        else run(std::false_type());
    } else {
        run(std::false_type());
    }
    const double result = acc.finish();
    denormal = acc.denormal();
    return result;
}

// One chunk of stars for one walker: selects the family.  The two f64 mixtures with two running products (BG_FIXED_DENSITY,
// BG_GAUSS) stay inline at the end: as functions of their own, hipcc issues the two frexp of their narrow-range rescale
// in the other order.
// FAST: 0 = plain (the reference's expressions term by term), 1 = fast formulation, 2 = fast formulation with the
// narrow-range products of BgFixedAcc::add (MODEL_BGFIXED, MODEL_PROFILE_BGDENS) / BgGaussAcc::add (MODEL_BGGAUSS,
// MODEL_PROFILE_BGGAUSS); for the models without background the same as 1.
// TAB_BIASED: `exptab` is the exponent-biased table (exp_tab_bias; MODEL_BGFIXED kernels with the narrow-range variant).
// BOUNDED (MODEL_BGFIXED, fixed centre, FAST == 2, PF, TAB_BIASED; host guard mcd_guard.h: bounded_rescale): the
// narrow-range loop without the exponent clamp, rescaling after every `rescale_iters` 8-star iterations (R / 8).
// BLOCK (with BOUNDED; option "block_step", host guard mcd_guard.h: block_step_admitted): the bounded quadratic loop does its
// fold, its rescale and its prefetch in one block per 32-star band (chunk_bgfixed_fast: block step); no other loop changes.
// `series` (MODEL_BGFIXED, fixed centre, FAST == 2, f64): the records are sorted by verr, so a chunk whose verr^2 band is
// narrow for every walker of the wave takes the reciprocal root from a per-chunk series (RootSeries) -- a wave-wide vote;
// with `direct` (option "root_direct") such a chunk takes the direct form of the series (RootDirect) where the chunk's
// verr^2 is at most 1/8 of every walker's variance -- a second vote.
template <int MODEL, bool FREE, class T, class A, int FAST, bool PF = false, bool TAB_BIASED = false, bool BOUNDED = false,
          bool BLOCK = false>
MCD_HD double chunk_loglike(RecPtr<T> r, int count, const WalkerConsts<T>& w, bool& denormal,
                            const double* __restrict__ exptab, int rescale_iters = 1, bool series = false, bool direct = false,
                            RecPtr<T> r_split = nullptr, const double* __restrict__ split_const = nullptr,
                            const QuadArgs& quad = QuadArgs()) {
    constexpr int BG = bg_kind(MODEL);
    denormal = false;
    if constexpr (!FAST) {
        if constexpr (BG == BG_NONE) return chunk_plain<MODEL, FREE, T, A>(r, count, w);
        else return chunk_plain_mixture<MODEL, FREE, T, A>(r, count, w);
    } else if constexpr (sizeof(T) == 4) {
        if constexpr (BG == BG_NONE) return chunk_const_f32<MODEL, FREE, A, PF>(r, count, w);
        else return chunk_mixture_f32<MODEL, FREE, A, PF>(r, count, w);
    } else if constexpr (BG == BG_NONE) {
        if constexpr (FAST == 2 && MODEL == MODEL_PROFILE && !FREE) return chunk_profile_narrow<PF>(r, count, w);
        else return chunk_const_fast<MODEL, FREE, PF>(r, count, w);
    } else if constexpr (BG == BG_FIXED) {
        return chunk_bgfixed_fast<MODEL, FREE, FAST, PF, TAB_BIASED, BOUNDED, BLOCK>(r, count, w, denormal, exptab, rescale_iters, series, direct, r_split, split_const, quad);
    } else if constexpr (BG == BG_FIXED_DENSITY) {
        // BG_FIXED_DENSITY, f64 fast forms
        constexpr int ND = record_doubles(MODEL, FREE);
        constexpr int XB = geometry_doubles(MODEL, FREE);
        constexpr bool NARROW = FAST == 2;          // f_back >= 2^-20 bounds every mixture value from below (mcd_guard.h)
        BgFixedAcc acc;
        acc.init();
        auto four = [&](RecPtr<double> r4) {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                RecPtr<double> rr = r4 + j * ND;
                double d, n;
                star_d_n<MODEL, double, FREE, true, NARROW>(rr, w, d, n);
                acc.add_density<NARROW>(d, n, rr[XB + 2], w.fb, rr[XB + 1], exptab);
            }
        };
        const int n4 = count >> 2;
        if constexpr (NARROW) {
            for (int g = 0; g < n4; ++g, r += 4 * ND) {
                RecordPrefetch<4 * ND * 8, PF> pf;
                pf.issue(r + 4 * ND);
                four(r);
                pf.retire(acc.l.p);
                if (g & 1) { MCD_KEEP_BRANCH(); acc.rescale_density_narrow(); }    // wave-uniform: a scalar branch, not a select
            }
            if (n4 & 1) acc.rescale_density_narrow();
        } else {
            for (int g = 0; g < n4; ++g, r += 4 * ND) {
                RecordPrefetch<4 * ND * 8, PF> pf;
                pf.issue(r + 4 * ND);
                four(r);
                pf.retire(acc.l.p);
                acc.rescale_density();
            }
        }
        for (int j = n4 * 4; j < count; ++j, r += ND) {
            double d, n;
            star_d_n<MODEL, double, FREE, true, NARROW>(r, w, d, n);
            acc.add_density<NARROW>(d, n, r[XB + 2], w.fb, r[XB + 1], exptab);
            acc.rescale_density();
        }
        const double result = acc.finish_density();
        denormal = acc.denormal();
        return result;
    } else {
        // BG_GAUSS, f64 fast forms.  MODEL_BGGAUSS has norm = verr^2 + sigma^2 and verr^2 + sigma_back^2: doubled norms are one
        // FMA each (HALVED form; 8 norm for the narrow-range variant's one-step Newton reciprocal roots)
        constexpr int ND = record_doubles(MODEL, FREE);
        constexpr int XB = geometry_doubles(MODEL, FREE);
        constexpr bool HALVED = MODEL == MODEL_BGGAUSS;
        constexpr bool NARROW = FAST == 2;
        constexpr double kScale = NARROW ? 8.0 : 2.0;
        const double s2x = kScale * w.s2, sb2x = kScale * w.sb2;
        BgGaussAcc acc;
        acc.init();
        auto one = [&](RecPtr<double> rr) {
            double d, n;
            star_d_n<MODEL, double, FREE, true, NARROW>(rr, w, d, n);
            if constexpr (HALVED) acc.add<true, NARROW>(d, fma_(kScale, rr[1], s2x), rr[0] - w.vb, fma_(kScale, rr[1], sb2x), rr[XB], w.fb, exptab);
            else acc.add<false, NARROW>(d, n, rr[0] - w.vb, rr[1] + w.sb2, rr[XB], w.fb, exptab);
        };
        auto four = [&](RecPtr<double> r4) {
#pragma unroll
            for (int j = 0; j < 4; ++j) one(r4 + j * ND);
        };
        const int n4 = count >> 2;
        if constexpr (NARROW) {
            for (int g = 0; g < n4; ++g, r += 4 * ND) {
                RecordPrefetch<4 * ND * 8, PF> pf;
                pf.issue(r + 4 * ND);
                four(r);
                pf.retire(acc.ly.p);
                if (g & 1) { MCD_KEEP_BRANCH(); acc.rescale_narrow(); }    // wave-uniform: a scalar branch, not a select
            }
            if (n4 & 1) acc.rescale_narrow();
        } else {
            for (int g = 0; g < n4; ++g, r += 4 * ND) {
                RecordPrefetch<4 * ND * 8, PF> pf;
                pf.issue(r + 4 * ND);
                four(r);
                pf.retire(acc.ly.p);
                acc.rescale();
            }
        }
        for (int j = n4 * 4; j < count; ++j, r += ND) {
            one(r);
            acc.rescale();
        }
        const double result = acc.finish<HALVED>(count);
        denormal = acc.denormal();
        return result;
    }
}

// Per-star log-likelihood pieces for the membership / no_sum outputs: cluster lnL, background lnL, prior m.
template <int MODEL, bool FREE, class T>
MCD_HD void star_components(RecPtr<T> r, const WalkerConsts<T>& w, T& lc, T& lb, T& m) {
    constexpr int XB = geometry_doubles(MODEL, FREE);
    constexpr int BG = bg_kind(MODEL);
    T d, n;
    star_d_n<MODEL, T, FREE>(r, w, d, n);
    lc = gauss_lnl(d, n);
    if (BG == BG_FIXED) { lb = r[XB]; m = r[XB + 1]; }
    else if (BG == BG_FIXED_DENSITY) { lb = r[XB]; const T rho = r[XB + 2]; m = rho / (rho + w.fb); }
    else if (BG == BG_GAUSS) { lb = gauss_lnl(r[0] - w.vb, r[1] + w.sb2); const T rho = r[XB]; m = rho / (rho + w.fb); }
    else { lb = T(-INFINITY); m = T(1); }
}

}  // namespace mcd

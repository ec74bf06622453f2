/*
 * mcd.h -- C-ABI of the MI355X-native log-likelihood hot path of mcmc_dynamics.
 *
 * The reference (skamann/mcmc-dynamics, pure Python) has no FFI of its own; its boundary for this
 * path is the bound method `Runner.lnprob` handed to emcee (analysis/runner.py:288-306, :403).
 * The entry points below are what a ctypes/cffi binding inside `Runner` binds to replace the
 * NumPy/astropy body of that method:
 *
 *   mcd_catalog_create   replaces the per-instance column extraction of `Runner.__init__`
 *                        (analysis/runner.py:75-81, :96-106) and the walker-independent part of
 *                        `calc_xy_offset` + `arctan2` (utils/coordinates/calc_xy_offset.py:9-33,
 *                        analysis/constant.py:106-107): star columns are copied to HBM ONCE.
 *   mcd_loglike_batch    replaces `ConstantFit.lnlike` / `ConstantFitGB.lnlike` /
 *                        `Runner._calculate_lnlike` (analysis/constant.py:113-154, :293-364;
 *                        analysis/runner.py:240-286) for W walkers per call.
 *   mcd_membership       replaces `ConstantFitGB.calculate_membership_probabilities`
 *                        (analysis/constant.py:366-374) and the ModelFit variants (analysis/model.py:458-510, 625-687).
 *
 * Conventions
 *   - plain pointers and sizes only; all arrays are float64 unless stated; canonical units of the
 *     reference: deg (ra, dec, centres), km/s (velocities), dimensionless (pmember, density, f_back).
 *   - the caller owns every host buffer; the library copies inputs during the call and never keeps
 *     a host pointer.  `out` buffers are caller-allocated.
 *   - every function returns 0 on success or a negative mcd_status; `mcd_last_error()` returns a
 *     thread-local message.  No C++ exception crosses this boundary.
 *   - results are deterministic: fixed chunking and a fixed reduction tree (no float atomics).
 */
#ifndef MCD_H
#define MCD_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MCD_ABI_VERSION 1          /* bumped when an existing signature or struct layout changes; additions keep it */
#define MCD_UNIQUE_ID_BYTES 128

typedef struct mcd_ctx mcd_ctx;          /* devices + streams (+ RCCL communicator when > 1 rank) */
typedef struct mcd_catalog mcd_catalog;  /* HBM-resident star records of one Runner instance     */

typedef enum {
    MCD_OK = 0,
    MCD_ERR_INVALID = -1,   /* bad argument (null pointer, size, enum, K mismatch)  */
    MCD_ERR_HIP = -2,       /* a HIP runtime call failed (message has the call)     */
    MCD_ERR_RCCL = -3,      /* an RCCL call failed                                  */
    MCD_ERR_NO_DEVICE = -4, /* no usable gfx950 device                              */
    MCD_ERR_NONFINITE = -5, /* a NaN log-likelihood inside mcd_stretch_move         */
    MCD_ERR_NOMEM = -6      /* host memory exhausted inside the library             */
} mcd_status;

/* which per-star likelihood the catalogue is evaluated with */
typedef enum {
    MCD_MODEL_CONST = 0,          /* ConstantFit, no background  (runner.py:264-271)                 */
    MCD_MODEL_CONST_BGFIXED = 1,  /* ConstantFit + fixed per-star background lnL and pmember
                                     (runner.py:272-286; background/gaussian.py:23-28)              */
    MCD_MODEL_CONST_BGGAUSS = 2,  /* ConstantFitGB: per-walker (v_back, sigma_back, f_back) and the
                                     `density` prior (constant.py:293-364)                          */
    MCD_MODEL_PROFILE = 3,        /* ModelFit: Lynden-Bell rotation curve + Plummer dispersion profile
                                     (analysis/model.py:93-222)                                     */
    MCD_MODEL_PROFILE_BGGAUSS = 4,/* ModelFitGB: + per-walker Gaussian background, density prior
                                     (analysis/model.py:391-456)                                    */
    MCD_MODEL_PROFILE_BGDENS = 5, /* ModelFitConstantBackground: fixed per-star background lnL, density prior
                                     with per-walker f_back (analysis/model.py:565-623)             */
    MCD_MODEL_PROFILE_BGFIXED = 6,/* ModelFit(background=Gaussian / SingleStars): the profiles of MCD_MODEL_PROFILE
                                     with the fixed per-star background lnL and pmember mixture that
                                     Runner._calculate_lnlike applies to every subclass
                                     (analysis/model.py:182-222 -> analysis/runner.py:272-286)      */
    MCD_MODEL_DOUBLE = 7,         /* DoubleModelFit: TWO Lynden-Bell components (r^2 in both denominators, so that
                                     zero second amplitudes give MCD_MODEL_PROFILE) on one Plummer dispersion profile;
                                     the second peak radius is r_peak_ratio * r_peak.  Columns: v_sys, sigma_max, a,
                                     v_maxx, v_maxy, r_peak, v_maxx_c, v_maxy_c, r_peak_ratio [, ra_center, dec_center].
                                     MCD_F64 only (mcd_catalog_create refuses the float32 precisions)            */
    MCD_MODEL_DOUBLE_BGGAUSS = 8, /* DoubleModelFitGB: + per-walker Gaussian background and density prior, as
                                     MCD_MODEL_PROFILE_BGGAUSS: [, v_back, sigma_back, f_back] behind the centre */
    /* 9 is unassigned: mcd_catalog_create answers it with "unknown model", as it always has */
    MCD_MODEL_CONST_ESCALE = 10,  /* ConstantFitES: MCD_MODEL_CONST with a fitted velocity-error scale, one per row:
                                     variance = err_scale^2 verr^2 + sigma_max^2, v_los unchanged.  Columns: v_sys,
                                     sigma_max, v_maxx, v_maxy, err_scale [, ra_center, dec_center] (K = 5 / 7).
                                     err_scale = 1 gives MCD_MODEL_CONST's bits.  No background; MCD_F64 only
                                     (mcd_catalog_create refuses the float32 precisions); no narrow-range variant */
    MCD_MODEL_PROFILE_ESCALE = 11 /* ModelFitES: MCD_MODEL_PROFILE likewise, variance = err_scale^2 verr^2 +
                                     sigma_los^2(r).  Columns: v_sys, sigma_max, a, v_maxx, v_maxy, r_peak, err_scale
                                     [, ra_center, dec_center] (K = 7 / 9)                                         */
} mcd_model;

typedef enum {
    MCD_CENTRE_FIXED = 0,  /* (ra_center, dec_center) fixed: sin/cos(theta_i) precomputed at upload */
    MCD_CENTRE_FREE = 1    /* centre is a walker parameter: geometry recomputed per term            */
} mcd_centre;

typedef enum {
    MCD_F64 = 0,        /* float64 terms, float64 accumulation (parity mode)      */
    MCD_F32 = 1,        /* float32 terms, float32 accumulation                     */
    MCD_F32_ACC64 = 2   /* float32 terms, float64 accumulation                     */
} mcd_precision;

/* Catalogue description.  Pointers not needed by `model` may be NULL. */
typedef struct {
    int64_t n_stars;
    const double* ra;         /* deg  */
    const double* dec;        /* deg  */
    const double* v;          /* km/s */
    const double* verr;       /* km/s */
    const double* lnlike_bg;  /* CONST_BGFIXED, PROFILE_BGFIXED, PROFILE_BGDENS: background(v, verr) per star */
    const double* pmember;    /* CONST_BGFIXED, PROFILE_BGFIXED: prior membership probability      */
    const double* density;    /* *_BGGAUSS, PROFILE_BGDENS: normalised stellar surface density     */
    int32_t model;            /* mcd_model     */
    int32_t centre;           /* mcd_centre    */
    int32_t precision;        /* mcd_precision */
    int32_t reserved;
    double ra_center;         /* deg; used when centre == MCD_CENTRE_FIXED                         */
    double dec_center;        /* deg                                                               */
    int64_t n_bins;           /* 0 or 1: one parameter set for all stars.  B > 1: radial bins
                                 (utils/files/data_reader.py:71-140); stars must be sorted by bin   */
    const int64_t* bin_offsets; /* n_bins + 1 offsets into the star arrays when n_bins > 1        */
} mcd_catalog_desc;

/* ---- context ------------------------------------------------------------------------------ */

/* Single process driving n_dev devices (dev_ids == NULL: devices 0..n_dev-1).  With n_dev > 1 the
 * catalogue is sharded over the devices and per-walker partial sums are combined with one
 * ncclAllReduce(sum, f64, count = outputs) per batched call (communicator from ncclCommInitAll). */
/* MCD_FORCE_RCCL=1 in the environment: a one-device context also creates its communicator with ncclCommInitAll and
 * runs the all-reduce inside ncclGroupStart/End (lets a single-GPU box exercise the call sequence of this mode). */
int mcd_ctx_create(int n_dev, const int* dev_ids, mcd_ctx** out);

/* One process per GPU (torchrun-style).  Rank 0 calls mcd_get_unique_id and distributes the
 * MCD_UNIQUE_ID_BYTES blob out of band; every rank then calls mcd_ctx_create_rank.  Each rank
 * uploads ITS shard of the stars; mcd_loglike_batch all-reduces so every rank gets the total.
 * n_ranks == 1 needs no id (unique_id may be NULL) and never touches RCCL -- unless the environment
 * variable MCD_FORCE_RCCL=1 is set and an id is given: then a 1-rank communicator is created and the
 * all-reduce runs on it (lets a single-GPU box exercise the RCCL call path). */
int mcd_get_unique_id(void* out_id);
int mcd_ctx_create_rank(int device, int rank, int n_ranks, const void* unique_id, mcd_ctx** out);

/* ---- collective deadline (contexts with a communicator; nothing equivalent in the reference, whose only parallelism
 * is the process pool of analysis/runner.py:398-403) -------------------------------------------------------------
 * Every wait on a stream that carries an all-reduce (mcd_loglike_batch / _fetch, mcd_sync, mcd_stretch_move) polls
 * instead of blocking: after `collective_timeout_ms` (option below; default 120000, 0 = wait for ever; the environment
 * variable MCD_COLLECTIVE_TIMEOUT_MS sets the default of new contexts) the call returns MCD_ERR_RCCL with the stage in
 * mcd_last_error(), and the context is marked FAILED: every later call on it (and on its catalogues) returns
 * MCD_ERR_RCCL at once, and the destroy functions no longer synchronise the blocked streams (they would never
 * return) -- the process is expected to report and exit non-zero.  There is no fallback inside the process.
 *
 * mcd_ctx_abort may be called from ANOTHER host thread while a call is waiting (e.g. by the host application's own
 * control channel when a peer rank reports that it failed): the waiting call returns MCD_ERR_RCCL within a
 * millisecond instead of running into the deadline.  This is how a rank that fails in the middle of a block of
 * mcd_stretch_move keeps its peers from waiting inside the collective (mcmc_dynamics_amd/hostgroup.py: abort). */
int mcd_ctx_set_option(mcd_ctx* ctx, const char* key, int64_t value);   /* "collective_timeout_ms" */
int mcd_ctx_abort(mcd_ctx* ctx, const char* reason);                    /* thread-safe; reason may be NULL */
int mcd_ctx_failed(const mcd_ctx* ctx);                                 /* 1 after a deadline / abort / mid-block error */

int mcd_ctx_destroy(mcd_ctx* ctx);
int mcd_ctx_n_devices(const mcd_ctx* ctx);
/* What RCCL itself reports for the communicator of the context's first device: ncclCommCount, ncclCommUserRank and
 * ncclGetVersion (e.g. 22707).  comm_size = 0 / comm_rank = -1 when the context has no communicator (single device:
 * RCCL is never loaded).  A measurement harness echoes these to prove the collective really spans N ranks. */
int mcd_ctx_comm_info(const mcd_ctx* ctx, int* comm_size, int* comm_rank, int* rccl_version);

/* ---- catalogue ---------------------------------------------------------------------------- */

int mcd_catalog_create(mcd_ctx* ctx, const mcd_catalog_desc* desc, mcd_catalog** out);
int mcd_catalog_destroy(mcd_catalog* cat);

/* Number of columns K of the resolved parameter table expected by mcd_loglike_batch:
 *   CONST    : v_sys, sigma_max, v_maxx, v_maxy [, ra_center, dec_center]
 *   *_BGGAUSS: ... + v_back, sigma_back, f_back
 *   PROFILE, PROFILE_BGFIXED: v_sys, sigma_max, a, v_maxx, v_maxy, r_peak [, ra_center, dec_center] (a, r_peak in arcsec)
 *   PROFILE_BGGAUSS: ... + v_back, sigma_back, f_back        PROFILE_BGDENS: ... + f_back
 *   DOUBLE: v_sys, sigma_max, a, v_maxx, v_maxy, r_peak, v_maxx_c, v_maxy_c, r_peak_ratio [, ra_center, dec_center]
 *   DOUBLE_BGGAUSS: ... + v_back, sigma_back, f_back          (K = 9, 11, 12 or 14; r_peak_ratio is dimensionless)
 * (order of config/constant.json:6-11, constant_with_background.json:6-14, model_with_background.json:6-16;
 * config/model.json interleaves the centre between v_maxx and v_maxy -- the host maps columns by name). */
int mcd_catalog_param_count(const mcd_catalog* cat);
int64_t mcd_catalog_n_stars(const mcd_catalog* cat);      /* stars held by THIS process */
int64_t mcd_catalog_n_outputs(const mcd_catalog* cat, int64_t n_walkers); /* W * max(1, n_bins) */

/* ---- evaluation --------------------------------------------------------------------------- */

/* Log-likelihood of W walkers.  params: row-major [max(1,n_bins)][W][K]; out: [max(1,n_bins)][W].
 * Synchronous: H2D of params, kernels, reduction, (all-reduce), D2H of out. */
int mcd_loglike_batch(mcd_catalog* cat, int64_t n_walkers, int32_t k, const double* params, double* out);

/* Device-resident pipeline used by throughput measurements and by callers that keep walkers on the
 * GPU: stage params once, enqueue any number of evaluations, fetch the last result. */
int mcd_params_upload(mcd_catalog* cat, int64_t n_walkers, int32_t k, const double* params);
int mcd_loglike_enqueue(mcd_catalog* cat);                 /* asynchronous on the catalogue's stream(s) */
int mcd_loglike_fetch(mcd_catalog* cat, double* out);      /* waits, copies [max(1,n_bins)][W] doubles    */
int mcd_sync(mcd_catalog* cat);

/* Posterior membership probability per star for ONE parameter row (BGGAUSS models):
 * m e^{lc} / (m e^{lc} + (1 - m) e^{lb}); out has n_stars doubles (this process' shard). */
int mcd_membership(mcd_catalog* cat, int32_t k, const double* params, double* out);
/* Per-star mixture log-likelihood for ONE parameter row, `lnlike(values, no_sum=True)` of
 * ModelFitConstantBackground (analysis/model.py:565-623); defined for every background model. */
int mcd_loglike_per_star(mcd_catalog* cat, int32_t k, const double* params, double* out);
/* Log-likelihood AND its gradient with respect to the K kernel columns (units of the kernel: km/s, arcsec for a and
 * r_peak, degrees for the centre).  params [max(1,B)][W][K]; out [max(1,B)][W] (may be NULL); grad [max(1,B)][W][K].
 * out equals mcd_loglike_batch with option "fast_path" = 0 to rounding.  A star exactly on a walker's free centre
 * contributes 0 to the centre columns of the constant-rotation models (theta is undefined there).  float64 catalogues only
 * (MCD_ERR_INVALID otherwise).  Synchronous, deterministic (fixed-order sums: bit-identical from run to run); device and
 * rank shards are summed by one all-reduce of the 1 + K fields under the collective deadline.  Honours option "timing"
 * (mcd_last_kernel_ms: the gradient kernel, as the main kernel for values). */
int mcd_loglike_grad_batch(mcd_catalog* cat, int64_t n_walkers, int32_t k, const double* params, double* out,
                           double* grad);
/* Per-star summaries over S posterior samples (params: row-major [S][K], the kernel columns of mcd_loglike_batch).
 * lppd[i]    = log( (1/S) sum_s exp(lnL_is) )      lnl_var[i] = sample variance (S-1) of lnL_is (0 when S == 1)
 * pmem_mean[i], pmem_std[i]: mean and standard deviation (S-1; 0 when S == 1) of the membership probability
 * lnL_is is the star's term of lnlike (the mixture for background models), so sum_i lppd_i == lnlike(row) when S == 1.
 * Any output pointer may be NULL (not computed); pmem_* must be NULL for models without a background.
 * Un-binned catalogues only; out arrays hold this process' n_stars; synchronous.  The pointwise terms of WAIC (Watanabe;
 * Gelman, Hwang & Vehtari 2014) and the posterior mean of the membership probability of mcd_membership.  The samples
 * reach the device in passes of at most 65536 rows (catalogue option "posterior_pass"); deterministic: no atomics, and
 * the partial states of sample slices are merged in a fixed order.  With option "timing" on, mcd_last_kernel_ms gives
 * the HIP-event time of the kernels (walker prep, slice and merge kernels of every pass, summed over the shards). */
int mcd_pointwise_posterior(mcd_catalog* cat, int64_t n_samples, int32_t k, const double* params,
                            double* lppd, double* lnl_var, double* pmem_mean, double* pmem_std);
/* Pareto-smoothed importance-sampling leave-one-out cross-validation per star over S posterior samples (params:
 * row-major [S][K], the kernel columns of mcd_loglike_batch), as psis() / loo() of the R package loo state it (Vehtari,
 * Gelman & Gabry 2017): log ratios r_s = -lnL_is (lnL_is as in mcd_pointwise_posterior), a generalized Pareto fit to the
 * M = min(ceil(0.2 S), ceil(3 sqrt(S / r_eff))) largest, smoothed and truncated weights.
 * elpd_loo[i] = log sum_s w_s exp(lnL_is) / sum_s w_s     pareto_k[i] = the fitted shape k^ (+inf when M < 5 or the fit
 * fails; -inf when the tail is constant -- loo says +inf there)     lppd[i] as mcd_pointwise_posterior computes it (to
 * rounding)     n_eff[i] = r_eff / sum_s w~_s^2 (normalised weights).
 * Any output pointer may be NULL.  r_eff > 0 (MCD_ERR_INVALID otherwise); M <= 2560 (S / r_eff up to ~7.3e5).
 * Un-binned catalogues only; out arrays hold this process' n_stars; synchronous.  Device scratch (the sample table and a
 * tile of [star][S] float64 terms) stays within catalogue option "loo_scratch_mb" (default 2048) and is released on
 * every exit path; the samples reach the device in passes of "posterior_pass" rows.  Deterministic: no floating-point
 * atomics, fixed reduction orders, and a star's result depends on its own terms only (not on tiles, shards or ranks).
 * With option "timing" on, mcd_last_kernel_ms gives the HIP-event time of the kernels (sample prep, term and tail
 * kernels of every tile, summed over the shards). */
int mcd_psis_loo(mcd_catalog* cat, int64_t n_samples, int32_t k, const double* params, double r_eff,
                 double* elpd_loo, double* pareto_k, double* lppd, double* n_eff);
/* Per-star posterior predictive checks over S posterior samples (params: row-major [S][K], the kernel columns of
 * mcd_loglike_batch).  With d = v_i - v_los,is and n = verr_i^2 + sigma_los,is^2 of star i under sample s:
 *   z = d / sqrt(n)   t = erfc(|z| / sqrt 2)   pit = Phi(z) (the cluster component's CDF at v_i)
 * out[f][i], f < MCD_PRED_FIELDS: mean and standard deviation (S-1; 0 when S == 1) over the samples of z, the means of t
 * (MCD_PRED_TAIL_P) and pit, mean and standard deviation of the model's v_los (v_sys included) and of sigma_los.
 * pit_mix[i] (may be NULL; MODEL_BGGAUSS / MODEL_PROFILE_BGGAUSS only, MCD_ERR_INVALID for any other model): the mean of
 * m pit + (1 - m) Phi((v_i - v_back) / sqrt(verr_i^2 + sigma_back^2)), m = density_i / (density_i + f_back), the CDF of
 * the whole mixture at v_i.  A star whose term is not finite (sigma_los = 0 with verr = 0) gets non-finite outputs; that
 * is no error and touches no other star.  Un-binned catalogues only; `out` must not be NULL; the arrays hold this
 * process' n_stars; synchronous; an MCD_ERR_INVALID call leaves the outputs untouched.  float32 catalogues: terms in
 * float, everything else in float64.  Samples reach the device in passes of "posterior_pass" rows; deterministic: no
 * atomics, partial states of sample slices merged in a fixed order.  With option "timing" on, mcd_last_kernel_ms gives the
 * HIP-event time of the kernels as for mcd_pointwise_posterior. */
enum { MCD_PRED_Z_MEAN, MCD_PRED_Z_STD, MCD_PRED_TAIL_P, MCD_PRED_PIT,
       MCD_PRED_VLOS_MEAN, MCD_PRED_VLOS_STD, MCD_PRED_SIGMA_MEAN, MCD_PRED_SIGMA_STD, MCD_PRED_FIELDS };
int mcd_posterior_predictive(mcd_catalog* cat, int64_t n_samples, int32_t k, const double* params,
                             double* out      /* [MCD_PRED_FIELDS][n_stars] */,
                             double* pit_mix  /* [n_stars], or NULL */);
/* Leave-one-out expectations per star under the PSIS weights of mcd_psis_loo (same params, r_eff, tail rules and
 * smoothing): with lw_is the smoothed, truncated log weights and w~_is = exp(lw_is) / sum_s exp(lw_is),
 *   E_loo,i[x] = sum_s w~_is x_is,
 * accumulated as sum_s e_s x_s / sum_s e_s with e_s = exp(lw_s - max lw) in sample order per lane, then over the wave.
 * loo_pred[f][i], f < MCD_LOOX_FIELDS: the expectations of pit, z, v_los and sigma_los of mcd_posterior_predictive's
 * (star, sample) term -- loo_pred[MCD_LOOX_PIT] is the leave-one-out probability integral transform (LOO-PIT);
 * loo_pit_mix[i] that of the mixture CDF (Gaussian-background models only, MCD_ERR_INVALID otherwise).
 * loo_func[q][i] = sum_s w~_is func[s][q] for n_func <= MCD_LOO_MAX_FUNC star-independent functions of the sample
 * (func row-major [S][n_func]): with func = the parameters, the case-deletion posterior means E[theta | y_-i].
 * pareto_k / n_eff: bit for bit those of mcd_psis_loo.  Every output pointer may be NULL; all NULL is MCD_OK without
 * work.  n_func outside [0, MCD_LOO_MAX_FUNC], or func / loo_func NULL with n_func > 0, is MCD_ERR_INVALID; an invalid
 * call leaves the outputs untouched.  M < 5, a failed fit and a constant tail keep the raw truncated weights; S = 1
 * gives w~ = 1.  A star with non-finite terms gets non-finite outputs and touches no other star.  Un-binned catalogues
 * only; this process' n_stars; synchronous; float32 catalogues: terms in float, everything else in float64.  Device
 * scratch ([star][rows][S] tiles with rows = 1 + the rows asked for, the sample table and func) stays within option
 * "loo_scratch_mb" and is released on every exit path; options "posterior_pass" and "timing" as for mcd_psis_loo.
 * Deterministic: no floating-point atomics; a star's bits depend on its own rows only. */
enum { MCD_LOOX_PIT, MCD_LOOX_Z, MCD_LOOX_VLOS, MCD_LOOX_SIGMA, MCD_LOOX_FIELDS };
#define MCD_LOO_MAX_FUNC 16
int mcd_psis_loo_expect(mcd_catalog* cat, int64_t n_samples, int32_t k, const double* params, double r_eff,
                        int32_t n_func, const double* func  /* [S][n_func] row-major, or NULL when n_func == 0 */,
                        double* loo_func     /* [n_func][n_stars], or NULL */,
                        double* loo_pred     /* [MCD_LOOX_FIELDS][n_stars], or NULL */,
                        double* loo_pit_mix  /* [n_stars] or NULL; Gaussian-background models only */,
                        double* pareto_k, double* n_eff  /* [n_stars] or NULL each */);
/* Exact leave-out refits: E ensembles that each leave out their own set of stars share ONE evaluation of the catalogue.
 * Hold-out sets: set_offsets[n_sets + 1], non-decreasing, set_offsets[0] = 0, set_offsets[n_sets] <= n_stars; set e is the
 * stars [set_offsets[e], set_offsets[e + 1]) in catalogue order (the caller orders the stars so), the stars from
 * set_offsets[n_sets] on belong to no set, a set may be empty.  With l_i(theta) the star's plain term (what
 * mcd_loglike_per_star returns) and rows theta[e][w] (params: row-major [E][W][K], the kernel columns of mcd_loglike_batch):
 *   train[e][w] = sum of l_i over the stars outside set e      test[e][w] = sum of l_i over set e (+0.0 for an empty set)
 * train + test equals mcd_loglike_batch with option "fast_path" = 0 to rounding.  Every row meets every star once; the
 * chunk sums are added per star range in a fixed order and `train` is the sum of the other ranges' sums in ascending
 * order -- no difference of two sums is formed.  `test` may be NULL.  Synchronous and deterministic: bit-identical from run
 * to run, independent of earlier calls.  The plan of (set_offsets, E W) and its buffers stay with the catalogue.
 * MCD_ERR_INVALID, with a message and nothing written: a binned or a float32 catalogue; several devices or a
 * communicator; invalid offsets; n_sets < 1; E W > 65536; a foreign k; range sums ((n_sets + 1) x roundup64(E W) x 8
 * bytes) beyond 256 MiB.  Waits under the context's deadline; honours option "timing" (mcd_last_kernel_ms: the main kernel). */
int mcd_holdout_loglike(mcd_catalog* cat, int32_t n_sets, const int64_t* set_offsets, int64_t n_walkers, int32_t k,
                        const double* params /* [E][W][K] */, double* train /* [E][W] */,
                        double* test /* [E][W], may be NULL */);
/* ... and the closing step: for star i of set e and that set's S sample rows (params: row-major [E][S][K]),
 *   lppd[i] = log( (1/S) sum_s exp(l_i(theta[e][s])) )      lnl_var[i] = sample variance (S-1) of l_i (0 when S == 1)
 * with the accumulators and merge rules of mcd_pointwise_posterior on the set's star range: one set that covers the
 * catalogue gives that call's bits.  Outputs hold set_offsets[n_sets] stars; either may be NULL.  Refusals as above
 * (without the row cap); samples go up in passes of "posterior_pass" rows; synchronous, deterministic, honours "timing". */
int mcd_holdout_pointwise(mcd_catalog* cat, int32_t n_sets, const int64_t* set_offsets, int64_t n_samples, int32_t k,
                          const double* params /* [E][S][K] */, double* lppd /* [set_offsets[E]] */,
                          double* lnl_var /* may be NULL */);
/* Replicated-data predictive checks per range of stars (Gelman, Meng & Stern 1996).  For sample row s (params: row-major
 * [S][K], the kernel columns of mcd_loglike_batch) and star i (index in catalogue order), with d, n as for
 * mcd_posterior_predictive:  z_obs = d / sqrt(n), and a replicate drawn from the model at that row:
 *   g = the standard normal, u = the uniform of (seed, s, i) (mcd_replicate_numbers gives both)
 *   z_rep = g                                   when the model has no background, or u < m, the model's membership prior
 *         = ((mu_b - v_i) + d + sqrt(verr_i^2 + sigma_b^2) g) / sqrt(n)      otherwise (a background star)
 * with m = pmember_i or density_i / (density_i + f_back) and (mu_b, sigma_b) = the row's (v_back, sigma_back) for the
 * Gaussian-background models, (bg_mean, bg_sigma) for the fixed-background ones (ignored otherwise; NaN: none).
 * Ranges: order[range_offsets[n_ranges]] holds the stars of range 0, then of range 1, ...: range r is
 * order[range_offsets[r] .. range_offsets[r + 1]); stars in no range are absent; a range may be empty (all +0.0).
 * out[s][r][f][0 / 1], f < MCD_REP_FIELDS, for z = z_obs / z_rep over the stars of range r: sum z, z^2, z^3, z^4,
 * sum z sin(theta), sum z cos(theta) (theta: the position angle the model's v_los uses), max |z|, the count of |z| > 3.
 * A replicate is a function of (seed, s + option "replicate_row0", i) alone: ranges, chunking and passes never change
 * it.  A non-finite term makes that row's fields of that range non-finite and touches nothing else.  Synchronous and
 * deterministic: a range's chunk sums are combined in a fixed order, bit-identical from run to run and independent of
 * earlier calls.  Rows beyond 65536 run in passes.  MCD_ERR_INVALID, with a message and nothing written: a binned or a
 * float32 catalogue; several devices or a communicator; offsets that do not start at 0 or decrease; an index in `order`
 * out of range or repeated; a fixed-background model without finite bg_mean and bg_sigma >= 0; n_samples < 1; a foreign
 * k; more ranges than the 256 MiB of partial sums allow.  Waits under the context's deadline; honours option "timing"
 * (mcd_last_kernel_ms: the main kernel, summed over the passes) and option "chunk_len" (a forced nominal chunk length). */
enum { MCD_REP_S1, MCD_REP_S2, MCD_REP_S3, MCD_REP_S4, MCD_REP_SIN, MCD_REP_COS, MCD_REP_MAX, MCD_REP_TAIL3, MCD_REP_FIELDS };
int mcd_replicate_check(mcd_catalog* cat, int64_t n_samples, int32_t k, const double* params /* [S][K] */,
                        uint64_t seed, int32_t n_ranges, const int64_t* range_offsets /* [R+1] */,
                        const int64_t* order /* [range_offsets[R]] */, double bg_mean, double bg_sigma /* NaN: none */,
                        double* out /* [S][R][MCD_REP_FIELDS][2]: observed, replicated */);
/* The generator's numbers for sample rows sample0 .. and stars star0 ..: g, u row-major [S][N]; either may be NULL.
 * Host only, as mcd_chain_numbers. */
int mcd_replicate_numbers(uint64_t seed, int64_t sample0, int64_t n_samples, int64_t star0, int64_t n_stars,
                          double* g /* [S][N] */, double* u /* [S][N] */);

/* Weighted log-likelihood and gradient: every parameter row sees the catalogue under its own star weights (the
 * nonparametric and the weighted-likelihood bootstrap: Rubin 1981; Newton & Raftery 1994; Lyddon, Holmes & Walker 2019).
 * With l_i(theta) the star's plain term (what mcd_loglike_per_star returns), rows theta[r] (params: row-major [R][K], the
 * kernel columns of mcd_loglike_batch) and b = row_replicate[r], the replicate of row r:
 *   out[r] = sum_i w(b, i) l_i(theta[r])        grad[r][k] = sum_i w(b, i) dl_i/dtheta_k(theta[r])
 * the terms and partial derivatives of mcd_loglike_grad_batch, added per chunk in star order and over the chunks in a
 * fixed order.  Several rows may share a replicate.  The weights, by `scheme`:
 *   MCD_WEIGHT_EXPONENTIAL  w = -log(u), Exp(1);  MCD_WEIGHT_POISSON  w = the Poisson(1) count whose cumulative
 *     probabilities bracket u: both generated on the device from (seed, replicate, star) alone, star = the index in
 *     catalogue order; u = ((x >> 11) + 0.5) 2^-53 of the generator word x (mcd_bootstrap_weights gives the same
 *     numbers on the host, bit for bit).  Replicate ids are any non-negative int64: neither ordered nor dense.
 *   MCD_WEIGHT_EXPLICIT     w = weights[b][i] (row-major [n_replicates][n_stars], finite and >= 0); row_replicate
 *     indexes its rows.  Every call checks the array and fingerprints its contents; the transposed copy on the device is
 *     kept with the catalogue while (n_replicates, fingerprint) stand -- keyed by contents, never by address.
 * Weights are NOT normalised: their sum over the stars is about n_stars, not n_stars (the Newton-Raftery form).
 * A star of weight 0 is selected out, not multiplied: it adds exactly +0.0 to every field of that row, even where its
 * term is not finite.  Either output may be NULL; both NULL is MCD_OK without work.  Synchronous and deterministic:
 * bit-identical from run to run, independent of earlier calls, and a generated weight does not depend on the chunk plan.
 * MCD_ERR_INVALID, with a message and nothing written: a binned or a float32 catalogue; several devices or a communicator;
 * a foreign k; n_rows < 1 or > 65536; an unknown scheme; row_replicate NULL or negative; for MCD_WEIGHT_EXPLICIT an index
 * outside [0, n_replicates), weights NULL, a negative or non-finite weight, n_replicates x n_stars x 8 bytes beyond
 * 256 MiB.  The work buffers of a row count stay with the catalogue.  Waits under the context's deadline; honours
 * option "timing" (mcd_last_kernel_ms: the main kernel) and option "chunk_len". */
enum { MCD_WEIGHT_EXPONENTIAL = 0, MCD_WEIGHT_POISSON = 1, MCD_WEIGHT_EXPLICIT = 2 };
typedef struct {
    int32_t scheme;                /* MCD_WEIGHT_* */
    uint64_t seed;                 /* generated schemes */
    int64_t n_replicates;          /* MCD_WEIGHT_EXPLICIT: rows of `weights`; ignored otherwise */
    const int64_t* row_replicate;  /* [n_rows] */
    const double* weights;         /* MCD_WEIGHT_EXPLICIT: [n_replicates][n_stars]; NULL otherwise */
} mcd_weight_desc;
int mcd_weighted_loglike_grad(mcd_catalog* cat, int64_t n_rows, int32_t k, const double* params /* [R][K] */,
                              const mcd_weight_desc* w, double* out /* [R], may be NULL */,
                              double* grad /* [R][K], may be NULL */);
/* The weighted log-likelihood alone: out[r] = sum_i w(row_replicate[r], i) l_i(theta[r]), for callers that read no
 * gradient (a stretch-move chain under bootstrap weights: the bagged posterior).  mcd_weighted_loglike_grad with
 * grad = NULL computes the same sums through the gradient kernel, 1 + K of them per row; this call runs a kernel that
 * carries one.  The term is mcd_loglike_per_star's, the weights and their selection rule are those above (same
 * descriptor, same generator, same explicit table: one table is kept per catalogue, whichever of the two calls uploaded
 * it).  The two calls agree to rounding; equal bits are not promised (the gradient kernel's value comes out of its own term).
 * Refusals as above, under this call's name, with nothing written; out = NULL is MCD_OK without work.  Synchronous and
 * deterministic, independent of earlier calls; the work buffers of a row count stay with the catalogue, in a cache apart
 * from the gradient call's.  Waits under the context's deadline; honours options "timing" and "chunk_len". */
int mcd_weighted_loglike(mcd_catalog* cat, int64_t n_rows, int32_t k, const double* params /* [R][K] */,
                         const mcd_weight_desc* w, double* out /* [R], may be NULL */);
/* The generated weights of replicates rep0 .. and stars star0 .., row-major [n_reps][n_stars], for a generated scheme.
 * Host only, as mcd_replicate_numbers. */
int mcd_bootstrap_weights(int32_t scheme, uint64_t seed, int64_t rep0, int64_t n_reps, int64_t star0, int64_t n_stars,
                          double* w /* [n_reps][n_stars] */);

/* Simulated catalogues, resident on the device: every parameter row sees the catalogue with the velocities of its own
 * simulation (simulation-based calibration: Cook, Gelman & Rubin 2006; Talts et al. 2018; injection-recovery).  Positions
 * and verr stay the observed ones; only the velocities are replaced, by a set of n_sims velocity columns kept on the
 * catalogue's device.
 * mcd_simulate draws simulation sim0 + e at the truth row truths[e] (row-major [E][K], the kernel columns of
 * mcd_loglike_batch).  For star i (index in catalogue order), with (d*, n*) of that row as for mcd_posterior_predictive and
 * g, u the numbers of mcd_replicate_check's stream at (seed, sim0 + e, i) (mcd_replicate_numbers gives both, bit for bit):
 *   v' = (v_i - d*) + sqrt(n*) g                         the model has no background, or u < m* (a cluster star)
 *      = mu_b + sqrt(verr_i^2 + sigma_b^2) g             otherwise (a background star)
 * with m* and (mu_b, sigma_b) as for mcd_replicate_check: the truth row's membership prior and (v_back, sigma_back), or
 * (bg_mean, bg_sigma) for the fixed-background models (ignored otherwise; NaN: none).  A velocity is a function of
 * (seed, sim0 + e, i, truth row) alone: n_sims, the chunk plan and the launch shape never change it.  The set stays
 * resident and replaces the previous one; with `velocities` it is also copied back, row-major [E][n_stars].  A non-finite
 * generated velocity (a truth row outside the model's domain) is MCD_ERR_NONFINITE: the message names the first
 * (simulation, star), and no set is left resident.
 * mcd_simulated_set makes the caller's own velocities (row-major [E][n_stars], finite) the resident set, with the
 * (bg_mean, bg_sigma) the fixed-background models evaluate them under.
 * mcd_simulated_loglike: out[r] = sum_i l_i(theta[r]; v'(row_sim[r], i)), l_i the star's plain term (what
 * mcd_loglike_per_star returns) with v' in place of v_i, added per chunk in star order and over the chunks in a fixed
 * order.  The background term of the fixed-background models is the Gaussian (bg_mean, bg_sigma) of the set at v'; the
 * catalogue's lnlike_bg column, which belongs to the observed velocities, is not read.  A set that holds the observed
 * velocities gives mcd_loglike_per_star's sum for the other families.  Several rows may share a simulation; out = NULL is
 * MCD_OK without work.  Synchronous and deterministic: given the resident set, bit-identical from run to run.
 * mcd_simulated_info: the simulations of the resident set, 0 when there is none.
 * MCD_ERR_INVALID, with a message, nothing written and the resident set untouched: a binned or a float32 catalogue;
 * several devices or a communicator; a foreign k; n_sims < 1; sim0 < 0; n_sims x n_stars x 8 bytes beyond 1 GiB; n_rows
 * < 1 or > 65536; no resident set; a row_sim outside [0, n_sims); a fixed-background model without finite bg_mean and
 * bg_sigma >= 0; a non-finite explicit velocity.  A set is released with the catalogue.  All three wait under the
 * context's deadline and honour option "timing" (mcd_last_kernel_ms: the main kernel) and option "chunk_len". */
int mcd_simulate(mcd_catalog* cat, int64_t n_sims, int32_t k, const double* truths /* [E][K] */, uint64_t seed, int64_t sim0,
                 double bg_mean, double bg_sigma /* NaN: none */, double* velocities /* [E][n_stars], may be NULL */);
int mcd_simulated_set(mcd_catalog* cat, int64_t n_sims, const double* velocities /* [E][n_stars] */, double bg_mean,
                      double bg_sigma);
int mcd_simulated_loglike(mcd_catalog* cat, int64_t n_rows, int32_t k, const double* params /* [R][K] */,
                          const int64_t* row_sim /* [R] */, double* out /* [R], may be NULL */);
int mcd_simulated_info(const mcd_catalog* cat, int64_t* n_sims);
/* mcd_simulated_loglike with its gradient (MAP fits of simulated catalogues: the parametric bootstrap, a simulated null
 * distribution of a likelihood-ratio statistic): out[r] as above, and
 *   grad[r][k] = sum_i dl_i/dtheta_k(theta[r]; v'(row_sim[r], i))
 * with respect to the K kernel columns, in their units (as mcd_loglike_grad_batch; the partials of the residual and of the
 * variance do not depend on the velocity).  out[r] has mcd_simulated_loglike's bits.  Un-binned MCD_F64 catalogues, one
 * device, no communicator.  MCD_ERR_INVALID, with a message, out and grad untouched and the resident set as it was: the
 * refusals of mcd_simulated_loglike, and a null grad.  out = NULL gives the same gradient.  Synchronous and deterministic:
 * given the resident set, bit-identical from run to run.  The work buffers of a row count stay with the catalogue, in a
 * cache apart from the value call's.  Waits under the context's deadline; honours options "timing" (mcd_last_kernel_ms:
 * the main kernel) and "chunk_len". */
int mcd_simulated_loglike_grad(mcd_catalog* cat, int64_t n_rows, int32_t k, const double* params /* [R][K] */,
                               const int64_t* row_sim /* [R] */, double* out /* [R], may be NULL */,
                               double* grad /* [R][K] */);

/* Background log-likelihood of n test stars against the kernel-density estimate built from n_comp comparison
 * stars: replaces background.SingleStars.__call__ (background/single_stars.py:42-77), the O(n * n_comp) precompute
 * whose output is the `lnlike_bg` column of a MCD_MODEL_CONST_BGFIXED / _PROFILE_BGDENS catalogue (runner.py:96-106).
 *   out_i = log( (1 / n_comp) sum_j N(v_i - comp_j; verr_i^2 + sigma_int^2) ),   all velocities in km/s.
 * Runs on the first device of `ctx`; host buffers in, n doubles out; synchronous.  n = 0 is a no-op; n_comp = 0 is
 * MCD_ERR_INVALID (the reference raises on the empty maximum). `kernel_ms`, if not NULL, receives the HIP-event time
 * of the two kernels. */
int mcd_kde_background(mcd_ctx* ctx, int64_t n_comp, const double* comp, int64_t n, const double* v,
                       const double* verr, double sigma_int, double* out, double* kernel_ms);

/* ---- sampler support ---------------------------------------------------------------------- */

/* One block of affine-invariant stretch-move steps with the per-half-step host loop inside the library: proposals from
 * the complementary half of the ensemble, box prior, ONE mcd_loglike_batch of n_walkers / 2 rows, accept / reject.
 * Replaces the Python loop around `Runner.lnprob` that emcee's EnsembleSampler runs for the reference
 * (analysis/runner.py:403-419; prior: runner.py:182-217, parameter.py:684-705) when the prior is a box, as in the shipped
 * parameter files.  All random numbers are the caller's, in the layout of mcmc_dynamics_amd/sampler.py:
 *   order [n_steps][W]       permutation of 0..W-1 per step: first half = order[:W/2], second = order[W/2:]
 *   zz    [n_steps][2][W/2]  stretch factors z ~ g(z), thr [n_steps][2][W/2] = log(u) - (n_dim - 1) log(z)
 *   pick  [n_steps][2][W/2]  partner index into the complementary half
 * pos [W][n_dim] and lnp [W] are updated in place; chain [n_steps][W][n_dim], lnprob_chain [n_steps][W] (either may be
 * NULL) receive the state after every step; accepted [W] (may be NULL) is incremented.  The chain is bit-identical to the
 * one the Python loop produces from the same numbers.  Returns MCD_ERR_NONFINITE when the likelihood produced a NaN (emcee
 * raises "Probability function returned NaN").
 *
 * Binned catalogues (desc->n_bins = B = the catalogue's number of radial bins): B independent ensembles, one per bin --
 * the reference runs one MCMC per bin (bin/run_tests.py:75-124) -- advance in lockstep and share every evaluation (one
 * launch of B x W/2 rows per half step).  Every array gains a bin dimension in front of the walker dimension:
 * pos [B][W][n_dim], lnp [B][W], accepted [B][W], order [n_steps][B][W], zz / thr / pick [n_steps][2][B][W/2],
 * chain [n_steps][B][W][n_dim], lnprob_chain [n_steps][B][W]; prior bounds and column map are shared by the bins.
 *
 * Where it runs.  A float64 catalogue on one device per process (single GPU, or one rank of a multi-process job) keeps
 * the ensemble RESIDENT on the device for the block: positions, log-probabilities and the block's random numbers are
 * uploaded once, one small kernel per half step accepts / rejects the previous half step and proposes the next one
 * (prior, resolved parameter rows, walker constants, range guard), and the whole block is a chain of launches the host
 * waits for once -- no host round trip between two evaluations (option "device_chain", default 1; csrc/mcd_stretch.hip).
 * The numbers are the host-driven loop's, bit for bit.  What only the host loop can handle -- a NaN, a re-run request of
 * the fast mixture kernels, a proposal table for which the range guard picks another kernel family than was enqueued, a
 * half step with every proposal outside the prior (binned: an ensemble without a valid proposal) -- makes the library
 * discard the block and run it host-driven from the same inputs; mcd_stretch_info counts both kinds.  pos, lnp and
 * accepted are only ever written with final values; chain / lnprob_chain of a block that moves more than 16 MB are
 * filled part by part while the device works on (a discarded block's rows are overwritten by its host-driven re-run).
 * Binned catalogues run resident for ensembles of up to 512 walkers and 12 columns. */
typedef struct {
    int64_t n_walkers;          /* W, even */
    int32_t n_dim;              /* free parameters (columns of pos) */
    int32_t k;                  /* mcd_catalog_param_count(cat) */
    const int32_t* col_source;  /* [k] index of the free parameter feeding kernel column j, or -1 for a constant column */
    const double* col_const;    /* [k] value of a constant column (a fixed parameter), in the kernel's unit */
    const double* col_factor;   /* [k] unit factor applied to a free-parameter column (1.0: none) */
    const double* lo;           /* [n_dim] inclusive prior bounds; -inf / +inf where unbounded */
    const double* hi;
    int32_t fixed_ok;           /* 0: a fixed parameter violates its own bounds, every proposal is rejected (runner.py:207-214) */
    int32_t n_bins;             /* 0 or 1: one ensemble (un-binned catalogue); B > 1: B lock-stepped ensembles, one per
                                 * parameter set (radial bin) of the catalogue -- must equal its number of bins */
} mcd_stretch_desc;

int mcd_stretch_move(mcd_catalog* cat, const mcd_stretch_desc* desc, int64_t n_steps, double* pos, double* lnp,
                     const int32_t* order, const double* zz, const double* thr, const int32_t* pick, double* chain,
                     double* lnprob_chain, int64_t* accepted);
/* Blocks of mcd_stretch_move that ran resident on the device / host-driven, blocks the device discarded (they were then
 * run host-driven and count there too) and the status bits of the last discarded one (1 NaN, 2 re-run request, 4 kernel
 * family changed, 8 no proposal inside the prior).  Any pointer may be NULL. */
/* The same block with its random numbers GENERATED INSIDE the library from a counter-based generator (Philox4x64-10, the
 * algorithm of numpy.random.Philox; mcmc_dynamics_amd/csrc/mcd_rng.h): the chain is a function of (seed, step, half step,
 * ensemble, walker) alone -- no numbers cross PCIe, blocks of any length continue each other (step0 = index of the block's first
 * step), and any step can be replayed on the host: mcd_chain_numbers returns the numbers of steps step0 .. step0 + n_steps - 1 in
 * the layout mcd_stretch_move takes (order [n_steps][B][W], zz / thr / pick [n_steps][2][B][W/2]), so that
 * mcd_stretch_move(..., those arrays, ...) gives the same chain bit for bit (tests/test_gpu_device_chain.py).  The logarithms
 * of the acceptance thresholds are a fixed sequence of IEEE operations (det_log), not libm calls, for that reason.
 * emcee (analysis/runner.py:403-419) draws from NumPy's Mersenne twister on the host instead. */
int mcd_stretch_move_seeded(mcd_catalog* cat, const mcd_stretch_desc* desc, int64_t n_steps, double* pos, double* lnp,
                            uint64_t seed, int64_t step0, double* chain, double* lnprob_chain, int64_t* accepted);
int mcd_chain_numbers(uint64_t seed, int64_t step0, int64_t n_steps, int64_t n_bins, int64_t n_walkers, int32_t n_dim,
                      int32_t* order, double* zz, double* thr, int32_t* pick);

int mcd_stretch_info(const mcd_catalog* cat, int64_t* device_blocks, int64_t* host_blocks, int64_t* discarded_blocks,
                     int32_t* last_discard_status);

/* Structured priors on the free parameters, on top of the inclusive box lo / hi of the descriptor (the reference writes
 * them as `lnprior` expressions over scipy's norm / lognorm, parameter.py:64-74, 684-705).  Per free parameter:
 *   kind 0  flat        --                     0
 *   kind 1  normal      p0 = loc, p1 = scale   -log(scale) - 1/2 log(2 pi) - 1/2 ((x - loc) / scale)^2
 *   kind 2  lognormal   p0 = mu,  p1 = s       -log(s) - 1/2 log(2 pi) - log(x) - 1/2 ((log(x) - mu) / s)^2
 *                       (scipy's lognorm(s, scale=exp(mu))); x <= 0 is outside the prior
 * i.e. the un-truncated log-density, evaluated at the full float64 value by one text of code on host and device
 * (mcmc_dynamics_amd/csrc/mcd_prior.h; the logarithm is det_log, no libm call per proposal): resident and host-driven
 * blocks give the same chain bit for bit.  A proposal is inside the prior when it is inside the box and every lognormal
 * coordinate is > 0; one that is not is treated as a proposal outside the box is.  lnp / lnprob_chain of the *_prior
 * entry points hold log-likelihood plus log-prior (lnp of mcd_stretch_move*_prior is the caller's on entry, as before).
 * prior == NULL, or all kinds 0, is the entry point without `_prior`, bit for bit.  p1 <= 0, a non-finite p0 / p1 of a
 * non-flat kind, an unknown kind or n_dim different from the descriptor's: MCD_ERR_INVALID, nothing written.  In
 * mcd_hmc_block_prior the potential is -(lnlike + lnprior) and the prior's derivative joins the gradient; a lognormal
 * coordinate <= 0 on a trajectory rejects the proposal, at the block's start it is MCD_ERR_NONFINITE. */
typedef struct {
    int32_t n_dim;          /* free parameters: must equal the descriptor's n_dim */
    const int32_t* kind;    /* [n_dim] 0 flat, 1 normal, 2 lognormal */
    const double* p0;       /* [n_dim] loc / mu (ignored for kind 0) */
    const double* p1;       /* [n_dim] scale / s > 0 (ignored for kind 0) */
} mcd_prior_desc;

/* value [n_rows] = log-prior of the rows x [n_rows][n_dim] WITHOUT the box (-inf where a lognormal coordinate is <= 0),
 * grad [n_rows][n_dim] (may be NULL) its derivatives (0 for such a row): the host compilation of the header the blocks
 * use, so that a caller can reproduce their numbers bit for bit.  Needs no device. */
int mcd_prior_eval(const mcd_prior_desc* prior, int64_t n_rows, const double* x, double* value, double* grad);
int mcd_stretch_move_prior(mcd_catalog* cat, const mcd_stretch_desc* desc, int64_t n_steps, double* pos, double* lnp,
                           const int32_t* order, const double* zz, const double* thr, const int32_t* pick, double* chain,
                           double* lnprob_chain, int64_t* accepted, const mcd_prior_desc* prior);
int mcd_stretch_move_seeded_prior(mcd_catalog* cat, const mcd_stretch_desc* desc, int64_t n_steps, double* pos, double* lnp,
                                  uint64_t seed, int64_t step0, double* chain, double* lnprob_chain, int64_t* accepted,
                                  const mcd_prior_desc* prior);

/* One block of differential-evolution steps (ter Braak 2006; with a jittered scale, Nelson et al. 2013) in place of the
 * stretch move: the same red / blue half steps, the same launch of W/2 rows per half step, one value evaluation per
 * proposal.  For slot j of half step h (s = pos[first[j]], first / second the halves of order[i]):
 *   proposal  s + (x_a - x_b) g, x_a = pos[second[pick_a]], x_b = pos[second[pick_b]], pick_a != pick_b both in 0 .. W/2 - 1
 *             (a subtraction, a multiplication, an addition per coordinate, never contracted)
 *   accept    iff thr < lnp_new - lnp_old (thr = log u: the proposal is symmetric, there is no (P - 1) log z term)
 * `desc` is the stretch move's descriptor and everything it says about the box, fixed_ok, the column map and the B
 * lock-stepped ensembles of a binned catalogue holds here (desc->n_bins must equal the catalogue's number of parameter
 * sets); `prior` (may be NULL) as in the *_prior entry points.  Array layouts: pos [B][W][P], lnp [B][W], order
 * [n_steps][B][W], pick_a / pick_b / gamma / thr [n_steps][2][B][W/2], chain [n_steps][B][W][P] or NULL, lnprob_chain
 * [n_steps][B][W] or NULL, accepted [B][W] or NULL (added to).  W must be even and >= 4: a half holds two distinct partners.
 *
 * A float64 catalogue on one device in one process runs the block RESIDENT (mcmc_dynamics_amd/csrc/mcd_de.hip: one small
 * kernel per half step accepts, proposes, applies the priors, builds the table rows and their walker constants and judges
 * the range guard); everything else, and any block in which the device met a NaN, a re-run request, a changed kernel
 * family or an ensemble without a proposal inside the prior, runs HOST-DRIVEN from the same inputs around mcd_loglike_batch
 * (mcd_de.h: de_block).  The two give the same chain bit for bit.  Option "device_chain" = 0 forces the host-driven form.
 *
 * mcd_de_move_seeded generates the numbers inside the library: g = gamma0 (1 + sigma n), n a standard normal (polar method
 * with det_log: no libm call decides a bit); the samplers' defaults are gamma0 = 2.38 / sqrt(2 P), sigma = 1e-5.  The
 * generator is Philox4x64-10 under a key constant of its own -- the stream is independent of mcd_chain_numbers' of the same
 * seed -- and a number is a function of (seed, step, half step, ensemble, slot) alone: blocks of any length continue each
 * other through step0, and mcd_de_numbers (needs no device) returns the numbers of steps step0 .. step0 + n_steps - 1 in the
 * layout mcd_de_move takes, so that mcd_de_move(..., those arrays, ...) gives the same chain bit for bit.
 *
 * MCD_ERR_INVALID, nothing written: gamma0 <= 0 or non-finite, sigma < 0 or non-finite, W < 4 or odd (seeded: W > 1048576),
 * desc->n_bins different from the catalogue's, an index outside its range, a null array.  MCD_ERR_NONFINITE: the
 * log-probability returned NaN.  (Added entry points: MCD_ABI_VERSION stays at 1.) */
int mcd_de_move(mcd_catalog* cat, const mcd_stretch_desc* desc, const mcd_prior_desc* prior /* may be NULL */, int64_t n_steps,
                double* pos, double* lnp, const int32_t* order, const int32_t* pick_a, const int32_t* pick_b,
                const double* gamma, const double* thr, double* chain, double* lnprob_chain, int64_t* accepted);
int mcd_de_move_seeded(mcd_catalog* cat, const mcd_stretch_desc* desc, const mcd_prior_desc* prior /* may be NULL */,
                       double gamma0, double sigma, int64_t n_steps, double* pos, double* lnp, uint64_t seed, int64_t step0,
                       double* chain, double* lnprob_chain, int64_t* accepted);
int mcd_de_numbers(uint64_t seed, int64_t step0, int64_t n_steps, int64_t n_bins, int64_t n_walkers, int32_t n_dim,
                   double gamma0, double sigma, int32_t* order, int32_t* pick_a, int32_t* pick_b, double* gamma, double* thr);
/* Blocks of mcd_de_move* that ran resident / host-driven, blocks the device discarded (they were then run host-driven and
 * count there too) and the status bits of the last discarded one, as mcd_stretch_info -- which keeps counting stretch
 * blocks only.  Any pointer may be NULL. */
int mcd_de_info(const mcd_catalog* cat, int64_t* device_blocks, int64_t* host_blocks, int64_t* discarded_blocks,
                int32_t* last_discard_status);

/* One block of Hamiltonian Monte Carlo steps (Duane et al. 1987; Neal 2011) on the gradient of mcd_loglike_grad_batch:
 * W independent chains, each step n_leap leapfrog points, i.e. n_leap value-and-gradient evaluations of W rows.  The
 * reference has no gradient-based sampler -- this stands beside mcd_stretch_move_seeded as a second way to drive the chain
 * that emcee's stretch move drives for it (analysis/runner.py:403-419), for posteriors on which that move mixes slowly.
 * The algebra is mcmc_dynamics_amd/csrc/mcd_hmc.h, one text for host and device:
 *   map     the column map, bounds and fixed_ok of mcd_stretch_move; n_walkers = W >= 1 (odd allowed), n_dim = P <= 12,
 *           n_bins 0 or 1
 *   chol    [P][P] row-major LOWER Cholesky factor L of the INVERSE mass matrix, M^-1 = L L^T -- the factor of an estimate
 *           of the posterior covariance (entries above the diagonal must be 0, the diagonal positive).  Momenta are
 *           p = L^-T z with z standard normal, the kinetic energy is 1/2 |L^T p|^2, a drift is q += eps L L^T p.
 *   step    eps = step_size (1 + jitter r), r uniform in [-1, 1), drawn per walker and step
 *   prior   the box lo <= q <= hi (inclusive).  With a DIAGONAL chol a coordinate that leaves the box after a drift is
 *           mirrored at the bound and its momentum component negated (a hard wall: exact, reversible).  With a DENSE chol a
 *           trajectory that leaves the box is ended and its proposal rejected.  Detailed balance holds either way.
 *   accept  iff log(u) < H0 - H1, H = -lnlike + kinetic.  A non-finite value or gradient on the way rejects the proposal (a
 *           divergent trajectory is no error); fixed_ok == 0 rejects everything.
 * Every number of a step is a function of (seed, step0 + i, walker) alone (Philox4x64-10 with a key of its own, normals by
 * Marsaglia's polar method with det_log: no libm call), so blocks of any length continue each other through step0, and
 * mcd_hmc_numbers returns them: z [n_steps][W][P], thr [n_steps][W] = log(u), eps_factor [n_steps][W] = r.
 *   pos [W][P]           in: where the block starts; out: where it ends
 *   lnp [W]              out only: the log-likelihood at pos (the block evaluates its own starting point)
 *   chain [n_steps][W][P], lnprob_chain [n_steps][W], energy_error [n_steps][W]   the state after every step and
 *                        |H1 - H0| of its proposal (+inf for a trajectory that ended early); each may be NULL
 *   accepted [W]         incremented; may be NULL
 * pos, lnp and accepted are only ever written with final values.  Returns MCD_ERR_NONFINITE when a walker STARTS outside
 * the box or with a non-finite log-likelihood or gradient, MCD_ERR_INVALID (pos untouched) for a binned or a float32
 * catalogue: lock-stepped ensembles have no HMC block, and the gradient is float64.
 *
 * Where it runs.  One device per process without a communicator: RESIDENT -- the starting point costs one host round
 * trip, then begin / (walker prep, gradient kernel, reduction, leap) x n_leap per step are one chain of launches on the
 * catalogue's stream, the trajectory state stays in a device scratch that is released with the catalogue, and the host
 * waits once under the context's deadline (csrc/mcd_hmc.hip).  Everything else -- option "device_chain" = 0, several
 * devices or ranks, option "timing", more than 65536 walkers or more than 512 MB of rows per block -- runs HOST-DRIVEN: the
 * same loop around mcd_loglike_grad_batch, whose all-reduce makes it multi-rank.  Both give the same chain bit for bit;
 * mcd_hmc_info counts the blocks of either kind. */
typedef struct {
    mcd_stretch_desc map;
    const double* chol;     /* [n_dim][n_dim] lower Cholesky factor of the inverse mass matrix */
    double step_size;       /* eps > 0 */
    double jitter;          /* 0 <= j < 1 */
    int32_t n_leap;         /* L >= 1 */
} mcd_hmc_desc;

int mcd_hmc_block(mcd_catalog* cat, const mcd_hmc_desc* desc, int64_t n_steps, double* pos, double* lnp, uint64_t seed,
                  int64_t step0, double* chain, double* lnprob_chain, int64_t* accepted, double* energy_error);
int mcd_hmc_block_prior(mcd_catalog* cat, const mcd_hmc_desc* desc, int64_t n_steps, double* pos, double* lnp, uint64_t seed,
                        int64_t step0, double* chain, double* lnprob_chain, int64_t* accepted, double* energy_error,
                        const mcd_prior_desc* prior);      /* mcd_prior_desc: above, with mcd_stretch_move_prior */
int mcd_hmc_numbers(uint64_t seed, int64_t step0, int64_t n_steps, int64_t n_walkers, int32_t n_dim, double* z, double* thr,
                    double* eps_factor);
int mcd_hmc_info(const mcd_catalog* cat, int64_t* device_blocks, int64_t* host_blocks);

/* One block of parallel-tempering steps (Swendsen & Wang 1986; Geyer 1991): T ensembles ("rungs") of W walkers each sample
 * prior(x) L(x)^beta_t on a ladder 1 = beta_0 > beta_1 > ... > beta_{T-1} >= 0.  Every rung advances by the stretch move of
 * mcd_stretch_move_seeded (ensemble index = rung: the numbers are mcd_chain_numbers' for n_bins = T), adjacent rungs
 * exchange walkers by a Metropolis swap, and the rungs' log-likelihood series give the marginal likelihood (the Python
 * layer's evidence_summary).  The reference has one ensemble at one temperature (analysis/runner.py:403-419).  The algebra
 * is mcmc_dynamics_amd/csrc/mcd_temper.h, one text for host and device:
 *   half steps  h = 0, 1 in every rung at once: proposal q - (q - s) z from the other half of the walker's own rung; inside
 *               the prior iff inside the inclusive box and every prior's support; accept iff
 *               thr < beta_t (ll_new - ll_old) [+ (lp_new - lp_old) with mcd_temper_block_prior], in this order.  A proposal
 *               outside the prior or with a non-finite ll_new is rejected at every rung, beta = 0 included; a NaN ll_new is
 *               MCD_ERR_NONFINITE; fixed_ok == 0 rejects everything.
 *   swap phase  after half step 1 of absolute step s: the pairs (t, t + 1) with t = s (mod 2), walker w of rung t with walker
 *               w of rung t + 1; accept iff log(u) < (beta_t - beta_{t+1}) (ll_{t+1} - ll_t); the walkers then exchange
 *               position, log-likelihood and log-prior.  One generator call per (step, t, w) with a key of its own:
 *               mcd_temper_numbers returns log(u) as swap_thr [n_steps][T-1][W] (every pair, active or not).
 *   pos [T][W][P], lnlike [T][W]   in: where the block starts and the log-likelihood there; out: where it ends
 *   lnprior [T][W]       out: the log-prior at pos (0 inside the box without structured priors); the block computes the
 *                        start positions' values itself, whatever the array holds on entry
 *   chain [n_steps][n_chain_temps][W][P], lnlike_chain [n_steps][T][W]   the state after every step's swap phase; may be NULL
 *   accepted [T][W], swap_proposed [T-1], swap_accepted [T-1]   incremented; each may be NULL.  accepted counts by slot
 *                        (rung, walker index), not by the walker that travels through the ladder.
 * pos, lnlike, lnprior and the counts are only ever written with final values.  Returns MCD_ERR_NONFINITE when a walker
 * STARTS outside the prior or with a non-finite log-likelihood, MCD_ERR_INVALID (nothing touched) for a binned or a float32
 * catalogue, an odd W, a ladder that does not start at 1 or is not strictly decreasing within [0, 1], n_chain_temps outside
 * 1 .. T, n_dim > 12 or a descriptor whose k is not the catalogue's.
 *
 * Evaluations run the PLAIN kernels (option "fast_path" = 0) in both forms, whatever the option says, and leave it as it
 * was: the hot rungs roam the whole prior box, where the fast families' range guard would refuse often.
 * Where it runs.  One device per process without a communicator: RESIDENT -- propose / (walker prep, main kernel, reduction)
 * / accept-and-propose / ... / swap-and-record are one chain of launches on the catalogue's stream, T W/2 parameter rows
 * per launch, and the host waits once (csrc/mcd_temper.hip).  Everything else -- option "device_chain" = 0, several devices
 * or ranks, option "timing", W > 8192, more than 512 MB of numbers and rows per block, or no memory for the arena -- runs
 * HOST-DRIVEN: the same loop around mcd_loglike_batch.  Both give the same chain bit for bit; mcd_temper_info counts the
 * blocks of either kind. */
typedef struct {
    mcd_stretch_desc map;       /* n_bins <= 1; n_walkers = W per rung (even, >= 2) */
    int32_t n_temps;            /* T >= 1 */
    const double* betas;        /* [T], betas[0] == 1, strictly decreasing, >= 0 */
    int32_t n_chain_temps;      /* positions of rungs 0 .. n_chain_temps-1 are stored (1: the posterior only) */
} mcd_temper_desc;

int mcd_temper_block(mcd_catalog* cat, const mcd_temper_desc* desc, int64_t n_steps, double* pos, double* lnlike,
                     double* lnprior, uint64_t seed, int64_t step0, double* chain, double* lnlike_chain, int64_t* accepted,
                     int64_t* swap_proposed, int64_t* swap_accepted);
int mcd_temper_block_prior(mcd_catalog* cat, const mcd_temper_desc* desc, int64_t n_steps, double* pos, double* lnlike,
                           double* lnprior, uint64_t seed, int64_t step0, double* chain, double* lnlike_chain,
                           int64_t* accepted, int64_t* swap_proposed, int64_t* swap_accepted,
                           const mcd_prior_desc* prior);      /* mcd_prior_desc: above, with mcd_stretch_move_prior */
int mcd_temper_numbers(uint64_t seed, int64_t step0, int64_t n_steps, int32_t n_temps, int64_t n_walkers, double* swap_thr);
int mcd_temper_info(const mcd_catalog* cat, int64_t* device_blocks, int64_t* host_blocks);

/* Moment matching for PSIS-LOO (Paananen, Piironen, Buerkner & Vehtari 2021; loo_moment_match.default of the R package loo):
 * the cheaper remedy, before a refit, for the stars whose Pareto k^ is too large.  The S posterior draws (row-major [S][P],
 * the free parameters in their own units, resolved into kernel rows by `map` as in mcd_stretch_move) are moved towards each
 * star's leave-one-out posterior by affine maps theta -> A theta + b that match the importance-weighted mean, then the
 * variances, then (cov, S > 10 P) the covariance; a trial is kept when it lowers k^.  The algebra, the order of the trials
 * and the meaning of `iterations` / `accepted` are mcmc_dynamics_amd/csrc/mcd_mmatch.h.  With l_i the star's plain term and
 * L_-i the sum of all others (mcd_holdout_loglike's test and train for the singleton set {i}), the log weights are
 *   baseline  -l_i(theta_s)                                        lp0_s = L_-i + l_i + lnprior, by these plain terms
 *   trial     L_-i(theta') + lnprior(theta') - lp0_s               -inf for a row outside the prior (box, support, fixed_ok)
 *   split     (split, and at least one trial kept) the first floor(S/2) rows transformed, the rest as drawn:
 *             L_-i + lnprior - logaddexp(lp, lp(T^-1 .) - log|det A|) -- the estimate no longer depends on the draws that
 *             chose the map
 * each smoothed with the tail rules of mcd_psis_loo.  Per star of `stars` (ascending, distinct): elpd = log sum w~ exp(l_i)
 * over the final rows, pareto_k and n_eff = r_eff / sum w~^2 of the final weights, k_before (the baseline's k^; elpd and
 * pareto_k equal mcd_psis_loo's to rounding when max_iters = 0), k_loop (k^ when the loop ended), iterations, accepted
 * [n_match][3] per level, and the total map A [n_match][P][P], b [n_match][P] (identity and 0 when nothing was kept).
 * Stars run in lock-stepped groups of floor(65536 / S); rows, weights, moments and kernel tables stay on the device, one
 * hold-out evaluation per trial and group, and only per-star scalars come back between two of them.  Synchronous and
 * deterministic: bit-identical from run to run, independent of earlier calls.  Any output pointer may be NULL.
 * MCD_ERR_INVALID, with a message and nothing written: a binned or a float32 catalogue; several devices or a communicator;
 * n_dim outside 1 .. 12; n_samples > 65536 or with a PSIS tail shorter than 5; star indices unsorted, repeated or outside
 * the catalogue; r_eff <= 0; max_iters < 0; a bad prior descriptor.  MCD_ERR_NONFINITE (nothing written): a draw outside
 * the prior.  Device scratch is released on every exit path; waits under the context's deadline; honours option "timing"
 * (mcd_last_kernel_ms: the hold-out main kernels of all rounds). */
typedef struct {
    mcd_stretch_desc map;     /* column map, box, fixed_ok; n_walkers ignored, n_bins 0 or 1 */
    int32_t max_iters;        /* >= 0; 0: baseline only */
    int32_t cov, split;       /* 0 / 1 */
    double k_threshold, r_eff;
} mcd_mmatch_desc;
int mcd_moment_match(mcd_catalog* cat, const mcd_mmatch_desc* d, const mcd_prior_desc* prior /* may be NULL */,
                     int64_t n_samples, const double* draws /* [S][P] */, int64_t n_match,
                     const int64_t* stars /* ascending, distinct */,
                     double* elpd, double* pareto_k, double* n_eff, double* k_before, double* k_loop, /* [n_match] */
                     int32_t* iterations, int32_t* accepted /* [n_match][3] */, double* A /* [n_match][P][P] */,
                     double* b /* [n_match][P] */);

/* ---- convergence diagnostics of a stored chain ------------------------------------------- */

/* Integrated autocorrelation time (the estimator of emcee's autocorr.integrated_time), split-R-hat (Gelman et al., BDA3)
 * and the pooled moments of a chain in the samplers' layout chain[n_steps][n_groups][n_walkers][n_dim], float64: n_groups
 * independent ensembles (the bins of a binned catalogue, or 1).  The reference has no such diagnostic: its users call
 * emcee's sampler.get_autocorr_time().  Per (group g, parameter p), outputs [n_groups][n_dim]:
 *   tau, window, found   with y the series of one walker minus its FIRST value and then minus its mean,
 *                        a_k = sum_t y_t y_{t+k}, rho_k = the walkers' mean of a_k / a_0, tau_k = 2 sum_{j<=k} rho_j - 1:
 *                        window = the smallest k <= max_lag with k >= c tau_k, found = 1, tau = tau_window; when there is
 *                        none, found = 0, tau = tau_{max_lag}, window = max_lag (the chain is too short for max_lag)
 *   rhat                 m = 2 n_walkers half-chains of n = n_steps / 2 steps: sqrt(((n-1)/n Wv + B/n) / Wv); NaN for
 *                        n_steps < 4 or Wv = 0
 *   mean, var            over the n_steps x n_walkers samples (var with ddof = 1)
 *   rho                  NULL, or [n_groups][n_dim][max_lag + 1]
 * A walker that never moves (a_0 = 0) makes rho, tau and rhat of its (g, p) NaN and found 0, as emcee's estimate is NaN.
 * ctx == NULL: the loop of mcmc_dynamics_amd/csrc/mcd_diag.h on the host, no device needed.  Otherwise the kernels of
 * csrc/mcd_diag.hip on the context's first device, waited for under the context's deadline: the chain goes up in tiles of
 * whole groups within scratch_mb MiB of device memory (0: 1024).  One text, one order of every sum: host and device
 * results are bit-identical, and independent of the tile plan.  No collective: every rank of a multi-rank job holds the
 * whole chain and calls this locally.  MCD_ERR_INVALID (nothing written) for n_steps < 2, max_lag outside
 * [1, n_steps - 1], c <= 0, a dimension < 1, a NULL output other than rho, or a scratch_mb that cannot hold one group. */
typedef struct {
    int64_t n_steps, n_groups, n_walkers;
    int32_t n_dim;
    int64_t max_lag;
    double c;
    int64_t scratch_mb;
} mcd_diag_desc;

int mcd_chain_diagnostics(mcd_ctx* ctx, const mcd_diag_desc* d, const double* chain, double* tau, int64_t* window,
                          int32_t* found, double* rhat, double* mean, double* var, double* rho);
/* Of the calling thread's last mcd_chain_diagnostics: groups per device tile, tiles, and the HIP-event time of its kernels
 * in milliseconds (0 for ctx == NULL).  Any pointer may be NULL. */
int mcd_chain_diagnostics_info(int64_t* tile_groups, int64_t* n_tiles, double* kernel_ms);

/* ---- introspection for the measurement harness ------------------------------------------- */

const char* mcd_last_error(void);
int mcd_abi_version(void);
/* HIP-event time of the most recent mcd_loglike_batch / enqueue+sync: main kernel only, and the
 * whole device-side sequence (prep + main + reduce), milliseconds, device 0 of this process. */
double mcd_last_kernel_ms(const mcd_catalog* cat);
double mcd_last_device_ms(const mcd_catalog* cat);
/* Tuning / measurement switches, per catalogue.  Keys:
 *   "timing"        1: record HIP events around every enqueue (default 0); 2: additionally keep one
 *                      event pair per main-kernel launch for mcd_timing_collect
 *   "timing_stride" n: with "timing" = 2, record the event pair on every n-th launch only (default 1); the events cost a
 *                      signal packet each between back-to-back kernels, so a throughput harness samples
 *   "timing_discard" (any value): drop the event pairs recorded so far without reading them -- cheap, unlike
 *                      mcd_timing_collect, whose hipEventElapsedTime calls idle the GPU for milliseconds
 *   "timing_reserve" n: create the event pairs for n launches of "timing" = 2 now, so that a measured loop does not
 *                      pay for hipEventCreate
 *   "fast_path"     0: always use the plain per-term log/divide kernels; 1 (default): the fast formulations
 *                      (fraction tree / log-product / single-exp mixtures) are used whenever the per-call range
 *                      guard allows, including the narrow-range variant of the fixed-background mixture;
 *                      2: as 1 but never the narrow-range variant (testing aid)
 *   "zero_copy"     1 (default): on a single device mcd_loglike_batch lets the kernels read the parameter table
 *                      from / write the results to pinned mapped host memory instead of issuing H2D / D2H copies
 *   "spin_us"       microseconds mcd_sync / fetch / batch poll the stream (hipStreamQuery) before they fall back to the
 *                      blocking hipStreamSynchronize, whose interrupt wake-up adds 50 - 500 us of jitter to waits longer
 *                      than a fraction of a millisecond (default 20000; 0: always block)
 *   "device_chain"  1 (default): mcd_stretch_move and mcd_hmc_block keep the ensemble resident on the device where
 *                      they can (see there); 0: host-driven blocks only
 *   "prefetch"      software prefetch of the star records of the next loop iteration (a second instantiation of the fast
 *                      kernels): -1 (default) by shape -- mixture models from 8 MiB of records per device up (it hides
 *                      the memory latency there: +8 % at 256 walkers to +45 % at 64 on 1e6 stars), models without
 *                      background only for un-binned catalogues from 128 MiB up (their 16-star loop hides the latency
 *                      itself; the prefetch costs binned and many-walker shapes 3 - 6 %); 0 off, 1 on.  Results do not
 *                      depend on it.
 *   "narrow_bounded" 1 (default): where the range guard finds every mixture value of a fixed-centre MODEL_CONST_BGFIXED
 *                      catalogue inside a bounded domain (no exponent argument below -700, 16 or 32 factors between two
 *                      rescales), the narrow-range kernel with prefetch runs its bounded loop -- fewer instructions per
 *                      term, the same bits; 0 never.  mcd_last_narrow_bounded tells which loop ran.
 *   "verr_sorted"   the main kernel of an un-binned float64 fixed-centre MODEL_CONST_BGFIXED catalogue reads a second copy of
 *                      the records ordered by verr (one more record array in device memory, made on first use); every
 *                      per-star output keeps catalogue order.  -1 (default): from 8 MiB of records per device, unless an
 *                      explicit "chunk_len" pins the chunks to catalogue stars; 0 never; 1 always.  A sum over the stars in another fixed order: results agree with catalogue order to
 *                      rounding, not bit for bit.
 *   "root_series"   1 (default): on verr-sorted records, a chunk whose verr^2 values lie within 2^-13 (relative to
 *                      verr^2 + sigma^2) of their midpoint for every walker of a wave takes the reciprocal root from a
 *                      four-term series about that midpoint instead of v_rsq_f64 and a Newton step (more accurate and
 *                      fewer issue slots per term); 0 never.  mcd_last_series_chunks counts the chunks.
 *   "root_direct"   1 (default): a chunk that takes the series root, and whose midpoint verr^2 is at most 1/8 of
 *                      verr^2 + sigma^2 for every walker of the wave, evaluates the same cubic in verr^2 itself, with
 *                      coefficients re-centred once per chunk: one float64 instruction per term fewer, relative error of
 *                      the root <= 4.6e-16; 0: every series chunk keeps the form about the midpoint (the results of a
 *                      library without this option, bit for bit).  mcd_last_direct_chunks counts the chunks.
 *   "exp_split"     1 (default): the chunks in the direct form evaluate the exponent with the record's offset split once per
 *                      star by the record preparation (integer table steps in the rounding constant, the fraction in the
 *                      record's 1 - pmember; a third verr-ordered array of 64 bytes per star in device memory): one float64
 *                      instruction per term fewer, results equal to rounding; refused per call where the range guard
 *                      cannot place every mixture value, scaled by up to 1.2016, inside the rescale interval.  0: never
 *                      (the results of a library without this option, bit for bit).  mcd_last_exp_split tells.
 *   "root_quad"     1 (default): in a launch with the split exponent offset, a chunk in the direct form whose 32-star blocks
 *                      (records 32 b .. 32 b + 31 of the verr-ordered array) are each narrower than 2^-17.5 (verr^2 + sigma^2)
 *                      in half-width for every walker of the wave replaces the cubic by a quadratic per block, whose
 *                      coefficients the record preparation leaves in the blocks' first two records: one float64
 *                      instruction per term fewer, relative error of the root <= 4.9e-16, results equal to rounding.  0: never
 *                      (the results of a library without this option, bit for bit).  mcd_last_root_quad tells,
 *                      mcd_last_quad_chunks counts the chunks.
 *   "block_step"    1 (default): a launch of the bounded narrow-range loop (R = 32) that offers the quadratic form runs the
 *                      kernel whose quadratic loop does its per-band work -- the fold of the coefficients, the rescale of the
 *                      running product and the prefetch of a whole band of records -- in one block per 32 stars; admitted
 *                      per call where 56 raw factors fit between two rescales.  The same results, bit for bit.  0: never
 *                      (the kernels of a library without this option).  mcd_last_block_step tells.
 *   "target_waves"  number of waves the chunking aims for per device (default 10240)
 *   "chunk_len"     explicit nominal chunk length in stars (rounded up to a multiple of 32; 0, the default: derived from
 *                      "target_waves"); tuning aid
 *   "tail_split"    chunk schedule: 0 equal-length chunks; 1 (default): the last ~15 % of a large parameter set is
 *                      cut into half- and quarter-length chunks so that the launch ends on short waves; 2-4:
 *                      other guided schedules kept for tuning (see build_workset in mcd_api_catalog.hip)
 *   "balance"       balanced single-round chunk plans for small catalogues (every workgroup of the launch resident at once,
 *                      chunks of equal length: no tail, no second round): -1 (default) by work -- 2, 4 or 8 workgroups per
 *                      CU below ~1e6 work units, the multi-round table beyond; 0 never; 1 .. 8 forced
 *   "combine"       balanced plans run as 8- / 16-wave workgroups that add up their chunks' sums themselves (one partial
 *                      sum per workgroup and walker instead of one per chunk): 1 (default) the largest the plan allows,
 *                      0 never, 8 / 16 at most that many waves
 *   "two_lanes"     1 (default): pipelined evaluations (mcd_loglike_enqueue back to back) alternate between two streams
 *                      with their own partial-sum and result buffers, so that one launch's tail and reduction overlap
 *                      the next launch's start; 0: one stream.  Results do not depend on it.
 *   "fused_reduce"  1 (default): resident stretch-move blocks whose launches leave <= 256 partial sums per walker run
 *                      without the reduction kernel (the step kernel adds them up, same code, same order); 0: never
 *   "defer_guard"   1 (default): resident blocks of ONE ensemble judge the range guard of all their launches after the
 *                      last step instead of between two main kernels (same verdicts, same discards); 0: in the step kernel
 *   "f32_domain"    1 (default): float32 catalogues refuse parameter tables outside the float32 accuracy domain (below)
 *   "replicate_row0"  index that the generator of mcd_replicate_check gives the first row of its table (default 0): a
 *                      table split over several calls reproduces the one-call result bit for bit
 * Returns MCD_ERR_INVALID for an unknown key. */
int mcd_set_option(mcd_catalog* cat, const char* key, int64_t value);
/* With "timing" = 2: waits for the device, returns the summed HIP-event duration (ms) of all main-kernel
 * launches on device 0 of this process since the last collect / option change and their number. */
int mcd_timing_collect(mcd_catalog* cat, double* total_kernel_ms, int64_t* n_launches);
/* Number of batches this catalogue re-evaluated with the plain kernels because a fast mixture kernel met the regime in
 * which the reference's log-sum-exp (runner.py:282-284) itself runs on denormal numbers -- a star with pmember == 1,
 * f_back == 0 or density == 0 that lies > 37 sigma from the only remaining component.  Only the literal expression
 * reproduces the reference's value there; the re-evaluation is automatic and synchronous inside fetch / batch. */
int64_t mcd_rerun_count(const mcd_catalog* cat);
/* 1 when the most recent main-kernel launch used the instantiation that prefetches the next loop iteration's star records
 * (option "prefetch"), 0 when not, -1 before the first launch.  The harness picks the per-term instruction count of the
 * roofline by it (csrc/isa_mix.json holds both instantiations). */
int mcd_last_prefetch(const mcd_catalog* cat);
/* Rescale interval R (16 or 32 factors) when the most recent main-kernel launch ran the bounded narrow-range loop (option
 * "narrow_bounded"), 0 when it ran another loop, -1 before the first launch.  mcd_last_fast_level reports 2 for it. */
int mcd_last_narrow_bounded(const mcd_catalog* cat);
/* Chunks of the most recent main-kernel launch (summed over this process' devices) in which every wave took the series
 * root (option "root_series"): counted on the host from the chunk table and the smallest sigma of the call's parameter
 * table.  0 when the launch did not read verr-sorted records or ran another kernel family (and for the launches of the
 * resident stretch-move chain, whose tables never reach the host), -1 before the first launch. */
int64_t mcd_last_series_chunks(const mcd_catalog* cat);
/* ... of which chunks in which every wave took the direct form of the series (option "root_direct"), counted the same way:
 * never more than mcd_last_series_chunks, whose meaning it does not change; 0 and -1 as there. */
int64_t mcd_last_direct_chunks(const mcd_catalog* cat);
/* 1 when the direct chunks of the most recent main-kernel launch ran with the split exponent offset (option "exp_split"), 0
 * when not (option off, refused by the guard, another kernel family, the resident chain), -1 before the first launch. */
int mcd_last_exp_split(const mcd_catalog* cat);
/* 1 when the most recent main-kernel launch offered its direct chunks the quadratic form on 32-star bands (option
 * "root_quad" on a launch with the split exponent offset), 0 when not, -1 before the first launch. */
int mcd_last_root_quad(const mcd_catalog* cat);
/* ... and the chunks in which every wave took it, counted as mcd_last_direct_chunks is and never more than that; 0 and -1
 * as there. */
int64_t mcd_last_quad_chunks(const mcd_catalog* cat);
/* 1 when the most recent main-kernel launch ran the kernel with one block step per 32-star band (option "block_step"), 0 when
 * not (option off, refused by the guard, no bounded launch with the quadratic form), -1 before the first launch. */
int mcd_last_block_step(const mcd_catalog* cat);
/* Kernel family the range guard chose for the batch staged last: 0 plain, 1 fast formulation, 2 narrow-range variant of
 * the mixture kernels (no per-star exponent bookkeeping; chunks holding a star outside its domain -- a certain member, an
 * extreme background likelihood, an empty component -- still run the fast formulation); -1 before any call. */
int mcd_last_fast_level(const mcd_catalog* cat);

/* float32 accuracy domain (MCD_F32, MCD_F32_ACC64).  The float32 kernels round every record field and walker constant to
 * 24 bits first; they stay within 1e-6 (MCD_F32_ACC64) / 2e-5 (MCD_F32) of the float64 kernels -- fixed centre; 2e-5 /
 * 1e-4 with a free centre -- on the scale max(|lnL|, N, 32) only while
 *     kappa_v = (max|v| + |v_sys| + |v_maxx| + |v_maxy|) / sqrt(min(verr^2) + min(sigma^2))      <= 96
 *     kappa_theta = (|v_maxx| + |v_maxy|) / sqrt(min(verr^2) + min(sigma^2)) * 2^-23 / sep_harm   <= 2e-5   (free centre;
 *                   sep_harm: harmonic mean angular separation [rad] of the stars from the catalogue's centroid)
 * and variances, residuals and mixture values lie in the float32 ranges (norm within 2^-15 .. 2^15, |v - v_los| <= 2^15,
 * lnL_bg within -80 .. 60, pmember <= 1 - 2^-20, density and f_back within 2^-20 .. 2^20); derivation in
 * mcmc_dynamics_amd/csrc/mcd_guard.h (f32_domain), evidence in profiles/r03_fuzz_f32.txt (tools/fuzz_f32.py: errors up to
 * 8.5e-4 outside on its ranges, 0.58 in the wider campaign of round 2).  A parameter table outside the domain is REFUSED: mcd_params_upload / mcd_loglike_batch return
 * MCD_ERR_INVALID with the reason (option "f32_domain" = 0: evaluate regardless).  mcd_last_f32_domain reports the verdict
 * on the last staged table (1 inside, 0 outside; always 1 for MCD_F64 catalogues) and the two condition numbers. */
int mcd_last_f32_domain(const mcd_catalog* cat, double* kappa_v, double* kappa_theta);
/* The same verdict accumulated over EVERY table the catalogue has staged since mcd_catalog_create -- a block of
 * mcd_stretch_move / mcd_stretch_move_seeded stages two tables per step and mcd_last_f32_domain reports only the last:
 *   calls               tables staged outside the domain (evaluated with option "f32_domain" = 0, refused with 1);
 *   worst_kappa_v,
 *   worst_kappa_theta   the largest condition numbers of any staged table, inside the domain or not;
 *   reason              the reason of the most recent table outside ("" when calls == 0): a static string, never freed.
 * Host-side counters; any of the four pointers may be null.  All zero for an MCD_F64 catalogue.  MCD_ERR_INVALID for a
 * null catalogue.  (An added entry point: MCD_ABI_VERSION stays at 1.) */
int mcd_f32_outside(const mcd_catalog* cat, int64_t* calls, double* worst_kappa_v, double* worst_kappa_theta,
                    const char** reason);
/* Launch geometry of the main kernel for the last call: workgroups, walker tile (walkers that
 * reuse one star record load), chunks per parameter set, bytes per star record. */
int mcd_last_launch_info(const mcd_catalog* cat, int64_t* n_workgroups, int32_t* walker_tile,
                         int64_t* n_chunks, int32_t* record_bytes);

#ifdef __cplusplus
}
#endif
#endif /* MCD_H */

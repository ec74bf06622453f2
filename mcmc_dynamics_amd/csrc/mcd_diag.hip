// mcd_diag.hip -- gfx950 kernels of mcd_chain_diagnostics: integrated autocorrelation time, split-R-hat and pooled moments
// of a stored chain.  The arithmetic and the order of every sum are in mcd_diag.h, one text with the host loop; DESIGN.md
// section 3.13 has the mapping and the measurements.
//
// Four kernels per tile of whole groups, x [T][ns] (ns = groups x W x P series, consecutive series adjacent):
//   diag_moments_kernel  lane = series: two walks over t (the mean of x_t - x_0, then the M2s), every load of a row coalesced
//   diag_lag_kernel      lane = series, a wave owns 64 series x one block of kDiagLags lags: kDiagLags running sums and a
//                        ring of kDiagLags older values in registers (static slots: diag_lag_steps), one walk over t with
//                        kDiagLags fmas per new value.  The four waves of a workgroup take four consecutive lag blocks of
//                        the same 64 series, so that the rows one of them fetched serve the others from the vector L1; the
//                        tile is re-read once per lag block from L2 / the Infinity Cache.  Writes a_k to a [k][series] scratch.
//   diag_rho_kernel      one thread per (group, parameter, lag): the walkers' a_k / a_0 added in walker order
//   diag_final_kernel    one thread per (group, parameter): prefix sum over the lags, the window, R-hat, the pooled moments
// No atomics, no barriers, no LDS: every number is produced by one thread in the header's order.
#include <hip/hip_runtime.h>
#include <cstdint>

#include "mcd_launch.h"   // kWave
#include "mcd_diag.h"

namespace mcd {
namespace {

constexpr int kDiagWaves = 4;              // lag blocks (waves) per workgroup of the lag kernel

__global__ __launch_bounds__(kWave) void diag_moments_kernel(const double* __restrict__ x, int64_t T, int64_t ns,
                                                             double* __restrict__ mom) {
    const int64_t s = (int64_t)blockIdx.x * kWave + threadIdx.x;
    if (s >= ns) return;
    diag_series_moments(x + s, ns, T, mom + s, ns);
}

__global__ __launch_bounds__(kWave * kDiagWaves) void diag_lag_kernel(const double* __restrict__ x, int64_t T, int64_t ns,
                                                                      int64_t L, int64_t n_groups4,
                                                                      const double* __restrict__ mom, double* __restrict__ a) {
    const int lane = (int)(threadIdx.x & (kWave - 1)), wave = (int)(threadIdx.x / kWave);
    const int64_t tile = (int64_t)blockIdx.x / n_groups4;
    const int64_t k0 = (((int64_t)blockIdx.x % n_groups4) * kDiagWaves + wave) * kDiagLags;
    if (k0 > L) return;                                    // (wave-uniform)
    const int64_t s = tile * kWave + lane;
    const int64_t sc = s < ns ? s : ns - 1;                // idle lanes repeat the last series and store nothing
    double acc[kDiagLags];
    diag_lag_walk(x + sc, ns, T, mom[DM_X0 * ns + sc], mom[DM_MEAN * ns + sc], k0, acc);
    if (s < ns) {
#pragma unroll
        for (int j = 0; j < kDiagLags; ++j)
            if (k0 + j <= L) a[(k0 + j) * ns + s] = acc[j];
    }
}

// rho_rows [ng P][L + 1]; thread = (row, k) with k fastest
__global__ __launch_bounds__(256) void diag_rho_kernel(const double* __restrict__ a, int64_t ns, int64_t ng, int64_t W, int P,
                                                       int64_t L, double* __restrict__ rho_rows) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= ng * P * (L + 1)) return;
    const int64_t k = i % (L + 1), row = i / (L + 1);
    const int64_t g = row / P;
    const int p = (int)(row % P);
    rho_rows[i] = diag_rho_mean(a, ns, g * W * P, W, P, p, k);
}

__global__ __launch_bounds__(kWave) void diag_final_kernel(const double* __restrict__ rho_rows, const double* __restrict__ mom,
                                                           int64_t T, int64_t ns, int64_t ng, int64_t W, int P, int64_t L,
                                                           double c, double* __restrict__ tau, int64_t* __restrict__ window,
                                                           int32_t* __restrict__ found, double* __restrict__ rhat,
                                                           double* __restrict__ mean, double* __restrict__ var) {
    const int64_t row = (int64_t)blockIdx.x * kWave + threadIdx.x;
    if (row >= ng * P) return;
    DiagWindow win;
    const double* r = rho_rows + row * (L + 1);
    for (int64_t k = 0; k <= L; ++k) win.feed(r[k], c);
    tau[row] = win.tau;
    window[row] = win.window;
    found[row] = win.found;
    diag_group_moments(mom, ns, (row / P) * W * P, W, P, (int)(row % P), T, rhat + row, mean + row, var + row);
}

}  // namespace

hipError_t launch_diag(hipStream_t s, const double* x, int64_t T, int64_t ng, int64_t W, int P, int64_t L, double c, double* a,
                       double* mom, double* rho_rows, double* tau, int64_t* window, int32_t* found, double* rhat, double* mean,
                       double* var) {
    const int64_t ns = ng * W * P;
    if (ns <= 0 || T < 2 || L < 1 || L > T - 1) return hipErrorInvalidValue;
    const int64_t tiles = (ns + kWave - 1) / kWave;
    const int64_t lag_blocks = (L + 1 + kDiagLags - 1) / kDiagLags;
    const int64_t groups4 = (lag_blocks + kDiagWaves - 1) / kDiagWaves;
    const int64_t rho_threads = ng * P * (L + 1);
    if (tiles * groups4 > INT32_MAX || (rho_threads + 255) / 256 > INT32_MAX) return hipErrorInvalidValue;
    hipLaunchKernelGGL(diag_moments_kernel, dim3((unsigned)tiles), dim3(kWave), 0, s, x, T, ns, mom);
    hipLaunchKernelGGL(diag_lag_kernel, dim3((unsigned)(tiles * groups4)), dim3(kWave * kDiagWaves), 0, s, x, T, ns, L, groups4,
                       (const double*)mom, a);
    hipLaunchKernelGGL(diag_rho_kernel, dim3((unsigned)((rho_threads + 255) / 256)), dim3(256), 0, s, (const double*)a, ns, ng, W,
                       P, L, rho_rows);
    hipLaunchKernelGGL(diag_final_kernel, dim3((unsigned)((ng * P + kWave - 1) / kWave)), dim3(kWave), 0, s,
                       (const double*)rho_rows, (const double*)mom, T, ns, ng, W, P, L, c, tau, window, found, rhat, mean, var);
    return hipGetLastError();
}

}  // namespace mcd

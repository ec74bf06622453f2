// TEST INFRASTRUCTURE ONLY -- psis_row (csrc/mcd_psis_row.h: the radix select, the index scan, the ballot gather, the rank
// sort, the GPD fit and the sums of one row by one wave) on rows given by the caller, so that tests/test_gpu_psis_rows.py
// can feed the selection rows no likelihood kernel produces.  Never loaded by the product package.
#include <hip/hip_runtime.h>
#include <cmath>
#include <cstdint>

#include "mcd_psis_row.h"

using namespace mcd;

namespace {

constexpr int kFields = 8;                 // PsisRow: khat, mw, m2, a1, a2, a3, a4, lmax

// One wave per row; dynamic LDS: psis_tail_lds_bytes(M).  ratio, lnl, wout: [n][S]; fields: [n][kFields]
template <bool LOO>
__global__ __launch_bounds__(kWave) void psis_row_kernel(const double* __restrict__ ratio, const double* __restrict__ lnl,
                                                         int64_t S, int64_t M, double* __restrict__ fields,
                                                         double* __restrict__ wout) {
    extern __shared__ uint64_t lds64[];
    const int64_t row = blockIdx.x;
    const double* __restrict__ r = ratio + row * S;
    const double* __restrict__ l = lnl + row * S;
    const PsisRow p = psis_row<LOO>([&](int64_t s) { return r[s]; }, [&](int64_t s) { return l[s]; }, S, M, lds64,
                                    wout + row * S);
    if (lane_id() == 0) {
        double* f = fields + row * kFields;
        f[0] = p.khat;
        f[1] = p.mw;
        f[2] = p.m2;
        f[3] = p.a1;
        f[4] = p.a2;
        f[5] = p.a3;
        f[6] = p.a4;
        f[7] = p.lmax;
    }
}

struct DeviceBuffers {
    double *ratio = nullptr, *lnl = nullptr, *fields = nullptr, *wout = nullptr;
    ~DeviceBuffers() {
        (void)hipFree(ratio);
        (void)hipFree(lnl);
        (void)hipFree(fields);
        (void)hipFree(wout);
    }
};

}  // namespace

// ratio, lnl: [n][S] on the host; loo != 0: psis_row<true> (the caller passes ratio == -lnl).  fields: [n][8] in PsisRow's
// order; wout: [n][S], NaN where the kernel wrote nothing.  M as the entry points can produce it: M < 5 (no tail), or
// 5 <= M <= min(ceil(0.2 S), kPsisMaxTail), which leaves a cutoff (M + 1 <= S).  Returns the HIP error (0: success).
extern "C" int psis_row_harness(int64_t n, int64_t S, int64_t M, int loo, const double* ratio, const double* lnl,
                                double* fields, double* wout) {
    if (n <= 0 || S <= 0 || M < 0 || !ratio || !lnl || !fields || !wout) return (int)hipErrorInvalidValue;
    if (n > 65535 || S > (int64_t)1 << 24) return (int)hipErrorInvalidValue;
    if (M >= 5 && (M > kPsisMaxTail || (double)M > std::ceil(0.2 * (double)S) || M + 1 > S)) return (int)hipErrorInvalidValue;
    const size_t bytes = (size_t)n * (size_t)S * sizeof(double), fbytes = (size_t)n * kFields * sizeof(double);
    DeviceBuffers d;
    hipError_t e;
    if ((e = hipMalloc((void**)&d.ratio, bytes)) != hipSuccess) return (int)e;
    if ((e = hipMalloc((void**)&d.lnl, bytes)) != hipSuccess) return (int)e;
    if ((e = hipMalloc((void**)&d.fields, fbytes)) != hipSuccess) return (int)e;
    if ((e = hipMalloc((void**)&d.wout, bytes)) != hipSuccess) return (int)e;
    if ((e = hipMemcpy(d.ratio, ratio, bytes, hipMemcpyHostToDevice)) != hipSuccess) return (int)e;
    if ((e = hipMemcpy(d.lnl, lnl, bytes, hipMemcpyHostToDevice)) != hipSuccess) return (int)e;
    if ((e = hipMemset(d.fields, 0xff, fbytes)) != hipSuccess) return (int)e;      // all bits set: a NaN
    if ((e = hipMemset(d.wout, 0xff, bytes)) != hipSuccess) return (int)e;
    const size_t lds = psis_tail_lds_bytes(M);                                       // as the product's launches size it
    if (loo)
        hipLaunchKernelGGL(psis_row_kernel<true>, dim3((unsigned)n), dim3(kWave), lds, 0, d.ratio, d.lnl, S, M, d.fields,
                           d.wout);
    else
        hipLaunchKernelGGL(psis_row_kernel<false>, dim3((unsigned)n), dim3(kWave), lds, 0, d.ratio, d.lnl, S, M, d.fields,
                           d.wout);
    if ((e = hipGetLastError()) != hipSuccess) return (int)e;
    if ((e = hipDeviceSynchronize()) != hipSuccess) return (int)e;
    if ((e = hipMemcpy(fields, d.fields, fbytes, hipMemcpyDeviceToHost)) != hipSuccess) return (int)e;
    if ((e = hipMemcpy(wout, d.wout, bytes, hipMemcpyDeviceToHost)) != hipSuccess) return (int)e;
    return 0;
}

// erk_psi_probe.hip — test-only translation unit (tests/test_gpu_erk_psi_probe.py): the unicycle's ERK4
// stage map erk_unicycle of mpcg_device.h at given (z, pi), one point per lane of one wavefront per workgroup,
// in its plain form and with sin / cos of psi given by the caller (Cfg::PSI_SHARED).
// Writes xn, [B A] and the Hessian accumulated onto a given start of every lane.
// Host pointers in, host pointers out; returns the hipError_t of the first failing call (0 = ok).
#include <hip/hip_runtime.h>

#include <cstddef>

#include "mpcg.h"
#include "mpcg_device.h"

namespace {

using mpcg::NU;
constexpr int NX = 5, NZ = NU + NX;

// z [n][NZ], pi [n][NX], H0 [n][NZ][NZ] in; xn [n][NX], F [n][NX][NZ], H [n][NZ][NZ] out
template <bool PSI>
__global__ void __launch_bounds__(64) k_erk(mpcg_problem pr, int n, const double* z, const double* pi, const double* H0,
                                            double* xn, double* F, double* H) {
    const int i = blockIdx.x * 64 + threadIdx.x;
    if (i >= n) return;
    double zz[NZ], pp[NX], xx[NX], FF[NX][NZ], HH[NZ][NZ];
    for (int j = 0; j < NZ; ++j) zz[j] = z[(size_t)i * NZ + j];
    for (int j = 0; j < NX; ++j) pp[j] = pi[(size_t)i * NX + j];
    for (int a = 0; a < NZ; ++a)
        for (int b = 0; b < NZ; ++b) HH[a][b] = H0[((size_t)i * NZ + a) * NZ + b];
    double sp = 0.0, cp = 0.0;
    if (PSI) sincos(zz[4], &sp, &cp);
    mpcg::erk_unicycle<NX, PSI>(pr, zz, pp, xx, FF, HH, sp, cp);
    for (int a = 0; a < NX; ++a) {
        xn[(size_t)i * NX + a] = xx[a];
        for (int b = 0; b < NZ; ++b) F[((size_t)i * NX + a) * NZ + b] = FF[a][b];
    }
    for (int a = 0; a < NZ; ++a)
        for (int b = 0; b < NZ; ++b) H[((size_t)i * NZ + a) * NZ + b] = HH[a][b];
}

}  // namespace

extern "C" {

int probe_abi_version(void) { return MPCG_ABI_VERSION; }

// form 0: erk_unicycle forms sin / cos of psi; 1: given by the caller.  The unicycle without the slack state
int probe_erk_psi(const mpcg_problem* pr, int form, int n, const double* z, const double* pi, const double* H0,
                   double* xn, double* F, double* H) {
    if (n <= 0 || form < 0 || form > 1 || pr->model != MPCG_MODEL_UNICYCLE || pr->nx != NX) return -1;
    const size_t bytes[6] = {(size_t)n * NZ * sizeof(double),      (size_t)n * NX * sizeof(double),
                             (size_t)n * NZ * NZ * sizeof(double), (size_t)n * NX * sizeof(double),
                             (size_t)n * NX * NZ * sizeof(double), (size_t)n * NZ * NZ * sizeof(double)};
    const double* in[3] = {z, pi, H0};
    double* out[3] = {xn, F, H};
    double* d[6] = {};
    hipError_t err = hipSuccess;
    for (int j = 0; j < 6 && err == hipSuccess; ++j) err = hipMalloc(&d[j], bytes[j]);
    for (int j = 0; j < 3 && err == hipSuccess; ++j) err = hipMemcpy(d[j], in[j], bytes[j], hipMemcpyHostToDevice);
    if (err == hipSuccess) {
        const dim3 grid((n + 63) / 64), block(64);
        if (form == 0) k_erk<false><<<grid, block>>>(*pr, n, d[0], d[1], d[2], d[3], d[4], d[5]);
        if (form == 1) k_erk<true><<<grid, block>>>(*pr, n, d[0], d[1], d[2], d[3], d[4], d[5]);
        err = hipGetLastError();
    }
    if (err == hipSuccess) err = hipDeviceSynchronize();
    for (int j = 0; j < 3 && err == hipSuccess; ++j) err = hipMemcpy(out[j], d[3 + j], bytes[3 + j], hipMemcpyDeviceToHost);
    for (int j = 0; j < 6; ++j)
        if (d[j]) (void)hipFree(d[j]);
    return (int)err;
}

}  // extern "C"

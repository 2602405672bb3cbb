// fac_rows_probe.hip — test-only translation unit (tests/test_gpu_fac_rows_probe.py): the unicycle's
// ERK4 stage map erk_unicycle of mpcg_device.h at given (z, pi), one point per lane of one wavefront per
// workgroup, as the linearisation of the SQP kernel calls it (one stage per lane, with multipliers).
// Writes the Jacobian [B A] of every lane, so that the rows Cfg::FAC_INVARIANT_ROWS keeps in registers
// over the stages of the Riccati loop (psi+, v+, s+, slack+) can be compared across the lanes bit for bit.
// Host pointers in, host pointers out; returns the hipError_t of the first failing call (0 = ok).
#include <hip/hip_runtime.h>

#include <cstddef>

#include "mpcg.h"
#include "mpcg_device.h"

namespace {

using mpcg::NU;

// z [n][NZ], pi [n][NX] in; F [n][NX][NZ], xn [n][NX] out
template <int NX>
__global__ void __launch_bounds__(64) k_erk_wave(mpcg_problem pr, int n, const double* z, const double* pi, double* F,
                                                 double* xn) {
    constexpr int NZ = NU + NX;
    const int i = blockIdx.x * 64 + threadIdx.x;
    if (i >= n) return;
    double zz[NZ], pp[NX], xx[NX], FF[NX][NZ], HH[NZ][NZ];
    for (int j = 0; j < NZ; ++j) zz[j] = z[(size_t)i * NZ + j];
    for (int j = 0; j < NX; ++j) pp[j] = pi[(size_t)i * NX + j];
    for (int a = 0; a < NZ; ++a)
        for (int b = 0; b < NZ; ++b) HH[a][b] = 0.0;
    mpcg::erk_unicycle<NX>(pr, zz, pp, xx, FF, HH);
    for (int a = 0; a < NX; ++a) {
        xn[(size_t)i * NX + a] = xx[a];
        for (int b = 0; b < NZ; ++b) F[((size_t)i * NX + a) * NZ + b] = FF[a][b];
    }
}

template <int NX>
int run(const mpcg_problem* pr, int n, const double* z, const double* pi, double* F, double* xn) {
    constexpr int NZ = NU + NX;
    const size_t bytes[4] = {(size_t)n * NZ * sizeof(double), (size_t)n * NX * sizeof(double),
                             (size_t)n * NX * NZ * sizeof(double), (size_t)n * NX * sizeof(double)};
    double* d[4] = {};
    hipError_t err = hipSuccess;
    for (int j = 0; j < 4 && err == hipSuccess; ++j) err = hipMalloc(&d[j], bytes[j]);
    if (err == hipSuccess) err = hipMemcpy(d[0], z, bytes[0], hipMemcpyHostToDevice);
    if (err == hipSuccess) err = hipMemcpy(d[1], pi, bytes[1], hipMemcpyHostToDevice);
    if (err == hipSuccess) {
        k_erk_wave<NX><<<(n + 63) / 64, 64>>>(*pr, n, d[0], d[1], d[2], d[3]);
        err = hipGetLastError();
    }
    if (err == hipSuccess) err = hipDeviceSynchronize();
    if (err == hipSuccess) err = hipMemcpy(F, d[2], bytes[2], hipMemcpyDeviceToHost);
    if (err == hipSuccess) err = hipMemcpy(xn, d[3], bytes[3], hipMemcpyDeviceToHost);
    for (int j = 0; j < 4; ++j)
        if (d[j]) (void)hipFree(d[j]);
    return (int)err;
}

}  // namespace

extern "C" {

int probe_abi_version(void) { return MPCG_ABI_VERSION; }

// the unicycle (nx 5) or its slack model (nx 6), by pr->nx
int probe_erk_wave(const mpcg_problem* pr, int n, const double* z, const double* pi, double* F, double* xn) {
    if (n <= 0 || pr->model != MPCG_MODEL_UNICYCLE || (pr->nx != 5 && pr->nx != 6)) return -1;
    return pr->nx == 5 ? run<5>(pr, n, z, pi, F, xn) : run<6>(pr, n, z, pi, F, xn);
}

}  // extern "C"

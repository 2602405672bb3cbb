// mirror_probe.hip — test-only translation unit (tests/test_gpu_mirror_blocks.py): the MIRROR
// regularisation of mpcg_device.h on given 7 x 7 matrices, one matrix per lane, one wavefront per
// workgroup as in the SQP kernel.  Matrix i is run through
//   mirror<7, 7, true>   the block form, forced                  -> Hb[i]
//   mirror<7>            the general form                        -> Hg[i]
//   mirror_blocks_ok<7>  the lane's own half of the decision     -> ok[i]    (1.0 / 0.0)
//   mirror_stage<7>      what the linearisation calls            -> Hs[i], took[i] (1.0: block form)
// mirror_stage decides per wave: matrices 64 w .. 64 w + 63 share a decision, and the lanes past n
// have left before it, as the non-stage lanes have in the kernel.
// Host pointers in, host pointers out; returns the hipError_t of the first failing call (0 = ok).
#include <hip/hip_runtime.h>

#include <cstddef>

#include "mpcg.h"
#include "mpcg_device.h"

namespace {

constexpr int NZ = 7, NN = NZ * NZ;

__global__ void __launch_bounds__(64) k_mirror(int n, double eps, const double* A, double* Hb, double* Hg, double* Hs,
                                               double* ok, double* took) {
    const int i = blockIdx.x * 64 + threadIdx.x;
    if (i >= n) return;
    double M[NZ][NZ];
    auto load = [&]() {
        for (int a = 0; a < NZ; ++a)
            for (int b = 0; b < NZ; ++b) M[a][b] = A[(size_t)i * NN + a * NZ + b];
    };
    auto store = [&](double* out) {
        for (int a = 0; a < NZ; ++a)
            for (int b = 0; b < NZ; ++b) out[(size_t)i * NN + a * NZ + b] = M[a][b];
    };
    load();
    ok[i] = mpcg::mirror_blocks_ok<NZ>(M) ? 1.0 : 0.0;
    mpcg::mirror<NZ, NZ, true>(M, eps);
    store(Hb);
    load();
    mpcg::mirror<NZ>(M, eps);
    store(Hg);
    load();
    took[i] = mpcg::mirror_stage<NZ>(M, eps) ? 1.0 : 0.0;
    store(Hs);
}

}  // namespace

extern "C" {

int probe_abi_version(void) { return MPCG_ABI_VERSION; }

// A [n][7][7] in; Hb, Hg, Hs [n][7][7] and ok, took [n] out
int probe_mirror(int n, double eps, const double* A, double* Hb, double* Hg, double* Hs, double* ok, double* took) {
    if (n <= 0) return -1;
    const size_t mat = (size_t)n * NN * sizeof(double), vec = (size_t)n * sizeof(double);
    double* d[6] = {};
    const size_t bytes[6] = {mat, mat, mat, mat, vec, vec};
    double* const host[6] = {nullptr, Hb, Hg, Hs, ok, took};
    hipError_t err = hipSuccess;
    for (int j = 0; j < 6 && err == hipSuccess; ++j) err = hipMalloc(&d[j], bytes[j]);
    if (err == hipSuccess) err = hipMemcpy(d[0], A, mat, hipMemcpyHostToDevice);
    if (err == hipSuccess) {
        k_mirror<<<(n + 63) / 64, 64>>>(n, eps, d[0], d[1], d[2], d[3], d[4], d[5]);
        err = hipGetLastError();
    }
    if (err == hipSuccess) err = hipDeviceSynchronize();
    for (int j = 1; j < 6 && err == hipSuccess; ++j) err = hipMemcpy(host[j], d[j], bytes[j], hipMemcpyDeviceToHost);
    for (int j = 0; j < 6; ++j)
        if (d[j]) (void)hipFree(d[j]);
    return (int)err;
}

}  // extern "C"

// stage_probe.hip — test-only translation unit (tests/test_gpu_stage_functions.py): single-thread
// kernels that call the product's own per-stage device functions (mpcg_device.h, mpcg_bicycle.h)
// at given points and write what they return to plain buffers, so that the functions the SQP
// kernel inlines can be compared with the golden stage vectors and the oracle one array at a time.
// Host pointers in, host pointers out; every entry point returns the hipError_t of its first
// failing call (0 = ok).  Point i uses z[i], p[i] (and adj[i]); one block of one thread per point.
#include <hip/hip_runtime.h>

#include <cstddef>

#include "mpcg.h"
#include "mpcg_bicycle.h"
#include "mpcg_device.h"

namespace {

using mpcg::NU;
using mpcg::bike::NXB;
using mpcg::bike::NZB;
constexpr int HSB = (NZB - 1) * NZB / 2;  // packed adjoint Hessian of bike::discrete

template <int NX>
__global__ void k_stage_cost(mpcg_problem pr, int n, const double* z, const double* p, double* L, double* L0,
                             double* g, double* H) {
    constexpr int NZ = NU + NX;
    const int i = blockIdx.x;
    if (i >= n || threadIdx.x != 0) return;
    double zz[NZ], gg[NZ], HH[NZ][NZ];
    for (int j = 0; j < NZ; ++j) zz[j] = z[(size_t)i * NZ + j];
    const double* pp = p + (size_t)i * pr.npar;
    L[i] = mpcg::stage_cost<NX>(pr, pp, zz, gg, HH, true);
    for (int a = 0; a < NZ; ++a) {
        g[(size_t)i * NZ + a] = gg[a];
        for (int b = 0; b < NZ; ++b) H[((size_t)i * NZ + a) * NZ + b] = HH[a][b];
    }
    L0[i] = mpcg::stage_cost<NX>(pr, pp, zz, gg, HH, false);  // the value-only path (the merit evaluations)
}

__global__ void k_bike_cost(mpcg_problem pr, int n, int k, const double* z, const double* p, double* L, double* L0,
                            double* g, double* H) {
    const int i = blockIdx.x;
    if (i >= n || threadIdx.x != 0) return;
    double zz[NZB], gg[NZB], HH[NZB][NZB];
    for (int j = 0; j < NZB; ++j) zz[j] = z[(size_t)i * NZB + j];
    const double* pp = p + (size_t)i * pr.npar;
    L[i] = mpcg::bike::stage_cost(pr, pp, k, zz, gg, HH, true);
    for (int a = 0; a < NZB; ++a) {
        g[(size_t)i * NZB + a] = gg[a];
        for (int b = 0; b < NZB; ++b) H[((size_t)i * NZB + a) * NZB + b] = HH[a][b];
    }
    L0[i] = mpcg::bike::stage_cost(pr, pp, k, zz, gg, HH, false);
}

// xn [n][6]; F [n][4][8]: the rows of x+, y+, psi+, s+ over z without the slack column; Hs [n][36] packed
__global__ void k_bike_discrete(mpcg_problem pr, int n, const double* z, const double* p, const double* adj,
                                double* xn, double* F, double* Hs) {
    const int i = blockIdx.x;
    if (i >= n || threadIdx.x != 0) return;
    double zz[NZB], xx[NXB], FF[4][NZB - 1], HH[HSB];
    for (int j = 0; j < NZB; ++j) zz[j] = z[(size_t)i * NZB + j];
    mpcg::bike::discrete(pr, p + (size_t)i * pr.npar, zz, adj ? adj + (size_t)i * NXB : nullptr, xx, FF, HH);
    for (int j = 0; j < NXB; ++j) xn[(size_t)i * NXB + j] = xx[j];
    for (int a = 0; a < 4; ++a)
        for (int b = 0; b < NZB - 1; ++b) F[((size_t)i * 4 + a) * (NZB - 1) + b] = FF[a][b];
    for (int j = 0; j < HSB; ++j) Hs[(size_t)i * HSB + j] = HH[j];
}

// xn [n][NX]; F [n][NX][NZ] = [B A]; H [n][NZ][NZ] = Hess(adj' x+) added to zero
template <int NX>
__global__ void k_erk(mpcg_problem pr, int n, const double* z, const double* adj, double* xn, double* F, double* H) {
    constexpr int NZ = NU + NX;
    const int i = blockIdx.x;
    if (i >= n || threadIdx.x != 0) return;
    double zz[NZ], xx[NX], FF[NX][NZ], HH[NZ][NZ];
    for (int j = 0; j < NZ; ++j) zz[j] = z[(size_t)i * NZ + j];
    for (int a = 0; a < NZ; ++a)
        for (int b = 0; b < NZ; ++b) HH[a][b] = 0.0;
    mpcg::erk_unicycle<NX>(pr, zz, adj ? adj + (size_t)i * NX : nullptr, xx, FF, HH);
    for (int a = 0; a < NX; ++a) {
        xn[(size_t)i * NX + a] = xx[a];
        for (int b = 0; b < NZ; ++b) F[((size_t)i * NX + a) * NZ + b] = FF[a][b];
    }
    for (int a = 0; a < NZ; ++a)
        for (int b = 0; b < NZ; ++b) H[((size_t)i * NZ + a) * NZ + b] = HH[a][b];
}

// device copies of the host arrays of one call; results copied back by out()
struct Bufs {
    static constexpr int MAX = 12;
    double* d[MAX] = {};
    double* h[MAX] = {};
    size_t len[MAX] = {};
    int used = 0;
    hipError_t err = hipSuccess;

    double* in(const double* host, size_t count) { return add(const_cast<double*>(host), count, true); }
    double* out(double* host, size_t count) { return add(host, count, false); }
    double* add(double* host, size_t count, bool upload) {
        if (err != hipSuccess || host == nullptr || used == MAX) return nullptr;
        double* p = nullptr;
        err = hipMalloc(&p, count * sizeof(double));
        if (err != hipSuccess) return nullptr;
        d[used] = p;
        if (upload)
            err = hipMemcpy(p, host, count * sizeof(double), hipMemcpyHostToDevice);
        else {
            h[used] = host;
            len[used] = count;
        }
        ++used;
        return err == hipSuccess ? p : nullptr;
    }
    int finish() {
        if (err == hipSuccess) err = hipGetLastError();
        if (err == hipSuccess) err = hipDeviceSynchronize();
        for (int i = 0; i < used && err == hipSuccess; ++i)
            if (h[i]) err = hipMemcpy(h[i], d[i], len[i] * sizeof(double), hipMemcpyDeviceToHost);
        for (int i = 0; i < used; ++i) (void)hipFree(d[i]);
        return (int)err;
    }
};

template <int NX>
int run_stage_cost(const mpcg_problem* pr, int n, const double* z, const double* p, double* L, double* L0, double* g,
                   double* H) {
    constexpr int NZ = NU + NX;
    Bufs b;
    const double *dz = b.in(z, (size_t)n * NZ), *dp = b.in(p, (size_t)n * pr->npar);
    double *dL = b.out(L, n), *dL0 = b.out(L0, n), *dg = b.out(g, (size_t)n * NZ), *dH = b.out(H, (size_t)n * NZ * NZ);
    if (b.err == hipSuccess) k_stage_cost<NX><<<n, 1>>>(*pr, n, dz, dp, dL, dL0, dg, dH);
    return b.finish();
}

template <int NX>
int run_erk(const mpcg_problem* pr, int n, const double* z, const double* adj, double* xn, double* F, double* H) {
    constexpr int NZ = NU + NX;
    Bufs b;
    const double *dz = b.in(z, (size_t)n * NZ), *da = b.in(adj, (size_t)n * NX);
    double *dx = b.out(xn, (size_t)n * NX), *dF = b.out(F, (size_t)n * NX * NZ), *dH = b.out(H, (size_t)n * NZ * NZ);
    if (b.err == hipSuccess) k_erk<NX><<<n, 1>>>(*pr, n, dz, da, dx, dF, dH);
    return b.finish();
}

}  // namespace

extern "C" {

int probe_abi_version(void) { return MPCG_ABI_VERSION; }

// unicycle stage cost, nx 5 or 6 (pr->nx)
int probe_stage_cost(const mpcg_problem* pr, int n, const double* z, const double* p, double* L, double* L0, double* g,
                     double* H) {
    if (n <= 0 || pr->model != MPCG_MODEL_UNICYCLE || (pr->nx != 5 && pr->nx != 6)) return -1;
    return pr->nx == 5 ? run_stage_cost<5>(pr, n, z, p, L, L0, g, H) : run_stage_cost<6>(pr, n, z, p, L, L0, g, H);
}

// bicycle stage cost of stage k
int probe_bike_stage_cost(const mpcg_problem* pr, int n, int k, const double* z, const double* p, double* L,
                          double* L0, double* g, double* H) {
    if (n <= 0 || pr->model != MPCG_MODEL_BICYCLE_CA) return -1;
    Bufs b;
    const double *dz = b.in(z, (size_t)n * NZB), *dp = b.in(p, (size_t)n * pr->npar);
    double *dL = b.out(L, n), *dL0 = b.out(L0, n), *dg = b.out(g, (size_t)n * NZB);
    double* dH = b.out(H, (size_t)n * NZB * NZB);
    if (b.err == hipSuccess) k_bike_cost<<<n, 1>>>(*pr, n, k, dz, dp, dL, dL0, dg, dH);
    return b.finish();
}

// bicycle discrete map; adj may be NULL (Hs then holds what the function leaves without multipliers)
int probe_bike_discrete(const mpcg_problem* pr, int n, const double* z, const double* p, const double* adj, double* xn,
                        double* F, double* Hs) {
    if (n <= 0 || pr->model != MPCG_MODEL_BICYCLE_CA) return -1;
    Bufs b;
    const double *dz = b.in(z, (size_t)n * NZB), *dp = b.in(p, (size_t)n * pr->npar);
    const double* da = b.in(adj, (size_t)n * NXB);
    double *dx = b.out(xn, (size_t)n * NXB), *dF = b.out(F, (size_t)n * 4 * (NZB - 1));
    double* dH = b.out(Hs, (size_t)n * HSB);
    if (b.err == hipSuccess) k_bike_discrete<<<n, 1>>>(*pr, n, dz, dp, da, dx, dF, dH);
    return b.finish();
}

// ERK4 of the unicycle, nx 5 or 6 (pr->nx); adj may be NULL (H stays zero)
int probe_erk_unicycle(const mpcg_problem* pr, int n, const double* z, const double* adj, double* xn, double* F,
                       double* H) {
    if (n <= 0 || pr->model != MPCG_MODEL_UNICYCLE || (pr->nx != 5 && pr->nx != 6)) return -1;
    return pr->nx == 5 ? run_erk<5>(pr, n, z, adj, xn, F, H) : run_erk<6>(pr, n, z, adj, xn, F, H);
}

}  // extern "C"

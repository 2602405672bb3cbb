// mpcg_active.hip — entry points of the active-solve compaction (include/mpcg_active.h).
// Compiled on its own with -ffp-contract=off, like mpcg_guidance.hip; the kernels only copy and count.
#include <hip/hip_runtime.h>

#include <string>

#include "mpcg_active.h"
#include "mpcg_host.h"

using namespace mpcg::host;

struct mpcg_active_ws {
    int device, max_batch;
    int N, npar, nx, nu, nh;
    bool lam, qp, stats;
    mpcg::ActiveSizes z;
    mpcg_io dense;   // every pointer owned; the optional ones NULL when not asked for
    int *slot_of, *solve_of, *n_active;
    int* pinned;     // one host word
};

namespace {

// block sizes of `pr`; with_qp: whether the QP memory's size is needed (it needs a compiled instance)
int sizes_of(const char* who, const mpcg_problem* pr, bool with_qp, mpcg::ActiveSizes* z) {
    if (pr->N < 1 || pr->npar < 1 || pr->nx < 1 || pr->nx > MPCG_MAX_NX || pr->nu < 1 || pr->nu > MPCG_MAX_NU)
        return fail(who, "invalid problem dimensions");
    z->N = pr->N;
    z->nx = pr->nx;
    z->nu = pr->nu;
    z->params = pr->N * pr->npar;
    z->warm = (pr->N + 1) * (pr->nu + pr->nx);
    z->xinit = pr->nx;
    z->xtraj = (pr->N + 1) * pr->nx;
    z->utraj = pr->N * pr->nu;
    z->lam = mpcg_lam_size(pr);
    z->qp = 0;
    if (with_qp) {
        z->qp = mpcg_qp_mem_size(pr);
        if (z->qp < 0) return fail(who, "QP memory needs a compiled kernel instance of the problem");
    }
    return 0;
}

template <class T>
bool dev_alloc(T** p, size_t n) {
    return hipMalloc(reinterpret_cast<void**>(p), (n ? n : 1) * sizeof(T)) == hipSuccess;
}

}  // namespace

extern "C" {

int mpcg_active_plan(int batch, const unsigned char* enabled, int* slot_of, int* solve_of, int* n_active,
                     void* stream) {
    const char* who = "mpcg_active_plan";
    if (batch < 0) return fail(who, "negative batch");
    if (!enabled || !slot_of || !solve_of || !n_active) return fail(who, "invalid arguments");
    // (an empty batch still writes the count)
    hipLaunchKernelGGL(mpcg::active_plan_kernel, dim3(1), dim3(mpcg::ACT_PLAN_LANES), 0, (hipStream_t)stream, batch,
                       enabled, slot_of, solve_of, n_active);
    return launched("active plan");
}

int mpcg_active_gather(const mpcg_problem* pr, int batch, const int* slot_of, const mpcg_io* full,
                       const mpcg_io* dense, void* stream) {
    const char* who = "mpcg_active_gather";
    if (batch < 0) return fail(who, "negative batch");
    if (!pr || !slot_of || !full || !dense) return fail(who, "invalid arguments");
    if (!full->params || !full->warm || !full->xinit) return fail(who, "null input of the full batch");
    if (!dense->params || !dense->warm || !dense->xinit) return fail(who, "null input of the dense batch");
    mpcg::ActiveSizes z;
    if (sizes_of(who, pr, full->qp_in && dense->qp_in, &z) != 0) return -1;
    if (batch == 0) return 0;
    hipLaunchKernelGGL(mpcg::active_gather_kernel, dim3(batch), dim3(mpcg::ACT_COPY_LANES), 0, (hipStream_t)stream,
                       batch, z, slot_of, *full, *dense);
    return launched("active gather");
}

int mpcg_active_scatter(const mpcg_problem* pr, int batch, const int* slot_of, const mpcg_io* dense,
                        const mpcg_io* full, void* stream) {
    const char* who = "mpcg_active_scatter";
    if (batch < 0) return fail(who, "negative batch");
    if (!pr || !slot_of || !full || !dense) return fail(who, "invalid arguments");
    if ((full->xtraj || full->utraj) && !full->warm)
        return fail(who, "the fill of xtraj / utraj needs the warm start of the full batch");
    if ((full->xtraj && !dense->xtraj) || (full->utraj && !dense->utraj) || (full->pobj && !dense->pobj) ||
        (full->exit_code && !dense->exit_code) || (full->info && !dense->info) ||
        (full->lam_out && !dense->lam_out) || (full->qp_out && !dense->qp_out) || (full->stats && !dense->stats))
        return fail(who, "an output of the full batch has no dense counterpart");
    mpcg::ActiveSizes z;
    if (sizes_of(who, pr, full->qp_out != nullptr, &z) != 0) return -1;
    if (batch == 0) return 0;
    hipLaunchKernelGGL(mpcg::active_scatter_kernel, dim3(batch), dim3(mpcg::ACT_COPY_LANES), 0, (hipStream_t)stream,
                       batch, z, slot_of, *dense, *full);
    return launched("active scatter");
}

mpcg_active_ws* mpcg_active_ws_create(const mpcg_problem* pr, int max_batch, int with_lam, int with_qp,
                                      int with_stats) {
    const char* who = "mpcg_active_ws_create";
    if (!pr || max_batch < 1) {
        fail(who, "invalid arguments");
        return nullptr;
    }
    mpcg::ActiveSizes z;
    if (sizes_of(who, pr, with_qp != 0, &z) != 0) return nullptr;
    mpcg_active_ws* ws = new mpcg_active_ws();
    ws->max_batch = max_batch;
    ws->N = pr->N, ws->npar = pr->npar, ws->nx = pr->nx, ws->nu = pr->nu, ws->nh = mpcg_num_h(pr);
    ws->lam = with_lam != 0, ws->qp = with_qp != 0, ws->stats = with_stats != 0;
    ws->z = z;
    const size_t B = (size_t)max_batch;
    double *params = nullptr, *warm = nullptr, *xinit = nullptr, *lam_in = nullptr, *qp_in = nullptr;
    bool ok = hipGetDevice(&ws->device) == hipSuccess;
    ok = ok && dev_alloc(&params, B * z.params) && dev_alloc(&warm, B * z.warm) && dev_alloc(&xinit, B * z.xinit);
    ok = ok && dev_alloc(&ws->dense.xtraj, B * z.xtraj) && dev_alloc(&ws->dense.utraj, B * z.utraj) &&
         dev_alloc(&ws->dense.pobj, B) && dev_alloc(&ws->dense.exit_code, B) &&
         dev_alloc(&ws->dense.info, B * MPCG_INFO_STRIDE);
    if (ws->lam) ok = ok && dev_alloc(&lam_in, B * z.lam) && dev_alloc(&ws->dense.lam_out, B * z.lam);
    if (ws->qp) ok = ok && dev_alloc(&qp_in, B * z.qp) && dev_alloc(&ws->dense.qp_out, B * z.qp);
    if (ws->stats) ok = ok && dev_alloc(&ws->dense.stats, B * MPCG_STATS_STRIDE);
    ok = ok && dev_alloc(&ws->slot_of, B) && dev_alloc(&ws->solve_of, B) && dev_alloc(&ws->n_active, 1);
    ok = ok && hipHostMalloc(reinterpret_cast<void**>(&ws->pinned), sizeof(int), hipHostMallocDefault) == hipSuccess;
    ws->dense.params = params, ws->dense.warm = warm, ws->dense.xinit = xinit;
    ws->dense.lam_in = lam_in, ws->dense.qp_in = qp_in;
    if (!ok) {
        (void)hipGetLastError();
        mpcg_active_ws_destroy(ws);
        fail(who, "allocation failed");
        return nullptr;
    }
    return ws;
}

void mpcg_active_ws_destroy(mpcg_active_ws* ws) {
    if (!ws) return;
    const mpcg_io& d = ws->dense;
    const void* dev[] = {d.params, d.warm, d.xinit, d.lam_in, d.xtraj, d.utraj, d.pobj, d.exit_code, d.info,
                         d.lam_out, d.qp_in, d.qp_out, d.stats, ws->slot_of, ws->solve_of, ws->n_active};
    for (const void* p : dev)
        if (p) (void)hipFree(const_cast<void*>(p));
    if (ws->pinned) (void)hipHostFree(ws->pinned);
    delete ws;
}

int mpcg_active_ws_read_plan(const mpcg_active_ws* ws, int batch, int* slot_of, int* solve_of, void* stream) {
    const char* who = "mpcg_active_ws_read_plan";
    if (!ws || batch < 0) return fail(who, "invalid arguments");
    if (batch > ws->max_batch) return fail(who, "batch exceeds the workspace's max_batch");
    if (batch == 0) return 0;
    const size_t n = (size_t)batch * sizeof(int);
    hipError_t e = hipSuccess;
    if (slot_of) e = hipMemcpyAsync(slot_of, ws->slot_of, n, hipMemcpyDeviceToDevice, (hipStream_t)stream);
    if (e == hipSuccess && solve_of)
        e = hipMemcpyAsync(solve_of, ws->solve_of, n, hipMemcpyDeviceToDevice, (hipStream_t)stream);
    return e == hipSuccess ? 0 : hip_fail(who, "copy", e);
}

int mpcg_solve_active(const mpcg_problem* pr, int batch, const mpcg_io* io, const unsigned char* enabled,
                      mpcg_active_ws* ws, int* n_active_host, void* stream) {
    const char* who = "mpcg_solve_active";
    if (batch < 0) return fail(who, "negative batch");
    if (!pr || !io || !enabled || !ws) return fail(who, "invalid arguments");
    if (!io->params || !io->warm || !io->xinit) return fail(who, "null input");
    if (!io->xtraj || !io->utraj || !io->pobj || !io->exit_code) return fail(who, "null output");
    if (batch > ws->max_batch) return fail(who, "batch exceeds the workspace's max_batch");
    if (pr->N != ws->N || pr->npar != ws->npar || pr->nx != ws->nx || pr->nu != ws->nu || mpcg_num_h(pr) != ws->nh)
        return fail(who, "the workspace was created for other problem dimensions");
    if ((io->lam_in || io->lam_out) && !ws->lam) return fail(who, "the workspace was created without multiplier blocks");
    if ((io->qp_in || io->qp_out) && !ws->qp) return fail(who, "the workspace was created without QP memory");
    if (io->stats && !ws->stats) return fail(who, "the workspace was created without NLP residuals");
    int device = -1;
    if (hipGetDevice(&device) != hipSuccess || device != ws->device)
        return fail(who, "the workspace lives on another device than the current one");
    hipStream_t st = (hipStream_t)stream;
    hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(st, &cap) != hipSuccess) (void)hipGetLastError();
    if (cap != hipStreamCaptureStatusNone)
        return fail(who, "not capturable into a graph: the count is read on the host");
    // the dense launch takes exactly the optional buffers the full launch would
    mpcg_io dense = ws->dense;
    if (!io->lam_in) dense.lam_in = nullptr;
    if (!io->lam_out) dense.lam_out = nullptr;
    if (!io->qp_in) dense.qp_in = nullptr;
    if (!io->qp_out) dense.qp_out = nullptr;
    if (!io->stats) dense.stats = nullptr;
    if (!io->info) dense.info = nullptr;
    if (mpcg_active_plan(batch, enabled, ws->slot_of, ws->solve_of, ws->n_active, stream) != 0) return -1;
    if (mpcg_active_gather(pr, batch, ws->slot_of, io, &dense, stream) != 0) return -1;
    hipError_t e = hipMemcpyAsync(ws->pinned, ws->n_active, sizeof(int), hipMemcpyDeviceToHost, st);
    if (e != hipSuccess) return hip_fail(who, "copy of the count", e);
    e = hipStreamSynchronize(st);
    if (e != hipSuccess) return hip_fail(who, "synchronisation", e);
    const int n = *ws->pinned;
    if (n < 0 || n > batch) return fail(who, "the plan's count lies outside 0 .. batch");
    if (n_active_host) *n_active_host = n;
    if (n > 0 && mpcg_solve(pr, n, &dense, stream) != 0) return -1;
    return mpcg_active_scatter(pr, batch, ws->slot_of, &dense, io, stream);
}

}  // extern "C"

// mpcg_active.h — the active-solve compaction on the GPU: the plan of a batch whose disabled
// solves are skipped, the gather of the enabled solves' inputs into a dense batch and the scatter of
// its outputs back (guidance_constraints.cpp:311-318 skips a disabled planner before solve()).
// ABI and the fill of a disabled solve: include/mpcg_active.h; host restatement: active.py
// (plan_host, gather_host, scatter_host).
//
// Three kernels, all copies and integer counts (nothing is rounded), no scratch, no queue loop:
//   active_plan_kernel     ONE workgroup of 1024 lanes (16 wavefronts) walks the batch in passes of 1024:
//                          a lane's rank inside its wavefront is the popcount of the ballot below it, the
//                          16 wave totals meet in LDS and every lane adds those before its own wave in
//                          index order, the running base is carried in a register between passes.  The
//                          batch is a few times 10^4 at most: the launch is latency, not bandwidth.
//   active_gather_kernel   one workgroup of 256 lanes per solve of the FULL batch; a disabled solve returns
//                          at once.  Consecutive lanes copy consecutive doubles (8-byte accesses: a warm
//                          block of 147 doubles is not 16-byte aligned for odd b).
//   active_scatter_kernel  the same shape; a disabled solve writes the fill.
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/mpcg_active.h"  // the public header of the same name

namespace mpcg {

constexpr int ACT_PLAN_LANES = 1024;
constexpr int ACT_PLAN_WAVES = ACT_PLAN_LANES / 64;
constexpr int ACT_COPY_LANES = 256;

// block sizes in doubles (ints for info) of one solve
struct ActiveSizes {
    int params, warm, xinit, xtraj, utraj, lam, qp, nx, nu, N;
};

__global__ __launch_bounds__(ACT_PLAN_LANES) void active_plan_kernel(int batch, const unsigned char* __restrict__ enabled,
                                                                     int* __restrict__ slot_of,
                                                                     int* __restrict__ solve_of,
                                                                     int* __restrict__ n_active) {
    __shared__ int wave_total[ACT_PLAN_WAVES];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int base = 0;   // enabled solves of the passes before this one: the same value in every lane
    for (int start = 0; start < batch; start += ACT_PLAN_LANES) {   // uniform trip count: the barriers are safe
        const int b = start + tid;
        const bool en = b < batch && enabled[b] != 0;
        const unsigned long long m = __ballot(en);
        const int rank = __popcll(m & ((1ull << lane) - 1ull));
        if (lane == 0) wave_total[wave] = __popcll(m);
        __syncthreads();
        int before = 0, total = 0;
        for (int w = 0; w < ACT_PLAN_WAVES; ++w) {
            const int t = wave_total[w];
            before += w < wave ? t : 0;
            total += t;
        }
        if (b < batch) {
            const int slot = base + before + rank;   // < batch: at most b enabled solves precede b
            slot_of[b] = en ? slot : -1;
            if (en) solve_of[slot] = b;
        }
        base += total;
        __syncthreads();   // wave_total is rewritten by the next pass
    }
    for (int i = base + tid; i < batch; i += ACT_PLAN_LANES) solve_of[i] = -1;
    if (tid == 0) n_active[0] = base;
}

__device__ __forceinline__ void act_copy(double* __restrict__ dst, const double* __restrict__ src, int n) {
    for (int i = threadIdx.x; i < n; i += ACT_COPY_LANES) dst[i] = src[i];
}

__device__ __forceinline__ void act_fill(double* __restrict__ dst, int n, double v) {
    for (int i = threadIdx.x; i < n; i += ACT_COPY_LANES) dst[i] = v;
}

__global__ __launch_bounds__(ACT_COPY_LANES) void active_gather_kernel(int batch, ActiveSizes z,
                                                                       const int* __restrict__ slot_of, mpcg_io full,
                                                                       mpcg_io dense) {
    const int b = blockIdx.x;
    if (b >= batch) return;
    const int slot = slot_of[b];
    if (slot < 0 || slot >= batch) return;
    const size_t s = (size_t)slot, f = (size_t)b;
    act_copy(const_cast<double*>(dense.params) + s * z.params, full.params + f * z.params, z.params);
    act_copy(const_cast<double*>(dense.warm) + s * z.warm, full.warm + f * z.warm, z.warm);
    act_copy(const_cast<double*>(dense.xinit) + s * z.xinit, full.xinit + f * z.xinit, z.xinit);
    if (full.lam_in && dense.lam_in)
        act_copy(const_cast<double*>(dense.lam_in) + s * z.lam, full.lam_in + f * z.lam, z.lam);
    if (full.qp_in && dense.qp_in) act_copy(const_cast<double*>(dense.qp_in) + s * z.qp, full.qp_in + f * z.qp, z.qp);
}

__global__ __launch_bounds__(ACT_COPY_LANES) void active_scatter_kernel(int batch, ActiveSizes z,
                                                                        const int* __restrict__ slot_of,
                                                                        mpcg_io dense, mpcg_io full) {
    const int b = blockIdx.x;
    if (b >= batch) return;
    const int slot = slot_of[b];
    const size_t f = (size_t)b;
    const int tid = threadIdx.x;
    if (slot >= 0 && slot < batch) {
        const size_t s = (size_t)slot;
        if (full.xtraj) act_copy(full.xtraj + f * z.xtraj, dense.xtraj + s * z.xtraj, z.xtraj);
        if (full.utraj) act_copy(full.utraj + f * z.utraj, dense.utraj + s * z.utraj, z.utraj);
        if (full.lam_out) act_copy(full.lam_out + f * z.lam, dense.lam_out + s * z.lam, z.lam);
        if (full.qp_out) act_copy(full.qp_out + f * z.qp, dense.qp_out + s * z.qp, z.qp);
        if (full.stats && tid < MPCG_STATS_STRIDE)
            full.stats[f * MPCG_STATS_STRIDE + tid] = dense.stats[s * MPCG_STATS_STRIDE + tid];
        if (full.info && tid < MPCG_INFO_STRIDE)
            full.info[f * MPCG_INFO_STRIDE + tid] = dense.info[s * MPCG_INFO_STRIDE + tid];
        if (tid == 0) {
            if (full.pobj) full.pobj[f] = dense.pobj[s];
            if (full.exit_code) full.exit_code[f] = dense.exit_code[s];
        }
        return;
    }
    // a solve that was not run: the fill of include/mpcg_active.h
    const double inf = __longlong_as_double(0x7ff0000000000000LL), nan = __longlong_as_double(0x7ff8000000000000LL);
    const int nvar = z.nu + z.nx;
    const double* w = full.warm + f * z.warm;
    if (full.xtraj)
        for (int i = tid; i < z.xtraj; i += ACT_COPY_LANES) {
            const int k = i / z.nx, j = i - k * z.nx;
            full.xtraj[f * z.xtraj + i] = w[k * nvar + z.nu + j];
        }
    if (full.utraj)
        for (int i = tid; i < z.utraj; i += ACT_COPY_LANES) {
            const int k = i / z.nu, j = i - k * z.nu;
            full.utraj[f * z.utraj + i] = w[k * nvar + j];
        }
    if (full.lam_out) act_fill(full.lam_out + f * z.lam, z.lam, 0.0);
    if (full.qp_out)
        for (int i = tid; i < z.qp; i += ACT_COPY_LANES) full.qp_out[f * z.qp + i] = i == 0 ? nan : 0.0;
    if (full.stats && tid < MPCG_STATS_STRIDE) full.stats[f * MPCG_STATS_STRIDE + tid] = nan;
    if (full.info && tid < MPCG_INFO_STRIDE) full.info[f * MPCG_INFO_STRIDE + tid] = 0;
    if (tid == 0) {
        if (full.pobj) full.pobj[f] = inf;
        if (full.exit_code) full.exit_code[f] = MPCG_ACTIVE_EXIT_SKIPPED;
    }
}

}  // namespace mpcg

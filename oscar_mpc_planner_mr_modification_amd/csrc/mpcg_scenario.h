// mpcg_scenario.h — the SH-MPC scenario sampler on the GPU: every parallel solver's obstacle samples
// formed from the predictions and a pre-drawn bank of standard-normal pairs, reduced to the scenario
// halfspaces in the same launch, the sample tensor for tests and recordings, and the bookkeeping between
// two SH-MPC control steps.
// ABI, the sampler's definition and the reference lines: include/mpcg_scenario.h; host restatement:
// scenario_sampler.py.
//
// scenario_sample_prepare_kernel<PL>, one workgroup of 4 wavefronts per (scene, copy), the layout of
// scenario_prepare_kernel (mpcg_prepare.h):
//   bank      lane l keeps z of the samples m = l, l + 64, .. (PL per lane) and their obstacle in
//             registers for the whole launch: z does not depend on the stage
//   stage     wave w takes the stages k = 1 + w, 5 + w, ..: lane j < n_obs turns prediction k - 1 of
//             obstacle j into (mx, my, c, s, major, minor) in the wave's own LDS row, one barrier per
//             round of 4 stages (the trip count is the same in every wave), then every lane forms
//             its samples and their distances to p_k in registers
//   reduction a sorted list of each lane's 4 closest, n_scen DPP arg-min rounds over the heads on
//             (distance, index), the list rebuilt from the samples after the lane's last pick when it
//             runs dry: as in scenario_prepare_kernel, so equal distances go to the lower index
//   rows      lane r recomputes the q of round r's pick from (m, k) and forms its row
// then the N x npar parameter block is streamed out.  No sample is stored to global memory.
// No atomics, no communication between workgroups; every loop is bounded by a count taken before it.
// Compiled only into mpcg_scenario.hip with -ffp-contract=off and written with explicitly rounded
// operations in the host restatement's order.
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/mpcg_scenario.h"  // the public header of the same name

namespace mpcg {
namespace scen {

constexpr int MAX_N = MPCG_SCENARIO_MAX_N, MAX_ROWS = MPCG_SCENARIO_MAX_ROWS, MAX_OBS = MPCG_SCENARIO_MAX_OBS;
constexpr int TOPK = 4;  // per-lane candidate list of the arg-min rounds
constexpr int NVMAX = MPCG_NU + MPCG_MAX_NX;
constexpr double DUMMY_B = 100.0;

// include/mpcg_scenario.h, mix
__host__ __device__ inline unsigned long long mix(unsigned long long seed, unsigned long long draw,
                                                  unsigned long long index) {
    unsigned long long x = (seed ^ (draw * 0x9E3779B97F4A7C15ULL)) + index * 0xD1B54A32D192ED03ULL;
    x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ULL;
    x = (x ^ (x >> 27)) * 0x94D049BB133111EBULL;
    return x ^ (x >> 31);
}

__device__ __forceinline__ int batch_of(const mpcg_scenario_sample_io& io, int sol, int j) {
    const size_t e = (size_t)sol * io.n_obs + j;
    if (io.batch_idx) {
        // device data the entry point cannot check: an entry outside the bank reads its nearest batch
        const int b = io.batch_idx[e];
        return b < 0 ? 0 : (b >= io.n_batches ? io.n_batches - 1 : b);
    }
    return (int)(mix(io.seed, io.draw, (unsigned long long)e) % (unsigned long long)io.n_batches);
}

__device__ __forceinline__ double norm2_rn(double dx, double dy) {
    return __dsqrt_rn(__dadd_rn(__dmul_rn(dx, dx), __dmul_rn(dy, dy)));
}

__device__ __forceinline__ double readlane_dbl(double v, int lane) {
    const int lo = __builtin_amdgcn_readlane(__double2loint(v), lane);
    const int hi = __builtin_amdgcn_readlane(__double2hiint(v), lane);
    return __hiloint2double(hi, lo);
}

// one DPP step of a wave arg-min over (distance, index), as in mpcg_prepare.h: lanes outside the row
// mask compare with themselves
template <int CTRL, int ROWS>
__device__ __forceinline__ void dpp_argmin_step(double& d, int& i) {
    const int lo = __builtin_amdgcn_update_dpp(__double2loint(d), __double2loint(d), CTRL, ROWS, 0xf, false);
    const int hi = __builtin_amdgcn_update_dpp(__double2hiint(d), __double2hiint(d), CTRL, ROWS, 0xf, false);
    const int oi = __builtin_amdgcn_update_dpp(i, i, CTRL, ROWS, 0xf, false);
    const double od = __hiloint2double(hi, lo);
    if (od < d || (od == d && oi < i)) {
        d = od;
        i = oi;
    }
}

// the stage constants of one obstacle from its prediction entry o = (x, y, angle, major, minor):
// K = (mx, my, c, s, major, minor)
__device__ __forceinline__ void stage_constants(const double* __restrict__ o, double* K) {
    const double ang = o[2];
    double c = 1.0, s = 0.0;
    if (ang != 0.0) {
        c = cos(ang);
        s = sin(ang);
    }
    K[0] = o[0]; K[1] = o[1]; K[2] = c; K[3] = s; K[4] = o[3]; K[5] = o[4];
}

// q = (mx + (c ex - s ey), my + (s ex + c ey)), ex = major z0, ey = minor z1
__device__ __forceinline__ void sample_point(const double* K, double z0, double z1, double& qx, double& qy) {
    const double ex = __dmul_rn(K[4], z0), ey = __dmul_rn(K[5], z1);
    qx = __dadd_rn(K[0], __dsub_rn(__dmul_rn(K[2], ex), __dmul_rn(K[3], ey)));
    qy = __dadd_rn(K[1], __dadd_rn(__dmul_rn(K[3], ex), __dmul_rn(K[2], ey)));
}

struct SampleLds {
    double warm[MAX_N + 1][NVMAX];
    double rows[MAX_N][MAX_ROWS][3];
    double obs[4][MAX_OBS][6];  // per wave: the stage constants of every obstacle
    double rad[MAX_OBS];        // robot_radius + radius_j
    int batch[MAX_OBS];         // the copy's bank batch per obstacle
};

// PL: samples per lane held in registers (M <= 64 PL); instances 8 / 20 / 32
template <int PL>
__global__ __launch_bounds__(256) void scenario_sample_prepare_kernel(mpcg_problem pr, int n_scenes, int P,
                                                                      mpcg_scenario_sample_io in,
                                                                      double* __restrict__ params,
                                                                      double* __restrict__ warm,
                                                                      double* __restrict__ xinit) {
    __shared__ SampleLds L;
    const int sol = blockIdx.x;
    const int sc = sol / P;
    if (sc >= n_scenes) return;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int N = pr.N, npar = pr.npar, nx = pr.nx, NV = MPCG_NU + nx, NS = pr.n_scen;
    const int n_obs = in.n_obs, n_per = in.n_per, M = n_obs * n_per;
    const double dt = pr.dt;
    const double* st = in.state + (size_t)sc * nx;

    // ---- warm start: the main solver's, or Solver::initializeWithBraking (other entries 0)
    if (in.main_warm) {
        const double* mw = in.main_warm + (size_t)sc * (N + 1) * NV;
        for (int e = tid; e < (N + 1) * NV; e += 256) L.warm[e / NV][e % NV] = mw[e];
    } else if (tid == 0) {
        double x = st[0], y = st[1], psi = st[2], v = st[3], s = st[4];
        const double a = -fabs(in.deceleration);
        const double c = cos(psi), sn = sin(psi);
        for (int k = 0; k <= N; ++k) {
            if (k > 0) {
                x = __dadd_rn(x, __dmul_rn(__dmul_rn(v, dt), c));
                y = __dadd_rn(y, __dmul_rn(__dmul_rn(v, dt), sn));
                s = __dadd_rn(s, __dmul_rn(v, dt));
                v = fmax(__dadd_rn(v, __dmul_rn(a, dt)), 0.0);
            }
            double* w = L.warm[k];
            w[0] = a; w[1] = 0.0; w[2] = x; w[3] = y; w[4] = psi; w[5] = v; w[6] = s;
            for (int i = 7; i < NV; ++i) w[i] = 0.0;
        }
    }
    // ---- the copy's batch and the radius per obstacle
    if (tid >= 64 && tid < 64 + n_obs) {
        const int j = tid - 64;
        L.batch[j] = batch_of(in, sol, j);
        L.rad[j] = __dadd_rn(in.robot_radius, in.obst_meta[((size_t)sc * n_obs + j) * 2]);
    }
    __syncthreads();

    // ---- this lane's z and obstacle per register slot, for every stage
    double z0[PL], z1[PL];
    int ob[PL];
    int mine = 0;  // samples of this lane
#pragma unroll
    for (int jj = 0; jj < PL; ++jj) {
        const int m = lane + 64 * jj;
        z0[jj] = 0.0;
        z1[jj] = 0.0;
        ob[jj] = 0;
        if (m < M) {
            const int j = m / n_per, i = m - j * n_per;
            const double* z = in.bank + ((size_t)L.batch[j] * n_per + i) * 2;
            z0[jj] = z[0];
            z1[jj] = z[1];
            ob[jj] = j;
            ++mine;
        }
    }

    // ---- sample -> halfspace reduction, one stage per wave at a time, 4 stages per round
    const double INF = __longlong_as_double(0x7ff0000000000000LL);
    constexpr int BIG = 0x7fffffff;
    const int rounds = (N - 1 + 3) / 4;
    for (int rd = 0; rd < rounds; ++rd) {
        const int k = 1 + 4 * rd + wave;
        const bool active = k < N;
        double(*K)[6] = L.obs[wave];
        if (active && lane < n_obs)
            stage_constants(in.obst + (((size_t)sc * n_obs + lane) * N + (k - 1)) * 5, K[lane]);
        __syncthreads();
        if (!active) continue;  // the last round of this wave; no barrier follows it
        const double rx = L.warm[k][2], ry = L.warm[k][3];
        double dist[PL];
#pragma unroll
        for (int jj = 0; jj < PL; ++jj) {
            double d = INF;
            if (lane + 64 * jj < M) {
                double qx, qy;
                sample_point(K[ob[jj]], z0[jj], z1[jj], qx, qy);
                d = norm2_rn(__dsub_rn(qx, rx), __dsub_rn(qy, ry));
            }
            dist[jj] = d;
        }
        int left = mine;  // samples of this lane not picked yet
        // each lane keeps its TOPK closest samples sorted by (distance, index); the list is rebuilt from
        // the samples after the last pick when it runs dry
        double td[TOPK];
        int ti[TOPK];
        double lastd = -1.0;
        int lasti = -1;
        auto rebuild = [&]() {
#pragma unroll
            for (int t = 0; t < TOPK; ++t) { td[t] = INF; ti[t] = BIG; }
#pragma unroll
            for (int jj = 0; jj < PL; ++jj) {
                double x = dist[jj];
                int xi = lane + 64 * jj;
                if (!(x > lastd || (x == lastd && xi > lasti))) continue;
#pragma unroll
                for (int t = 0; t < TOPK; ++t)
                    if (x < td[t]) {  // strict: equal distances keep the lower index first
                        const double y = td[t];
                        const int yi = ti[t];
                        td[t] = x; ti[t] = xi;
                        x = y; xi = yi;
                    }
            }
        };
        rebuild();
        // lane r keeps round r's pick; the rows are formed after the rounds, one per lane
        double pick_d = 0.0;
        int pick_i = BIG;
        for (int r = 0; r < NS; ++r) {
            double bd = td[0];
            int bi = ti[0];
            dpp_argmin_step<0xB1, 0xf>(bd, bi);   // quad_perm [1,0,3,2]
            dpp_argmin_step<0x4E, 0xf>(bd, bi);   // quad_perm [2,3,0,1]
            dpp_argmin_step<0x124, 0xf>(bd, bi);  // row_ror:4
            dpp_argmin_step<0x128, 0xf>(bd, bi);  // row_ror:8
            dpp_argmin_step<0x142, 0xa>(bd, bi);  // row_bcast:15
            dpp_argmin_step<0x143, 0xc>(bd, bi);  // row_bcast:31
            bd = readlane_dbl(bd, 63);
            bi = __builtin_amdgcn_readlane(bi, 63);
            const bool found = bi < M;
            if (found && lane == (bi & 63)) {
                lastd = td[0];
                lasti = ti[0];
                --left;
#pragma unroll
                for (int t = 0; t + 1 < TOPK; ++t) { td[t] = td[t + 1]; ti[t] = ti[t + 1]; }
                td[TOPK - 1] = INF;
                ti[TOPK - 1] = BIG;
            }
            if (__any(left > 0 && ti[0] == BIG)) {
                if (left > 0 && ti[0] == BIG) rebuild();
            }
            if (lane == r) {
                pick_d = bd;
                pick_i = bi;
            }
        }
        if (lane < NS) {
            double a1 = 0.0, a2 = 0.0, b = 0.0;
            if (pick_i < M) {
                // the pick's q again from (m, k): its z from the bank, its obstacle's stage constants
                const int j = pick_i / n_per, i = pick_i - j * n_per;
                const double* z = in.bank + ((size_t)L.batch[j] * n_per + i) * 2;
                double qx, qy;
                sample_point(K[j], z[0], z[1], qx, qy);
                const double dn = fmax(pick_d, 1e-9);
                a1 = __ddiv_rn(__dsub_rn(qx, rx), dn);
                a2 = __ddiv_rn(__dsub_rn(qy, ry), dn);
                b = __dsub_rn(__dadd_rn(__dmul_rn(a1, qx), __dmul_rn(a2, qy)), L.rad[j]);
            }
            L.rows[k][lane][0] = a1;
            L.rows[k][lane][1] = a2;
            L.rows[k][lane][2] = b;
        }
    }
    __syncthreads();

    // ---- stream out the parameter block, warm start and xinit
    const double* base = in.stage_params + (size_t)sc * npar;
    double* Pp = params + (size_t)sol * N * npar;
    const int s0 = pr.i_scen0;
    for (int e = tid; e < N * npar; e += 256) {
        const int k = e / npar, idx = e - k * npar;
        double v = base[idx];
        if (idx >= s0 && idx < s0 + 3 * NS) {
            const int i = (idx - s0) / 3, c = (idx - s0) - 3 * i;
            v = k == 0 ? (c == 2 ? DUMMY_B : 0.0) : L.rows[k][i][c];
        }
        Pp[e] = v;
    }
    double* W = warm + (size_t)sol * (N + 1) * NV;
    for (int e = tid; e < (N + 1) * NV; e += 256) W[e] = L.warm[e / NV][e % NV];
    if (tid < nx) xinit[(size_t)sol * nx + tid] = st[tid];
}

// The sample tensor [S*P][N][M][2] (stage 0: the stage-1 values); one workgroup per (scene, copy).
__global__ __launch_bounds__(256) void scenario_samples_kernel(mpcg_problem pr, int n_scenes, int P,
                                                               mpcg_scenario_sample_io in,
                                                               double* __restrict__ samples) {
    __shared__ int batch[MAX_OBS];
    const int sol = blockIdx.x;
    const int sc = sol / P;
    if (sc >= n_scenes) return;
    const int tid = threadIdx.x;
    const int N = pr.N, n_obs = in.n_obs, n_per = in.n_per, M = n_obs * n_per;
    if (tid < n_obs) batch[tid] = batch_of(in, sol, tid);
    __syncthreads();
    double* out = samples + (size_t)sol * N * M * 2;
    const int total = N * M;
    for (int e = tid; e < total; e += 256) {
        const int k = e / M, m = e - k * M;
        const int kk = k == 0 ? 1 : k;
        const int j = m / n_per, i = m - j * n_per;
        double K[6];
        stage_constants(in.obst + (((size_t)sc * n_obs + j) * N + (kk - 1)) * 5, K);
        const double* z = in.bank + ((size_t)batch[j] * n_per + i) * 2;
        double qx, qy;
        sample_point(K, z[0], z[1], qx, qy);
        out[(size_t)e * 2 + 0] = qx;
        out[(size_t)e * 2 + 1] = qy;
    }
}

// Between two SH-MPC control steps (include/mpcg_scenario.h, mpcg_scenario_advance); one workgroup per scene.
__global__ __launch_bounds__(64) void scenario_advance_kernel(mpcg_problem pr, int n_scenes, int P,
                                                              mpcg_scenario_step_io io,
                                                              double* __restrict__ main_warm,
                                                              double* __restrict__ lam_next) {
    const int sc = blockIdx.x;
    if (sc >= n_scenes) return;
    const int lane = threadIdx.x;
    const int N = pr.N, nx = pr.nx, NU = MPCG_NU, NV = NU + nx;
    const double dt = pr.dt;
    const int best = io.best[sc];
    const double* st = io.state_next + (size_t)sc * nx;
    double* W = main_warm + (size_t)sc * (N + 1) * NV;
    if (best >= 0) {
        // [state, out_2, ..., out_{N-1}, out_{N-1}, out_{N-1}]; stage 0's inputs: out_1's
        const int b = sc * P + best;
        const double* xt = io.xtraj + (size_t)b * (N + 1) * nx;
        const double* ut = io.utraj + (size_t)b * N * NU;
        for (int e = lane; e < (N + 1) * NV; e += 64) {
            const int k = e / NV, i = e - k * NV;
            const int src = k == 0 ? 1 : (k >= N - 1 ? N - 1 : k + 1);
            W[e] = i < NU ? ut[src * NU + i] : (k == 0 ? st[i - NU] : xt[src * nx + i - NU]);
        }
    } else if (lane == 0) {
        // Solver::initializeWithBraking(state_next)
        double x = st[0], y = st[1], psi = st[2], v = st[3], s = st[4];
        const double a = -fabs(io.deceleration);
        const double c = cos(psi), sn = sin(psi);
        for (int k = 0; k <= N; ++k) {
            if (k > 0) {
                x = __dadd_rn(x, __dmul_rn(__dmul_rn(v, dt), c));
                y = __dadd_rn(y, __dmul_rn(__dmul_rn(v, dt), sn));
                s = __dadd_rn(s, __dmul_rn(v, dt));
                v = fmax(__dadd_rn(v, __dmul_rn(a, dt)), 0.0);
            }
            double* w = W + k * NV;
            w[0] = a; w[1] = 0.0; w[2] = x; w[3] = y; w[4] = psi; w[5] = v; w[6] = s;
            for (int i = 7; i < NV; ++i) w[i] = 0.0;
        }
    }
    // carried multipliers of every copy (Solver_acados_reset zeroes them after a failure)
    if (lam_next) {
        const int Ls = N * (nx + pr.n_lin + pr.n_ell + pr.n_scen);
        for (int p = 0; p < P; ++p) {
            const size_t i = (size_t)sc * P + p;
            const bool ok = io.exit_code[i] == 1 && io.lam_out;
            double* dst = lam_next + i * Ls;
            const double* src = ok ? io.lam_out + i * Ls : nullptr;
            for (int e = lane; e < Ls; e += 64) dst[e] = ok ? src[e] : 0.0;
        }
    }
}

}  // namespace scen
}  // namespace mpcg

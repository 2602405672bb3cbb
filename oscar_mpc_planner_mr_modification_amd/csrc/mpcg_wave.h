// mpcg_wave.h — the wave arg-min on (value, index) by cross-lane exchanges, shared by the
// reference-path tracking (mpcg_path.h: distance^2 of 64 samples, index = lane) and the decomp
// halfspaces (mpcg_decomp.h: each lane's best (dist, point index)).  One 64-lane wavefront.
#pragma once
#include <hip/hip_runtime.h>

namespace mpcg {

constexpr int WAVE_LANES = 64;

// the index of the smallest (d, idx) of the wavefront, the same value in every lane; equal d: the
// lowest idx.  d must not be a NaN (the callers map a NaN to +inf: a total order).
__device__ __forceinline__ int wave_argmin(double d, int idx) {
    int l = idx;
    for (int off = WAVE_LANES / 2; off > 0; off >>= 1) {
        const double od = __shfl_xor(d, off, WAVE_LANES);
        const int ol = __shfl_xor(l, off, WAVE_LANES);
        if (od < d || (od == d && ol < l)) {
            d = od;
            l = ol;
        }
    }
    return __builtin_amdgcn_readfirstlane(l);
}

}  // namespace mpcg

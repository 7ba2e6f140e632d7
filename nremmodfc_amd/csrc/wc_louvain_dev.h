// wc_louvain_dev.h -- what the two Louvain kernels (wc_louvain.hip, wc_louvain_sign.hip) share on the
// device: one wave per problem, the lowest-index argmax over the wave, np.unique's relabelling, and
// the visiting order of a sweep.  Device code only; every function expects a 64-thread workgroup.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "wc_device.h"

namespace wclv {

constexpr int kMaxN = 96;
constexpr int kWave = 64;           // threads of a Louvain workgroup: one wave
constexpr int kSweepGuard = 1000;   // graph_utils.py:1071, :788
constexpr double kTol = 1e-10;      // :1066, :1081; :772, :807

// np.max and np.argmax of one value per lane: the largest, at the lowest index that attains it.
// Every lane returns the same pair.  All 64 lanes must be active.
__device__ __forceinline__ void wave_argmax(double& v, int& idx) {
#pragma unroll
    for (int off = kWave / 2; off; off >>= 1) {
        const double ov = __shfl_xor(v, off);
        const int oi = __shfl_xor(idx, off);
        if (ov > v || (ov == v && oi < idx)) {
            v = ov;
            idx = oi;
        }
    }
}

// np.unique(lab, return_inverse=True): lab[i] <- the number of distinct values below lab[i], values
// in [0, n).  Returns the number of distinct values.  The wave is synchronised on entry and on return.
__device__ inline int relabel(int n, int* lab, int* used, int* newlab) {
    const int lane = threadIdx.x;
    for (int v = lane; v < n; v += kWave) used[v] = 0;
    __syncthreads();
    for (int i = lane; i < n; i += kWave) used[lab[i]] = 1;  // equal values from several lanes
    __syncthreads();
    for (int v = lane; v < n; v += kWave) {
        int c = 0;
        for (int x = 0; x < v; ++x) c += used[x];
        newlab[v] = c;
    }
    int K = 0;
    for (int x = 0; x < n; ++x) K += used[x];
    __syncthreads();
    for (int i = lane; i < n; i += kWave) lab[i] = newlab[lab[i]];
    __syncthreads();
    return K;
}

// order[0 .. n) <- the nodes of sweep t in visiting order: the stable argsort of n Philox words
// (include/wcsde.h).  keys [n] is scratch.  The wave is synchronised on return.
__device__ inline void sweep_order(uint64_t t, uint64_t seed, int n, uint32_t* keys, int* order) {
    const int lane = threadIdx.x;
    for (int i = lane; i < n; i += kWave) {
        uint32_t x[4];
        wcdev::philox_ctr(t, (uint32_t)i >> 2, seed, x);
        const int k = i & 3;
        keys[i] = k == 0 ? x[0] : (k == 1 ? x[1] : (k == 2 ? x[2] : x[3]));
    }
    __syncthreads();
    for (int i = lane; i < n; i += kWave) {
        const uint32_t k = keys[i];
        int rank = 0;
        for (int j = 0; j < n; ++j) {
            const uint32_t kj = keys[j];
            rank += kj < k || (kj == k && j < i);
        }
        order[rank] = i;
    }
    __syncthreads();
}

}  // namespace wclv

// wc_louvain.hip -- Louvain community search and agreement matrices of a batch of N x N matrices on
// gfx950: the partition that wc_graph_modules (wc_graph.hip) takes as an input.
//
// Replaces, for B matrices and R seeds at once, the host loops of the reference's graph_utils.py:
//   community_louvain (:958-1122), from the objective matrix on     -> wc_graph_louvain
//   agreement (:890-932) and the counting loop of get_agreement_matrix (:935-956)
//                                                                   -> wc_graph_agreement
// No symmetry is assumed: the expressions are evaluated as the reference writes them, so a directed
// matrix gives what the reference gives.
//
// One problem is one (matrix, seed) pair and one wave: a 64-thread workgroup with the objective
// matrix and the node-to-module sums Hnm in LDS (2 N (N | 1) fp64, 149 KB at N = 96; the odd row
// stride lets the lanes walk a column without bank conflicts).  The algorithm is a serial walk over
// the nodes in which every step depends on the moves before it; what is parallel inside a problem
// is one row of N candidate modules (a lane holds modules m and m + 64) and one column update of N
// rows.  A single wave does both without a workgroup barrier between waves; thousands of problems
// fill the chip.  The reference's H and Hm are updated there but never read by a decision: they
// are left out.
//
// Every sum has a fixed order (ascending index) and there are no atomics: a (matrix, seed) pair
// gives the same bits alone and inside any batch.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include "wc_common.h"
#include "wc_device.h"
#include "wc_louvain_dev.h"

namespace {

using wclv::kMaxN;
using wclv::kWave;
using wclv::kSweepGuard;
using wclv::kTol;
using wclv::wave_argmax;
using wclv::relabel;
constexpr int kAgThreads = 256;
constexpr int kAgChunk = 32;        // partitions staged in LDS at a time
constexpr int kAgPairs = kMaxN * kMaxN / kAgThreads;  // pairs (i, j) per thread: 36

// ---- wc_graph_louvain: one wave per (matrix, seed) ----
__global__ void __launch_bounds__(kWave) louvain_kernel(int R, int N, const double* __restrict__ obj_all,
                                                        const double* __restrict__ norm,
                                                        const int32_t* __restrict__ ci0_all,
                                                        const uint64_t* __restrict__ seeds,
                                                        int32_t* __restrict__ ci_out, double* __restrict__ q_out,
                                                        int32_t* __restrict__ info) {
    extern __shared__ __attribute__((aligned(16))) double lds[];
    const int S = N | 1;
    double* Bs = lds;                                   // [N][S] the objective matrix of this level
    double* Hs = Bs + N * S;                            // [N][S] Hnm: node-to-module sums
    int* Mb = reinterpret_cast<int*>(Hs + N * S);       // [N] module of a node of this level
    int* ci = Mb + N;                                   // [N] module of an original node
    int* order = ci + N;                                // [N] the sweep's visiting order
    uint32_t* keys = reinterpret_cast<uint32_t*>(order + N);  // [N]
    int* used = reinterpret_cast<int*>(keys + N);       // [N]
    int* newlab = used + N;                             // [N]
    const int lane = threadIdx.x;
    const size_t prob = blockIdx.x, b = prob / R;
    const double* G = obj_all + b * N * N;
    const double s = norm[b];
    const uint64_t seed = seeds[prob % R];

    int bad = !isfinite(s);
    for (int idx = lane; idx < N * N; idx += kWave) {
        const double x = G[idx];
        bad |= !isfinite(x);
        Bs[idx / N * S + idx % N] = x;
    }
    for (int i = lane; i < N; i += kWave) {
        int c = ci0_all ? ci0_all[b * N + i] : i;
        if (c < 0 || c >= N) {
            bad = 1;
            c = 0;
        }
        Mb[i] = c;
    }
    bad = __syncthreads_or(bad);
    if (bad) {  // uniform: a non-finite entry or a label out of range; nothing is indexed by it
        for (int i = lane; i < N; i += kWave) ci_out[prob * N + i] = -1;
        if (lane == 0) {
            q_out[prob] = NAN;
            if (info) info[prob * 2] = info[prob * 2 + 1] = 0;
        }
        return;
    }
    if (ci0_all) relabel(N, Mb, used, newlab);
    // :1054-1056, Hnm[:, m] = sum of obj[:, j] over the nodes j of module m, j ascending
    for (int i = lane; i < N; i += kWave) {
        ci[i] = Mb[i];
        for (int m = 0; m < N; ++m) Hs[i * S + m] = 0.0;
        for (int j = 0; j < N; ++j) Hs[i * S + Mb[j]] += Bs[i * S + j];
    }
    __syncthreads();
    double q = 0.0;  // :1062, every lane the same sum in the same order
    for (int i = 0; i < N; ++i) q += Hs[i * S + Mb[i]];
    q /= s;
    double q0 = -INFINITY;

    int n = N, levels = 0;
    uint64_t t = 0;  // sweeps so far, over all levels
    bool first = true, stuck = false;
    while (q - q0 > kTol) {
        bool moved = true;
        for (int it = 1; moved; ++it) {
            if (it > kSweepGuard) {
                stuck = true;
                break;
            }
            moved = false;
            wclv::sweep_order(t, seed, n, keys, order);
            ++t;
            for (int p = 0; p < n; ++p) {
                const int u = order[p], ma = Mb[u];
                const double hma = Hs[u * S + ma], buu = Bs[u * S + u];
                const int m1 = lane + kWave;
                double v = -INFINITY;  // :1077-1078, dQ of modules lane and lane + 64
                int mb = lane;
                if (lane < n) v = lane == ma ? 0.0 : Hs[u * S + lane] - hma + buu;
                if (m1 < n) {
                    const double d1 = m1 == ma ? 0.0 : Hs[u * S + m1] - hma + buu;
                    if (d1 > v) {
                        v = d1;
                        mb = m1;
                    }
                }
                wave_argmax(v, mb);
                if (v > kTol) {  // uniform; :1085-1091
                    moved = true;
                    for (int i = lane; i < n; i += kWave) {
                        const double c = Bs[i * S + u];
                        Hs[i * S + mb] += c;
                        Hs[i * S + ma] -= c;
                    }
                    if (lane == 0) Mb[u] = mb;
                    __syncthreads();
                }
            }
        }
        if (stuck) break;

        const int K = relabel(n, Mb, used, newlab);  // :1093
        for (int i = lane; i < N; i += kWave) ci[i] = first ? Mb[i] : Mb[ci[i]];  // :1096-1102
        first = false;
        // :1104-1112, pooled in two steps: over the columns of a module (into Hs), then over the
        // rows of a module; the upper triangle is computed and mirrored
        for (int r = lane; r < n; r += kWave) {
            for (int j = 0; j < K; ++j) Hs[r * S + j] = 0.0;
            for (int c = 0; c < n; ++c) Hs[r * S + Mb[c]] += Bs[r * S + c];
        }
        __syncthreads();
        for (int idx = lane; idx < K * K; idx += kWave) {
            const int i = idx / K, j = idx % K;
            if (i > j) continue;
            double acc = 0.0;
            for (int r = 0; r < n; ++r)
                if (Mb[r] == i) acc += Hs[r * S + j];
            Bs[i * S + j] = acc;
            Bs[j * S + i] = acc;
        }
        __syncthreads();
        for (int idx = lane; idx < K * K; idx += kWave) Hs[idx / K * S + idx % K] = Bs[idx / K * S + idx % K];  // :1115
        for (int i = lane; i < K; i += kWave) Mb[i] = i;
        __syncthreads();
        n = K;
        q0 = q;
        double tr = 0.0;  // :1120
        for (int i = 0; i < n; ++i) tr += Bs[i * S + i];
        q = tr / s;
        ++levels;
    }

    for (int i = lane; i < N; i += kWave) ci_out[prob * N + i] = stuck ? -1 : ci[i];
    if (lane == 0) {
        q_out[prob] = stuck ? NAN : q;
        if (info) {
            info[prob * 2] = levels;
            info[prob * 2 + 1] = (int32_t)t;
        }
    }
}

size_t louvain_lds_bytes(int N) {
    return sizeof(double) * 2 * (size_t)N * (N | 1) + sizeof(int) * 6 * (size_t)N;
}

// ---- wc_graph_agreement: one workgroup per matrix, a thread for up to 36 pairs (i, j) ----
__global__ void __launch_bounds__(kAgThreads) agreement_kernel(int R, int N, const int32_t* __restrict__ ci_all,
                                                               double* __restrict__ D) {
    __shared__ int lab[kAgChunk * kMaxN];
    const int tid = threadIdx.x;
    const size_t b = blockIdx.x;
    const int32_t* C = ci_all + b * (size_t)R * N;
    int cnt[kAgPairs];
#pragma unroll
    for (int k = 0; k < kAgPairs; ++k) cnt[k] = 0;
    int bad = 0;
    for (int r0 = 0; r0 < R; r0 += kAgChunk) {
        const int rc = R - r0 < kAgChunk ? R - r0 : kAgChunk;
        for (int idx = tid; idx < rc * N; idx += kAgThreads) {
            const int c = C[(size_t)r0 * N + idx];
            bad |= c < 0;
            lab[idx] = c;
        }
        __syncthreads();
#pragma unroll
        for (int k = 0; k < kAgPairs; ++k) {
            const int idx = tid + kAgThreads * k;
            if (idx < N * N) {
                const int i = idx / N, j = idx % N;
                int c = 0;
                for (int r = 0; r < rc; ++r) c += lab[r * N + i] == lab[r * N + j];
                cnt[k] += c;
            }
        }
        __syncthreads();
    }
    bad = __syncthreads_or(bad);
#pragma unroll
    for (int k = 0; k < kAgPairs; ++k) {
        const int idx = tid + kAgThreads * k;
        if (idx < N * N) D[b * N * N + idx] = bad ? NAN : (idx / N == idx % N ? 0.0 : (double)cnt[k]);
    }
}

const char* const kWhyMaxN = "one matrix per workgroup, in LDS";

}  // namespace

extern "C" {

int wc_graph_louvain(int B, int R, int N, const double* obj, const double* norm, const int32_t* ci0,
                     const uint64_t* seeds, int32_t* ci, double* q, int32_t* info, void* stream) {
    wc_clear_err();
    const char* fn = "wc_graph_louvain";
    if (int rc = wc_check_seeded(fn, B, R, N, 2, nullptr, kMaxN, kWhyMaxN, "workgroups")) return rc;
    if (!obj || !norm || !seeds || !ci || !q)
        return wc_fail(WC_EINVAL, "wc_graph_louvain: obj, norm, seeds, ci or q is NULL");
    const size_t b = B, r = R, n = N;
    const WcSpan ins[4] = {{"obj", obj, b * n * n * 8, 8}, {"norm", norm, b * 8, 8}, {"ci0", ci0, b * n * 4, 4},
                         {"seeds", seeds, r * 8, 8}};
    const WcSpan outs[3] = {{"ci", ci, b * r * n * 4, 4}, {"q", q, b * r * 8, 8}, {"info", info, b * r * 2 * 4, 4}};
    if (int rc = wc_check_spans(fn, ins, 4, outs, 3)) return rc;
    const size_t lds = louvain_lds_bytes(N);
    if (int rc = wc_raise_lds(fn, louvain_kernel, lds)) return rc;
    hipLaunchKernelGGL(louvain_kernel, dim3((unsigned)(B * R)), dim3(kWave), lds, static_cast<hipStream_t>(stream), R, N,
                       obj, norm, ci0, seeds, ci, q, info);
    return wc_hip_check(fn);
}

int wc_graph_agreement(int B, int R, int N, const int32_t* ci, double* D, void* stream) {
    wc_clear_err();
    const char* fn = "wc_graph_agreement";
    if (int rc = wc_check_seeded(fn, B, R, N, 2, nullptr, kMaxN, kWhyMaxN, nullptr)) return rc;  // the grid is B
    if (!ci || !D) return wc_fail(WC_EINVAL, "wc_graph_agreement: ci or D is NULL");
    const size_t b = B, r = R, n = N;
    const WcSpan ins[1] = {{"ci", ci, b * r * n * 4, 4}};
    const WcSpan outs[1] = {{"D", D, b * n * n * 8, 8}};
    if (int rc = wc_check_spans(fn, ins, 1, outs, 1)) return rc;
    hipLaunchKernelGGL(agreement_kernel, dim3(B), dim3(kAgThreads), 0, static_cast<hipStream_t>(stream), R, N, ci, D);
    return wc_hip_check(fn);
}

}  // extern "C"

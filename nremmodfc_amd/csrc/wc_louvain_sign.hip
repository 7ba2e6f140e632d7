// wc_louvain_sign.hip -- Louvain community search on matrices with weights of both signs, for a batch
// of N x N matrices and R seeds on gfx950: the reference's modularity_louvain_und_sign
// (graph_utils.py:697-855; Rubinov & Sporns 2011), decision for decision       -> wc_graph_louvain_sign
//
// One problem is one (matrix, seed) pair and one wave, as in wc_louvain.hip, whose argmax, relabelling
// and visiting order it shares (wc_louvain_dev.h).  The signed search keeps four N x N matrices: the
// positive and the negative weights W0, W1 and the node-to-module degrees knm0, knm1.  Four do not
// fit the CU's 160 KB of LDS at N = 96 (298 KB), so
//   in LDS     knm0, knm1 [N][N | 1] (a node visit reads a row of each, a move updates two columns of
//              each), the node and module degrees kn0, kn1, km0, km1, the diagonals of W0 and W1, and
//              the integer arrays: 155.9 KB at N = 96;
//   in global  W0 and W1, which a visit does not need: they are read for a column on a move and for
//              pooling.  At the first level they are w itself, split by sign as it is read (the R
//              seeds of a matrix share it in L2); from the second level on the pooled matrices lie in
//              the workgroup's slot of the workspace, 2 N^2 fp64.
// The grid is bounded by the number of slots and a workgroup strides over the problems; a slot belongs
// to a workgroup, not to a problem, and all of a problem's state is set anew, so a pair gives the same
// bits alone, in any batch and with any workspace.  Every sum has a fixed order (ascending index) and
// there are no atomics.
//
// dQ is evaluated one rounding at a time, as numpy evaluates the reference's expression: no fma.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include "wc_common.h"
#include "wc_device.h"
#include "wc_louvain_dev.h"

#pragma clang fp contract(off)

namespace {

using wclv::kMaxN;
using wclv::kSweepGuard;
using wclv::kTol;
using wclv::kWave;
constexpr int kLevelGuard = 300;  // graph_utils.py:773

// W0 (sign 0) or W1 (sign 1) at [i][j] of the current level: w split by sign, or the pooled matrix
// of the slot (two dense [n][n] matrices, N^2 apart)
__device__ __forceinline__ double weight(const double* w, const double* slot, bool first, int N, int n, int sign,
                                         int i, int j) {
    if (first) {
        const double x = w[i * N + j];
        return sign ? (x < 0.0 ? -x : 0.0) : (x > 0.0 ? x : 0.0);
    }
    return slot[sign * N * N + i * n + j];
}

// w and ws are not __restrict__: the slot is written by pooling and read by the level after it
__global__ void __launch_bounds__(kWave) louvain_sign_kernel(int P, int R, int N, const double* w_all, double gamma,
                                                             int qtype, const uint64_t* __restrict__ seeds,
                                                             int32_t* __restrict__ ci_out, double* __restrict__ q_out,
                                                             int32_t* __restrict__ info, double* ws) {
    extern __shared__ __attribute__((aligned(16))) double lds[];
    const int S = N | 1;
    double* H0 = lds;                 // [N][S] knm0: positive node-to-module degrees
    double* H1 = H0 + N * S;          // [N][S] knm1
    double* kn0 = H1 + N * S;         // [N] node degrees (column sums of W0, W1)
    double* kn1 = kn0 + N;
    double* km0 = kn1 + N;            // [N] module degrees
    double* km1 = km0 + N;
    double* dg0 = km1 + N;            // [N] W0[u][u], W1[u][u]
    double* dg1 = dg0 + N;
    int* Mb = reinterpret_cast<int*>(dg1 + N);  // [N] module of a node of this level
    int* ci = Mb + N;                           // [N] module of an original node
    int* order = ci + N;                        // [N] the sweep's visiting order
    uint32_t* keys = reinterpret_cast<uint32_t*>(order + N);  // [N]
    int* used = reinterpret_cast<int*>(keys + N);             // [N]
    int* newlab = used + N;                                   // [N]
    const int lane = threadIdx.x;
    double* slot = ws + (size_t)blockIdx.x * 2 * N * N;

    for (int prob = blockIdx.x; prob < P; prob += gridDim.x) {
        const size_t b = prob / R;
        const double* w = w_all + b * N * N;
        const uint64_t seed = seeds[prob % R];
        __syncthreads();  // the problem before this one has left the LDS

        // level 1: knm = W (:780-781), split by sign as it is read
        int bad = 0;
        for (int idx = lane; idx < N * N; idx += kWave) {
            const double x = w[idx];
            bad |= !isfinite(x);
            H0[idx / N * S + idx % N] = x > 0.0 ? x : 0.0;
            H1[idx / N * S + idx % N] = x < 0.0 ? -x : 0.0;
        }
        bad = __syncthreads_or(bad);
        if (bad) {  // uniform: a non-finite entry
            for (int i = lane; i < N; i += kWave) ci_out[(size_t)prob * N + i] = -1;
            if (lane == 0) {
                q_out[prob] = NAN;
                if (info) info[(size_t)prob * 2] = info[(size_t)prob * 2 + 1] = 0;
            }
            continue;
        }

        // :776-783: the degrees of a level's n nodes from knm = W, every node its own module
        auto degrees = [&](int n) {
            for (int j = lane; j < n; j += kWave) {
                double a0 = 0.0, a1 = 0.0;
                for (int i = 0; i < n; ++i) {
                    a0 += H0[i * S + j];
                    a1 += H1[i * S + j];
                }
                kn0[j] = km0[j] = a0;
                kn1[j] = km1[j] = a1;
                dg0[j] = H0[j * S + j];
                dg1[j] = H1[j * S + j];
                Mb[j] = j;
            }
            __syncthreads();
        };
        degrees(N);
        double s0 = 0.0, s1 = 0.0;  // :740-741 as the sum of the node degrees, every lane the same sum
        for (int j = 0; j < N; ++j) {
            s0 += kn0[j];
            s1 += kn1[j];
        }
        double d0 = qtype == 4 ? 0.0 : (qtype == 3 ? 1.0 / (s0 + s1) : 1.0 / s0);  // :743-759
        double d1 = qtype == 1 ? 0.0 : ((qtype == 0 || qtype == 3) ? 1.0 / (s0 + s1) : 1.0 / s1);
        if (s0 == 0.0) {  // :761-766
            s0 = 1.0;
            d0 = 0.0;
        }
        if (s1 == 0.0) {
            s1 = 1.0;
            d1 = 0.0;
        }

        int n = N, levels = 0;
        uint64_t t = 0;  // sweeps so far, over all levels
        bool first = true, stuck = false;
        double q = 0.0, qprev = -1.0;  // :771
        while (q - qprev > kTol) {
            if (levels >= kLevelGuard) {  // :773
                stuck = true;
                break;
            }
            bool moved = true;
            for (int it = 1; moved; ++it) {
                if (it > kSweepGuard) {  // :788
                    stuck = true;
                    break;
                }
                moved = false;
                wclv::sweep_order(t, seed, n, keys, order);
                ++t;
                for (int p = 0; p < n; ++p) {
                    const int u = order[p], ma = Mb[u];
                    const double k0 = kn0[u], k1 = kn1[u], g0 = gamma * k0, g1 = gamma * k1;
                    const double w0 = dg0[u], w1 = dg1[u];
                    const double h0 = H0[u * S + ma], h1 = H1[u * S + ma], m0 = km0[ma], m1 = km1[ma];
                    double v = -INFINITY;  // :797-804, dQ of modules lane and lane + 64
                    int mb = lane;
#pragma unroll
                    for (int half = 0; half < 2; ++half) {
                        const int m = lane + half * kWave;
                        if (m < n) {
                            const double e0 = g0 * ((km0[m] + k0) - m0), e1 = g1 * ((km1[m] + k1) - m1);
                            const double dq0 = ((H0[u * S + m] + w0) - h0) - e0 / s0;
                            const double dq1 = ((H1[u * S + m] + w1) - h1) - e1 / s1;
                            const double a = d0 * dq0, c = d1 * dq1;
                            const double dq = m == ma ? 0.0 : a - c;
                            if (half == 0 || dq > v) {
                                v = dq;
                                mb = m;
                            }
                        }
                    }
                    wclv::wave_argmax(v, mb);
                    if (v > kTol) {  // uniform; :807-822
                        moved = true;
                        for (int i = lane; i < n; i += kWave) {
                            const double c0 = weight(w, slot, first, N, n, 0, i, u);
                            const double c1 = weight(w, slot, first, N, n, 1, i, u);
                            H0[i * S + mb] += c0;
                            H0[i * S + ma] -= c0;
                            H1[i * S + mb] += c1;
                            H1[i * S + ma] -= c1;
                        }
                        if (lane == 0) {
                            km0[mb] += k0;
                            km0[ma] -= k0;
                            km1[mb] += k1;
                            km1[ma] -= k1;
                            Mb[u] = mb;
                        }
                        __syncthreads();
                    }
                }
            }
            if (stuck) break;

            const int K = wclv::relabel(n, Mb, used, newlab);  // :826
            for (int i = lane; i < N; i += kWave) ci[i] = first ? Mb[i] : Mb[ci[i]];  // :829-830
            // :833-844, pooled in two steps: over the columns of a module (into knm, which the level
            // has done with), then over the rows of a module; the upper triangle is computed and
            // mirrored into the slot.  K = n where nothing moved.
            for (int r = lane; r < n; r += kWave) {
                for (int j = 0; j < K; ++j) H0[r * S + j] = H1[r * S + j] = 0.0;
                for (int c = 0; c < n; ++c) {
                    const int m = Mb[c];
                    H0[r * S + m] += weight(w, slot, first, N, n, 0, r, c);
                    H1[r * S + m] += weight(w, slot, first, N, n, 1, r, c);
                }
            }
            __syncthreads();  // every read of the slot's old level is done
            for (int idx = lane; idx < K * K; idx += kWave) {
                const int i = idx / K, j = idx % K;
                if (i > j) continue;
                double a0 = 0.0, a1 = 0.0;
                for (int r = 0; r < n; ++r)
                    if (Mb[r] == i) {
                        a0 += H0[r * S + j];
                        a1 += H1[r * S + j];
                    }
                slot[i * K + j] = slot[j * K + i] = a0;
                slot[N * N + i * K + j] = slot[N * N + j * K + i] = a1;
            }
            __syncthreads();
            for (int idx = lane; idx < K * K; idx += kWave) {  // :780-781 of the next level
                H0[idx / K * S + idx % K] = slot[idx];
                H1[idx / K * S + idx % K] = slot[N * N + idx];
            }
            __syncthreads();
            n = K;
            first = false;
            ++levels;
            degrees(n);
            // :848-850; sum(W W) = sum of kn^2, W being mirrored; every lane the same sums
            double tr0 = 0.0, tr1 = 0.0, sq0 = 0.0, sq1 = 0.0;
            for (int j = 0; j < n; ++j) {
                tr0 += dg0[j];
                tr1 += dg1[j];
                sq0 += kn0[j] * kn0[j];
                sq1 += kn1[j] * kn1[j];
            }
            const double a = d0 * (tr0 - sq0 / s0), c = d1 * (tr1 - sq1 / s1);
            qprev = q;
            q = a - c;
        }

        for (int i = lane; i < N; i += kWave) ci_out[(size_t)prob * N + i] = stuck ? -1 : ci[i];
        if (lane == 0) {
            q_out[prob] = stuck ? NAN : q;
            if (info) {
                info[(size_t)prob * 2] = levels;
                info[(size_t)prob * 2 + 1] = (int32_t)t;
            }
        }
    }
}

size_t lds_bytes(int N) {
    return sizeof(double) * (2 * (size_t)N * (N | 1) + 6 * (size_t)N) + sizeof(int) * 6 * (size_t)N;
}

}  // namespace

extern "C" {

int wc_graph_louvain_sign(int B, int R, int N, const double* w, double gamma, int qtype, const uint64_t* seeds,
                          int32_t* ci, double* q, int32_t* info, void* workspace, size_t ws_bytes, void* stream) {
    wc_clear_err();
    const char* fn = "wc_graph_louvain_sign";
    if (int rc = wc_check_seeded(fn, B, R, N, 2, nullptr, kMaxN,
                                 "the node-to-module degrees of one matrix per workgroup, in LDS", "problems"))
        return rc;
    if (qtype < 0 || qtype > 4) return wc_fail(WC_EINVAL, "%s: qtype = %d, must be 0 .. 4 (sta, pos, smp, gja, neg)", fn, qtype);
    if (!isfinite(gamma)) return wc_fail(WC_EINVAL, "%s: gamma is not finite", fn);
    if (!w || !seeds || !ci || !q || !workspace)
        return wc_fail(WC_EINVAL, "%s: w, seeds, ci, q or workspace is NULL", fn);
    const size_t b = B, r = R, n = N, probs = b * r;
    WcSlots plan;
    if (int rc = wc_plan_slots(fn, workspace, ws_bytes, 2 * n * n * sizeof(double), "16 N^2", probs, &plan)) return rc;
    const WcSpan ins[2] = {{"w", w, b * n * n * 8, 8}, {"seeds", seeds, r * 8, 8}};
    const WcSpan outs[4] = {{"ci", ci, b * r * n * 4, 4}, {"q", q, b * r * 8, 8}, {"info", info, b * r * 2 * 4, 4},
                            plan.span};
    if (int rc = wc_check_spans(fn, ins, 2, outs, 4)) return rc;
    const size_t lds = lds_bytes(N);
    if (int rc = wc_raise_lds(fn, louvain_sign_kernel, lds)) return rc;
    hipLaunchKernelGGL(louvain_sign_kernel, dim3((unsigned)plan.slots), dim3(kWave), lds, static_cast<hipStream_t>(stream),
                       (int)probs, R, N, w, gamma, qtype, seeds, ci, q, info, static_cast<double*>(workspace));
    return wc_hip_check(fn);
}

}  // extern "C"

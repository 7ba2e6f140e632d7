// wc_phaseconn.hip -- time-domain connectivity between the columns of a simulation on the device
// (gfx950, fp64): phase-locking value, phase-lag index, weighted phase-lag index and the pairwise
// orthogonalised amplitude-envelope correlation, from the unit phasors u [M][B][N][2] that
// wc_hilbert_phase* writes and the envelopes a [M][B][N] of wc_hilbert_envelope.  For a pair i < j
//   c(t) = u_i.x u_j.x + u_i.y u_j.y
//   s(t) = u_i.y u_j.x - u_i.x u_j.y       two rounded products and one subtraction, never an FMA:
//                                          two identical columns give s = 0 exactly, not the
//                                          rounding residue of one product
//   plv      = sqrt((sum c)^2 + (sum s)^2) / M                         diagonal 1
//   pli      = |sum sign(s)| / M, sign(0) = 0                          diagonal 0
//   wpli     = |sum a_i a_j s| / sum |a_i a_j s|                       diagonal 0
//   aec_orth = (corr(a_i |s|, a_j) + corr(a_j |s|, a_i)) / 2           diagonal 0
// with Pearson's corr over t from raw moments; a zero denominator gives NaN.  The file is compiled
// with floating-point contraction off; every FMA in it is written out.
//
// Pass 1 (pc_pair_kernel<AMP>): workgroup (blockIdx.x = simulation b and 32 x 32 column-tile pair
// ti <= tj, blockIdx.y = time block of kBlk = 4096 samples), wc_csd.hip's cs_gram_kernel shape: 256
// threads with a 2 x 2 block of pairs each, 16 samples of both tiles' phasors (and envelopes) staged
// through LDS at a time.  A pair's sums are one chain in time order over the block; the block's
// partial sums go to the workspace, [b][tile pair][block][K][32][32].  Two instantiations:
//   phase      K = 3: sum c, sum s, sum sign(s)                                   (plv, pli)
//   amplitude  K = 8: sum w, sum |w| (w = a_i a_j s); with p = a_i |s|, q = a_j |s|:
//              sum p, sum p^2, sum p a_j, sum q, sum q^2, sum q a_i              (wpli, aec_orth)
// and pc_col_kernel leaves sum a and sum a^2 of every column and block, [b][block][N][2].
// Pass 2 (pc_final_kernel<AMP>): workgroup (b, tile pair), the same thread-to-pair map; adds the
// blocks' partials in block order, forms the measures and writes both triangles and the diagonal.
// No atomics.  kBlk is a constant, so an entry depends on its two columns' samples, M and the
// measure only: not on N, B, the tile it falls in, the workspace or the run.  The amplitude
// instantiation reuses the phase instantiation's partials once pass 2 has read them: the workspace
// is the larger of the two, plus the columns' sums.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <algorithm>
#include "wc_common.h"

#pragma clang fp contract(off)

namespace {

typedef double d2 __attribute__((ext_vector_type(2)));  // (cos, sin)

constexpr int kTile = 32;         // columns per strip (kTile / 16 = 2 x 2 pairs per thread)
constexpr int kKS = 16;           // samples staged in LDS at a time
constexpr int kThreads = 256;
constexpr int kBlk = 4096;        // samples per time block: 300,000 x 90 gives 6 x 74 = 444 workgroups
constexpr int kMaxN = 1024;       // at most 528 tile pairs
constexpr int64_t kMaxM = 524288; // the Hilbert range
constexpr int kKPhase = 3, kKAmp = 8;
constexpr int kCell = kTile * kTile;
constexpr int kColLanes = kThreads / kTile;  // pc_col_kernel: time lanes per column
constexpr int kAll = WC_CONN_PLV | WC_CONN_PLI | WC_CONN_WPLI | WC_CONN_AEC_ORTH;

// tile pair tp of nt tiles -> (ti <= tj), rows of the upper triangle in order
__device__ __forceinline__ void pc_tiles(int tp, int nt, int& ti, int& tj) {
    ti = 0;
    while (tp >= nt - ti) {
        tp -= nt - ti;
        ++ti;
    }
    tj = ti + tp;
}

template <bool AMP>
__global__ void __launch_bounds__(kThreads) pc_pair_kernel(int B, int N, int64_t M, int ntp, const double* __restrict__ ph,
                                                           const double* __restrict__ amp,
                                                           double* __restrict__ part) {
    constexpr int K = AMP ? kKAmp : kKPhase, R = kTile / 16;
    __shared__ d2 Ui[kKS][kTile], Uj[kKS][kTile];
    __shared__ double Ai[AMP ? kKS : 1][kTile], Aj[AMP ? kKS : 1][kTile];
    const int tid = threadIdx.x;
    const int b = blockIdx.x / ntp, tp = blockIdx.x % ntp, blk = blockIdx.y, nblk = gridDim.y;
    int ti, tj;
    pc_tiles(tp, (N + kTile - 1) / kTile, ti, tj);
    const int64_t t0 = (int64_t)blk * kBlk;
    const int len = (int)min((int64_t)kBlk, M - t0);
    const int li = (tid / 16) * R, lj = (tid % 16) * R;

    double acc[R][R][K];
#pragma unroll
    for (int p = 0; p < R; ++p)
#pragma unroll
        for (int q = 0; q < R; ++q)
#pragma unroll
            for (int k = 0; k < K; ++k) acc[p][q][k] = 0.0;

    for (int k0 = 0; k0 < len; k0 += kKS) {
        const int kmax = min(kKS, len - k0);
        for (int e = tid; e < kKS * kTile; e += kThreads) {
            const int ks = e / kTile, cc = e % kTile;
            const int ci = ti * kTile + cc, cj = tj * kTile + cc;
            const int64_t row = ((t0 + k0 + ks) * B + b) * N;  // ks >= kmax: never read
            const bool in_i = ks < kmax && ci < N, in_j = ks < kmax && cj < N;
            Ui[ks][cc] = in_i ? d2{ph[2 * (row + ci)], ph[2 * (row + ci) + 1]} : d2{0.0, 0.0};  // 8-byte aligned
            Uj[ks][cc] = in_j ? d2{ph[2 * (row + cj)], ph[2 * (row + cj) + 1]} : d2{0.0, 0.0};
            if constexpr (AMP) {
                Ai[ks][cc] = in_i ? amp[row + ci] : 0.0;
                Aj[ks][cc] = in_j ? amp[row + cj] : 0.0;
            }
        }
        __syncthreads();
        for (int ks = 0; ks < kmax; ++ks) {
            d2 u[R], v[R];
            double a[R], c[R];
#pragma unroll
            for (int p = 0; p < R; ++p) {
                u[p] = Ui[ks][li + p];
                v[p] = Uj[ks][lj + p];
                if constexpr (AMP) {
                    a[p] = Ai[ks][li + p];
                    c[p] = Aj[ks][lj + p];
                }
            }
#pragma unroll
            for (int p = 0; p < R; ++p)
#pragma unroll
                for (int q = 0; q < R; ++q) {
                    double* s_ = acc[p][q];
                    const double m1 = u[p].y * v[q].x, m2 = u[p].x * v[q].y;
                    const double s = m1 - m2;
                    if constexpr (!AMP) {
                        s_[0] += __builtin_fma(u[p].x, v[q].x, u[p].y * v[q].y);
                        s_[1] += s;
                        s_[2] += s > 0.0 ? 1.0 : (s < 0.0 ? -1.0 : 0.0);
                    } else {
                        const double w = (a[p] * c[q]) * s, as = fabs(s);
                        const double pp = a[p] * as, qq = c[q] * as;
                        s_[0] += w;
                        s_[1] += fabs(w);
                        s_[2] += pp;
                        s_[3] = __builtin_fma(pp, pp, s_[3]);
                        s_[4] = __builtin_fma(pp, c[q], s_[4]);
                        s_[5] += qq;
                        s_[6] = __builtin_fma(qq, qq, s_[6]);
                        s_[7] = __builtin_fma(qq, a[p], s_[7]);
                    }
                }
        }
        __syncthreads();
    }

    double* o = part + (((int64_t)b * ntp + tp) * nblk + blk) * (K * kCell);
#pragma unroll
    for (int k = 0; k < K; ++k)
#pragma unroll
        for (int p = 0; p < R; ++p)
#pragma unroll
            for (int q = 0; q < R; ++q) o[k * kCell + (li + p) * kTile + lj + q] = acc[p][q][k];
}

// workgroup (blockIdx.x = simulation b and group of 32 columns, blockIdx.y = time block): thread
// (column cc, lane q) adds the block's samples q, q + 8, ... in order, lane sums are added in lane
// order: col [b][block][N][2] = (sum a, sum a^2)
__global__ void __launch_bounds__(kThreads) pc_col_kernel(int B, int N, int64_t M, int ncg,
                                                          const double* __restrict__ amp, double* __restrict__ col) {
    __shared__ double r1[kColLanes][kTile], r2[kColLanes][kTile];
    const int tid = threadIdx.x, cc = tid % kTile, q = tid / kTile;
    const int b = blockIdx.x / ncg, c = (blockIdx.x % ncg) * kTile + cc, blk = blockIdx.y, nblk = gridDim.y;
    const int64_t t0 = (int64_t)blk * kBlk;
    const int len = (int)min((int64_t)kBlk, M - t0);
    double s1 = 0.0, s2 = 0.0;
    if (c < N)
        for (int k = q; k < len; k += kColLanes) {
            const double a = amp[((t0 + k) * B + b) * N + c];
            s1 += a;
            s2 = __builtin_fma(a, a, s2);
        }
    r1[q][cc] = s1;
    r2[q][cc] = s2;
    __syncthreads();
    if (q == 0 && c < N) {
        for (int h = 1; h < kColLanes; ++h) {
            s1 += r1[h][cc];
            s2 += r2[h][cc];
        }
        double* o = col + (((int64_t)b * nblk + blk) * N + c) * 2;
        o[0] = s1;
        o[1] = s2;
    }
}

// Pearson's r of p (sums sp, spp) with a (sums sa, saa), cross moment spa, over T samples
__device__ __forceinline__ double pc_corr(double sp, double spp, double spa, double sa, double saa, double T) {
    const double cov = spa - sp * sa / T, vp = spp - sp * sp / T, va = saa - sa * sa / T;
    const double den = vp * va;
    if (!(den > 0.0)) return NAN;
    const double r = cov / sqrt(den);
    return r > 1.0 ? 1.0 : (r < -1.0 ? -1.0 : r);
}

// workgroup blockIdx.x = (b, tile pair): out0 / out1 [B][N][N] = plv / pli (phase) or wpli / aec_orth
// (amplitude); either may be NULL
template <bool AMP>
__global__ void __launch_bounds__(kThreads) pc_final_kernel(int N, int64_t M, int ntp, int nblk,
                                                            const double* __restrict__ part,
                                                            const double* __restrict__ col, double* out0,
                                                            double* out1) {
    constexpr int K = AMP ? kKAmp : kKPhase, R = kTile / 16;
    const int tid = threadIdx.x;
    const int b = blockIdx.x / ntp, tp = blockIdx.x % ntp;
    int ti, tj;
    pc_tiles(tp, (N + kTile - 1) / kTile, ti, tj);
    const int li = (tid / 16) * R, lj = (tid % 16) * R;
    const double T = (double)M;
    const double* pb = part + ((int64_t)b * ntp + tp) * nblk * (K * kCell);
    const int64_t ob = (int64_t)b * N * N;
#pragma unroll
    for (int p = 0; p < R; ++p)
#pragma unroll
        for (int q = 0; q < R; ++q) {
            const int i = ti * kTile + li + p, j = tj * kTile + lj + q;
            if (i > j || j >= N) continue;
            double v0, v1;
            if (i == j) {
                v0 = AMP ? 0.0 : 1.0;
                v1 = 0.0;
            } else {
                double s[K];
#pragma unroll
                for (int k = 0; k < K; ++k) s[k] = 0.0;
                for (int blk = 0; blk < nblk; ++blk)
#pragma unroll
                    for (int k = 0; k < K; ++k)
                        s[k] += pb[((int64_t)blk * K + k) * kCell + (li + p) * kTile + lj + q];
                if constexpr (!AMP) {
                    v0 = sqrt(s[0] * s[0] + s[1] * s[1]) / T;
                    v1 = fabs(s[2]) / T;
                } else {
                    v0 = fabs(s[0]) / s[1];  // 0 / 0: NaN
                    v1 = 0.0;
                    if (out1) {
                        double ai = 0.0, aai = 0.0, aj = 0.0, aaj = 0.0;
                        for (int blk = 0; blk < nblk; ++blk) {
                            const double* cb = col + ((int64_t)b * nblk + blk) * N * 2;
                            ai += cb[2 * i];
                            aai += cb[2 * i + 1];
                            aj += cb[2 * j];
                            aaj += cb[2 * j + 1];
                        }
                        v1 = 0.5 * (pc_corr(s[2], s[3], s[4], aj, aaj, T) + pc_corr(s[5], s[6], s[7], ai, aai, T));
                    }
                }
            }
            if (out0) {
                out0[ob + (int64_t)i * N + j] = v0;
                out0[ob + (int64_t)j * N + i] = v0;
            }
            if (out1) {
                out1[ob + (int64_t)i * N + j] = v1;
                out1[ob + (int64_t)j * N + i] = v1;
            }
        }
}

struct PcPlan {
    int nt, ntp, nblk, ncg;
    size_t part, col;  // bytes of the pairs' partial sums and of the columns' sums
};

bool pc_plan(int B, int N, int64_t M, int measures, PcPlan& p) {
    if (B < 1 || N < 1 || N > kMaxN || M < 2 || M > kMaxM || measures <= 0 || (measures & ~kAll)) return false;
    p.nt = (N + kTile - 1) / kTile;
    p.ntp = p.nt * (p.nt + 1) / 2;
    p.ncg = p.nt;
    p.nblk = (int)((M + kBlk - 1) / kBlk);
    if ((int64_t)B * p.ntp > INT32_MAX) return false;  // gridDim.x
    const bool amp = measures & (WC_CONN_WPLI | WC_CONN_AEC_ORTH);
    p.part = (size_t)B * p.ntp * p.nblk * (amp ? kKAmp : kKPhase) * kCell * sizeof(double);
    p.col = (measures & WC_CONN_AEC_ORTH) ? ((size_t)B * p.nblk * N * 2 * sizeof(double) + 15) / 16 * 16 : 0;
    return true;
}

}  // namespace

size_t wc_phase_conn_workspace_size(int B, int N, int64_t M, int measures) {
    PcPlan p;
    return pc_plan(B, N, M, measures, p) ? p.part + p.col : 0;
}

int wc_phase_conn(int B, int N, int64_t M, const double* phasor, const double* amp, int measures, double* out,
                  void* workspace, size_t ws_bytes, void* stream) {
    wc_clear_err();
    const char* fn = "wc_phase_conn";
    if (B < 1) return wc_fail(WC_EINVAL, "wc_phase_conn: B < 1");
    if (N < 1) return wc_fail(WC_EINVAL, "wc_phase_conn: N < 1");
    if (M < 2) return wc_fail(WC_EINVAL, "wc_phase_conn: M < 2");
    if (measures <= 0 || (measures & ~kAll))
        return wc_fail(WC_EINVAL, "wc_phase_conn: measures must be a non-empty set of WC_CONN_PLV .. WC_CONN_AEC_ORTH");
    const bool want_amp = measures & (WC_CONN_WPLI | WC_CONN_AEC_ORTH);
    if (!phasor || !out) return wc_fail(WC_EINVAL, "wc_phase_conn: phasor or out is NULL");
    if (want_amp && !amp)
        return wc_fail(WC_EINVAL, "wc_phase_conn: amp is NULL (WC_CONN_WPLI and WC_CONN_AEC_ORTH need the envelopes)");
    if (N > kMaxN) return wc_fail(WC_EUNSUPPORTED, "wc_phase_conn: N = %d > 1024 columns per simulation", N);
    if (M > kMaxM) return wc_fail(WC_EUNSUPPORTED, "wc_phase_conn: M = %lld > 524288 (the Hilbert range)", (long long)M);
    PcPlan p;
    if (!pc_plan(B, N, M, measures, p))
        return wc_fail(WC_EINVAL, "wc_phase_conn: 2^31 workgroups or more (B times the tile pairs)");
    // B N <= 32 B nt <= 32 B ntp < 2^36 and M < 2^20: the phasors are below 2^60 bytes
    const size_t nmeas = (size_t)__builtin_popcount((unsigned)measures);
    const size_t cells = (size_t)M * (size_t)B * (size_t)N;
    const WcSpan ins[2] = {{"phasor", phasor, cells * 16, 8}, {"amp", amp, cells * 8, 8}};
    const WcSpan outs[2] = {{"out", out, nmeas * B * N * N * 8, 8}, {"workspace", workspace, ws_bytes, 16}};
    // aliasing is refused before alignment here, and the workspace's alignment after its size
    if (int rc = wc_check_alias(fn, outs, 1, ins, 2)) return rc;
    if (int rc = wc_check_align(fn, ins, 2)) return rc;
    if (int rc = wc_check_align(fn, outs, 1)) return rc;
    if (int rc = wc_check_workspace(fn, "wc_phase_conn_workspace_size", workspace, ws_bytes, p.part + p.col)) return rc;
    if (int rc = wc_check_align(fn, outs + 1, 1)) return rc;

    hipStream_t st = static_cast<hipStream_t>(stream);
    double* part = static_cast<double*>(workspace);
    double* col = reinterpret_cast<double*>(static_cast<char*>(workspace) + p.part);
    const double* ph = phasor;
    const size_t mat = (size_t)B * N * N;
    double* o[4] = {nullptr, nullptr, nullptr, nullptr};  // plv, pli, wpli, aec_orth
    {
        double* next = out;
        for (int k = 0; k < 4; ++k)
            if (measures & (1 << k)) {
                o[k] = next;
                next += mat;
            }
    }
    const dim3 g1((unsigned)(B * p.ntp), (unsigned)p.nblk), g2((unsigned)(B * p.ntp));
    if (measures & (WC_CONN_PLV | WC_CONN_PLI)) {
        hipLaunchKernelGGL(pc_pair_kernel<false>, g1, dim3(kThreads), 0, st, B, N, M, p.ntp, ph, amp, part);
        hipLaunchKernelGGL(pc_final_kernel<false>, g2, dim3(kThreads), 0, st, N, M, p.ntp, p.nblk, part, col, o[0], o[1]);
    }
    if (want_amp) {
        if (o[3])
            hipLaunchKernelGGL(pc_col_kernel, dim3((unsigned)(B * p.ncg), (unsigned)p.nblk), dim3(kThreads), 0, st, B, N,
                               M, p.ncg, amp, col);
        hipLaunchKernelGGL(pc_pair_kernel<true>, g1, dim3(kThreads), 0, st, B, N, M, p.ntp, ph, amp, part);
        hipLaunchKernelGGL(pc_final_kernel<true>, g2, dim3(kThreads), 0, st, N, M, p.ntp, p.nblk, part, col, o[2], o[3]);
    }
    return wc_hip_check("wc_phase_conn");
}

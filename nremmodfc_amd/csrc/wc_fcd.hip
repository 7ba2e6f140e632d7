// wc_fcd.hip -- dynamic functional connectivity of a batch of simulations on gfx950: sliding-window
// FC with its FCD matrix (Hansen et al. 2015) and the phase-coherence FCD (Deco & Kringelbach 2016).
// Nothing in the reference computes either; the definitions are in include/wcsde.h and restated in
// numpy in tests/fcd_reference.py.
//
// wc_fcd, for a chunk of simulations whose window patterns fit the workspace, two kernels:
//   patterns_kernel  one workgroup per (simulation, window): column means, then the centred window in
//                    LDS 32 rows at a time and the N x N products in registers (thread (ty, tx) of the
//                    16 x 16 grid keeps the cells (ty + 16 a, tx + 16 c), c >= a: the upper triangle),
//                    r_ij = c_ij (1 / sd_i) (1 / sd_j) clipped to [-1, 1] as np.corrcoef, the pattern's mean and
//                    its centred norm by fixed-order tree sums; the centred pattern and the norm go to
//                    the workspace, the pattern itself to winfc where asked.
//   gram_kernel      one workgroup per (simulation, 64 x 64 tile of the upper triangle of fcd): the
//                    products of the centred patterns, 32 entries of the P at a time through LDS, 4 x 4
//                    cells a thread, divided by the two norms, clipped, written with their mirror.
// The patterns of a simulation (nw P doubles: 8.6 MB at the shipped shape) exist only in the workspace,
// for as many simulations at a time as it holds; every sum has one fixed order that depends on
// (N, M, win, step) alone, so a simulation's bits depend neither on B nor on the workspace.
//
// wc_fcd_phase needs no patterns: with d_t[i][j] = c_i c_j + s_i s_j,
//   sum_{i,j} d_t[i][j] d_u[i][j] = CC^2 + SS^2 + CS^2 + SC^2,  CC = sum_i c_i(t) c_i(u), CS = sum_i c_i(t) s_i(u) ...
// of which the strict upper triangle is half of what is left without the diagonal's sum_i q_i(t) q_i(u),
// q = c^2 + s^2: five dot products of length N for a pair of times instead of P products.  The closed
// form's rounding is of the order of N^2 ulps against norms^2 >= N (N - 2) / 4 for unit phasors: harmless
// from N = 3 on; N = 2, where a norm can be as small as it likes, multiplies its one entry directly.
// Three kernels, no workspace: phase_norms_kernel sums every time's norm explicitly over its P entries (an
// exactly zero norm stays exactly zero) and keeps it on the diagonal of fcd; phase_kernel, one workgroup
// per 32 x 32 tile of the upper triangle, 32 nodes at a time through LDS, reads the norms there and writes
// everything but the diagonal; phase_diagonal_kernel turns the norms into 1 (or NaN).
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include "wc_common.h"

namespace {

constexpr int kMaxN = 96;
constexpr int kMaxP = kMaxN * (kMaxN - 1) / 2;  // 4560
constexpr int kThreads = 256;
constexpr int kGrid = 16;      // threads per side of the 16 x 16 thread grid (kThreads = kGrid^2)
constexpr int kRows = 32;      // rows of a window in LDS at a time
constexpr int kTile = 64;      // side of a tile of fcd (4 x 4 cells a thread)
constexpr int kKc = 32;        // pattern entries of a tile's rows in LDS at a time
constexpr int kPhaseTile = 32; // side of a tile of fcd_phase (2 x 2 cells a thread)
constexpr int kPhaseNc = 32;   // nodes of a tile's times in LDS at a time
constexpr int kMinSims = 8;    // simulations in flight that the minimum workspace holds

// a norm that a correlation can be divided by: not 0, not NaN, not infinite
__device__ __forceinline__ bool usable(double n) { return n > 0.0 && n < INFINITY; }

// cos(theta_i - theta_j) = c_i c_j + s_i s_j with both products rounded, as numpy evaluates it: contracted
// into an fma, two phases exactly pi / 2 apart would give the rounding of one product instead of 0
__device__ __forceinline__ double cos_diff(double ci, double si, double cj, double sj) {
#pragma clang fp contract(off)
    const double a = ci * cj, b = si * sj;
    return a + b;
}

// Sum of v over the workgroup in a fixed tree order, returned to every thread; red [kThreads].
__device__ __forceinline__ double block_sum(double v, double* red) {
    const int tid = threadIdx.x;
    red[tid] = v;
    __syncthreads();
    for (int o = kThreads / 2; o > 0; o >>= 1) {
        if (tid < o) red[tid] += red[tid + o];
        __syncthreads();
    }
    const double r = red[0];
    __syncthreads();
    return r;
}

// Tile q of the upper triangle, rows first: (0,0) (0,1) .. (0,T-1) (1,1) ..
__device__ __forceinline__ void tile_of(int q, int T, int* ti, int* tj) {
    int i = 0;
    while (q >= T - i) {
        q -= T - i;
        ++i;
    }
    *ti = i;
    *tj = i + q;
}

// The strict upper triangle of the correlation matrix of one window, row-major, into buf [P].
// xw: row 0 of the window, this simulation's columns; ld: doubles between rows.  buf holds the
// centred rows [kRows][16 R] first (16 R <= 96: 3072 doubles), the pattern afterwards.
template <int R>
__device__ __forceinline__ void window_pattern(int N, int W, const double* __restrict__ xw, size_t ld,
                                               const double* mean, double* sd /* 1 / sd */, double* buf) {
    constexpr int Np = R * kGrid;
    const int tid = threadIdx.x, ty = tid / kGrid, tx = tid % kGrid;
    double acc[R][R];
#pragma unroll
    for (int a = 0; a < R; ++a)
#pragma unroll
        for (int c = 0; c < R; ++c) acc[a][c] = 0.0;
    for (int t0 = 0; t0 < W; t0 += kRows) {
        const int tc = min(kRows, W - t0);
        for (int idx = tid; idx < tc * Np; idx += kThreads) {
            const int t = idx / Np, n = idx % Np;
            buf[idx] = n < N ? xw[(size_t)(t0 + t) * ld + n] - mean[n] : 0.0;
        }
        __syncthreads();
        for (int t = 0; t < tc; ++t) {
            double xi[R], xj[R];
#pragma unroll
            for (int a = 0; a < R; ++a) xi[a] = buf[t * Np + ty + kGrid * a];
#pragma unroll
            for (int c = 0; c < R; ++c) xj[c] = buf[t * Np + tx + kGrid * c];
#pragma unroll
            for (int a = 0; a < R; ++a)
#pragma unroll
                for (int c = a; c < R; ++c) acc[a][c] = fma(xi[a], xj[c], acc[a][c]);
        }
        __syncthreads();
    }
    if (ty == tx) {
#pragma unroll
        for (int a = 0; a < R; ++a)
            if (ty + kGrid * a < N) sd[ty + kGrid * a] = 1.0 / sqrt(acc[a][a]);
    }
    __syncthreads();
#pragma unroll
    for (int a = 0; a < R; ++a)
#pragma unroll
        for (int c = a; c < R; ++c) {
            const int i = ty + kGrid * a, j = tx + kGrid * c;
            // a constant column: acc = 0 exactly and 1 / sd = inf, 0 * inf = NaN as numpy's 0 / 0
            if (i < j && j < N) buf[i * N - i * (i + 1) / 2 + j - i - 1] = clip1(acc[a][c] * sd[i] * sd[j]);
        }
    __syncthreads();
}

// ---- wc_fcd, first kernel: one workgroup per (simulation of the chunk, window) ----
__global__ void __launch_bounds__(kThreads) patterns_kernel(int B, int N, int win, int step, int nw, int b0,
                                                            const double* __restrict__ x, double* __restrict__ ws,
                                                            size_t slot_doubles, double* __restrict__ winfc) {
    __shared__ double buf[kMaxP];
    __shared__ double red[kThreads];
    __shared__ double mean[kMaxN], sd[kMaxN];
    const int tid = threadIdx.x;
    const int slot = blockIdx.x / nw, k = blockIdx.x % nw;
    const int b = b0 + slot;
    const int P = N * (N - 1) / 2;
    const size_t ld = (size_t)B * N;
    const double* xw = x + (size_t)k * step * ld + (size_t)b * N;

    if (tid < N) {
        double s = 0.0;
#pragma unroll 8
        for (int t = 0; t < win; ++t) s += xw[(size_t)t * ld + tid];  // loads ahead of the adds, which stay in order
        mean[tid] = s / win;
    }
    __syncthreads();
    switch ((N + kGrid - 1) / kGrid) {
        case 1: window_pattern<1>(N, win, xw, ld, mean, sd, buf); break;
        case 2: window_pattern<2>(N, win, xw, ld, mean, sd, buf); break;
        case 3: window_pattern<3>(N, win, xw, ld, mean, sd, buf); break;
        case 4: window_pattern<4>(N, win, xw, ld, mean, sd, buf); break;
        case 5: window_pattern<5>(N, win, xw, ld, mean, sd, buf); break;
        default: window_pattern<6>(N, win, xw, ld, mean, sd, buf); break;
    }
    double s = 0.0;
    for (int p = tid; p < P; p += kThreads) s += buf[p];
    const double m = block_sum(s, red) / P;
    double* pat = ws + (size_t)slot * slot_doubles + (size_t)k * P;
    double* raw = winfc ? winfc + ((size_t)b * nw + k) * P : nullptr;
    double q = 0.0;
    for (int p = tid; p < P; p += kThreads) {
        const double v = buf[p], d = v - m;
        q = fma(d, d, q);
        pat[p] = d;
        if (raw) raw[p] = v;
    }
    q = block_sum(q, red);
    if (tid == 0) ws[(size_t)slot * slot_doubles + (size_t)nw * P + k] = sqrt(q);
}

// ---- wc_fcd, second kernel: one workgroup per (simulation of the chunk, tile of the upper triangle) ----
__global__ void __launch_bounds__(kThreads) gram_kernel(int nw, int P, int tiles_side, int tiles,
                                                        const double* __restrict__ ws, size_t slot_doubles,
                                                        double* __restrict__ fcd) {
    __shared__ double As[kKc][kTile + 1], Bs[kKc][kTile + 1];
    const int tid = threadIdx.x, ty = tid / kGrid, tx = tid % kGrid;
    const int slot = blockIdx.x / tiles;
    int ti, tj;
    tile_of(blockIdx.x % tiles, tiles_side, &ti, &tj);
    const int k0 = ti * kTile, l0 = tj * kTile;
    const double* pat = ws + (size_t)slot * slot_doubles;
    const double* norms = pat + (size_t)nw * P;
    double* out = fcd + (size_t)slot * nw * nw;

    double acc[4][4];
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int c = 0; c < 4; ++c) acc[a][c] = 0.0;
    for (int p0 = 0; p0 < P; p0 += kKc) {
#pragma unroll
        for (int m = 0; m < kTile * kKc / kThreads; ++m) {
            const int idx = tid + kThreads * m, kk = idx % kKc, r = idx / kKc, p = p0 + kk;
            As[kk][r] = (k0 + r < nw && p < P) ? pat[(size_t)(k0 + r) * P + p] : 0.0;
            Bs[kk][r] = (l0 + r < nw && p < P) ? pat[(size_t)(l0 + r) * P + p] : 0.0;
        }
        __syncthreads();
#pragma unroll 4
        for (int kk = 0; kk < kKc; ++kk) {
            double va[4], vb[4];
#pragma unroll
            for (int a = 0; a < 4; ++a) va[a] = As[kk][ty + kGrid * a];
#pragma unroll
            for (int c = 0; c < 4; ++c) vb[c] = Bs[kk][tx + kGrid * c];
#pragma unroll
            for (int a = 0; a < 4; ++a)
#pragma unroll
                for (int c = 0; c < 4; ++c) acc[a][c] = fma(va[a], vb[c], acc[a][c]);
        }
        __syncthreads();
    }
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const int k = k0 + ty + kGrid * a, l = l0 + tx + kGrid * c;
            if (k >= nw || l >= nw) continue;
            if (k < l) {
                const double nk = norms[k], nl = norms[l];
                const double v = (usable(nk) && usable(nl)) ? clip1(acc[a][c] / nk / nl) : NAN;
                out[(size_t)k * nw + l] = v;
                out[(size_t)l * nw + k] = v;
            } else if (k == l) {
                const double nk = norms[k];
                out[(size_t)k * nw + k] = usable(nk) ? 1.0 : NAN;
            }
        }
}

// ---- wc_fcd_phase, first kernel: the norms, kept on the diagonal of fcd until the third kernel ----
// One workgroup per (simulation, 16 times): 16 threads a time, thread q of them the rows i = q, q + 16, ..
// of its upper triangle; the 16 parts added in order.
__global__ void __launch_bounds__(kThreads) phase_norms_kernel(int B, int N, int M, int groups, int b0,
                                                               const double* __restrict__ phasor,
                                                               double* __restrict__ fcd) {
    __shared__ double C[kGrid][kMaxN + 1], S[kGrid][kMaxN + 1];
    __shared__ double part[kThreads];
    const int tid = threadIdx.x, r = tid / kGrid, q = tid % kGrid;
    const int b = b0 + blockIdx.x / groups;
    const int t0 = (blockIdx.x % groups) * kGrid;
    for (int idx = tid; idx < kGrid * N; idx += kThreads) {
        const int rr = idx / N, n = idx % N, t = t0 + rr;
        double c = 0.0, s = 0.0;
        if (t < M) {
            const double* z = phasor + (((size_t)t * B + b) * N + n) * 2;
            c = z[0];
            s = z[1];
        }
        C[rr][n] = c;
        S[rr][n] = s;
    }
    __syncthreads();
    double acc = 0.0;
    for (int i = q; i < N; i += kGrid)
        for (int j = i + 1; j < N; ++j) {
            const double d = cos_diff(C[r][i], S[r][i], C[r][j], S[r][j]);
            acc = fma(d, d, acc);
        }
    part[tid] = acc;
    __syncthreads();
    if (q == 0 && t0 + r < M) {
        double s = 0.0;
        for (int k = 0; k < kGrid; ++k) s += part[tid + k];
        fcd[((size_t)b * M + t0 + r) * M + t0 + r] = sqrt(s);
    }
}

// ---- wc_fcd_phase, second kernel: one workgroup per (simulation, tile of the upper triangle) ----
// Reads the norms from the diagonal, writes everything but the diagonal.
__global__ void __launch_bounds__(kThreads) phase_kernel(int B, int N, int M, int tiles_side, int tiles, int b0,
                                                         const double* __restrict__ phasor, double* fcd) {
    // the tile's rows (a) and columns (b), kPhaseNc nodes at a time
    __shared__ double Ca[kPhaseTile][kPhaseNc + 1], Sa[kPhaseTile][kPhaseNc + 1];
    __shared__ double Cb[kPhaseTile][kPhaseNc + 1], Sb[kPhaseTile][kPhaseNc + 1];
    const int tid = threadIdx.x, ty = tid / kGrid, tx = tid % kGrid;
    const int b = b0 + blockIdx.x / tiles;
    int ti, tj;
    tile_of(blockIdx.x % tiles, tiles_side, &ti, &tj);
    const int t0 = ti * kPhaseTile, u0 = tj * kPhaseTile;

    double cc[2][2], ss[2][2], cs[2][2], sc[2][2], dg[2][2];
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int c = 0; c < 2; ++c) cc[a][c] = ss[a][c] = cs[a][c] = sc[a][c] = dg[a][c] = 0.0;
    for (int n0 = 0; n0 < N; n0 += kPhaseNc) {
#pragma unroll
        for (int m = 0; m < kPhaseTile * kPhaseNc / kThreads; ++m) {
            const int idx = tid + kThreads * m, r = idx / kPhaseNc, nn = idx % kPhaseNc, n = n0 + nn;
            double ca = 0.0, sa = 0.0, cb = 0.0, sb = 0.0;  // past N or M: zeros, which add nothing to a sum
            if (n < N && t0 + r < M) {
                const double* z = phasor + (((size_t)(t0 + r) * B + b) * N + n) * 2;
                ca = z[0];
                sa = z[1];
            }
            if (n < N && u0 + r < M) {
                const double* z = phasor + (((size_t)(u0 + r) * B + b) * N + n) * 2;
                cb = z[0];
                sb = z[1];
            }
            Ca[r][nn] = ca;
            Sa[r][nn] = sa;
            Cb[r][nn] = cb;
            Sb[r][nn] = sb;
        }
        __syncthreads();
#pragma unroll 4
        for (int nn = 0; nn < kPhaseNc; ++nn) {
            double ca[2], sa[2], qa[2], cb[2], sb[2], qb[2];
#pragma unroll
            for (int a = 0; a < 2; ++a) {
                ca[a] = Ca[ty + kGrid * a][nn];
                sa[a] = Sa[ty + kGrid * a][nn];
                qa[a] = fma(ca[a], ca[a], sa[a] * sa[a]);
                cb[a] = Cb[tx + kGrid * a][nn];
                sb[a] = Sb[tx + kGrid * a][nn];
                qb[a] = fma(cb[a], cb[a], sb[a] * sb[a]);
            }
#pragma unroll
            for (int a = 0; a < 2; ++a)
#pragma unroll
                for (int c = 0; c < 2; ++c) {
                    cc[a][c] = fma(ca[a], cb[c], cc[a][c]);
                    ss[a][c] = fma(sa[a], sb[c], ss[a][c]);
                    cs[a][c] = fma(ca[a], sb[c], cs[a][c]);
                    sc[a][c] = fma(sa[a], cb[c], sc[a][c]);
                    dg[a][c] = fma(qa[a], qb[c], dg[a][c]);
                }
        }
        if (n0 + kPhaseNc < N) __syncthreads();  // the last nodes stay in LDS (N = 2 reads them below)
    }
    double* out = fcd + (size_t)b * M * M;
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int c = 0; c < 2; ++c) {
            const int rt = ty + kGrid * a, ru = tx + kGrid * c;
            const int t = t0 + rt, u = u0 + ru;
            if (t >= u || u >= M) continue;
            const double nt = out[(size_t)t * M + t], nu = out[(size_t)u * M + u];
            double up;
            if (N == 2) {  // one entry a pattern: the closed form would divide its rounding by a norm near 0
                up = cos_diff(Ca[rt][0], Sa[rt][0], Ca[rt][1], Sa[rt][1]) *
                     cos_diff(Cb[ru][0], Sb[ru][0], Cb[ru][1], Sb[ru][1]);
            } else {
                const double all = fma(cc[a][c], cc[a][c],
                                       fma(ss[a][c], ss[a][c], fma(cs[a][c], cs[a][c], sc[a][c] * sc[a][c])));
                up = 0.5 * (all - dg[a][c]);
            }
            const double v = (usable(nt) && usable(nu)) ? clip1(up / nt / nu) : NAN;
            out[(size_t)t * M + u] = v;
            out[(size_t)u * M + t] = v;
        }
}

// ---- wc_fcd_phase, third kernel: the diagonal, 1 where the norm kept there can be divided by ----
__global__ void __launch_bounds__(kThreads) phase_diagonal_kernel(int M, int64_t count, double* __restrict__ fcd) {
    const int64_t idx = (int64_t)blockIdx.x * kThreads + threadIdx.x;  // (simulation, time)
    if (idx >= count) return;
    double* d = fcd + (size_t)(idx / M) * M * M + (size_t)(idx % M) * (M + 1);
    *d = usable(*d) ? 1.0 : NAN;
}

struct Shape {
    int nw, P;
    size_t slot_doubles;  // a simulation in flight: nw P centred pattern entries, nw norms
};

// Shapes and limits of wc_fcd; what == nullptr: no message (the workspace query).
int check_shape(const char* what, int B, int N, int M, int win, int step, Shape* sh) {
    const char* fmt = what ? "%s: %s" : nullptr;
    if (B < 1) return wc_fail(WC_EINVAL, fmt, what, "B < 1");
    if (N < 3) return wc_fail(WC_EINVAL, fmt, what, "N < 3 (a pattern needs at least 3 entries)");
    if (N > kMaxN) return wc_fail(WC_EUNSUPPORTED, fmt, what, "N > 96 (one window's correlation matrix per workgroup)");
    if (win < 2) return wc_fail(WC_EINVAL, fmt, what, "win < 2");
    if (win > M) return wc_fail(WC_EINVAL, fmt, what, "win > M");
    if (step < 1) return wc_fail(WC_EINVAL, fmt, what, "step < 1");
    const int64_t nw = ((int64_t)M - win) / step + 1;
    if (nw > WC_FCD_MAX_WINDOWS) return wc_fail(WC_EUNSUPPORTED, fmt, what, "more than WC_FCD_MAX_WINDOWS = 4096 windows");
    sh->nw = (int)nw;
    sh->P = N * (N - 1) / 2;
    sh->slot_doubles = (size_t)nw * sh->P + (size_t)nw;
    return WC_OK;
}

}  // namespace

extern "C" {

size_t wc_fcd_workspace_size(int B, int N, int M, int win, int step) {
    Shape sh;
    if (check_shape(nullptr, B, N, M, win, step, &sh)) return 0;
    return sizeof(double) * sh.slot_doubles * (size_t)(B < kMinSims ? B : kMinSims);
}

int wc_fcd(int B, int N, int M, const double* x, int win, int step, double* fcd, double* winfc, void* workspace,
           size_t ws_bytes, void* stream) {
    wc_clear_err();
    Shape sh;
    const char* fn = "wc_fcd";
    if (int rc = check_shape(fn, B, N, M, win, step, &sh)) return rc;
    if (!x || !fcd) return wc_fail(WC_EINVAL, "wc_fcd: x or fcd is NULL");
    const size_t b = (size_t)B, nw = (size_t)sh.nw;
    const WcSpan ins[1] = {{"x", x, (size_t)M * b * N * 8, 8}};
    const WcSpan outs[2] = {{"fcd", fcd, b * nw * nw * 8, 8}, {"winfc", winfc, b * nw * sh.P * 8, 8}};
    const WcSpan wsp = {"workspace", workspace, ws_bytes, 8};
    if (int rc = wc_check_align(fn, &wsp, 1)) return rc;
    if (int rc = wc_check_spans(fn, ins, 1, outs, 2)) return rc;
    const size_t slot_bytes = sizeof(double) * sh.slot_doubles;
    const size_t need = slot_bytes * (size_t)(B < kMinSims ? B : kMinSims);
    if (int rc = wc_check_workspace(fn, "wc_fcd_workspace_size", workspace, ws_bytes, need)) return rc;
    if (int rc = wc_check_alias(fn, &wsp, 1, ins, 1)) return rc;
    if (int rc = wc_check_alias(fn, &wsp, 1, outs, 2)) return rc;

    const int tiles_side = (sh.nw + kTile - 1) / kTile, tiles = tiles_side * (tiles_side + 1) / 2;
    size_t slots = ws_bytes / slot_bytes;  // >= min(B, kMinSims) >= 1
    const size_t per_sim = (size_t)(sh.nw > tiles ? sh.nw : tiles);
    if (slots > (size_t)INT32_MAX / per_sim) slots = (size_t)INT32_MAX / per_sim;  // workgroups of one launch
    if (slots > (size_t)B) slots = (size_t)B;
    double* ws = static_cast<double*>(workspace);
    hipStream_t st = static_cast<hipStream_t>(stream);
    wc_chunks(B, (int64_t)slots, [&](int64_t b0, int64_t nb) {
        hipLaunchKernelGGL(patterns_kernel, dim3((unsigned)nb * sh.nw), dim3(kThreads), 0, st, B, N, win, step, sh.nw,
                           (int)b0, x, ws, sh.slot_doubles, winfc);
        hipLaunchKernelGGL(gram_kernel, dim3((unsigned)nb * tiles), dim3(kThreads), 0, st, sh.nw, sh.P, tiles_side,
                           tiles, ws, sh.slot_doubles, fcd + (size_t)b0 * sh.nw * sh.nw);
    });
    return wc_hip_check("wc_fcd");
}

int wc_fcd_phase(int B, int N, int M, const double* phasor, double* fcd, void* stream) {
    wc_clear_err();
    if (B < 1) return wc_fail(WC_EINVAL, "wc_fcd_phase: B < 1");
    if (N < 2) return wc_fail(WC_EINVAL, "wc_fcd_phase: N < 2");
    if (N > kMaxN) return wc_fail(WC_EUNSUPPORTED, "wc_fcd_phase: N > 96 (a tile's phasors in one workgroup's LDS)");
    if (M < 1) return wc_fail(WC_EINVAL, "wc_fcd_phase: M < 1");
    if (M > WC_FCD_PHASE_MAX_M)
        return wc_fail(WC_EUNSUPPORTED, "wc_fcd_phase: M > WC_FCD_PHASE_MAX_M = 4096 samples");
    if (!phasor || !fcd) return wc_fail(WC_EINVAL, "wc_fcd_phase: phasor or fcd is NULL");
    const WcSpan ins[1] = {{"phasor", phasor, (size_t)M * B * N * 16, 8}};
    const WcSpan outs[1] = {{"fcd", fcd, (size_t)B * M * M * 8, 8}};
    if (int rc = wc_check_spans("wc_fcd_phase", ins, 1, outs, 1)) return rc;
    const int tiles_side = (M + kPhaseTile - 1) / kPhaseTile, tiles = tiles_side * (tiles_side + 1) / 2;
    const int groups = (M + kGrid - 1) / kGrid;
    const int64_t per_launch = INT32_MAX / (tiles > groups ? tiles : groups);  // simulations whose workgroups fit a launch
    hipStream_t st = static_cast<hipStream_t>(stream);
    wc_chunks(B, per_launch, [&](int64_t b0, int64_t nb) {
        double* out = fcd + (size_t)b0 * M * M;
        hipLaunchKernelGGL(phase_norms_kernel, dim3((unsigned)(nb * groups)), dim3(kThreads), 0, st, B, N, M, groups,
                           (int)b0, phasor, fcd);
        hipLaunchKernelGGL(phase_kernel, dim3((unsigned)(nb * tiles)), dim3(kThreads), 0, st, B, N, M, tiles_side, tiles,
                           (int)b0, phasor, fcd);
        hipLaunchKernelGGL(phase_diagonal_kernel, dim3((unsigned)((nb * M + kThreads - 1) / kThreads)), dim3(kThreads), 0,
                           st, M, nb * M, out);
    });
    return wc_hip_check("wc_fcd_phase");
}

}  // extern "C"

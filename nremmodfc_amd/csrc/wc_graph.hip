// wc_graph.hip -- weighted graph measures of a batch of N x N matrices on gfx950: shortest paths and
// what follows from them (characteristic path length, global efficiency, eccentricity, radius,
// diameter), local efficiency, clustering coefficient, transitivity, strengths and degrees.
//
// Replaces, for B matrices at once, the host loops of the reference's graph_utils.py:
//   distance_wei (:1462-1529) + charpath (:1533-1591) + efficiency_wei(local=False) (:597-690)
//                                                          -> wc_graph_paths
//   efficiency_wei(local=True) (:667-685)                  -> wc_graph_local_efficiency
//   clustering_coef_wu (:1305-1323), transitivity_wu (:1673-1689), strengths_und (:1766-1778),
//   degrees_und (:1721-1737)                               -> wc_graph_clustering
//   betweenness_wei (:1983-2052), betweenness_bin (:1929-1980) -> wc_graph_betweenness
//   participation_coef (:271-307), module_degree_zscore (:2103-2140), and the modularity Q of a
//   given partition                                        -> wc_graph_modules
// No symmetry is assumed: the expressions are evaluated as the reference writes them, so a directed
// matrix gives what the reference gives.
//
// Shortest paths are Floyd-Warshall in LDS, one workgroup per matrix (N <= 96), instead of the
// reference's Dijkstra per source.  With D[k][k] = 0 and lengths >= 0, iteration k changes neither
// row k nor column k (D[i][k] + D[k][k] is never strictly below D[i][k]), and those are all that the
// iteration reads of other cells: the update is in place, one barrier per k.  The 256 threads form a
// 16 x 16 grid and thread (ty, tx) keeps the cells (ty + 16 a, tx + 16 b), a, b < R = ceil(n / 16),
// in registers: 2 R LDS reads for R^2 updates per k, an LDS write only where a path improves.
// The hop count of the reference's B matrix rides along in LDS: 1 on an edge, h[i][k] + h[k][j]
// where D[i][k] + D[k][j] < D[i][j] strictly (equal to Dijkstra's count where the shortest path is
// unique).
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include "wc_common.h"

namespace {

constexpr int kMaxN = 96;
constexpr int kThreads = 256;
constexpr int kGrid = 16;  // threads per side of the 16 x 16 thread grid (kThreads = kGrid^2)

// graph_utils.py:38-43: sign(x) |x|^(1/3).  pow, not cbrt: within an ulp or two of numpy's.
__device__ __forceinline__ double cuberoot(double x) {
    return x == 0.0 ? 0.0 : copysign(pow(fabs(x), 1.0 / 3.0), x);
}

// All-pairs shortest paths of D [n][n] (row stride n) in LDS, in place; H the hop counts (HOPS).
// D is complete and the workgroup synchronised on entry and on return.  Cells past n hold 0 in
// registers: a sum of lengths is never below it.
template <int R, bool HOPS>
__device__ __forceinline__ void floyd_warshall(int n, double* D, int* H) {
    const int ty = threadIdx.x / kGrid, tx = threadIdx.x % kGrid;
    double d[R][R];
#pragma unroll
    for (int a = 0; a < R; ++a)
#pragma unroll
        for (int b = 0; b < R; ++b) {
            const int i = ty + kGrid * a, j = tx + kGrid * b;
            d[a][b] = (i < n && j < n) ? D[i * n + j] : 0.0;
        }
    for (int k = 0; k < n; ++k) {
        double dik[R], dkj[R];
#pragma unroll
        for (int a = 0; a < R; ++a) {
            const int i = ty + kGrid * a;
            dik[a] = i < n ? D[i * n + k] : 0.0;
        }
#pragma unroll
        for (int b = 0; b < R; ++b) {
            const int j = tx + kGrid * b;
            dkj[b] = j < n ? D[k * n + j] : 0.0;
        }
#pragma unroll
        for (int a = 0; a < R; ++a)
#pragma unroll
            for (int b = 0; b < R; ++b) {
                const double s = dik[a] + dkj[b];
                if (s < d[a][b]) {  // never for a cell past n, nor in row k or column k
                    const int i = ty + kGrid * a, j = tx + kGrid * b;
                    d[a][b] = s;
                    D[i * n + j] = s;
                    if (HOPS) H[i * n + j] = H[i * n + k] + H[k * n + j];
                }
            }
        __syncthreads();
    }
}

template <bool HOPS>
__device__ __forceinline__ void floyd_warshall_n(int n, double* D, int* H) {
    switch ((n + kGrid - 1) / kGrid) {
        case 0: break;
        case 1: floyd_warshall<1, HOPS>(n, D, H); break;
        case 2: floyd_warshall<2, HOPS>(n, D, H); break;
        case 3: floyd_warshall<3, HOPS>(n, D, H); break;
        case 4: floyd_warshall<4, HOPS>(n, D, H); break;
        case 5: floyd_warshall<5, HOPS>(n, D, H); break;
        default: floyd_warshall<6, HOPS>(n, D, H); break;
    }
}

// connection length of a weight (invert, graph_utils.py:68-90): 1/w where w != 0
__device__ __forceinline__ double length_of(double w) { return w != 0.0 ? 1.0 / w : 0.0; }

// ---- wc_graph_paths: one workgroup per matrix ----
__global__ void __launch_bounds__(kThreads) paths_kernel(int N, const double* __restrict__ w_all, int lengths,
                                                         int include_infinite, double* __restrict__ dist,
                                                         int* __restrict__ hops, double* __restrict__ stats,
                                                         double* __restrict__ ecc) {
    extern __shared__ __attribute__((aligned(16))) double lds[];
    double* D = lds;               // [N][N]
    double* rsum = D + N * N;      // [N] row sums of D, of 1/D, row maxima, counts of entries
    double* rinv = rsum + N;
    double* rmax = rinv + N;
    int* rcnt = reinterpret_cast<int*>(rmax + N);
    int* H = rcnt + N + (N & 1);   // [N][N], only with hops
    const int tid = threadIdx.x;
    const size_t b = blockIdx.x;
    const double* W = w_all + b * N * N;

    int bad = 0;
    for (int idx = tid; idx < N * N; idx += kThreads) {
        const double x = W[idx];
        bad |= !(x >= 0.0);  // negative or NaN
        const int i = idx / N, j = idx % N;
        const double L = lengths ? x : length_of(x);
        D[idx] = i == j ? 0.0 : (L != 0.0 ? L : INFINITY);
        if (hops) H[idx] = (i != j && L != 0.0) ? 1 : 0;
    }
    bad = __syncthreads_or(bad);
    if (bad) {  // uniform: the reference is undefined here; nothing of this matrix is computed
        for (int idx = tid; idx < N * N; idx += kThreads) {
            if (dist) dist[b * N * N + idx] = NAN;
            if (hops) hops[b * N * N + idx] = -1;
        }
        if (stats && tid < 4) stats[b * 4 + tid] = NAN;
        if (ecc)
            for (int i = tid; i < N; i += kThreads) ecc[b * N + i] = NAN;
        return;
    }
    if (hops)
        floyd_warshall_n<true>(N, D, H);
    else
        floyd_warshall_n<false>(N, D, H);

    for (int idx = tid; idx < N * N; idx += kThreads) {
        if (dist) dist[b * N * N + idx] = D[idx];
        if (hops) hops[b * N * N + idx] = H[idx];
    }
    if (!stats && !ecc) return;
    // charpath: the diagonal left out, infinite entries kept or dropped
    if (tid < N) {
        double s = 0.0, si = 0.0, mx = -INFINITY;
        int c = 0;
        for (int j = 0; j < N; ++j) {
            const double v = D[tid * N + j];
            if (j == tid || (!include_infinite && isinf(v))) continue;
            s += v;
            si += 1.0 / v;
            mx = fmax(mx, v);
            ++c;
        }
        rsum[tid] = s;
        rinv[tid] = si;
        rmax[tid] = c ? mx : NAN;  // a row with nothing left has no eccentricity
        rcnt[tid] = c;
        if (ecc) ecc[b * N + tid] = rmax[tid];
    }
    __syncthreads();
    if (stats && tid == 0) {
        double s = 0.0, si = 0.0, lo = NAN, hi = NAN;  // fmin / fmax pass over the rows without one
        int c = 0;
        for (int i = 0; i < N; ++i) {
            s += rsum[i];
            si += rinv[i];
            c += rcnt[i];
            lo = fmin(lo, rmax[i]);
            hi = fmax(hi, rmax[i]);
        }
        stats[b * 4 + 0] = s / c;  // no entry at all: 0/0 = NaN, numpy's mean of nothing
        stats[b * 4 + 1] = si / c;
        stats[b * 4 + 2] = lo;
        stats[b * 4 + 3] = hi;
    }
}

size_t paths_lds_bytes(int N, bool hops) {
    return sizeof(double) * ((size_t)N * N + 3 * N) + sizeof(int) * (N + (N & 1) + (hops ? (size_t)N * N : 0));
}

// ---- wc_graph_local_efficiency: one workgroup per (matrix, node u) ----
__global__ void __launch_bounds__(kThreads) local_efficiency_kernel(int N, const double* __restrict__ w_all,
                                                                    double* __restrict__ eloc) {
    extern __shared__ __attribute__((aligned(16))) double lds[];
    double* D = lds;                                   // [k][k] lengths, distances, then cuberoot(1/D)
    double* sw = D + N * N;                            // [N] symmetrised cube-root weights to u
    double* red = sw + N;                              // [kThreads]
    int* nb = reinterpret_cast<int*>(red + kThreads);  // [N] is v a neighbour of u
    int* V = nb + N;                                   // [N] the neighbours, ascending
    int* sa = V + N;                                   // [N] symmetrised adjacency to u
    const int tid = threadIdx.x;
    const size_t b = blockIdx.x / N;
    const int u = blockIdx.x % N;
    const double* W = w_all + b * N * N;

    int bad = 0;
    for (int idx = tid; idx < N * N; idx += kThreads) bad |= !(W[idx] >= 0.0);
    if (tid < N) nb[tid] = (W[u * N + tid] != 0.0 || W[tid * N + u] != 0.0) ? 1 : 0;
    bad = __syncthreads_or(bad);
    if (bad) {
        if (tid == 0) eloc[b * N + u] = NAN;
        return;
    }
    int k = 0;
    for (int v = 0; v < N; ++v) k += nb[v];
    if (tid < N && nb[tid]) {
        int pos = 0;
        for (int v = 0; v < tid; ++v) pos += nb[v];
        V[pos] = tid;
        const double out = W[u * N + tid], in = W[tid * N + u];
        sw[pos] = cuberoot(out) + cuberoot(in);
        sa[pos] = (out != 0.0) + (in != 0.0);
    }
    __syncthreads();
    // lengths among the neighbours: paths stay inside the neighbourhood
    for (int idx = tid; idx < k * k; idx += kThreads) {
        const int a = idx / k, c = idx % k;
        const double L = length_of(W[V[a] * N + V[c]]);
        D[idx] = a == c ? 0.0 : (L != 0.0 ? L : INFINITY);
    }
    __syncthreads();
    floyd_warshall_n<false>(k, D, nullptr);
    // e = 1/D with a zero diagonal (1/inf = 0), se = cuberoot(e) + cuberoot(e^T)
    for (int idx = tid; idx < k * k; idx += kThreads) D[idx] = idx / k == idx % k ? 0.0 : cuberoot(1.0 / D[idx]);
    __syncthreads();
    double part = 0.0;
    for (int idx = tid; idx < k * k; idx += kThreads) {
        const int a = idx / k, c = idx % k;
        part += sw[a] * sw[c] * (D[a * k + c] + D[c * k + a]);
    }
    red[tid] = part;
    __syncthreads();
    for (int o = kThreads / 2; o > 0; o >>= 1) {
        if (tid < o) red[tid] += red[tid + o];
        __syncthreads();
    }
    if (tid == 0) {
        const double numer = red[0] / 2;
        long long s1 = 0, s2 = 0;
        for (int a = 0; a < k; ++a) {
            s1 += sa[a];
            s2 += sa[a] * sa[a];
        }
        // no neighbour or one: numer is exactly 0 and so is E
        eloc[b * N + u] = numer != 0.0 ? numer / (double)(s1 * s1 - s2) : 0.0;
    }
}

size_t local_efficiency_lds_bytes(int N) {
    return sizeof(double) * ((size_t)N * N + N + kThreads) + sizeof(int) * 3 * (size_t)N;
}

// ---- wc_graph_clustering: one workgroup per matrix ----
// cyc3_i = sum_j (ws ws)_ij ws_ji with ws = cuberoot(w) in LDS, padded by zeros to Np, whole 16-tiles.
// Thread (ty, tx) of the 16 x 16 grid accumulates the R x R cells (ty + 16 a, tx + 16 b) of ws ws in
// registers, multiplies by ws^T and sums its rows; the 16 lanes of one ty then add up by shuffles.
// (The same product on v_mfma_f64_16x16x4_f64, 16 x 16 tiles dealt to the four waves, measured
// slower: 4.73 ms against 3.90 ms for 20,000 matrices of 90 nodes, docs/CHANGELOG.md.  The MI355X data
// sheet gives vector and matrix fp64 the same peak, and the tiles' A and B operands come from LDS
// one double per lane per MFMA, without the register reuse of the R x R cells.)
template <int R>
__device__ __forceinline__ void cyc3_rows(int Np, const double* S, double* cyc3) {
    const int ty = threadIdx.x / kGrid, tx = threadIdx.x % kGrid;
    double acc[R][R];
#pragma unroll
    for (int a = 0; a < R; ++a)
#pragma unroll
        for (int c = 0; c < R; ++c) acc[a][c] = 0.0;
    for (int k = 0; k < Np; ++k) {
        double sik[R], skj[R];
#pragma unroll
        for (int a = 0; a < R; ++a) sik[a] = S[(ty + kGrid * a) * Np + k];
#pragma unroll
        for (int c = 0; c < R; ++c) skj[c] = S[k * Np + tx + kGrid * c];
#pragma unroll
        for (int a = 0; a < R; ++a)
#pragma unroll
            for (int c = 0; c < R; ++c) acc[a][c] = fma(sik[a], skj[c], acc[a][c]);
    }
#pragma unroll
    for (int a = 0; a < R; ++a) {
        const int i = ty + kGrid * a;
        double v = 0.0;
#pragma unroll
        for (int c = 0; c < R; ++c) v = fma(acc[a][c], S[(tx + kGrid * c) * Np + i], v);
        for (int o = kGrid / 2; o > 0; o >>= 1) v += __shfl_xor(v, o);
        if (tx == 0) cyc3[i] = v;
    }
}

__device__ __forceinline__ void cyc3_all(int Np, const double* S, double* cyc3) {
    switch (Np / kGrid) {
        case 1: cyc3_rows<1>(Np, S, cyc3); break;
        case 2: cyc3_rows<2>(Np, S, cyc3); break;
        case 3: cyc3_rows<3>(Np, S, cyc3); break;
        case 4: cyc3_rows<4>(Np, S, cyc3); break;
        case 5: cyc3_rows<5>(Np, S, cyc3); break;
        default: cyc3_rows<6>(Np, S, cyc3); break;
    }
    __syncthreads();
}

__global__ void __launch_bounds__(kThreads) clustering_kernel(int N, const double* __restrict__ w_all,
                                                              double* __restrict__ clustering,
                                                              double* __restrict__ transitivity,
                                                              double* __restrict__ strengths,
                                                              int* __restrict__ degrees) {
    extern __shared__ __attribute__((aligned(16))) double lds[];
    const int Np = (N + 15) / 16 * 16;
    double* S = lds;               // [Np][Np] cuberoot(w), zero padded
    double* cyc3 = S + Np * Np;    // [Np]
    int* K = reinterpret_cast<int*>(cyc3 + Np);  // [N] non-zeros of a row
    const int tid = threadIdx.x;
    const size_t b = blockIdx.x;
    const double* W = w_all + b * N * N;

    // strengths_und and degrees_und: column sums and column counts of non-zeros; K: row counts
    if (tid < N) {
        double s = 0.0;
        int deg = 0, k = 0;
        for (int r = 0; r < N; ++r) {
            const double x = W[r * N + tid];  // coalesced over tid
            s += x;
            deg += x != 0.0;
        }
        if (strengths) strengths[b * N + tid] = s;
        if (degrees) degrees[b * N + tid] = deg;
        if (clustering || transitivity) {
            for (int c = 0; c < N; ++c) k += !(W[tid * N + c] == 0.0);  // logical_not(W == 0): NaN counts
            K[tid] = k;
        }
    }
    if (!clustering && !transitivity) return;
    for (int idx = tid; idx < Np * Np; idx += kThreads) {
        const int i = idx / Np, j = idx % Np;
        S[idx] = (i < N && j < N) ? cuberoot(W[i * N + j]) : 0.0;
    }
    __syncthreads();
    cyc3_all(Np, S, cyc3);
    if (clustering && tid < N) {
        const double k = (double)K[tid];
        clustering[b * N + tid] = cyc3[tid] == 0.0 ? 0.0 : cyc3[tid] / (k * (k - 1.0));
    }
    if (transitivity && tid == 0) {
        double s = 0.0;
        long long kk = 0;
        for (int i = 0; i < N; ++i) {
            s += cyc3[i];
            kk += (long long)K[i] * (K[i] - 1);
        }
        transitivity[b] = s / (double)kk;
    }
}

size_t clustering_lds_bytes(int N) {
    const size_t Np = (size_t)(N + 15) / 16 * 16;
    return sizeof(double) * (Np * Np + Np) + sizeof(int) * (size_t)N;
}

// The node measures below repeat the reference's sums and products one rounding at a time.
#pragma clang fp contract(off)

// ---- wc_graph_betweenness: one workgroup per matrix, one wave per source ----
// Brandes' algorithm as betweenness_wei writes it (graph_utils.py:1983-2052).  The lengths lie in LDS;
// wave k of the 16 takes the sources k, k + 16, ...; lane l owns the nodes l and l + 64 and keeps, of
// each, the distance D, the number of shortest paths NP, the dependency DP, the round in which it was
// settled and its predecessors as a 96-bit mask, all in registers.  One Dijkstra round: the wave-wide minimum
// of D over the unsettled nodes, a ballot of the nodes at that minimum (all of them are settled
// together), and for every settled v one conflict-free row read L[v][.] with the relaxation
// D[v] + L[v][w] in every lane: < replaces predecessors and path count, == adds to them.  The
// dependency pass walks the rounds backwards (a predecessor is settled in an earlier round than its
// successor, so a round's DP is final when it is reached), a round's nodes in descending order like
// the reference's Q: (1 + DP[w]) / NP[w] and w's mask are broadcast and the lanes whose bit is set add
// that times their NP.  NP[w] == 1 for a whole round (always, where shortest paths are unique) skips
// the division: x / 1 is x.  BC adds up per lane over the wave's sources; the waves combine
// through LDS in a fixed order.  No atomics: the bits do not depend on the batch.
template <int CTRL, int ROWS>
__device__ __forceinline__ uint32_t min_dpp(uint32_t x) {  // a lane that the move leaves out keeps its own
    const uint32_t y = (uint32_t)__builtin_amdgcn_update_dpp((int)x, (int)x, CTRL, ROWS, 0xf, false);
    return y < x ? y : x;
}

// minimum of an unsigned word over the 64 lanes: within a row of 16 by quad permutes and mirrors, then
// lane 15 of rows 0 and 2 into rows 1 and 3, lane 31 into rows 2 and 3; lane 63 holds it
__device__ __forceinline__ uint32_t wave_min(uint32_t x) {
    x = min_dpp<0xB1, 0xf>(x);   // quad_perm [1, 0, 3, 2]
    x = min_dpp<0x4E, 0xf>(x);   // quad_perm [2, 3, 0, 1]
    x = min_dpp<0x141, 0xf>(x);  // row_half_mirror
    x = min_dpp<0x140, 0xf>(x);  // row_mirror
    x = min_dpp<0x142, 0xa>(x);  // row_bcast:15
    x = min_dpp<0x143, 0xc>(x);  // row_bcast:31
    return (uint32_t)__builtin_amdgcn_readlane((int)x, 63);
}

// lane: the same in every lane of the wave
__device__ __forceinline__ double read_lane(double x, int lane) {
    const int lo = __builtin_amdgcn_readlane(__double2loint(x), lane);
    const int hi = __builtin_amdgcn_readlane(__double2hiint(x), lane);
    return __hiloint2double(hi, lo);
}

__device__ __forceinline__ uint64_t read_lane(uint64_t x, int lane) {
    const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)x, lane);
    const uint32_t hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(x >> 32), lane);
    return ((uint64_t)hi << 32) | lo;
}

// minimum of non-negative doubles over the 64 lanes, wave-uniform: they order as their bit patterns do,
// so the high words first and then the low words of the lanes that hold the least high word
__device__ __forceinline__ double wave_min(double x) {
    const uint32_t hi = (uint32_t)__double2hiint(x), lo = (uint32_t)__double2loint(x);
    const uint32_t mh = wave_min(hi);
    const uint32_t ml = wave_min(hi == mh ? lo : 0xFFFFFFFFu);
    return __hiloint2double((int)mh, (int)ml);
}

constexpr int kUnsettled = -1, kNoNode = -2;

struct Node {  // one of a lane's two nodes
    double d, np, dp;
    int round;
    uint64_t plo;  // predecessors 0 .. 63
    uint32_t phi;  // predecessors 64 .. 95
};

__device__ __forceinline__ void relax(Node& x, double len, double dv, double npv, uint64_t blo, uint32_t bhi) {
    if (x.round != kUnsettled || len == 0.0) return;
    const double cand = dv + len;
    if (cand < x.d) {
        x.d = cand;
        x.np = npv;
        x.plo = blo;
        x.phi = bhi;
    } else if (cand == x.d) {
        x.np += npv;
        x.plo |= blo;
        x.phi |= bhi;
    }
}

// 16 waves a matrix: a wave's round is one chain of dependent instructions (minimum, ballot, row read,
// relaxation), so the kernel runs at the rate at which a SIMD finds another wave to issue from.  With
// two workgroups a CU (the lengths of 90 nodes take 65 KB of LDS) that is 8 waves a SIMD, the most
// there are; 20,000 matrices of 90 nodes took 130, 63, 41 and 35 ms at 2, 4, 8 and 16 waves.
constexpr int kBcThreads = 1024;

__global__ void __launch_bounds__(kBcThreads) betweenness_kernel(int N, const double* __restrict__ w_all, int lengths,
                                                                 double* __restrict__ bc) {
    extern __shared__ __attribute__((aligned(16))) double lds[];
    double* Ls = lds;           // [N][N] lengths, 0 where there is no edge
    double* part = lds;         // [waves][N] the waves' sums, over the lengths once every wave is done
    const int tid = threadIdx.x;
    const size_t b = blockIdx.x;
    const double* W = w_all + b * N * N;

    int bad = 0;
    for (int idx = tid; idx < N * N; idx += kBcThreads) {
        const double x = W[idx];
        bad |= !(x >= 0.0);  // negative or NaN
        Ls[idx] = idx / N == idx % N ? 0.0 : (lengths ? x : length_of(x));
    }
    bad = __syncthreads_or(bad);
    if (bad) {  // uniform
        for (int i = tid; i < N; i += kBcThreads) bc[b * N + i] = NAN;
        return;
    }
    const int wave = tid >> 6, lane = tid & 63;
    const bool ok0 = lane < N, ok1 = lane + 64 < N;
    double bc0 = 0.0, bc1 = 0.0;
    for (int u = wave; u < N; u += kBcThreads / 64) {
        Node a = {INFINITY, 0.0, 0.0, ok0 ? kUnsettled : kNoNode, 0, 0};  // node lane
        Node c = {INFINITY, 0.0, 0.0, ok1 ? kUnsettled : kNoNode, 0, 0};  // node lane + 64
        if (lane == (u & 63)) {
            Node& src = u < 64 ? a : c;
            src.d = 0.0;
            src.np = 1.0;
        }
        int rounds = 0;
        while (rounds < N) {  // every round settles a node or more
            double m = fmin(a.round == kUnsettled ? a.d : INFINITY, c.round == kUnsettled ? c.d : INFINITY);
            m = wave_min(m);
            if (!(m < INFINITY)) break;  // every node settled, or the rest out of reach
            const bool s0 = a.round == kUnsettled && a.d == m, s1 = c.round == kUnsettled && c.d == m;
            uint64_t v0 = __ballot(s0);
            uint32_t v1 = (uint32_t)__ballot(s1);
            if (s0) a.round = rounds;
            if (s1) c.round = rounds;
            while (v0) {  // ascending, as the reference goes through V
                const int v = __builtin_amdgcn_readfirstlane(__ffsll((unsigned long long)v0) - 1);
                v0 &= v0 - 1;
                const double npv = read_lane(a.np, v);
                const double* row = Ls + v * N;
                relax(a, ok0 ? row[lane] : 0.0, m, npv, 1ull << v, 0u);
                relax(c, ok1 ? row[lane + 64] : 0.0, m, npv, 1ull << v, 0u);
            }
            while (v1) {
                const int l = __builtin_amdgcn_readfirstlane(__ffs(v1) - 1);
                v1 &= v1 - 1;
                const double npv = read_lane(c.np, l);
                const double* row = Ls + (l + 64) * N;
                relax(a, ok0 ? row[lane] : 0.0, m, npv, 0ull, 1u << l);
                relax(c, ok1 ? row[lane + 64] : 0.0, m, npv, 0ull, 1u << l);
            }
            ++rounds;
        }
        // dependencies: the nodes out of reach first (they count only where an infinite length made
        // them somebody's successor), then the rounds backwards; round 0 is the source alone
        for (int r = rounds; r >= 1; --r) {
            const bool last = r == rounds;
            const bool m0 = last ? (a.round == kUnsettled && (a.plo | a.phi)) : a.round == r;
            const bool m1 = last ? (c.round == kUnsettled && (c.plo | c.phi)) : c.round == r;
            if (m0) bc0 += a.dp;
            if (m1) bc1 += c.dp;
            double c0 = 1.0 + a.dp, c1 = 1.0 + c.dp;
            if (__any((m0 && a.np != 1.0) || (m1 && c.np != 1.0))) {
                c0 /= a.np;
                c1 /= c.np;
            }
            uint32_t w1 = (uint32_t)__ballot(m1);
            uint64_t w0 = __ballot(m0);
            while (w1) {
                const int l = __builtin_amdgcn_readfirstlane(31 - __clz((int)w1));
                w1 &= ~(1u << l);
                const double coef = read_lane(c1, l);
                const uint64_t plo = read_lane(c.plo, l);
                const uint64_t phi = (uint32_t)__builtin_amdgcn_readlane((int)c.phi, l);
                if ((plo >> lane) & 1) a.dp += coef * a.np;
                if ((phi >> lane) & 1) c.dp += coef * c.np;
            }
            while (w0) {
                const int l = __builtin_amdgcn_readfirstlane(63 - __clzll((long long)w0));
                w0 &= ~(1ull << l);
                const double coef = read_lane(c0, l);
                const uint64_t plo = read_lane(a.plo, l);
                const uint64_t phi = (uint32_t)__builtin_amdgcn_readlane((int)a.phi, l);
                if ((plo >> lane) & 1) a.dp += coef * a.np;
                if ((phi >> lane) & 1) c.dp += coef * c.np;
            }
        }
    }
    __syncthreads();
    if (ok0) part[wave * N + lane] = bc0;
    if (ok1) part[wave * N + lane + 64] = bc1;
    __syncthreads();
    if (tid < N) {
        double s = part[tid];
        for (int k = 1; k < kBcThreads / 64; ++k) s += part[k * N + tid];
        bc[b * N + tid] = s;
    }
}

size_t betweenness_lds_bytes(int N) { return sizeof(double) * (size_t)N * (N > kBcThreads / 64 ? N : kBcThreads / 64); }

// ---- wc_graph_modules: one workgroup per matrix, thread i for node i ----
// The matrix lies in LDS with an odd row stride (a thread walks its row or its column without bank
// conflicts); perm lists the nodes module by module, ascending within a module, so that a thread
// meets every module's members together and needs no table of per-module sums.  Sums run in index
// order within a module and over the modules in ascending order, as the reference's loops do.
__global__ void __launch_bounds__(kThreads) modules_kernel(int N, int K, const double* __restrict__ w_all,
                                                           const int32_t* __restrict__ ci_all, int degree, int zflag,
                                                           double gamma, double* __restrict__ part,
                                                           double* __restrict__ z, double* __restrict__ q) {
    extern __shared__ __attribute__((aligned(16))) double lds[];
    const int Ns = N | 1;
    double* Ws = lds;                                // [N][Ns]
    double* kout = Ws + N * Ns;                      // [N] row sums
    double* kin = kout + N;                          // [N] column sums
    double* koi = kin + N;                           // [N] within-module degrees
    double* qrow = koi + N;                          // [N] a row's share of Q
    int* lab = reinterpret_cast<int*>(qrow + N);     // [N] labels
    int* perm = lab + N;                             // [N] nodes by module
    const int tid = threadIdx.x;
    const size_t b = blockIdx.x;
    const double* W = w_all + b * N * N;

    for (int idx = tid; idx < N * N; idx += kThreads) Ws[idx / N * Ns + idx % N] = W[idx];
    int bad = 0;
    if (tid < N) {
        const int c = ci_all[b * N + tid];
        bad = c < 0 || c >= K;
        lab[tid] = c;
    }
    bad = __syncthreads_or(bad);
    if (bad) {  // uniform: a label out of range; nothing is indexed by it
        for (int i = tid; i < N; i += kThreads) {
            if (part) part[b * N + i] = NAN;
            if (z) z[b * N + i] = NAN;
        }
        if (q && tid == 0) q[b] = NAN;
        return;
    }
    const int i = tid < N ? tid : 0;
    const int mine = lab[i];
    int first = 0, count = 0;  // of this node's module in perm
    {
        int before = 0;
        for (int j = 0; j < N; ++j) {
            const int c = lab[j];
            first += c < mine;
            count += c == mine;
            before += c == mine && j < i;
        }
        if (tid < N) perm[first + before] = i;
    }
    __syncthreads();

    if (part && tid < N) {  // participation_coef (graph_utils.py:271-307)
        const int si = degree ? 1 : Ns, sj = degree ? Ns : 1;  // degree 'in': the transpose
        double ko = 0.0, kc2 = 0.0, km = 0.0;
        for (int j = 0; j < N; ++j) ko += Ws[i * si + j * sj];
        int cur = lab[perm[0]];
        for (int p = 0; p < N; ++p) {
            const int j = perm[p];
            if (lab[j] != cur) {
                kc2 += km * km;
                km = 0.0;
                cur = lab[j];
            }
            km += Ws[i * si + j * sj];
        }
        kc2 += km * km;
        part[b * N + i] = ko == 0.0 ? 0.0 : 1.0 - kc2 / (ko * ko);
    }
    if (z) {  // module_degree_zscore (graph_utils.py:2103-2140)
        if (tid < N) {
            double k = 0.0;
            for (int p = first; p < first + count; ++p) {
                const int j = perm[p];
                const double out = Ws[i * Ns + j], in = Ws[j * Ns + i];
                k += zflag == 3 ? out + in : (zflag == 2 ? in : out);
            }
            koi[i] = k;
        }
        __syncthreads();
        if (tid < N) {
            double s = 0.0, v = 0.0;
            for (int p = first; p < first + count; ++p) s += koi[perm[p]];
            const double mean = s / count;
            for (int p = first; p < first + count; ++p) {
                const double d = fabs(koi[perm[p]] - mean);
                v += d * d;
            }
            const double zz = (koi[i] - mean) / sqrt(v / count);  // the population's deviation
            z[b * N + i] = isnan(zz) ? 0.0 : zz;                  // the reference's Z[isnan(Z)] = 0
        }
    }
    if (q) {  // Newman / Leicht-Newman modularity of the partition
        if (tid < N) {
            double ro = 0.0, co = 0.0;
            for (int j = 0; j < N; ++j) {
                ro += Ws[i * Ns + j];
                co += Ws[j * Ns + i];
            }
            kout[i] = ro;
            kin[i] = co;
        }
        __syncthreads();
        double s = 0.0;
        for (int j = 0; j < N; ++j) s += kout[j];
        if (tid < N) {
            double acc = 0.0;
            for (int p = first; p < first + count; ++p) {
                const int j = perm[p];
                acc += Ws[i * Ns + j] - gamma * kout[i] * kin[j] / s;
            }
            qrow[i] = acc;
        }
        __syncthreads();
        if (tid == 0) {
            double acc = 0.0;
            for (int j = 0; j < N; ++j) acc += qrow[j];
            q[b] = acc / s;
        }
    }
}

size_t modules_lds_bytes(int N) {
    return sizeof(double) * ((size_t)N * (N | 1) + 4 * (size_t)N) + sizeof(int) * 2 * (size_t)N;
}

// ---- argument checks shared by the entry points ----
// shapes, w and at least one output; then w aligned, no output over w, every output aligned
int check_graph(const char* fn, int B, int N, const WcSpan& w, const WcSpan* outs, int nouts, bool per_node_grid) {
    if (B < 1) return wc_fail(WC_EINVAL, "%s: B < 1", fn);
    if (N < 2) return wc_fail(WC_EINVAL, "%s: N < 2", fn);
    if (N > kMaxN) return wc_fail(WC_EUNSUPPORTED, "%s: N = %d > 96 (one matrix per workgroup, in LDS)", fn, N);
    if (!w.p) return wc_fail(WC_EINVAL, "%s: w is NULL", fn);
    if (per_node_grid && (int64_t)B * N > INT32_MAX)
        return wc_fail(WC_EINVAL, "%s: 2^31 workgroups or more (B times N)", fn);
    bool any = false;
    for (int k = 0; k < nouts; ++k) any = any || outs[k].p;
    if (!any) return wc_fail(WC_EINVAL, "%s: every output is NULL", fn);
    if (int rc = wc_check_align(fn, &w, 1)) return rc;
    if (int rc = wc_check_alias(fn, outs, nouts, &w, 1)) return rc;
    return wc_check_align(fn, outs, nouts);
}

}  // namespace

extern "C" {

int wc_graph_paths(int B, int N, const double* w, int lengths, int include_infinite, double* dist, int* hops,
                   double* stats, double* ecc, void* stream) {
    wc_clear_err();
    const char* fn = "wc_graph_paths";
    const size_t b = B > 0 ? (size_t)B : 0, n = N > 0 ? (size_t)N : 0;
    const WcSpan outs[4] = {{"dist", dist, b * n * n * 8, 8}, {"hops", hops, b * n * n * 4, 8},
                            {"stats", stats, b * 4 * 8, 8}, {"ecc", ecc, b * n * 8, 8}};
    if (int rc = check_graph(fn, B, N, {"w", w, b * n * n * 8, 8}, outs, 4, false)) return rc;
    const size_t lds = paths_lds_bytes(N, hops != nullptr);
    if (int rc = wc_raise_lds(fn, paths_kernel, lds)) return rc;
    hipLaunchKernelGGL(paths_kernel, dim3(B), dim3(kThreads), lds, static_cast<hipStream_t>(stream), N, w, lengths,
                       include_infinite, dist, hops, stats, ecc);
    return wc_hip_check(fn);
}

int wc_graph_local_efficiency(int B, int N, const double* w, double* eloc, void* stream) {
    wc_clear_err();
    const char* fn = "wc_graph_local_efficiency";
    const size_t b = B > 0 ? (size_t)B : 0, n = N > 0 ? (size_t)N : 0;
    const WcSpan outs[1] = {{"eloc", eloc, b * n * 8, 8}};
    if (int rc = check_graph(fn, B, N, {"w", w, b * n * n * 8, 8}, outs, 1, true)) return rc;
    const size_t lds = local_efficiency_lds_bytes(N);
    if (int rc = wc_raise_lds(fn, local_efficiency_kernel, lds)) return rc;
    hipLaunchKernelGGL(local_efficiency_kernel, dim3((unsigned)(B * N)), dim3(kThreads), lds,
                       static_cast<hipStream_t>(stream), N, w, eloc);
    return wc_hip_check(fn);
}

int wc_graph_clustering(int B, int N, const double* w, double* clustering, double* transitivity, double* strengths,
                        int* degrees, void* stream) {
    wc_clear_err();
    const char* fn = "wc_graph_clustering";
    const size_t b = B > 0 ? (size_t)B : 0, n = N > 0 ? (size_t)N : 0;
    const WcSpan outs[4] = {{"clustering", clustering, b * n * 8, 8}, {"transitivity", transitivity, b * 8, 8},
                            {"strengths", strengths, b * n * 8, 8}, {"degrees", degrees, b * n * 4, 8}};
    if (int rc = check_graph(fn, B, N, {"w", w, b * n * n * 8, 8}, outs, 4, false)) return rc;
    const size_t lds = clustering_lds_bytes(N);
    if (int rc = wc_raise_lds(fn, clustering_kernel, lds)) return rc;
    hipLaunchKernelGGL(clustering_kernel, dim3(B), dim3(kThreads), lds, static_cast<hipStream_t>(stream), N, w,
                       clustering, transitivity, strengths, degrees);
    return wc_hip_check(fn);
}

int wc_graph_betweenness(int B, int N, const double* w, int lengths, double* bc, void* stream) {
    wc_clear_err();
    const char* fn = "wc_graph_betweenness";
    const size_t b = B > 0 ? (size_t)B : 0, n = N > 0 ? (size_t)N : 0;
    const WcSpan outs[1] = {{"bc", bc, b * n * 8, 8}};
    if (int rc = check_graph(fn, B, N, {"w", w, b * n * n * 8, 8}, outs, 1, false)) return rc;
    const size_t lds = betweenness_lds_bytes(N);
    if (int rc = wc_raise_lds(fn, betweenness_kernel, lds)) return rc;
    hipLaunchKernelGGL(betweenness_kernel, dim3(B), dim3(kBcThreads), lds, static_cast<hipStream_t>(stream), N, w,
                       lengths, bc);
    return wc_hip_check(fn);
}

int wc_graph_modules(int B, int N, int K, const double* w, const int32_t* ci, int degree, int zflag, double gamma,
                     double* part, double* z, double* q, void* stream) {
    wc_clear_err();
    const char* fn = "wc_graph_modules";
    const size_t b = B > 0 ? (size_t)B : 0, n = N > 0 ? (size_t)N : 0;
    const WcSpan labels = {"ci", ci, b * n * 4, 4};
    const WcSpan outs[3] = {{"part", part, b * n * 8, 8}, {"z", z, b * n * 8, 8}, {"q", q, b * 8, 8}};
    if (int rc = check_graph(fn, B, N, {"w", w, b * n * n * 8, 8}, outs, 3, false)) return rc;
    if (K < 1 || K > N) return wc_fail(WC_EINVAL, "wc_graph_modules: K must be in [1, N]");
    if (!ci) return wc_fail(WC_EINVAL, "wc_graph_modules: ci is NULL");
    if (int rc = wc_check_align(fn, &labels, 1)) return rc;
    if (degree != 0 && degree != 1) return wc_fail(WC_EINVAL, "wc_graph_modules: degree must be 0 (out) or 1 (in)");
    if (zflag < 0 || zflag > 3) return wc_fail(WC_EINVAL, "wc_graph_modules: zflag must be 0, 1, 2 or 3");
    if (int rc = wc_check_alias(fn, outs, 3, &labels, 1)) return rc;
    const size_t lds = modules_lds_bytes(N);
    if (int rc = wc_raise_lds(fn, modules_kernel, lds)) return rc;
    hipLaunchKernelGGL(modules_kernel, dim3(B), dim3(kThreads), lds, static_cast<hipStream_t>(stream), N, K, w, ci,
                       degree, zflag, gamma, part, z, q);
    return wc_hip_check(fn);
}

}  // extern "C"

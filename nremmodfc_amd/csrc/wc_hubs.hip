// wc_hubs.hip -- measures of hub organisation of a batch of N x N matrices on gfx950: the rich-club
// curves (weighted and binary), the assortativity coefficient (of strengths and of degrees) and the
// s-core.
//
// Replaces, for B matrices at once, the host loops of the reference's graph_utils.py:
//   rich_club_wu (:2528-2570), rich_club_wd (:2482-2525), rich_club_bu (:2440-2479),
//   rich_club_bd (:2396-2437)                              -> wc_graph_rich_club
//   assortativity_wei (:1869-1926), assortativity_bin (:1808-1866) -> wc_graph_assortativity
//   score_wu (:2573-2609)                                  -> wc_graph_score
// No symmetry is assumed and the diagonal is taken as given: the expressions are evaluated as the
// reference writes them.  One workgroup per matrix, the matrix in LDS; fixed order, no atomics: a
// matrix gives the same bits alone as inside any batch.  The definitions are in include/wcsde.h.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include "wc_common.h"

// The sums below are one rounding per operation, as the header states them.
#pragma clang fp contract(off)

namespace {

constexpr int kMaxN = 96;
constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;

__device__ __forceinline__ double shfl_xor(double x, int mask) {
    return __hiloint2double(__shfl_xor(__double2hiint(x), mask), __shfl_xor(__double2loint(x), mask));
}

// ---- wc_graph_rich_club: one workgroup per matrix ----
// With the nodes in descending order of degree (ties by index), the nodes kept at a level are the
// first n of that order, and the sum of the kept submatrix is the sum of the leading n x n block of
// the permuted matrix: shell a = row a and column a of that block up to the diagonal, lead[n] = shells
// 0 .. n-1.  All K levels, weighted and binary, read two tables of N + 1 entries; the work is O(N^2),
// not O(K N^2).  The matrix lies in LDS as it came, N^2 doubles at the front of the buffer the sort
// then orders.
//
// The order of all N^2 entries is a bitonic network over P = the next power of two, the rest -inf,
// descending.  A compare-exchange at distance j touches i and i + j, i running over j entries of every
// 2 j.  For j >= 32 the 32 lanes of a half-wave read 32 consecutive doubles, one bank row.  For
// j < 32 their first operands lie in 64 consecutive doubles and take only half of the residues modulo
// 32, each twice: a 2-way conflict on every read and write.  There the lanes whose i has bit 5 set
// take i + j first and i second: the two halves then cover all 32 residues.
__device__ __forceinline__ void bitonic_desc(double* S, int P) {
    for (int k = 2; k <= P; k <<= 1) {
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int t = threadIdx.x; t < P / 2; t += kThreads) {
                const int i = ((t & ~(j - 1)) << 1) | (t & (j - 1));
                const bool swap = j < 32 && (i & 32);
                const int p = swap ? i + j : i, q = swap ? i : i + j;
                const double x = S[p], y = S[q];
                const bool less = x < y;  // no NaN here; a multiset of bits is kept whatever the zeros' signs
                const double lo = less ? x : y, hi = less ? y : x;
                const bool desc = (i & k) == 0;
                const double vi = desc ? hi : lo, vj = desc ? lo : hi;  // for i and for i + j
                S[p] = swap ? vj : vi;
                S[q] = swap ? vi : vj;
            }
            __syncthreads();
        }
    }
}

__global__ void __launch_bounds__(kThreads) rich_club_kernel(int N, int P, const double* __restrict__ w_all,
                                                             int directed, int K, double* __restrict__ rw,
                                                             double* __restrict__ rb, int* __restrict__ nk,
                                                             double* __restrict__ ek, int* __restrict__ maxdeg) {
    extern __shared__ __attribute__((aligned(16))) double lds[];
    double* S = lds;                                  // [P] the matrix, then all entries in descending order
    double* bsum = S + P;                             // [P / 64] sums of 64 consecutive sorted entries
    double* shw = bsum + (P + 63) / 64;               // [N] shell sums
    double* leadw = shw + N;                          // [N + 1] sum of the leading n x n block
    int* shc = reinterpret_cast<int*>(leadw + N + 2); // [N] non-zeros of a shell
    int* leadc = shc + N;                             // [N + 1] non-zeros of the leading block
    int* deg = leadc + N + 1;                         // [N]
    int* rdeg = deg + N;                              // [N] non-zeros of a row
    int* perm = rdeg + N;                             // [N] nodes by descending degree, ties by index
    int* nge = perm + N;                              // [2 N + 3] nodes of degree >= l
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const size_t b = blockIdx.x;
    const double* W = w_all + b * N * N;
    const int NN = N * N;

    int bad = 0;
    for (int idx = tid; idx < P; idx += kThreads) {
        const double x = idx < NN ? W[idx] : -INFINITY;
        bad |= idx < NN && !(fabs(x) < INFINITY);  // NaN or an infinity
        S[idx] = x;
    }
    bad = __syncthreads_or(bad);
    if (bad) {  // uniform
        for (int k = tid; k < K; k += kThreads) {
            if (rw) rw[b * K + k] = NAN;
            if (rb) rb[b * K + k] = NAN;
            if (ek) ek[b * K + k] = NAN;
            if (nk) nk[b * K + k] = -1;
        }
        if (maxdeg && tid == 0) maxdeg[b] = -1;
        return;
    }
    // degrees: the non-zeros of a column, thread per column; of a row, wave per row
    if (tid < N) {
        int c = 0;
        for (int r = 0; r < N; ++r) c += S[r * N + tid] != 0.0;
        deg[tid] = c;
    }
    if (directed)
        for (int i = wave; i < N; i += kWaves) {
            const int c = __popcll(__ballot(lane < N && S[i * N + lane] != 0.0)) +
                          __popcll(__ballot(lane + 64 < N && S[i * N + lane + 64] != 0.0));
            if (lane == 0) rdeg[i] = c;
        }
    __syncthreads();
    if (directed && tid < N) deg[tid] += rdeg[tid];
    __syncthreads();
    if (tid < N) {
        const int d = deg[tid];
        int rank = 0;
        for (int j = 0; j < N; ++j) rank += deg[j] > d || (deg[j] == d && j < tid);
        perm[rank] = tid;
    }
    const int L = K + 1 < 2 * N + 2 ? K + 1 : 2 * N + 2;  // levels 0 .. L are counted
    for (int l = tid; l <= L; l += kThreads) {
        int c = 0;
        for (int j = 0; j < N; ++j) c += deg[j] >= l;
        nge[l] = c;
    }
    __syncthreads();
    // shell a, the partners b = a + 1 + t (mod N) so that a half-wave's rows differ in their columns
    if (tid < N) {
        const int a = tid, pa = perm[a];
        double s = 0.0;
        int c = 0;
        for (int t = 0; t < N; ++t) {
            int bb = a + 1 + t;
            bb -= bb >= N ? N : 0;
            if (bb > a) continue;
            const int pb = perm[bb];
            const double x = S[pa * N + pb];
            s += x;
            c += x != 0.0;
            if (bb < a) {
                const double y = S[pb * N + pa];
                s += y;
                c += y != 0.0;
            }
        }
        shw[a] = s;
        shc[a] = c;
    }
    __syncthreads();
    if (tid == 0) {
        double s = 0.0;
        int c = 0, m = 0;
        leadw[0] = 0.0;
        leadc[0] = 0;
        for (int a = 0; a < N; ++a) {
            s += shw[a];
            c += shc[a];
            leadw[a + 1] = s;
            leadc[a + 1] = c;
            m = deg[a] > m ? deg[a] : m;
        }
        if (maxdeg) maxdeg[b] = m;
    }
    __syncthreads();
    // binary: the nodes of degree > l
    for (int k = tid; k < K; k += kThreads) {
        const int n = nge[k + 2];
        const double e = leadw[n], nn = (double)n;
        if (nk) nk[b * K + k] = n;
        if (ek) ek[b * K + k] = e;
        if (rb) rb[b * K + k] = e / (nn * (nn - 1.0));
    }
    if (!rw) return;
    bitonic_desc(S, P);
    for (int g = wave; g < P / 64; g += kWaves) {  // P >= 64: N >= 8; below, one partial block
        double v = S[g * 64 + lane];
        for (int o = 32; o > 0; o >>= 1) v += shfl_xor(v, o);
        if (lane == 0) bsum[g] = v;
    }
    __syncthreads();
    // weighted: the nodes of degree >= l over the Er largest entries
    for (int k = tid; k < K; k += kThreads) {
        const int n = nge[k + 1];
        double r = NAN;
        if (n < N) {  // some node has a smaller degree
            const int er = leadc[n];
            double top = 0.0;
            for (int g = 0; g < er / 64; ++g) top += bsum[g];
            for (int i = er / 64 * 64; i < er; ++i) top += S[i];
            r = leadw[n] / top;
        }
        rw[b * K + k] = r;
    }
}

int sort_size(int N) {
    int P = 64;
    while (P < N * N) P <<= 1;
    return P;
}

size_t rich_club_lds_bytes(int N) {
    const size_t P = (size_t)sort_size(N);
    return sizeof(double) * (P + (P + 63) / 64 + 2 * (size_t)N + 2) + sizeof(int) * (8 * (size_t)N + 8);
}

// ---- wc_graph_assortativity: one workgroup per matrix, thread i for row i ----
// The matrix lies in LDS with an odd row stride, as in wc_graph.hip's modules_kernel.  Thread i adds
// up the three sums over the edges of its row in column order, thread 0 the rows in index order.  The
// sums of degrees are sums of integers and of halves below 2^53: exact in any order, so r_bin is the
// reference's own bits.
__global__ void __launch_bounds__(kThreads) assortativity_kernel(int N, const double* __restrict__ w_all, int flag,
                                                                 double* __restrict__ r_wei,
                                                                 double* __restrict__ r_bin) {
    extern __shared__ __attribute__((aligned(16))) double lds[];
    const int Ns = N | 1;
    double* Ws = lds;               // [N][Ns]
    double* sin_ = Ws + N * Ns;     // [N] column sums
    double* sout = sin_ + N;        // [N] row sums
    double* din = sout + N;         // [N] non-zeros of a column
    double* dout = din + N;         // [N] non-zeros of a row
    double* part = dout + N;        // [N][6] a row's sums: weighted ab, (a + b) / 2, (a^2 + b^2) / 2; binary
    int* cnt = reinterpret_cast<int*>(part + 6 * N);  // [N] a row's edges
    const int tid = threadIdx.x;
    const size_t b = blockIdx.x;
    const double* W = w_all + b * N * N;

    int bad = 0;
    for (int idx = tid; idx < N * N; idx += kThreads) {
        const double x = W[idx];
        bad |= !(fabs(x) < INFINITY);
        Ws[idx / N * Ns + idx % N] = x;
    }
    bad = __syncthreads_or(bad);
    if (bad) {  // uniform
        if (tid == 0) {
            if (r_wei) r_wei[b] = NAN;
            if (r_bin) r_bin[b] = NAN;
        }
        return;
    }
    if (tid < N) {
        double ci = 0.0, ri = 0.0;
        int cd = 0, rd = 0;
        for (int k = 0; k < N; ++k) {
            const double x = Ws[k * Ns + tid], y = Ws[tid * Ns + k];
            ci += x;
            ri += y;
            cd += x != 0.0;
            rd += y != 0.0;
        }
        sin_[tid] = ci;
        sout[tid] = ri;
        din[tid] = (double)cd;
        dout[tid] = (double)rd;
    }
    __syncthreads();
    // the two ends' values: flag 0 the undirected ones (columns) at both; 1 out/in, 2 in/out, 3 out/out,
    // 4 in/in for the degrees and, as the reference's assortativity_wei is written, in/out for the strengths
    const bool a_out = flag == 1 || flag == 3, b_out = flag == 2 || flag == 3;
    const double* sa = a_out ? sout : sin_;
    const double* sb = (b_out || flag == 4) ? sout : sin_;
    const double* da = a_out ? dout : din;
    const double* db = b_out ? dout : din;
    if (tid < N) {
        const int i = tid;
        double s1 = 0.0, s2 = 0.0, s3 = 0.0, d1 = 0.0, d2 = 0.0, d3 = 0.0;
        int c = 0;
        for (int j = flag == 0 ? i + 1 : 0; j < N; ++j) {
            if (!(Ws[i * Ns + j] > 0.0)) continue;
            const double x = sa[i], y = sb[j], u = da[i], v = db[j];
            s1 += x * y;
            s2 += 0.5 * (x + y);
            s3 += 0.5 * (x * x + y * y);
            d1 += u * v;
            d2 += 0.5 * (u + v);
            d3 += 0.5 * (u * u + v * v);
            ++c;
        }
        double* p = part + 6 * i;
        p[0] = s1, p[1] = s2, p[2] = s3, p[3] = d1, p[4] = d2, p[5] = d3;
        cnt[i] = c;
    }
    __syncthreads();
    if (tid < 2) {  // thread 0 the strengths, thread 1 the degrees
        double* out = tid ? r_bin : r_wei;
        if (out) {
            double t1 = 0.0, t2 = 0.0, t3 = 0.0;
            int e = 0;
            for (int i = 0; i < N; ++i) {
                t1 += part[6 * i + 3 * tid];
                t2 += part[6 * i + 3 * tid + 1];
                t3 += part[6 * i + 3 * tid + 2];
                e += cnt[i];
            }
            const double E = (double)e;
            const double term1 = t1 / E;
            const double h = t2 / E;
            const double term2 = h * h;
            const double term3 = t3 / E;
            out[b] = (term1 - term2) / (term3 - term2);  // no edge: 0 / 0
        }
    }
}

size_t assortativity_lds_bytes(int N) {
    return sizeof(double) * ((size_t)N * (N | 1) + 10 * (size_t)N) + sizeof(int) * (size_t)N;
}

// ---- wc_graph_score: one workgroup per matrix, one wave per level ----
// The matrix lies in LDS; a wave takes the levels wave, wave + waves, ...; lane l owns the columns l
// and l + 64 and the nodes still there are two ballots, so a pass needs no barrier.  A column is summed
// over the rows still there in ascending order; a peeled row holds zeros in the reference, and adding
// them changes no sum.
__global__ void __launch_bounds__(kThreads) score_kernel(int N, int S, const double* __restrict__ w_all,
                                                         const double* __restrict__ s_all, int* __restrict__ member,
                                                         int* __restrict__ sn, int* __restrict__ rounds) {
    extern __shared__ __attribute__((aligned(16))) double lds[];
    double* Ws = lds;  // [N][N]
    const int tid = threadIdx.x, waves = blockDim.x >> 6, wave = tid >> 6, lane = tid & 63;
    const size_t b = blockIdx.x;
    const double* W = w_all + b * N * N;

    int bad = 0;
    for (int idx = tid; idx < N * N; idx += blockDim.x) {
        const double x = W[idx];
        bad |= !(fabs(x) < INFINITY);
        Ws[idx] = x;
    }
    bad = __syncthreads_or(bad);
    const bool ok0 = lane < N, ok1 = lane + 64 < N;
    for (int lv = wave; lv < S; lv += waves) {
        const size_t o = b * S + lv;
        if (bad) {  // uniform
            if (member && ok0) member[o * N + lane] = -1;
            if (member && ok1) member[o * N + lane + 64] = -1;
            if (lane == 0) {
                if (sn) sn[o] = -1;
                if (rounds) rounds[o] = -1;
            }
            continue;
        }
        const double level = s_all[o];
        uint64_t m0 = __ballot(ok0);
        uint32_t m1 = (uint32_t)__ballot(ok1);
        int passes = 0;
        double s0 = 0.0, s1 = 0.0;
        for (int pass = 0; pass <= N; ++pass) {  // every pass but the last peels a node or more
            s0 = 0.0, s1 = 0.0;
            const bool in0 = (m0 >> lane) & 1, in1 = ok1 && ((m1 >> lane) & 1);
            for (int r = 0; r < N; ++r) {
                const bool there = r < 64 ? (m0 >> r) & 1 : (m1 >> (r - 64)) & 1;  // uniform
                if (!there) continue;
                if (in0) s0 += Ws[r * N + lane];
                if (in1) s1 += Ws[r * N + lane + 64];
            }
            const uint64_t p0 = __ballot(in0 && s0 > 0.0 && s0 < level);
            const uint32_t p1 = (uint32_t)__ballot(in1 && s1 > 0.0 && s1 < level);
            if (!p0 && !p1) break;
            m0 &= ~p0;
            m1 &= ~p1;
            ++passes;
        }
        const int size = __popcll(__ballot(s0 > 0.0)) + __popcll(__ballot(s1 > 0.0));
        if (member && ok0) member[o * N + lane] = (int)((m0 >> lane) & 1);
        if (member && ok1) member[o * N + lane + 64] = (int)((m1 >> lane) & 1);
        if (lane == 0) {
            if (sn) sn[o] = size;
            if (rounds) rounds[o] = passes;
        }
    }
}

size_t score_lds_bytes(int N) { return sizeof(double) * (size_t)N * N; }

// shapes, w and at least one output, in wc_graph.hip's order
int check_hubs(const char* fn, int B, int N, const WcSpan& w, const WcSpan* outs, int nouts) {
    if (B < 1) return wc_fail(WC_EINVAL, "%s: B < 1", fn);
    if (N < 2) return wc_fail(WC_EINVAL, "%s: N < 2", fn);
    if (N > kMaxN) return wc_fail(WC_EUNSUPPORTED, "%s: N = %d > 96 (one matrix per workgroup, in LDS)", fn, N);
    if (!w.p) return wc_fail(WC_EINVAL, "%s: w is NULL", fn);
    bool any = false;
    for (int k = 0; k < nouts; ++k) any = any || outs[k].p;
    if (!any) return wc_fail(WC_EINVAL, "%s: every output is NULL", fn);
    return WC_OK;
}

}  // namespace

extern "C" {

int wc_graph_rich_club(int B, int N, const double* w, int directed, int K, double* rw, double* rb, int32_t* nk,
                       double* ek, int32_t* maxdeg, void* stream) {
    wc_clear_err();
    const char* fn = "wc_graph_rich_club";
    const size_t b = B > 0 ? (size_t)B : 0, n = N > 0 ? (size_t)N : 0, k = K > 0 ? (size_t)K : 0;
    const WcSpan in = {"w", w, b * n * n * 8, 8};
    const WcSpan outs[5] = {{"rw", rw, b * k * 8, 8}, {"rb", rb, b * k * 8, 8}, {"nk", nk, b * k * 4, 4},
                            {"ek", ek, b * k * 8, 8}, {"maxdeg", maxdeg, b * 4, 4}};
    if (int rc = check_hubs(fn, B, N, in, outs, 5)) return rc;
    const int kmax = directed ? 2 * N : N;
    if (K < 1 || K > kmax)
        return wc_fail(WC_EINVAL, "%s: K = %d, must be in [1, %d] (%s)", fn, K, kmax,
                       directed ? "2 N, the largest in- plus out-degree" : "N, the largest degree");
    if (int rc = wc_check_spans(fn, &in, 1, outs, 5)) return rc;
    const size_t lds = rich_club_lds_bytes(N);
    if (int rc = wc_raise_lds(fn, rich_club_kernel, lds)) return rc;
    hipLaunchKernelGGL(rich_club_kernel, dim3(B), dim3(kThreads), lds, static_cast<hipStream_t>(stream), N,
                       sort_size(N), w, directed != 0, K, rw, rb, nk, ek, maxdeg);
    return wc_hip_check(fn);
}

int wc_graph_assortativity(int B, int N, const double* w, int flag, double* r_wei, double* r_bin, void* stream) {
    wc_clear_err();
    const char* fn = "wc_graph_assortativity";
    const size_t b = B > 0 ? (size_t)B : 0, n = N > 0 ? (size_t)N : 0;
    const WcSpan in = {"w", w, b * n * n * 8, 8};
    const WcSpan outs[2] = {{"r_wei", r_wei, b * 8, 8}, {"r_bin", r_bin, b * 8, 8}};
    if (int rc = check_hubs(fn, B, N, in, outs, 2)) return rc;
    if (flag < 0 || flag > 4) return wc_fail(WC_EINVAL, "%s: flag = %d, must be 0 .. 4", fn, flag);
    if (int rc = wc_check_spans(fn, &in, 1, outs, 2)) return rc;
    const size_t lds = assortativity_lds_bytes(N);
    if (int rc = wc_raise_lds(fn, assortativity_kernel, lds)) return rc;
    hipLaunchKernelGGL(assortativity_kernel, dim3(B), dim3(kThreads), lds, static_cast<hipStream_t>(stream), N, w,
                       flag, r_wei, r_bin);
    return wc_hip_check(fn);
}

int wc_graph_score(int B, int N, int S, const double* w, const double* s, int32_t* member, int32_t* sn,
                   int32_t* rounds, void* stream) {
    wc_clear_err();
    const char* fn = "wc_graph_score";
    const size_t b = B > 0 ? (size_t)B : 0, n = N > 0 ? (size_t)N : 0, ns = S > 0 ? (size_t)S : 0;
    const WcSpan ins[2] = {{"w", w, b * n * n * 8, 8}, {"s", s, b * ns * 8, 8}};
    const WcSpan outs[3] = {{"member", member, b * ns * n * 4, 4}, {"sn", sn, b * ns * 4, 4},
                            {"rounds", rounds, b * ns * 4, 4}};
    if (int rc = check_hubs(fn, B, N, ins[0], outs, 3)) return rc;
    if (S < 1) return wc_fail(WC_EINVAL, "%s: S < 1", fn);
    if ((int64_t)B * S > INT32_MAX) return wc_fail(WC_EINVAL, "%s: 2^31 cores or more (B times S)", fn);
    if (!s) return wc_fail(WC_EINVAL, "%s: s is NULL", fn);
    if (int rc = wc_check_spans(fn, ins, 2, outs, 3)) return rc;
    const size_t lds = score_lds_bytes(N);
    if (int rc = wc_raise_lds(fn, score_kernel, lds)) return rc;
    const int waves = S < kWaves ? S : kWaves;
    hipLaunchKernelGGL(score_kernel, dim3(B), dim3(64 * waves), lds, static_cast<hipStream_t>(stream), N, S, w, s,
                       member, sn, rounds);
    return wc_hip_check(fn);
}

}  // extern "C"

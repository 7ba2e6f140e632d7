// wc_nullmodel.hip -- degree- and strength-preserving null models of signed undirected matrices, for a
// batch of N x N matrices and R seeds on gfx950: the reference's randmio_und_signed
// (graph_utils.py:2165-2217) and null_model_und_sign (:2219-2338; Rubinov & Sporns 2011)
//                                                          -> wc_graph_rewire, wc_graph_null_model
//
// One problem is one (matrix, seed) pair and one workgroup of four waves; both entry points run the
// same kernel.  A problem has two phases.
//   Rewiring.  A Markov chain of itr iterations, each trying up to A attempts on four distinct nodes.
//     A failed attempt leaves the matrix as it was, so wave 0 evaluates 64 consecutive draws of the
//     run's Philox stream at once and commits the first that succeeds within the iteration's attempt
//     budget, counting the draws with four distinct nodes among the lanes before it (mbcnt): exactly
//     the sequential result.  The matrix lies in LDS as fp64, the weights move with the signs.
//   Weight assignment, once per sign.  P = S S^T takes the matrix's place in LDS.  Per period the live
//     keys P[i][j] are sorted with their position in the live list as the second key (every pair
//     distinct, so the sorting network gives the stable order): the bitonic network with every
//     comparator ascending, which sorts any m with the places from m on read as +inf, that is, left
//     out.  The k <= 64 picks of the period then rescale two rows and two columns of P each, in the
//     reference's order, one rounding per operation and no fma; the live list and the list of the
//     weights still to be given are compacted in place.
//   in LDS     the matrix / P [N][N], the sort keys [N (N - 1) / 2] uint64 with their uint16 positions,
//              the live list and the ranks of the remaining weights (uint16), S and the strengths:
//              144.2 KB at N = 96;
//   in global  the sorted weights Wv of both signs, which a period reads k times: the workgroup's slot
//              of the workspace, N (N - 1) / 2 fp64.
// The grid is bounded by the number of slots and a workgroup strides over the problems; a slot belongs
// to a workgroup, not to a problem, and all of a problem's state is set anew, so a pair gives the same
// bits alone, in any batch and with any workspace.  Every sum has a fixed order (ascending index) and
// there are no atomics.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include "wc_common.h"
#include "wc_device.h"

#pragma clang fp contract(off)

namespace {

constexpr int kMaxN = 96;
constexpr int kThreads = 256;
constexpr int kWave = 64;
constexpr int kMaxPeriod = 64;
constexpr int kMaxLive = kMaxN * (kMaxN - 1) / 2;                  // 4560
constexpr int kPerThread = (kMaxLive + kThreads - 1) / kThreads;   // 18: a thread's share of a list
constexpr uint32_t kQuadRewire = 0x8000u;  // Philox quad of the rewiring draws
constexpr uint32_t kQuadShuffle = 0x4000u; // ... of the shuffles: + 0x100 pass + (q >> 2)

// a double as an integer of the same order, -0.0 as 0.0
__device__ __forceinline__ uint64_t sort_key(double x) {
    if (x == 0.0) x = 0.0;
    const uint64_t b = (uint64_t)__double_as_longlong(x);
    return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}
__device__ __forceinline__ double key_value(uint64_t k) {
    return __longlong_as_double((long long)((k >> 63) ? (k & 0x7fffffffffffffffull) : ~k));
}

// key[0 .. m), idx[0 .. m) ascending by (key, idx): the bitonic network with every comparator
// ascending (the first step of a merge pairs i with its mirror image in the block), so that places
// from m on, read as +inf, never move and are left out.  Synchronised on entry and on return.
__device__ void sort_pairs(uint64_t* key, uint16_t* idx, int m) {
    const int tid = threadIdx.x;
    int n2 = 1;
    while (n2 < m) n2 <<= 1;
    __syncthreads();
    for (int k = 2; k <= n2; k <<= 1) {
        for (int j = k >> 1; j > 0; j >>= 1) {
            const int mask = j == (k >> 1) ? k - 1 : j;
            for (int p = tid; p < (n2 >> 1); p += kThreads) {
                const int i = ((p & ~(j - 1)) << 1) | (p & (j - 1));
                if (i >= m) break;  // i grows with p
                const int l = i ^ mask;
                if (l < m) {
                    const uint64_t ki = key[i], kl = key[l];
                    const uint16_t xi = idx[i], xl = idx[l];
                    if (kl < ki || (kl == ki && xl < xi)) {
                        key[i] = kl;
                        key[l] = ki;
                        idx[i] = xl;
                        idx[l] = xi;
                    }
                }
            }
            __syncthreads();
        }
    }
}

// a[0 .. m) without the places del[0 .. k), in place, the order kept.  Synchronised on return.
__device__ void compact(uint16_t* a, int m, const int* del, int k) {
    const int tid = threadIdx.x;
    uint16_t tmp[kPerThread];
#pragma unroll
    for (int u = 0; u < kPerThread; ++u) {
        const int x = tid + u * kThreads;
        tmp[u] = x < m ? a[x] : (uint16_t)0;
    }
    __syncthreads();
#pragma unroll
    for (int u = 0; u < kPerThread; ++u) {
        const int x = tid + u * kThreads;
        if (x < m) {
            int below = 0;
            bool dead = false;
            for (int q = 0; q < k; ++q) {
                const int d = del[q];
                below += d < x;
                dead |= d == x;
            }
            if (!dead) a[x - below] = tmp[u];
        }
    }
    __syncthreads();
}

__device__ __forceinline__ int sign_of(double x) { return (x > 0.0) - (x < 0.0); }

struct Lds {
    double *M, *Spos, *Sneg, *S, *yp, *yn, *wq;
    uint64_t* key;
    int *rc0, *rc1, *Rq, *oq, *pq, *mpos, *mval, *shared;
    uint32_t* words;
    uint16_t *idx, *live, *wl;
};

__host__ __device__ inline size_t lds_doubles(int N) { return (size_t)N * N + 5 * (size_t)N + kMaxPeriod; }
__host__ __device__ inline size_t lds_ints(int N) { return 2 * (size_t)N + 6 * kMaxPeriod + 8; }

size_t lds_bytes(int N) {
    const size_t E = (size_t)N * (N - 1) / 2;
    return 8 * (lds_doubles(N) + E) + 4 * lds_ints(N) + 2 * 3 * (E + 1);
}

// out is w0 [P][N][N] (wr with rewire_only); it is read back for r, so not __restrict__
__global__ void __launch_bounds__(kThreads) nullmodel_kernel(int P, int R, int N, const double* __restrict__ w_all,
                                                             int itr, int period, int neg_mode, int rewire_only,
                                                             const uint64_t* __restrict__ seeds, double* out_all,
                                                             double* r_out, int32_t* info, double* ws) {
    extern __shared__ __attribute__((aligned(16))) double lds[];
    const int E = N * (N - 1) / 2;
    Lds s;
    s.M = lds;                      // [N][N] the matrix, diagonal cleared; later P
    s.Spos = s.M + N * N;           // [N] column sums of the positive weights of w
    s.Sneg = s.Spos + N;            // [N] ... of the negative ones (negative sums)
    s.S = s.Sneg + N;               // [N] the strengths still to be given
    s.yp = s.S + N;                 // [N] strengths of w0
    s.yn = s.yp + N;
    s.wq = s.yn + N;                // [64] the weights of a period's picks
    s.key = reinterpret_cast<uint64_t*>(s.wq + kMaxPeriod);  // [E]
    s.rc0 = reinterpret_cast<int*>(s.key + E);               // [N] sign-s entries right of the diagonal, by row
    s.rc1 = s.rc0 + N;
    s.Rq = s.rc1 + N;               // [64] the ranks a period picks
    s.oq = s.Rq + kMaxPeriod;       // [64] their places in the live list
    s.pq = s.oq + kMaxPeriod;       // [64] i N + j of those places
    s.mpos = s.pq + kMaxPeriod;     // [64] the shuffle's displaced places and their values
    s.mval = s.mpos + kMaxPeriod;
    s.words = reinterpret_cast<uint32_t*>(s.mval + kMaxPeriod);  // [64]
    s.shared = reinterpret_cast<int*>(s.words + kMaxPeriod);     // [8] eff, draws
    s.idx = reinterpret_cast<uint16_t*>(s.shared + 8);           // [E]
    s.live = s.idx + E + 1;                                      // [E] positive edges, then negative ones
    s.wl = s.live + E + 1;                                       // [E] index into Wv of the weights left
    const int tid = threadIdx.x;
    double* Wv = ws + (size_t)blockIdx.x * E;  // the slot: sorted weights, positive then negative
    const int attempts = ((N & 1) ? ((((N - 1) / 2) & 1) ? (N + 1) / 2 : (N - 1) / 2) : N / 2) + 1;  // :2187, half to even

    for (int prob = blockIdx.x; prob < P; prob += gridDim.x) {
        const double* w = w_all + (size_t)(prob / R) * N * N;
        const uint64_t seed = seeds[prob % R];
        double* out = out_all + (size_t)prob * N * N;
        __syncthreads();  // the problem before this one has left the LDS

        int nonfinite = 0, asym = 0;
        for (int e = tid; e < N * N; e += kThreads) {
            const int i = e / N, j = e % N;
            const double x = w[e];
            nonfinite |= !isfinite(x);
            if (i != j) asym |= !(x == w[j * N + i]);
            s.M[e] = i == j ? 0.0 : x;  // :2264
        }
        nonfinite = __syncthreads_or(nonfinite);
        asym = __syncthreads_or(asym);
        int status = nonfinite ? 3 : (asym ? 2 : 0);
        int eff = 0, draws = 0;
        if (status == 0) {
            // what the assignment needs of w itself: strengths, sorted weights, the positive count
            int mp = 0, mn = 0, npos = 0;
            if (!rewire_only) {
                for (int t = tid; t < N; t += kThreads) {
                    double a0 = 0.0, a1 = 0.0;
                    int c0 = 0, c1 = 0;
                    for (int i = 0; i < N; ++i) {
                        const double x = s.M[i * N + t];
                        a0 += x > 0.0 ? x : 0.0;
                        a1 += x < 0.0 ? x : 0.0;
                    }
                    for (int c = t + 1; c < N; ++c) {
                        const double x = s.M[t * N + c];
                        c0 += x > 0.0;
                        c1 += x < 0.0;
                    }
                    s.Spos[t] = a0;
                    s.Sneg[t] = a1;
                    s.rc0[t] = c0;
                    s.rc1[t] = c1;
                }
                __syncthreads();
                for (int t = 0; t < N; ++t) {
                    mp += s.rc0[t];
                    mn += s.rc1[t];
                }
                npos = 2 * mp;
                for (int t = tid; t < N; t += kThreads) {
                    int o0 = 0, o1 = mp;
                    for (int r = 0; r < t; ++r) {
                        o0 += s.rc0[r];
                        o1 += s.rc1[r];
                    }
                    for (int c = t + 1; c < N; ++c) {
                        const double x = s.M[t * N + c];
                        if (x > 0.0) s.key[o0++] = sort_key(x);
                        if (x < 0.0) s.key[o1++] = sort_key(neg_mode ? -x : x);
                    }
                }
                for (int e = tid; e < mp + mn; e += kThreads) s.idx[e] = (uint16_t)e;
                sort_pairs(s.key, s.idx, mp);            // :2286
                sort_pairs(s.key + mp, s.idx + mp, mn);
                for (int e = tid; e < mp + mn; e += kThreads) {
                    Wv[e] = key_value(s.key[e]);
                    s.wl[e] = (uint16_t)e;
                }
            }

            // ---- rewiring (:2165-2217), wave 0 ----
            if ((rewire_only || npos < N * (N - 1)) && tid < kWave) {  // :2268
                uint64_t d0 = 0;
                int done = 0;
                const uint64_t below = tid ? (~0ull >> (64 - tid)) : 0ull;
                for (int it = 0; it < itr; ++it) {
                    int att = 0;
                    for (;;) {
                        uint32_t x[4];
                        wcdev::philox_ctr(d0 + (uint64_t)tid, kQuadRewire, seed, x);
                        const int a = (int)__umulhi(x[0], (uint32_t)N), b = (int)__umulhi(x[1], (uint32_t)N);
                        const int c = (int)__umulhi(x[2], (uint32_t)N), d = (int)__umulhi(x[3], (uint32_t)N);
                        const bool distinct = a != b && a != c && a != d && b != c && b != d && c != d;
                        double ab = 0.0, cd = 0.0, ad = 0.0, cb = 0.0;
                        bool ok = false;
                        if (distinct) {
                            ab = s.M[a * N + b];
                            cd = s.M[c * N + d];
                            ad = s.M[a * N + d];
                            cb = s.M[c * N + b];
                            ok = sign_of(ab) == sign_of(cd) && sign_of(ad) == sign_of(cb) && sign_of(ab) != sign_of(ad);
                        }
                        const uint64_t dm = __ballot(distinct), om = __ballot(ok);
                        const int ai = att + __popcll(dm & below);  // the attempt this draw would be
                        const uint64_t hit = om & __ballot(ai < attempts);
                        if (hit) {
                            const int first = __ffsll((long long)hit) - 1;
                            if (tid == first) {  // :2206-2210
                                s.M[a * N + d] = s.M[d * N + a] = ab;
                                s.M[a * N + b] = s.M[b * N + a] = ad;
                                s.M[c * N + b] = s.M[b * N + c] = cd;
                                s.M[c * N + d] = s.M[d * N + c] = cb;
                            }
                            __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
                            __builtin_amdgcn_wave_barrier();
                            ++done;
                            d0 += (uint64_t)first + 1;
                            break;
                        }
                        const uint64_t last = dm & __ballot(ai == attempts - 1);
                        if (last) {  // the budget ends on this draw
                            d0 += (uint64_t)__ffsll((long long)last);
                            break;
                        }
                        att += __popcll(dm);
                        d0 += kWave;
                    }
                }
                if (tid == 0) {
                    s.shared[0] = done;
                    s.shared[1] = (int)(uint32_t)d0;
                }
            } else if (tid == 0) {
                s.shared[0] = s.shared[1] = 0;
            }
            __syncthreads();
            eff = s.shared[0];
            draws = s.shared[1];

            if (rewire_only) {
                for (int e = tid; e < N * N; e += kThreads) out[e] = s.M[e];
            } else {
                // the live lists of the rewired pattern, row-major (:2287-2288), and an empty w0
                for (int t = tid; t < N; t += kThreads) {
                    int c0 = 0, c1 = 0;
                    for (int c = t + 1; c < N; ++c) {
                        const double x = s.M[t * N + c];
                        c0 += x > 0.0;
                        c1 += x < 0.0;
                    }
                    s.rc0[t] = c0;
                    s.rc1[t] = c1;
                }
                for (int e = tid; e < N * N; e += kThreads) out[e] = 0.0;
                __syncthreads();
                for (int t = tid; t < N; t += kThreads) {
                    int o0 = 0, o1 = mp;
                    for (int r = 0; r < t; ++r) {
                        o0 += s.rc0[r];
                        o1 += s.rc1[r];
                    }
                    for (int c = t + 1; c < N; ++c) {
                        const double x = s.M[t * N + c];
                        if (x > 0.0) s.live[o0++] = (uint16_t)(t * N + c);
                        if (x < 0.0) s.live[o1++] = (uint16_t)(t * N + c);
                    }
                }
                __syncthreads();

                for (int pass = 0; pass < 2 && status == 0; ++pass) {  // :2277
                    const int base = pass ? mp : 0, m0 = pass ? mn : mp;
                    if (m0 == 0) continue;
                    uint16_t* live = s.live + base;
                    uint16_t* wl = s.wl + base;
                    for (int t = tid; t < N; t += kThreads)
                        s.S[t] = pass ? (neg_mode ? -s.Sneg[t] : s.Sneg[t]) : s.Spos[t];  // :2285
                    __syncthreads();
                    for (int e = tid; e < N * N; e += kThreads) s.M[e] = s.S[e / N] * s.S[e % N];  // :2290
                    __syncthreads();
                    if (period == 0) {  // :2292-2294
                        for (int x = tid; x < m0; x += kThreads) {
                            s.key[x] = sort_key(s.M[live[x]]);
                            s.idx[x] = (uint16_t)x;
                        }
                        sort_pairs(s.key, s.idx, m0);
                        for (int x = tid; x < m0; x += kThreads) {
                            const int pos = live[s.idx[x]];
                            const double v = Wv[wl[x]];
                            out[pos] = out[pos % N * N + pos / N] = pass ? -v : v;
                        }
                        __syncthreads();
                        continue;
                    }
                    int pi = 0;
                    for (int m = m0; m > 0 && status == 0; m -= period, ++pi) {  // :2298-2299
                        const int k = m < period ? m : period;
                        for (int x = tid; x < m; x += kThreads) {
                            s.key[x] = sort_key(s.M[live[x]]);
                            s.idx[x] = (uint16_t)x;
                        }
                        if (tid < k) {
                            uint32_t x[4];
                            wcdev::philox_ctr((uint64_t)pi, kQuadShuffle + 0x100u * pass + ((uint32_t)tid >> 2), seed, x);
                            const int c = tid & 3;
                            s.words[tid] = c == 0 ? x[0] : (c == 1 ? x[1] : (c == 2 ? x[2] : x[3]));
                        }
                        __syncthreads();
                        if (tid == 0) {  // :2302, the first k values of a Fisher-Yates shuffle of 0 .. m-1
                            int nmap = 0;
                            for (int q = 0; q < k; ++q) {
                                const int j = q + (int)(((uint64_t)s.words[q] * (uint64_t)(m - q)) >> 32);
                                int vq = q, vj = j, ej = -1;
                                for (int e = 0; e < nmap; ++e) {
                                    if (s.mpos[e] == q) vq = s.mval[e];
                                    if (s.mpos[e] == j) {
                                        vj = s.mval[e];
                                        ej = e;
                                    }
                                }
                                s.Rq[q] = vj;
                                if (ej < 0) {
                                    ej = nmap++;
                                    s.mpos[ej] = j;
                                }
                                s.mval[ej] = vq;
                            }
                        }
                        sort_pairs(s.key, s.idx, m);  // :2301
                        if (tid < k) {
                            const int r = s.Rq[tid], o = s.idx[r];
                            s.oq[tid] = o;
                            s.pq[tid] = live[o];
                            s.wq[tid] = Wv[wl[r]];
                        }
                        __syncthreads();
                        for (int q = 0; q < k; ++q) {  // :2303-2319
                            const int pos = s.pq[q], i = pos / N, j = pos % N;
                            const double v = s.wq[q], si = s.S[i], sj = s.S[j];
                            if (si == 0.0 || sj == 0.0) {  // uniform: the reference divides by zero here
                                status = 1;
                                break;
                            }
                            const double fi = 1.0 - v / si, fj = 1.0 - v / sj;
                            if (tid < N) {
                                s.M[i * N + tid] *= fi;
                                s.M[tid * N + i] *= fi;
                            }
                            __syncthreads();
                            if (tid < N) {
                                s.M[j * N + tid] *= fj;
                                s.M[tid * N + j] *= fj;
                            }
                            if (tid == 0) {
                                out[i * N + j] = out[j * N + i] = pass ? -v : v;  // :2306, :2328
                                s.S[i] = si - v;
                                s.S[j] = sj - v;
                            }
                            __syncthreads();
                        }
                        if (status) break;
                        compact(live, m, s.oq, k);  // :2321-2326
                        compact(wl, m, s.Rq, k);
                    }
                }
                __syncthreads();
            }
        }

        if (status) {  // uniform
            for (int e = tid; e < N * N; e += kThreads) out[e] = NAN;
            if (status > 1) eff = draws = 0;
        }
        if (!rewire_only && r_out) {  // :2330-2337
            if (status == 0) {
                for (int t = tid; t < N; t += kThreads) {
                    double a0 = 0.0, a1 = 0.0;
                    for (int i = 0; i < N; ++i) {
                        const double x = out[i * N + t];
                        a0 += x > 0.0 ? x : 0.0;
                        a1 += x < 0.0 ? -x : 0.0;
                    }
                    s.yp[t] = a0;
                    s.yn[t] = a1;
                }
            }
            __syncthreads();
            if (tid < 2) {
                double r = NAN;
                if (status == 0) {
                    const double* y = tid ? s.yn : s.yp;
                    const double* x0 = tid ? s.Sneg : s.Spos;
                    const double sx = tid ? -1.0 : 1.0;
                    double mx = 0.0, my = 0.0;
                    for (int t = 0; t < N; ++t) {
                        mx += sx * x0[t];
                        my += y[t];
                    }
                    mx /= N;
                    my /= N;
                    double sxx = 0.0, syy = 0.0, sxy = 0.0;
                    for (int t = 0; t < N; ++t) {
                        const double dx = sx * x0[t] - mx, dy = y[t] - my;
                        sxx += dx * dx;
                        syy += dy * dy;
                        sxy += dx * dy;
                    }
                    r = sxy / sqrt(sxx) / sqrt(syy);
                    if (r > 1.0) r = 1.0;
                    if (r < -1.0) r = -1.0;
                }
                r_out[(size_t)prob * 2 + tid] = r;
            }
        }
        if (info && tid == 0) {
            info[(size_t)prob * 3] = eff;
            info[(size_t)prob * 3 + 1] = draws;
            info[(size_t)prob * 3 + 2] = status;
        }
    }
}

size_t slot_bytes(int N) { return sizeof(double) * ((size_t)N * (N - 1) / 2); }

// the checks the two entry points share, then the launch
int run(const char* fn, bool rewire_only, int B, int R, int N, const double* w, int bin_swaps, int period, int neg_mode,
        const uint64_t* seeds, double* out, const char* out_name, double* r, int32_t* info, void* workspace,
        size_t ws_bytes, void* stream) {
    wc_clear_err();
    if (int rc = wc_check_seeded(fn, B, R, N, 4, "a rewiring takes four distinct nodes", kMaxN,
                                 "one matrix per workgroup, in LDS", "problems"))
        return rc;
    if (bin_swaps < 0) return wc_fail(WC_EINVAL, "%s: bin_swaps = %d < 0", fn, bin_swaps);
    const int64_t itr = (int64_t)bin_swaps * (N * (N - 1) / 2);
    const int half = (N & 1) ? ((((N - 1) / 2) & 1) ? (N + 1) / 2 : (N - 1) / 2) : N / 2;
    if (itr * (half + 1) > INT32_MAX)
        return wc_fail(WC_EINVAL, "%s: bin_swaps = %d: %lld iterations of %d attempts reach 2^31", fn, bin_swaps,
                       (long long)itr, half + 1);
    if (!rewire_only) {
        if (period < 0) return wc_fail(WC_EINVAL, "%s: period = %d < 0", fn, period);
        if (period > kMaxPeriod)
            return wc_fail(WC_EUNSUPPORTED, "%s: period = %d > 64 (the picks of one period, in LDS)", fn, period);
        if (neg_mode != 0 && neg_mode != 1)
            return wc_fail(WC_EINVAL, "%s: neg_mode = %d, must be 0 (the reference's) or 1 (BCT)", fn, neg_mode);
    }
    if (!w || !seeds || !out || !workspace)
        return wc_fail(WC_EINVAL, "%s: w, seeds, %s or workspace is NULL", fn, out_name);
    const size_t b = B, rr = R, n = N, probs = b * rr;
    WcSlots plan;
    if (int rc = wc_plan_slots(fn, workspace, ws_bytes, slot_bytes(N), "4 N (N - 1)", probs, &plan)) return rc;
    const WcSpan ins[2] = {{"w", w, b * n * n * 8, 8}, {"seeds", seeds, rr * 8, 8}};
    const WcSpan outs[4] = {{out_name, out, probs * n * n * 8, 8}, {"r", r, probs * 2 * 8, 8},
                            {"info", info, probs * 3 * 4, 4}, plan.span};
    if (int rc = wc_check_spans(fn, ins, 2, outs, 4)) return rc;
    const size_t lds = lds_bytes(N);
    if (int rc = wc_raise_lds(fn, nullmodel_kernel, lds)) return rc;
    hipLaunchKernelGGL(nullmodel_kernel, dim3((unsigned)plan.slots), dim3(kThreads), lds, static_cast<hipStream_t>(stream),
                       (int)probs, R, N, w, (int)itr, period, neg_mode, rewire_only ? 1 : 0, seeds, out, r, info,
                       static_cast<double*>(workspace));
    return wc_hip_check(fn);
}

}  // namespace

extern "C" {

size_t wc_graph_null_model_slot_bytes(int N) { return N < 4 || N > kMaxN ? 0 : slot_bytes(N); }

int wc_graph_rewire(int B, int R, int N, const double* w, int bin_swaps, const uint64_t* seeds, double* wr,
                    int32_t* info, void* workspace, size_t ws_bytes, void* stream) {
    return run("wc_graph_rewire", true, B, R, N, w, bin_swaps, 0, 0, seeds, wr, "wr", nullptr, info, workspace, ws_bytes,
               stream);
}

int wc_graph_null_model(int B, int R, int N, const double* w, int bin_swaps, int period, int neg_mode,
                        const uint64_t* seeds, double* w0, double* r, int32_t* info, void* workspace, size_t ws_bytes,
                        void* stream) {
    return run("wc_graph_null_model", false, B, R, N, w, bin_swaps, period, neg_mode, seeds, w0, "w0", r, info, workspace,
               ws_bytes, stream);
}

}  // extern "C"

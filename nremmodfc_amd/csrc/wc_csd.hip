// wc_csd.hip -- cross-spectral density matrix and magnitude-squared coherence of the columns of a
// time-major x [T][C] on the device (gfx950, fp64): scipy.signal.csd / coherence with Welch's
// segmentation, any 2 <= nperseg <= 4096, P_xy = conj(X) Y averaged over the segments.
//
// Pass 1 (cs_spec_kernel) is wc_welch_psd.hip's segment transform -- the same segmentation, window,
// constant detrend, chirp, tables and in-LDS Stockham FFT (a private copy of the stages: that file
// is untouched) -- but it keeps the spectra.  A workgroup (512 threads) transforms one pair of
// segments (s, s + 1), s even, of G = 4096 / L neighbouring columns (one column at L = 8192) as
// A + i B in one complex Bluestein convolution.  The second FFT leaves z = L conj(convolution), so
//   Y[k] = DFT(A + i B)[k] = w[k] conj(z[k]) / L,      w[k] = exp(-i pi k^2 / n),
// and the two real segments' spectra are split out of it,
//   X_A[k] = (Y[k] + conj Y[n - k]) / 2,   X_B[k] = (Y[k] - conj Y[n - k]) / (2 i),
// the chirp factor applied to both terms before the split (w[n - k] is read from the table).  An
// odd last segment rides alone (B = 0).  The factors 1 / 2 and 1 / L are powers of two: exact.
//
// Workspace: W_8192 | chirp w [n] (padded to 16 entries) | chirp spectrum [L] | aux [F][C] complex |
// spectra [cs][F][C] complex (re, im), F = n / 2 + 1, cs an even number of segments ("chunk"): the
// columns of one bin of one segment are contiguous, which is what pass 2 reads (32 columns = 512
// bytes) and what a pass-1 workgroup writes G columns of at a time.  The minimum holds one pair of
// segments (a "segment block", 2 F C 16 bytes); the workspace only decides cs.
//
// Pass 2 (cs_gram_kernel): workgroup (bin f, 32 x 32 column-tile pair ti <= tj), 256 threads with a
// 2 x 2 block of complex accumulators each; 16 segments' two 32-column strips are staged through
// LDS (16 KB) at a time.  P[f][i][j] = sum_s conj(X_i) X_j is one chain of fp64 FMAs in segment
// order 0 .. nseg - 1; between chunks the running sum lives in out (the upper triangle; for the
// real-valued coherence output the imaginary part sits in the mirrored cell), a later chunk
// continues from it, and scale / nseg and the one-sided doubling are applied with the last chunk,
// which also writes the lower triangle as the exact conjugate and the diagonal's imaginary part
// as 0.  No atomics; the result is bit-identical for every workspace size and from run to run, and
// entry (i, j) depends on the samples of columns i and j only.
// Coherence: the diagonal is copied to aux, then |P_ij|^2 / (P_ii P_jj) elementwise in place (the
// scale cancels and is not applied).  Pair modes (column p with p + C / 2): cs_pair_kernel, a
// thread per (bin, pair) walks the chunk's segments; running sums (re, im, P_xx, P_yy) in aux.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <algorithm>
#include "wc_common.h"

namespace {

typedef double d2 __attribute__((ext_vector_type(2)));  // (re, im)

constexpr int kMaxN = 4096;       // nperseg: L = 8192 complex fp64 points are 128 KB of the CU's 160 KB
constexpr int kMinLogL = 6;       // L >= 64: at most 64 columns per workgroup
constexpr int kThreads = 512;
constexpr int kMinPts = 4096;     // points per workgroup (L = 8192: 8192)
constexpr int kTwG = 8192;        // global twiddle base: T[j] = exp(-2 pi i j / 8192)
constexpr int kTwL = 1024;        // LDS twiddle base (L <= 1024): every 8th entry of the above
constexpr int kTwLds = 768;       // radix 4 reads j = r k base / (4 P) < 3 base / 4
constexpr int kMaxMatC = 1024;    // matrix modes: at most 528 tile pairs per bin
constexpr int64_t kMaxC = 1 << 24;
constexpr int kMaxChunkPairs = 32768;  // pass 1: gridDim.y
constexpr int kTile = 32;         // pass 2: columns per strip (kTile / 16 = 2 x 2 accumulators per thread)
constexpr int kKS = 16;           // pass 2: segments staged in LDS at a time
constexpr int kGramThreads = 256;

__device__ __forceinline__ d2 cmul(d2 a, d2 w) {
    return d2{__builtin_fma(a.x, w.x, -a.y * w.y), __builtin_fma(a.x, w.y, a.y * w.x)};
}
__device__ __forceinline__ d2 cconj(d2 a) { return d2{a.x, -a.y}; }

// T[j] = exp(-2 pi i j / 8192), j < 8192
__global__ void cs_twiddle_kernel(d2* T) {
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= kTwG) return;
    double s, c;
    sincospi(2.0 * j / kTwG, &s, &c);
    T[j] = d2{c, -s};
}

// w[k] = exp(-i pi k^2 / n): k^2 mod 2 n in integers (k < 4096), then sincospi
__global__ void cs_chirp_kernel(int n, d2* w) {
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n) return;
    const int r = (k * k) % (2 * n);
    double s, c;
    sincospi((double)r / (double)n, &s, &c);
    w[k] = d2{c, -s};
}

// ---- forward FFT of the workgroup's G = PTS / N sub-FFTs of length N in LDS (item g at z + g (N + 1)):
// wc_welch_psd.hip's stages, operation for operation ----
template <int N, int PTS>
__device__ __forceinline__ void r2_stage(d2* z, int tid) {  // first stage, P = 1: no twiddles
    constexpr int S = N / 2, NP = N + 1, NB = PTS / 2 / kThreads;
    d2 u[NB][2];
#pragma unroll
    for (int j = 0; j < NB; ++j) {
        const int bf = tid + kThreads * j, g = bf / S, i = bf % S;
        u[j][0] = z[g * NP + i];
        u[j][1] = z[g * NP + i + S];
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < NB; ++j) {
        const int bf = tid + kThreads * j, g = bf / S, i = bf % S;
        z[g * NP + 2 * i] = u[j][0] + u[j][1];
        z[g * NP + 2 * i + 1] = u[j][0] - u[j][1];
    }
    __syncthreads();
}

// one radix-4 Stockham stage (P = product of the previous radices); T = W_TB
template <int N, int PTS, int TB, int P>
__device__ __forceinline__ void r4_stage(d2* z, const d2* T, int tid) {
    constexpr int S = N / 4, NP = N + 1, NB = PTS / 4 / kThreads;
    d2 u[NB][4];
#pragma unroll
    for (int j = 0; j < NB; ++j) {
        const int bf = tid + kThreads * j, g = bf / S, i = bf % S, k = i % P;
#pragma unroll
        for (int r = 0; r < 4; ++r) u[j][r] = z[g * NP + i + r * S];
        if constexpr (P > 1) {
#pragma unroll
            for (int r = 1; r < 4; ++r) u[j][r] = cmul(u[j][r], T[r * k * (TB / (4 * P))]);
        }
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < NB; ++j) {
        const int bf = tid + kThreads * j, g = bf / S, i = bf % S, k = i % P;
        const d2 a = u[j][0] + u[j][2], b = u[j][0] - u[j][2];
        const d2 c = u[j][1] + u[j][3], d = u[j][1] - u[j][3];
        d2* o = z + g * NP + (i - k) * 4 + k;
        o[0] = a + c;
        o[P] = d2{b.x + d.y, b.y - d.x};  // b - i d
        o[2 * P] = a - c;
        o[3 * P] = d2{b.x - d.y, b.y + d.x};  // b + i d
    }
    __syncthreads();
}

template <int N, int PTS, int TB, int P>
__device__ __forceinline__ void r4_stages(d2* z, const d2* T, int tid) {
    if constexpr (P < N) {
        r4_stage<N, PTS, TB, P>(z, T, tid);
        r4_stages<N, PTS, TB, P * 4>(z, T, tid);
    }
}

// every point of z written and a barrier passed before the call; ends with a barrier.  A real call,
// as in wc_welch_psd.hip (inlined twice, the stages' loads are scheduled across each other)
template <int LOGN, int PTS, int TB>
__device__ __noinline__ void fft_lds(d2* z, const d2* T, int tid) {
    constexpr int N = 1 << LOGN;
    if constexpr (LOGN & 1) {
        r2_stage<N, PTS>(z, tid);
        r4_stages<N, PTS, TB, 2>(z, T, tid);
    } else {
        r4_stages<N, PTS, TB, 1>(z, T, tid);
    }
}

struct CsArgs {
    int64_t C;          // columns of x
    int n, step;        // nperseg, nperseg - noverlap
    int nseg, s0;       // segments, first segment of the chunk (even)
    int detrend;
    const double* x;    // [T][C]
    const double* win;  // [n]
    const d2* T;        // W_8192
    const d2* w;        // chirp [n]
    d2* Bf;             // chirp spectrum [L]
    d2* spec;           // [cs][F][C]
};

template <int LOGN> struct CsShape {
    static constexpr int N = 1 << LOGN;
    static constexpr int PTS = N > kMinPts ? N : kMinPts;
    static constexpr int G = PTS / N, NP = N + 1, ES = kThreads / G, EPT = PTS / kThreads;
    static constexpr bool kLdsTw = N <= kTwL;
    static constexpr int TB = kLdsTw ? kTwL : kTwG;
    static constexpr size_t lds_bytes = ((size_t)G * NP + (kLdsTw ? kTwLds : 0)) * sizeof(d2);
};

// CHIRP: the chirp spectrum Bf = FFT_L(conj(w) at m mod L, |m| < n), one workgroup (item 0).
// Otherwise: workgroup (blockIdx.x = column group, blockIdx.y = segment pair of the chunk), item g = column.
template <int LOGN, bool CHIRP>
__global__ void __launch_bounds__(kThreads) cs_spec_kernel(const CsArgs a) {
    using S = CsShape<LOGN>;
    constexpr int N = S::N, G = S::G, NP = S::NP, ES = S::ES, EPT = S::EPT;
    extern __shared__ __attribute__((aligned(16))) d2 cs_smem[];
    d2* z = cs_smem;
    const int tid = threadIdx.x;
    const d2* T = a.T;
    if constexpr (S::kLdsTw) {
        d2* Tl = cs_smem + G * NP;
        for (int j = tid; j < kTwLds; j += kThreads) Tl[j] = a.T[j * (kTwG / kTwL)];
        T = Tl;
    }
    const int g = tid % G, e0 = tid / G;
    d2* zg = z + g * NP;
    const int n = a.n;

    if constexpr (CHIRP) {
#pragma unroll
        for (int j = 0; j < EPT; ++j) {
            const int e = e0 + ES * j;
            const int m = e < n ? e : (e > N - n ? N - e : -1);
            zg[e] = (g == 0 && m >= 0) ? cconj(a.w[m]) : d2{0.0, 0.0};
        }
        __syncthreads();
        fft_lds<LOGN, S::PTS, S::TB>(z, T, tid);
        if (g == 0) {
#pragma unroll
            for (int j = 0; j < EPT; ++j) a.Bf[e0 + ES * j] = zg[e0 + ES * j];
        }
        return;
    } else {
        const int64_t c = (int64_t)blockIdx.x * G + g;
        const bool live = c < a.C;
        d2* red = z;  // [kThreads], before the segments are written
        const int half = n / 2;
        // segments s and s + 1 (or s and nothing) ride one complex transform as A + i B
        const int s = a.s0 + 2 * (int)blockIdx.y;
        const bool two = s + 1 < a.nseg;
        const double* xc = a.x + c;
        const int64_t t0 = (int64_t)s * a.step;
        d2 xr[EPT];
#pragma unroll
        for (int j = 0; j < EPT; ++j) {
            const int e = e0 + ES * j;
            const bool in = live && e < n;
            xr[j] = d2{in ? xc[(t0 + e) * a.C] : 0.0, (in && two) ? xc[(t0 + a.step + e) * a.C] : 0.0};
        }
        d2 mean = d2{0.0, 0.0};
        if (a.detrend) {
            d2 p = d2{0.0, 0.0};
#pragma unroll
            for (int j = 0; j < EPT; ++j) p += xr[j];
            red[tid] = p;
            __syncthreads();
            for (int h = ES / 2; h >= 1; h >>= 1) {
                if (e0 < h) red[tid] += red[tid + h * G];
                __syncthreads();
            }
            mean = red[g] / (double)n;
            __syncthreads();
        }
#pragma unroll
        for (int j = 0; j < EPT; ++j) {
            const int e = e0 + ES * j;
            zg[e] = e < n ? cmul((xr[j] - mean) * a.win[e], a.w[e]) : d2{0.0, 0.0};
        }
        __syncthreads();
        fft_lds<LOGN, S::PTS, S::TB>(z, T, tid);
#pragma unroll
        for (int j = 0; j < EPT; ++j) {
            const int e = e0 + ES * j;
            zg[e] = cconj(cmul(zg[e], a.Bf[e]));
        }
        __syncthreads();
        fft_lds<LOGN, S::PTS, S::TB>(z, T, tid);  // z = L conj(convolution): L Y[k] = w[k] conj(z[k])
        if (!live) return;
        const int F = half + 1;
        const double sc = 0.5 / (double)N;
        d2* o = a.spec + (int64_t)(2 * blockIdx.y) * F * a.C + c;
#pragma unroll
        for (int j = 0; j < EPT; ++j) {
            const int e = e0 + ES * j;
            if (e <= half) {
                const int r = e ? n - e : 0;
                const d2 yk = cmul(cconj(zg[e]), a.w[e]);         // L Y[k]
                const d2 yr = cconj(cmul(cconj(zg[r]), a.w[r]));  // L conj Y[n - k]
                const d2 sum = yk + yr, dif = yk - yr;
                o[(int64_t)e * a.C] = sum * sc;
                if (two) o[((int64_t)F + e) * a.C] = d2{dif.y, -dif.x} * sc;  // / i
            }
        }
    }
}

__device__ __forceinline__ void cs_mac(d2& acc, d2 a, d2 b) {  // acc += conj(a) b
    acc.x = __builtin_fma(a.x, b.x, __builtin_fma(a.y, b.y, acc.x));
    acc.y = __builtin_fma(a.x, b.y, __builtin_fma(-a.y, b.x, acc.y));
}

__device__ __forceinline__ double cs_mult(int n, int f, double mult) {
    const bool twice = f > 0 && !(n % 2 == 0 && f == n / 2);
    return twice ? 2.0 * mult : mult;
}

// workgroup (blockIdx.x = tile pair ti <= tj, blockIdx.y = bin): the chunk's cs segments are added, in
// order, to the running sums of the tile's upper-triangle entries.
// coh == 0: out [F][C][C] (re, im).  coh == 1: out [F][C][C] real, re at (i, j), im at (j, i), i < j
__global__ void __launch_bounds__(kGramThreads) cs_gram_kernel(int C, int F, int n, int cs, int first, int last, int coh,
                                                               double mult, const d2* __restrict__ spec, double* out) {
    __shared__ d2 Xi[kKS][kTile], Xj[kKS][kTile];
    const int tid = threadIdx.x, f = blockIdx.y;
    const int nt = (C + kTile - 1) / kTile;
    int ti = 0, rem = blockIdx.x;
    while (rem >= nt - ti) {
        rem -= nt - ti;
        ++ti;
    }
    const int tj = ti + rem;
    constexpr int R = kTile / 16;
    const int i0 = ti * kTile + (tid / 16) * R, j0 = tj * kTile + (tid % 16) * R;
    double* of = out + (int64_t)f * C * C * (coh ? 1 : 2);

    d2 acc[R][R];
#pragma unroll
    for (int p = 0; p < R; ++p)
#pragma unroll
        for (int q = 0; q < R; ++q) {
            const int i = i0 + p, j = j0 + q;
            acc[p][q] = d2{0.0, 0.0};
            if (!first && i <= j && j < C) {
                if (coh) {
                    acc[p][q].x = of[(int64_t)i * C + j];
                    if (i != j) acc[p][q].y = of[(int64_t)j * C + i];
                } else {
                    acc[p][q] = d2{of[2 * ((int64_t)i * C + j)], of[2 * ((int64_t)i * C + j) + 1]};
                }
            }
        }

    const int li = (tid / 16) * R, lj = (tid % 16) * R;
    for (int k0 = 0; k0 < cs; k0 += kKS) {
        const int kmax = min(kKS, cs - k0);
        for (int q = tid; q < kKS * kTile; q += kGramThreads) {
            const int ks = q / kTile, cc = q % kTile;
            const int ci = ti * kTile + cc, cj = tj * kTile + cc;
            const d2* row = spec + ((int64_t)(k0 + ks) * F + f) * C;
            Xi[ks][cc] = (ks < kmax && ci < C) ? row[ci] : d2{0.0, 0.0};
            Xj[ks][cc] = (ks < kmax && cj < C) ? row[cj] : d2{0.0, 0.0};
        }
        __syncthreads();
        for (int ks = 0; ks < kmax; ++ks) {
            d2 a[R], b[R];
#pragma unroll
            for (int p = 0; p < R; ++p) {
                a[p] = Xi[ks][li + p];
                b[p] = Xj[ks][lj + p];
            }
#pragma unroll
            for (int p = 0; p < R; ++p)
#pragma unroll
                for (int q = 0; q < R; ++q) cs_mac(acc[p][q], a[p], b[q]);
        }
        __syncthreads();
    }

    const double m = (last && !coh) ? cs_mult(n, f, mult) : 1.0;
#pragma unroll
    for (int p = 0; p < R; ++p)
#pragma unroll
        for (int q = 0; q < R; ++q) {
            const int i = i0 + p, j = j0 + q;
            if (i > j || j >= C) continue;
            d2 v = acc[p][q];
            if (i == j) v.y = 0.0;
            if (coh) {
                of[(int64_t)i * C + j] = v.x;
                if (i != j) of[(int64_t)j * C + i] = v.y;
            } else {
                if (last) v = v * m;
                of[2 * ((int64_t)i * C + j)] = v.x;
                of[2 * ((int64_t)i * C + j) + 1] = v.y;
                if (last && i != j) {
                    of[2 * ((int64_t)j * C + i)] = v.x;
                    of[2 * ((int64_t)j * C + i) + 1] = -v.y;
                }
            }
        }
}

// coherence epilogue: the diagonal (the columns' power) is set aside, then every cell in place
__global__ void cs_diag_kernel(int C, int F, const double* out, double* diag) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (int64_t)F * C) return;
    const int64_t f = i / C, c = i % C;
    diag[i] = out[(f * C + c) * C + c];
}

__global__ void cs_coherence_kernel(int C, int F, const double* diag, double* out) {
    const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (int64_t)F * C * C) return;
    const int64_t f = idx / ((int64_t)C * C);
    const int i = (int)((idx / C) % C), j = (int)(idx % C);
    if (i > j) return;
    double* of = out + f * C * C;
    const double pii = diag[f * C + i], pjj = diag[f * C + j];
    if (i == j) {
        of[(int64_t)i * C + i] = (pii * pii) / (pii * pii);
        return;
    }
    const double re = of[(int64_t)i * C + j], im = of[(int64_t)j * C + i];
    const double v = __builtin_fma(re, re, im * im) / (pii * pjj);
    of[(int64_t)i * C + j] = v;
    of[(int64_t)j * C + i] = v;
}

// pair modes: thread (bin f, pair p) adds the chunk's segments to run [F][H][4] = (re, im, P_xx, P_yy)
__global__ void cs_pair_kernel(int64_t C, int F, int n, int cs, int first, int last, int coh, double mult,
                               const d2* __restrict__ spec, double* run, double* out) {
    const int64_t H = C / 2, idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= F * H) return;
    const int f = (int)(idx / H);
    const int64_t p = idx % H;
    d2 acc = d2{0.0, 0.0};
    double pxx = 0.0, pyy = 0.0;
    if (!first) {
        acc = d2{run[4 * idx], run[4 * idx + 1]};
        pxx = run[4 * idx + 2];
        pyy = run[4 * idx + 3];
    }
    for (int s = 0; s < cs; ++s) {
        const d2* row = spec + ((int64_t)s * F + f) * C;
        const d2 a = row[p], b = row[p + H];
        cs_mac(acc, a, b);
        pxx = __builtin_fma(a.x, a.x, __builtin_fma(a.y, a.y, pxx));
        pyy = __builtin_fma(b.x, b.x, __builtin_fma(b.y, b.y, pyy));
    }
    if (!last) {
        run[4 * idx] = acc.x;
        run[4 * idx + 1] = acc.y;
        run[4 * idx + 2] = pxx;
        run[4 * idx + 3] = pyy;
    } else if (coh) {
        out[idx] = __builtin_fma(acc.x, acc.x, acc.y * acc.y) / (pxx * pyy);
    } else {
        const double m = cs_mult(n, f, mult);
        out[2 * idx] = acc.x * m;
        out[2 * idx + 1] = acc.y * m;
    }
}

template <int LOGN, bool CHIRP>
hipError_t cs_launch(const CsArgs& a, dim3 grid, hipStream_t st) {
    auto kern = cs_spec_kernel<LOGN, CHIRP>;
    constexpr size_t lds = CsShape<LOGN>::lds_bytes;
    hipError_t e = hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(kern, grid, dim3(kThreads), lds, st, a);
    return hipSuccess;
}

template <bool CHIRP>
hipError_t cs_dispatch(int logL, const CsArgs& a, int pairs, hipStream_t st) {
    const int G = std::max(1, kMinPts >> logL);
    const dim3 grid = CHIRP ? dim3(1) : dim3((unsigned)((a.C + G - 1) / G), (unsigned)pairs);
    switch (logL) {
        case 6: return cs_launch<6, CHIRP>(a, grid, st);
        case 7: return cs_launch<7, CHIRP>(a, grid, st);
        case 8: return cs_launch<8, CHIRP>(a, grid, st);
        case 9: return cs_launch<9, CHIRP>(a, grid, st);
        case 10: return cs_launch<10, CHIRP>(a, grid, st);
        case 11: return cs_launch<11, CHIRP>(a, grid, st);
        case 12: return cs_launch<12, CHIRP>(a, grid, st);
        default: return cs_launch<13, CHIRP>(a, grid, st);
    }
}

struct CsPlan {
    int logL, nseg, F;
    size_t tab, aux, blk;  // bytes of the tables, of aux [F][C] complex, of one segment pair's spectra
};

CsPlan cs_plan(int64_t C, int64_t T, int n, int noverlap) {
    CsPlan p;
    p.logL = kMinLogL;
    while ((1 << p.logL) < 2 * n - 1) ++p.logL;
    p.nseg = (int)((T - n) / (n - noverlap) + 1);
    p.F = n / 2 + 1;
    p.tab = ((size_t)kTwG + (size_t)((n + 15) / 16 * 16) + ((size_t)1 << p.logL)) * sizeof(d2);
    p.aux = (size_t)p.F * (size_t)C * sizeof(d2);
    p.blk = 2 * p.aux;
    return p;
}

bool cs_shape_ok(int64_t C, int64_t T, int n, int noverlap) {
    return C > 0 && C <= kMaxC && n >= 2 && n <= kMaxN && noverlap >= 0 && noverlap < n && T >= n &&
           (T - n) / (n - noverlap) < INT32_MAX;
}

}  // namespace

size_t wc_csd_workspace_size(int64_t C, int64_t T, int nperseg, int noverlap) {
    if (!cs_shape_ok(C, T, nperseg, noverlap)) return 0;
    const CsPlan p = cs_plan(C, T, nperseg, noverlap);
    return p.tab + p.aux + p.blk;
}

int wc_csd(int64_t C, int64_t T, const double* x, int nperseg, int noverlap, const double* window, int detrend,
           double scale, int mode, double* out, void* workspace, size_t ws_bytes, void* stream) {
    wc_clear_err();
    char msg[200];
    const int n = nperseg;
    if (C <= 0) return wc_set_err(WC_EINVAL, "wc_csd: C <= 0");
    if (C > kMaxC) return wc_set_err(WC_EINVAL, "wc_csd: C > 2^24");
    if (n < 2) return wc_set_err(WC_EINVAL, "wc_csd: nperseg < 2");
    if (noverlap < 0 || noverlap >= n) return wc_set_err(WC_EINVAL, "wc_csd: noverlap outside 0 .. nperseg - 1");
    if (T < n) return wc_set_err(WC_EINVAL, "wc_csd: T < nperseg");
    if (!x || !window || !out) return wc_set_err(WC_EINVAL, "wc_csd: x, window or out is NULL");
    if (detrend != 0 && detrend != 1) return wc_set_err(WC_EINVAL, "wc_csd: detrend must be 0 (none) or 1 (constant)");
    if (!(scale > 0.0) || !isfinite(scale)) return wc_set_err(WC_EINVAL, "wc_csd: scale must be finite and positive");
    if (mode < WC_CSD_MATRIX || mode > WC_CSD_PAIR_COHERENCE)
        return wc_set_err(WC_EINVAL, "wc_csd: unknown mode (WC_CSD_MATRIX .. WC_CSD_PAIR_COHERENCE)");
    const bool pairs = mode == WC_CSD_PAIRS || mode == WC_CSD_PAIR_COHERENCE;
    const bool coh = mode == WC_CSD_COHERENCE || mode == WC_CSD_PAIR_COHERENCE;
    if (pairs && (C & 1)) return wc_set_err(WC_EINVAL, "wc_csd: a pair mode needs an even C (column i with i + C / 2)");
    if ((T - n) / (n - noverlap) >= INT32_MAX) return wc_set_err(WC_EINVAL, "wc_csd: 2^31 segments or more");
    if (n > kMaxN) {
        snprintf(msg, sizeof msg, "wc_csd: nperseg = %d > 4096 (the Bluestein FFT of 8192 points fills the LDS)", n);
        return wc_set_err(WC_EUNSUPPORTED, msg);
    }
    if (!pairs && C > kMaxMatC) {
        snprintf(msg, sizeof msg, "wc_csd: C = %lld > 1024 columns in a matrix mode", (long long)C);
        return wc_set_err(WC_EUNSUPPORTED, msg);
    }
    const int F = n / 2 + 1;
    {
        const size_t cells = pairs ? (size_t)F * (size_t)(C / 2) : (size_t)F * (size_t)C * (size_t)C;
        const uintptr_t x0 = (uintptr_t)x, x1 = x0 + (size_t)T * C * 8, p0 = (uintptr_t)out,
                        p1 = p0 + cells * (coh ? 8 : 16);
        if (p0 < x1 && x0 < p1) return wc_set_err(WC_EINVAL, "wc_csd: out must not alias x");
        if ((x0 & 7) || (p0 & 7) || ((uintptr_t)window & 7))
            return wc_set_err(WC_EINVAL, "wc_csd: x, window and out must be 8-byte aligned");
    }
    const CsPlan p = cs_plan(C, T, n, noverlap);
    const size_t need = p.tab + p.aux + p.blk;
    if (!workspace || ws_bytes < need) {
        snprintf(msg, sizeof msg, "wc_csd: workspace < %zu bytes (wc_csd_workspace_size)", need);
        return wc_set_err(WC_EWORKSPACE, msg);
    }
    if ((uintptr_t)workspace & 15) return wc_set_err(WC_EINVAL, "wc_csd: workspace must be 16-byte aligned");

    hipStream_t st = static_cast<hipStream_t>(stream);
    d2* Tw = static_cast<d2*>(workspace);
    d2* w = Tw + kTwG;
    d2* Bf = w + (n + 15) / 16 * 16;
    double* aux = reinterpret_cast<double*>(Bf + ((size_t)1 << p.logL));
    d2* spec = reinterpret_cast<d2*>(aux) + (size_t)F * (size_t)C;
    // segment pairs per chunk: what the workspace holds
    const int64_t all_pairs = ((int64_t)p.nseg + 1) / 2;
    const int cpairs = (int)std::min<int64_t>(std::min<int64_t>((int64_t)((ws_bytes - p.tab - p.aux) / p.blk), all_pairs),
                                              kMaxChunkPairs);

    hipLaunchKernelGGL(cs_twiddle_kernel, dim3(kTwG / 256), dim3(256), 0, st, Tw);
    hipLaunchKernelGGL(cs_chirp_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, n, w);
    CsArgs a{C, n, n - noverlap, p.nseg, 0, detrend, x, window, Tw, w, Bf, spec};
    hipError_t e = cs_dispatch<true>(p.logL, a, 1, st);
    const double mult = scale / (double)p.nseg;
    const int nt = (int)((C + kTile - 1) / kTile);
    for (int64_t s0 = 0; s0 < p.nseg && e == hipSuccess; s0 += 2 * (int64_t)cpairs) {
        const int cs = (int)std::min<int64_t>(2 * (int64_t)cpairs, p.nseg - s0);
        const int first = s0 == 0, last = s0 + cs >= p.nseg;
        a.s0 = (int)s0;
        e = cs_dispatch<false>(p.logL, a, (cs + 1) / 2, st);
        if (e != hipSuccess) break;
        if (pairs) {
            const int64_t tot = (int64_t)F * (C / 2);
            hipLaunchKernelGGL(cs_pair_kernel, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, st, C, F, n, cs, first,
                               last, (int)coh, mult, spec, aux, out);
        } else {
            hipLaunchKernelGGL(cs_gram_kernel, dim3((unsigned)(nt * (nt + 1) / 2), (unsigned)F), dim3(kGramThreads), 0, st,
                               (int)C, F, n, cs, first, last, (int)coh, mult, spec, out);
        }
    }
    if (e == hipSuccess && mode == WC_CSD_COHERENCE) {
        const int64_t nd = (int64_t)F * C, tot = nd * C;
        hipLaunchKernelGGL(cs_diag_kernel, dim3((unsigned)((nd + 255) / 256)), dim3(256), 0, st, (int)C, F, out, aux);
        hipLaunchKernelGGL(cs_coherence_kernel, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, st, (int)C, F, aux,
                           out);
    }
    if (e != hipSuccess) {
        snprintf(wc_errbuf(), 512, "wc_csd: %s", hipGetErrorString(e));
        return WC_EHIP;
    }
    return wc_hip_check("wc_csd");
}

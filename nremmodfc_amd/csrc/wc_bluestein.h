// wc_bluestein.h -- the in-LDS Stockham FFT and the Bluestein segment transform shared by the spectral
// kernels: wc_hilbert.hip uses the FFT stages and the twiddle and chirp table kernels (it defines
// WC_BLUESTEIN_FFT_ONLY, which leaves out the rest); wc_welch_psd.hip, wc_csd.hip and
// wc_spectrogram.hip (the Welch family) also the constants, tables, shape, segment-pair transform,
// dispatch and argument checks below.  Header only; everything has internal linkage.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <algorithm>
#include <type_traits>
#include "wc_common.h"

namespace {

typedef double d2 __attribute__((ext_vector_type(2)));  // (re, im)

constexpr int kThreads = 512;
constexpr int kTwLds = 768;       // LDS twiddles: radix 4 reads j = r k base / (4 P) < 3 base / 4 of W_1024

__device__ __forceinline__ d2 cmul(d2 a, d2 w) {
    return d2{__builtin_fma(a.x, w.x, -a.y * w.y), __builtin_fma(a.x, w.y, a.y * w.x)};
}
__device__ __forceinline__ d2 cconj(d2 a) { return d2{a.x, -a.y}; }

// T[j] = exp(-2 pi i j / LEN), j < LEN
template <int LEN>
__global__ void bs_twiddle_kernel(d2* T) {
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= LEN) return;
    double s, c;
    sincospi(2.0 * j / LEN, &s, &c);
    T[j] = d2{c, -s};
}

// w[k] = exp(-i pi k^2 / n): k^2 mod 2 n in integers of type I (int: k < 4096; int64_t: k < 2^19), then sincospi
template <class I>
__global__ void bs_chirp_kernel(I n, d2* w) {
    const I k = (I)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n) return;
    const I r = (k * k) % (2 * n);
    double s, c;
    sincospi((double)r / (double)n, &s, &c);
    w[k] = d2{c, -s};
}

// ---- forward FFT of the workgroup's G = PTS / N sub-FFTs of length N in LDS (item g at z + g (N + 1)) ----
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

// every point of z written and a barrier passed before the call; ends with a barrier
template <int LOGN, int PTS, int TB>
__device__ __forceinline__ void fft_lds(d2* z, const d2* T, int tid) {
    constexpr int N = 1 << LOGN;
    if constexpr (LOGN & 1) {
        r2_stage<N, PTS>(z, tid);
        r4_stages<N, PTS, TB, 2>(z, T, tid);
    } else {
        r4_stages<N, PTS, TB, 1>(z, T, tid);
    }
}

// The Welch family's form, a real call: inlined twice into wp_kernel's segment loop, the stages'
// loads are scheduled across each other and the kernel needs 150 .. 230 VGPRs (one workgroup per CU)
// and spills at L = 8192; called, 116 .. 132 and 248
template <int LOGN, int PTS, int TB>
__device__ __noinline__ void fft_lds_call(d2* z, const d2* T, int tid) {
    fft_lds<LOGN, PTS, TB>(z, T, tid);
}

#ifndef WC_BLUESTEIN_FFT_ONLY  // wc_hilbert.hip: its own four-step transform around the stages above
// ---- the Welch family: a workgroup holds G = PTS / N columns' points of one Bluestein convolution ----
constexpr int kMaxN = 4096;       // nperseg: L = 8192 complex fp64 points are 128 KB of the CU's 160 KB
constexpr int kMinLogL = 6;       // L >= 64: at most 64 columns per workgroup
constexpr int kMinPts = 4096;     // points per workgroup (L = 8192: 8192)
constexpr int kTwG = 8192;        // global twiddle base: T[j] = exp(-2 pi i j / 8192)
constexpr int kTwL = 1024;        // LDS twiddle base (L <= 1024): every 8th entry of the above

template <int LOGN> struct BsShape {
    static constexpr int N = 1 << LOGN;
    static constexpr int PTS = N > kMinPts ? N : kMinPts;
    static constexpr int G = PTS / N, NP = N + 1, ES = kThreads / G, EPT = PTS / kThreads;
    static constexpr bool kLdsTw = N <= kTwL;
    static constexpr int TB = kLdsTw ? kTwL : kTwG;
    static constexpr size_t lds_bytes = ((size_t)G * NP + (kLdsTw ? kTwLds : 0)) * sizeof(d2);
};

// The workgroup's dynamic LDS, BsShape<LOGN>::lds_bytes of it.  One array for every kernel of a translation
// unit, the chirp spectrum's included: fft_lds_call then gets the same z from all its callers, and the compiler
// addresses LDS in it directly (two arrays would make z a generic pointer, checked at every access)
__device__ __forceinline__ d2* bs_lds() {
    extern __shared__ __attribute__((aligned(16))) d2 bs_smem[];
    return bs_smem;
}

// the FFT's twiddles: the 768-entry W_1024 behind the points in LDS for L <= 1024, Tg = W_8192 above
template <int LOGN>
__device__ __forceinline__ const d2* bs_twiddles(d2* smem, const d2* Tg, int tid) {
    using S = BsShape<LOGN>;
    if constexpr (S::kLdsTw) {
        d2* Tl = smem + S::G * S::NP;
        for (int j = tid; j < kTwLds; j += kThreads) Tl[j] = Tg[j * (kTwG / kTwL)];
        return Tl;
    }
    return Tg;
}

// the chirp spectrum Bf = FFT_L(conj(w) at m mod L, |m| < n), one workgroup (item 0)
template <int LOGN>
__global__ void __launch_bounds__(kThreads) bs_chirp_spectrum_kernel(int n, const d2* Tg, const d2* w, d2* Bf) {
    using S = BsShape<LOGN>;
    constexpr int N = S::N, G = S::G, NP = S::NP, ES = S::ES, EPT = S::EPT;
    d2* z = bs_lds();
    const int tid = threadIdx.x;
    const d2* T = bs_twiddles<LOGN>(z, Tg, tid);
    const int g = tid % G, e0 = tid / G;
    d2* zg = z + g * NP;
#pragma unroll
    for (int j = 0; j < EPT; ++j) {
        const int e = e0 + ES * j;
        const int m = e < n ? e : (e > N - n ? N - e : -1);
        zg[e] = (g == 0 && m >= 0) ? cconj(w[m]) : d2{0.0, 0.0};
    }
    __syncthreads();
    fft_lds_call<LOGN, S::PTS, S::TB>(z, T, tid);
    if (g == 0) {
#pragma unroll
        for (int j = 0; j < EPT; ++j) Bf[e0 + ES * j] = zg[e0 + ES * j];
    }
}

// Segments s and s + 1 (two; or s alone, B = 0) of column xc, starting at sample t0, ride one complex
// Bluestein transform as A + i B: read, constant detrend (a fixed tree: each thread adds its own
// samples in order, then the threads of a column halve log2(512 / G) times through LDS), window times
// chirp, FFT, times the chirp spectrum, conjugate, FFT.  Leaves z = L conj(convolution), so
// L Y[k] = w[k] conj(z[k]), Y = DFT(A + i B), and ends with a barrier.  lt is the thread index (item
// lt % G, points lt / G + ES j); z may be overwritten once every thread has read its bins.
// a: the kernel's arguments, with C, n, step, detrend, win, w, Bf.
template <int LOGN, class Args>
__device__ __forceinline__ void bs_segment_pair(const Args& a, d2* z, const d2* T, int lt, const double* xc, int64_t t0,
                                                bool live, bool two) {
    using S = BsShape<LOGN>;
    constexpr int G = S::G, NP = S::NP, ES = S::ES, EPT = S::EPT;
    const int g = lt % G, e0 = lt / G, n = a.n;
    d2* zg = z + g * NP;
    d2* red = z;  // [kThreads], before the segments are written
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
        red[lt] = p;
        __syncthreads();
        for (int h = ES / 2; h >= 1; h >>= 1) {
            if (e0 < h) red[lt] += red[lt + h * G];
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
    fft_lds_call<LOGN, S::PTS, S::TB>(z, T, lt);
#pragma unroll
    for (int j = 0; j < EPT; ++j) {
        const int e = e0 + ES * j;
        zg[e] = cconj(cmul(zg[e], a.Bf[e]));
    }
    __syncthreads();
    fft_lds_call<LOGN, S::PTS, S::TB>(z, T, lt);
}

// the two real segments' spectra at bin e <= n / 2 out of zg = L conj(convolution), times sc:
//   X_A[k] = (Y[k] + conj Y[n - k]) / 2,   X_B[k] = (Y[k] - conj Y[n - k]) / (2 i),
// the chirp factor applied to both terms before the split (w[n - k] is read from the table)
__device__ __forceinline__ void bs_split(const d2* zg, const d2* w, int n, int e, double sc, d2& XA, d2& XB) {
    const int r = e ? n - e : 0;
    const d2 yk = cmul(cconj(zg[e]), w[e]);         // L Y[k]
    const d2 yr = cconj(cmul(cconj(zg[r]), w[r]));  // L conj Y[n - k]
    const d2 sum = yk + yr, dif = yk - yr;
    XA = sum * sc;
    XB = d2{dif.y, -dif.x} * sc;  // / i
}

// f(std::integral_constant<int, LOGN>) for LOGN = logL, 6 .. 13
template <class F>
int bs_dispatch(int logL, F&& f) {
    switch (logL) {
        case 6: return f(std::integral_constant<int, 6>{});
        case 7: return f(std::integral_constant<int, 7>{});
        case 8: return f(std::integral_constant<int, 8>{});
        case 9: return f(std::integral_constant<int, 9>{});
        case 10: return f(std::integral_constant<int, 10>{});
        case 11: return f(std::integral_constant<int, 11>{});
        case 12: return f(std::integral_constant<int, 12>{});
        default: return f(std::integral_constant<int, 13>{});
    }
}

// a kernel of BsShape<LOGN>: its dynamic LDS allowed, then launched; who names the entry point
template <int LOGN, class... P, class... A>
int bs_launch(const char* who, void (*kern)(P...), dim3 grid, hipStream_t st, const A&... args) {
    constexpr size_t lds = BsShape<LOGN>::lds_bytes;
    if (int rc = wc_raise_lds(who, kern, lds)) return rc;
    hipLaunchKernelGGL(kern, grid, dim3(kThreads), lds, st, args...);
    return WC_OK;
}

// workgroups (x = groups of G columns, y) of a transform kernel
inline dim3 bs_grid(int logL, int64_t cols, int ny) {
    const int G = std::max(1, kMinPts >> logL);
    return dim3((unsigned)((cols + G - 1) / G), (unsigned)ny);
}

// the head of every Welch-family workspace: W_8192 | chirp w [n] (padded to 16 entries) | chirp spectrum [L],
// L = max(64, nextpow2(2 n - 1)); T, w and Bf point into ws (sizes only: ws = nullptr)
struct BsTables {
    int logL;
    size_t bytes;
    d2 *T, *w, *Bf;
};

inline BsTables bs_layout(int n, void* ws) {
    BsTables t;
    t.logL = kMinLogL;
    while ((1 << t.logL) < 2 * n - 1) ++t.logL;
    const size_t nw = (size_t)((n + 15) / 16 * 16), L = (size_t)1 << t.logL;
    t.bytes = ((size_t)kTwG + nw + L) * sizeof(d2);
    t.T = static_cast<d2*>(ws);
    t.w = ws ? t.T + kTwG : nullptr;
    t.Bf = ws ? t.w + nw : nullptr;
    return t;
}

inline int bs_fill_tables(const char* who, const BsTables& t, int n, hipStream_t st) {
    hipLaunchKernelGGL(bs_twiddle_kernel<kTwG>, dim3(kTwG / 256), dim3(256), 0, st, t.T);
    hipLaunchKernelGGL(bs_chirp_kernel<int>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, n, t.w);
    return bs_dispatch(t.logL, [&](auto I) {
        constexpr int LOGN = decltype(I)::value;
        return bs_launch<LOGN>(who, bs_chirp_spectrum_kernel<LOGN>, dim3(1), st, n, (const d2*)t.T, (const d2*)t.w, t.Bf);
    });
}

// T - n < 2^31 steps of at least one sample: nseg fits an int
inline bool bs_shape_ok(int64_t C, int64_t T, int n, int noverlap) {
    return C > 0 && n >= 2 && n <= kMaxN && noverlap >= 0 && noverlap < n && T >= n && (T - n) / (n - noverlap) < INT32_MAX;
}

// the arguments every Welch-family entry point takes; who names it and oname its output in the message
inline int bs_check_args(const char* who, const char* oname, int64_t C, int64_t T, const double* x, int n, int noverlap,
                         const double* window, int detrend, double scale, const double* out, const void* workspace) {
    if (C <= 0) return wc_fail(WC_EINVAL, "%s: C <= 0", who);
    if (n < 2) return wc_fail(WC_EINVAL, "%s: nperseg < 2", who);
    if (noverlap < 0 || noverlap >= n) return wc_fail(WC_EINVAL, "%s: noverlap outside 0 .. nperseg - 1", who);
    if (T < n) return wc_fail(WC_EINVAL, "%s: T < nperseg", who);
    if (!x || !window || !out) return wc_fail(WC_EINVAL, "%s: x, window or %s is NULL", who, oname);
    if (detrend != 0 && detrend != 1) return wc_fail(WC_EINVAL, "%s: detrend must be 0 (none) or 1 (constant)", who);
    if (!(scale > 0.0) || !isfinite(scale)) return wc_fail(WC_EINVAL, "%s: scale must be finite and positive", who);
    if ((T - n) / (n - noverlap) >= INT32_MAX) return wc_fail(WC_EINVAL, "%s: 2^31 segments or more", who);
    if (n > kMaxN)
        return wc_fail(WC_EUNSUPPORTED, "%s: nperseg = %d > 4096 (the Bluestein FFT of 8192 points fills the LDS)", who, n);
    const WcSpan all[4] = {{"x", x, 0, 8}, {oname, out, 0, 8}, {"window", window, 0, 8}, {"workspace", workspace, 0, 16}};
    return wc_check_align(who, all, 4);
}
#endif  // WC_BLUESTEIN_FFT_ONLY

}  // namespace

// wc_spectrogram.hip -- scipy.signal.spectrogram of every column of a time-major x [T][C] on the
// device (gfx950, fp64): the one-sided spectrum of every Welch segment, nothing averaged, any
// 2 <= nperseg <= 4096, as a PSD, complex, magnitude or angle.
//
// The transform (sp_kernel) is wc_csd.hip's cs_spec_kernel -- the same segmentation, window, constant
// detrend, chirp, tables and in-LDS Stockham FFT (a private copy of the stages: that file and
// wc_welch_psd.hip are untouched).  A workgroup (512 threads) transforms one pair of segments
// (s, s + 1), s even, of G = 4096 / L neighbouring columns (one column at L = 8192) as A + i B in one
// complex Bluestein convolution.  The second FFT leaves z = L conj(convolution), so
//   Y[k] = DFT(A + i B)[k] = w[k] conj(z[k]) / L,      w[k] = exp(-i pi k^2 / n),
// and the two real segments' spectra are split out of it,
//   X_A[k] = (Y[k] + conj Y[n - k]) / 2,   X_B[k] = (Y[k] - conj Y[n - k]) / (2 i),
// the chirp factor applied to both terms before the split (w[n - k] is read from the table).  An
// odd last segment rides alone (B = 0).  The factors 1 / 2 and 1 / L are powers of two: exact.
//
// Where cs_spec_kernel parks the spectra in a workspace, the epilogue here writes the mode's value
// straight into out, segment-major [S][F][C] (F = n / 2 + 1): the G columns of a bin that a workgroup
// holds are contiguous.  The mode is a template parameter (the PSD carries no atan2):
//   WC_SPEC_PSD        (re^2 + im^2) scale, 2 scale at every bin but 0 and (even n) n / 2
//   WC_SPEC_COMPLEX    X sqrt(scale), interleaved (re, im); at bins 0 and (even n) n / 2 the two
//                      terms of the split are exact conjugates and the imaginary part is exactly 0
//   WC_SPEC_MAGNITUDE  sqrt(re^2 + im^2) sqrt(scale)
//   WC_SPEC_ANGLE      atan2(im, re) in [-pi, pi]; an exactly zero X gives 0
// sqrt(scale) comes from the host.  No atomics and no accumulation: a cell depends only on its
// column's samples in its segment pair, so a column's slab is bit-identical for every C and from
// run to run.  Segment pairs beyond one launch's gridDim.y (32,768, as wc_csd) go in further
// launches through s0.
//
// Workspace: W_8192 | chirp w [n] (padded to 16 entries) | chirp spectrum [L]: the tables only.
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
constexpr int64_t kMaxC = 1 << 24;
constexpr int kMaxPairs = 32768;  // segment pairs per launch: gridDim.y
constexpr int kChirp = -1;        // sp_kernel's MODE for the chirp spectrum

__device__ __forceinline__ d2 cmul(d2 a, d2 w) {
    return d2{__builtin_fma(a.x, w.x, -a.y * w.y), __builtin_fma(a.x, w.y, a.y * w.x)};
}
__device__ __forceinline__ d2 cconj(d2 a) { return d2{a.x, -a.y}; }

// T[j] = exp(-2 pi i j / 8192), j < 8192
__global__ void sp_twiddle_kernel(d2* T) {
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= kTwG) return;
    double s, c;
    sincospi(2.0 * j / kTwG, &s, &c);
    T[j] = d2{c, -s};
}

// w[k] = exp(-i pi k^2 / n): k^2 mod 2 n in integers (k < 4096), then sincospi
__global__ void sp_chirp_kernel(int n, d2* w) {
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n) return;
    const int r = (k * k) % (2 * n);
    double s, c;
    sincospi((double)r / (double)n, &s, &c);
    w[k] = d2{c, -s};
}

// ---- forward FFT of the workgroup's G = PTS / N sub-FFTs of length N in LDS (item g at z + g (N + 1)):
// wc_csd.hip's (wc_welch_psd.hip's) stages, operation for operation ----
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

struct SpArgs {
    int64_t C;          // columns of x
    int n, step;        // nperseg, nperseg - noverlap
    int nseg, s0;       // segments, first segment of the launch (even)
    int detrend;
    double mul;         // PSD: scale; complex, magnitude: sqrt(scale)
    const double* x;    // [T][C]
    const double* win;  // [n]
    const d2* T;        // W_8192
    const d2* w;        // chirp [n]
    d2* Bf;             // chirp spectrum [L]
    double* out;        // [S][F][C] cells of one double (complex: two)
};

template <int LOGN> struct SpShape {
    static constexpr int N = 1 << LOGN;
    static constexpr int PTS = N > kMinPts ? N : kMinPts;
    static constexpr int G = PTS / N, NP = N + 1, ES = kThreads / G, EPT = PTS / kThreads;
    static constexpr bool kLdsTw = N <= kTwL;
    static constexpr int TB = kLdsTw ? kTwL : kTwG;
    static constexpr size_t lds_bytes = ((size_t)G * NP + (kLdsTw ? kTwLds : 0)) * sizeof(d2);
};

// one cell of the output from the bin's spectrum X; twice: a doubled bin of the one-sided PSD
template <int MODE>
__device__ __forceinline__ void sp_store(double* o, int64_t cell, d2 X, double mul, bool twice) {
    if constexpr (MODE == WC_SPEC_PSD) {
        o[cell] = __builtin_fma(X.x, X.x, X.y * X.y) * (twice ? 2.0 * mul : mul);
    } else if constexpr (MODE == WC_SPEC_COMPLEX) {
        o[2 * cell] = X.x * mul;
        o[2 * cell + 1] = X.y * mul;
    } else if constexpr (MODE == WC_SPEC_MAGNITUDE) {
        o[cell] = sqrt(__builtin_fma(X.x, X.x, X.y * X.y)) * mul;
    } else {
        o[cell] = (X.x == 0.0 && X.y == 0.0) ? 0.0 : atan2(X.y, X.x);
    }
}

// MODE == kChirp: the chirp spectrum Bf = FFT_L(conj(w) at m mod L, |m| < n), one workgroup (item 0).
// Otherwise: workgroup (blockIdx.x = column group, blockIdx.y = segment pair of the launch), item g = column.
template <int LOGN, int MODE>
__global__ void __launch_bounds__(kThreads) sp_kernel(const SpArgs a) {
    using S = SpShape<LOGN>;
    constexpr int N = S::N, G = S::G, NP = S::NP, ES = S::ES, EPT = S::EPT;
    extern __shared__ __attribute__((aligned(16))) d2 sp_smem[];
    d2* z = sp_smem;
    const int tid = threadIdx.x;
    const d2* T = a.T;
    if constexpr (S::kLdsTw) {
        d2* Tl = sp_smem + G * NP;
        for (int j = tid; j < kTwLds; j += kThreads) Tl[j] = a.T[j * (kTwG / kTwL)];
        T = Tl;
    }
    const int g = tid % G, e0 = tid / G;
    d2* zg = z + g * NP;
    const int n = a.n;

    if constexpr (MODE == kChirp) {
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
        const int64_t seg = (int64_t)F * a.C;  // cells of one segment
        const int64_t o0 = (int64_t)s * seg + c;
#pragma unroll
        for (int j = 0; j < EPT; ++j) {
            const int e = e0 + ES * j;
            if (e <= half) {
                const int r = e ? n - e : 0;
                const d2 yk = cmul(cconj(zg[e]), a.w[e]);         // L Y[k]
                const d2 yr = cconj(cmul(cconj(zg[r]), a.w[r]));  // L conj Y[n - k]
                const d2 sum = yk + yr, dif = yk - yr;
                const bool twice = e > 0 && 2 * e != n;
                const int64_t cell = o0 + (int64_t)e * a.C;
                sp_store<MODE>(a.out, cell, sum * sc, a.mul, twice);
                if (two) sp_store<MODE>(a.out, cell + seg, d2{dif.y, -dif.x} * sc, a.mul, twice);  // / i
            }
        }
    }
}

template <int LOGN, int MODE>
hipError_t sp_launch(const SpArgs& a, dim3 grid, hipStream_t st) {
    auto kern = sp_kernel<LOGN, MODE>;
    constexpr size_t lds = SpShape<LOGN>::lds_bytes;
    hipError_t e = hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(kern, grid, dim3(kThreads), lds, st, a);
    return hipSuccess;
}

template <int MODE>
hipError_t sp_dispatch(int logL, const SpArgs& a, int pairs, hipStream_t st) {
    const int G = std::max(1, kMinPts >> logL);
    const dim3 grid = MODE == kChirp ? dim3(1) : dim3((unsigned)((a.C + G - 1) / G), (unsigned)pairs);
    switch (logL) {
        case 6: return sp_launch<6, MODE>(a, grid, st);
        case 7: return sp_launch<7, MODE>(a, grid, st);
        case 8: return sp_launch<8, MODE>(a, grid, st);
        case 9: return sp_launch<9, MODE>(a, grid, st);
        case 10: return sp_launch<10, MODE>(a, grid, st);
        case 11: return sp_launch<11, MODE>(a, grid, st);
        case 12: return sp_launch<12, MODE>(a, grid, st);
        default: return sp_launch<13, MODE>(a, grid, st);
    }
}

hipError_t sp_dispatch_mode(int mode, int logL, const SpArgs& a, int pairs, hipStream_t st) {
    switch (mode) {
        case WC_SPEC_PSD: return sp_dispatch<WC_SPEC_PSD>(logL, a, pairs, st);
        case WC_SPEC_COMPLEX: return sp_dispatch<WC_SPEC_COMPLEX>(logL, a, pairs, st);
        case WC_SPEC_MAGNITUDE: return sp_dispatch<WC_SPEC_MAGNITUDE>(logL, a, pairs, st);
        default: return sp_dispatch<WC_SPEC_ANGLE>(logL, a, pairs, st);
    }
}

int sp_log_l(int n) {
    int logL = kMinLogL;
    while ((1 << logL) < 2 * n - 1) ++logL;
    return logL;
}

size_t sp_tables(int n) {  // bytes
    return ((size_t)kTwG + (size_t)((n + 15) / 16 * 16) + ((size_t)1 << sp_log_l(n))) * sizeof(d2);
}

}  // namespace

size_t wc_spectrogram_workspace_size(int nperseg) {
    return (nperseg < 2 || nperseg > kMaxN) ? 0 : sp_tables(nperseg);
}

int wc_spectrogram(int64_t C, int64_t T, const double* x, int nperseg, int noverlap, const double* window,
                   int detrend, double scale, int mode, double* out, void* workspace, size_t ws_bytes, void* stream) {
    wc_clear_err();
    char msg[200];
    const int n = nperseg;
    if (C <= 0) return wc_set_err(WC_EINVAL, "wc_spectrogram: C <= 0");
    if (C > kMaxC) return wc_set_err(WC_EINVAL, "wc_spectrogram: C > 2^24");
    if (n < 2) return wc_set_err(WC_EINVAL, "wc_spectrogram: nperseg < 2");
    if (noverlap < 0 || noverlap >= n)
        return wc_set_err(WC_EINVAL, "wc_spectrogram: noverlap outside 0 .. nperseg - 1");
    if (T < n) return wc_set_err(WC_EINVAL, "wc_spectrogram: T < nperseg");
    if (!x || !window || !out) return wc_set_err(WC_EINVAL, "wc_spectrogram: x, window or out is NULL");
    if (detrend != 0 && detrend != 1)
        return wc_set_err(WC_EINVAL, "wc_spectrogram: detrend must be 0 (none) or 1 (constant)");
    if (!(scale > 0.0) || !isfinite(scale))
        return wc_set_err(WC_EINVAL, "wc_spectrogram: scale must be finite and positive");
    if (mode < WC_SPEC_PSD || mode > WC_SPEC_ANGLE)
        return wc_set_err(WC_EINVAL, "wc_spectrogram: unknown mode (WC_SPEC_PSD .. WC_SPEC_ANGLE)");
    if ((T - n) / (n - noverlap) >= INT32_MAX) return wc_set_err(WC_EINVAL, "wc_spectrogram: 2^31 segments or more");
    if (n > kMaxN) {
        snprintf(msg, sizeof msg,
                 "wc_spectrogram: nperseg = %d > 4096 (the Bluestein FFT of 8192 points fills the LDS)", n);
        return wc_set_err(WC_EUNSUPPORTED, msg);
    }
    const int F = n / 2 + 1;
    const int nseg = (int)((T - n) / (n - noverlap) + 1);
    {
        // S F C < 2^31 2^12 2^24 and T C < 2^63 2^24: sized in 128 bits
        const unsigned __int128 lim = (unsigned __int128)1 << 62;
        const unsigned __int128 xb = (unsigned __int128)T * (unsigned __int128)C * 8;
        const unsigned __int128 ob =
            (unsigned __int128)nseg * (unsigned)F * (unsigned __int128)C * (mode == WC_SPEC_COMPLEX ? 16 : 8);
        if (xb >= lim) return wc_set_err(WC_EINVAL, "wc_spectrogram: x of 2^62 bytes or more");
        if (ob >= lim) return wc_set_err(WC_EINVAL, "wc_spectrogram: an output of 2^62 bytes or more");
        const uintptr_t x0 = (uintptr_t)x, x1 = x0 + (size_t)xb, p0 = (uintptr_t)out, p1 = p0 + (size_t)ob;
        if (p0 < x1 && x0 < p1) return wc_set_err(WC_EINVAL, "wc_spectrogram: out must not alias x");
        if ((x0 & 7) || (p0 & 7) || ((uintptr_t)window & 7))
            return wc_set_err(WC_EINVAL, "wc_spectrogram: x, window and out must be 8-byte aligned");
    }
    const size_t need = sp_tables(n);
    if (!workspace || ws_bytes < need) {
        snprintf(msg, sizeof msg, "wc_spectrogram: workspace < %zu bytes (wc_spectrogram_workspace_size)", need);
        return wc_set_err(WC_EWORKSPACE, msg);
    }
    if ((uintptr_t)workspace & 15) return wc_set_err(WC_EINVAL, "wc_spectrogram: workspace must be 16-byte aligned");

    hipStream_t st = static_cast<hipStream_t>(stream);
    const int logL = sp_log_l(n);
    d2* Tw = static_cast<d2*>(workspace);
    d2* w = Tw + kTwG;
    d2* Bf = w + (n + 15) / 16 * 16;

    hipLaunchKernelGGL(sp_twiddle_kernel, dim3(kTwG / 256), dim3(256), 0, st, Tw);
    hipLaunchKernelGGL(sp_chirp_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, n, w);
    const double mul = mode == WC_SPEC_PSD ? scale : sqrt(scale);
    SpArgs a{C, n, n - noverlap, nseg, 0, detrend, mul, x, window, Tw, w, Bf, out};
    hipError_t e = sp_dispatch<kChirp>(logL, a, 1, st);
    for (int64_t s0 = 0; s0 < nseg && e == hipSuccess; s0 += 2 * (int64_t)kMaxPairs) {
        const int segs = (int)std::min<int64_t>(2 * (int64_t)kMaxPairs, nseg - s0);
        a.s0 = (int)s0;
        e = sp_dispatch_mode(mode, logL, a, (segs + 1) / 2, st);
    }
    if (e != hipSuccess) {
        snprintf(wc_errbuf(), 512, "wc_spectrogram: %s", hipGetErrorString(e));
        return WC_EHIP;
    }
    return wc_hip_check("wc_spectrogram");
}

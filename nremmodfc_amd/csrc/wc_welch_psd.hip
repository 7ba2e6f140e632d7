// wc_welch_psd.hip -- scipy.signal.welch(x, axis=0) per column on the device (gfx950): any segment
// length 2 <= nperseg <= 4096, any overlap, Hann or any other window, optional constant detrend
// (cortex_run.py:203-209: nperseg = 1000 and 400; the sweep's 4000).
//
// A segment's exact length-n DFT is a Bluestein convolution over a power-of-two FFT of length
//   L = max(64, nextpow2(2 n - 1)) <= 8192:
//   X[k] = w[k] sum_m (x[m] w[m]) conj(w)[k - m],  w[k] = exp(-i pi k^2 / n),
// with k^2 reduced mod 2 n in integers before sincospi (as wc_hilbert.hip).  Only |X[k]|^2 is
// wanted and |w[k]| = 1, so the convolution is the result: two forward FFTs (the inverse as
// conj(FFT(conj(.)))) with the chirp spectrum between them, and |.|^2 / L^2 after the second.
//
// The whole convolution stays in LDS.  A workgroup (512 threads) owns max(4096, L) complex fp64
// points: G = 4096 / L neighbouring columns of one segment for L <= 4096 (their samples are
// G * 8 contiguous bytes of the time-major array), one column for L = 8192.  The FFT is an
// in-place Stockham (every read of a stage, barrier, every write, barrier), radix 4 with a
// leading radix-2 stage for odd log2 L, as wc_hilbert.hip's; twiddles come from a 768-entry
// table of W_1024 in LDS for L <= 1024 and from the W_8192 table in global memory above.
// LDS: 65.0 .. 78.8 KB for L <= 4096 (two workgroups per CU), 128.0 KB for L = 8192 (one).
//
// Segments: nseg = (T - n) / step + 1 are cut into NB = ceil(nseg / SB) <= 16 blocks of
// SB = 2 ceil(nseg / 32) consecutive segments.  Workgroup (column group, block) walks its segments
// in order, two at a time: the input is real, so segments s and s + 1 of a column go through one
// complex transform as A + i B, and since only the sum of their periodograms is wanted,
//   |DFT A|^2[k] + |DFT B|^2[k] = (|Y[k]|^2 + |Y[n - k]|^2) / 2,  Y = DFT(A + i B),
// exactly, without splitting Y (an odd last segment rides alone, B = 0).  Every thread adds the
// sums of its own bins in registers and stores the block's to partial [NB][F][tc]; the second
// kernel adds the NB partials of a bin in block order and applies scale / nseg and the one-sided
// doubling.  No atomics; the blocks and pairs depend on (T, n, noverlap) only and a column's
// arithmetic on nothing but its own samples, so a column's PSD is bit-identical for every C, every
// position of the column and every workspace size (the workspace decides how many columns, tc, go
// through the two kernels at a time).
// The detrend means (one per segment) are a fixed tree: each thread adds its own samples in
// order, then the threads of a column halve log2(512 / G) times through LDS.
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
constexpr int kMaxBlocks = 16;    // segment blocks per column

__device__ __forceinline__ d2 cmul(d2 a, d2 w) {
    return d2{__builtin_fma(a.x, w.x, -a.y * w.y), __builtin_fma(a.x, w.y, a.y * w.x)};
}
__device__ __forceinline__ d2 cconj(d2 a) { return d2{a.x, -a.y}; }

// T[j] = exp(-2 pi i j / 8192), j < 8192
__global__ void wp_twiddle_kernel(d2* T) {
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= kTwG) return;
    double s, c;
    sincospi(2.0 * j / kTwG, &s, &c);
    T[j] = d2{c, -s};
}

// w[k] = exp(-i pi k^2 / n): k^2 mod 2 n in integers (k < 4096), then sincospi
__global__ void wp_chirp_kernel(int n, d2* w) {
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n) return;
    const int r = (k * k) % (2 * n);
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

// every point of z written and a barrier passed before the call; ends with a barrier.  A real call:
// inlined twice into the segment loop, the stages' loads are scheduled across each other and the
// kernel needs 150 .. 230 VGPRs (one workgroup per CU) and spills at L = 8192; called, 116 .. 132 and 248
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

struct WpArgs {
    int64_t C, c0;      // columns of x, first column of the tile
    int tc;             // columns of the tile
    int n, step;        // nperseg, nperseg - noverlap
    int nseg, sb;       // segments, segments per block
    int detrend;
    const double* x;    // [T][C]
    const double* win;  // [n]
    const d2* T;        // W_8192
    const d2* w;        // chirp [n]
    d2* Bf;             // chirp spectrum [L]
    double* partial;    // [NB][F][tc]
};

template <int LOGN> struct WpShape {
    static constexpr int N = 1 << LOGN;
    static constexpr int PTS = N > kMinPts ? N : kMinPts;
    static constexpr int G = PTS / N, NP = N + 1, ES = kThreads / G, EPT = PTS / kThreads;
    static constexpr bool kLdsTw = N <= kTwL;
    static constexpr int TB = kLdsTw ? kTwL : kTwG;
    static constexpr size_t lds_bytes = ((size_t)G * NP + (kLdsTw ? kTwLds : 0)) * sizeof(d2);
};

// CHIRP: the chirp spectrum Bf = FFT_L(conj(w) at m mod L, |m| < n), one workgroup (item 0).
// Otherwise: workgroup (blockIdx.x = column group, blockIdx.y = segment block), item g = column.
template <int LOGN, bool CHIRP>
__global__ void __launch_bounds__(kThreads) wp_kernel(const WpArgs a) {
    using S = WpShape<LOGN>;
    constexpr int N = S::N, G = S::G, NP = S::NP, ES = S::ES, EPT = S::EPT;
    extern __shared__ __attribute__((aligned(16))) d2 wp_smem[];
    d2* z = wp_smem;
    const int tid = threadIdx.x;
    const d2* T = a.T;
    if constexpr (S::kLdsTw) {
        d2* Tl = wp_smem + G * NP;
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
        const int c = blockIdx.x * G + g;
        const bool live = c < a.tc;
        d2* red = z;  // [kThreads], between segment pairs only
        const int half = n / 2;
        double acc[EPT];
#pragma unroll
        for (int j = 0; j < EPT; ++j) acc[j] = 0.0;
        const int s0 = blockIdx.y * a.sb, s1 = min(a.nseg, s0 + a.sb);
        for (int s = s0; s < s1; s += 2) {
            // segments s and s + 1 (or s and nothing) ride one complex transform as A + i B
            const bool two = s + 1 < s1;
            // the thread index is made opaque per pair, so that no per-point address is kept in
            // registers across the loop (with them: 130 .. 169 VGPRs, and 63 spilled at L = 8192)
            int lt = tid;
            asm volatile("" : "+v"(lt));
            const int g = lt % G, e0 = lt / G;
            d2* zg = z + g * NP;
            const double* xc = a.x + a.c0 + blockIdx.x * G + g;
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
            fft_lds<LOGN, S::PTS, S::TB>(z, T, lt);
#pragma unroll
            for (int j = 0; j < EPT; ++j) {
                const int e = e0 + ES * j;
                zg[e] = cconj(cmul(zg[e], a.Bf[e]));
            }
            __syncthreads();
            fft_lds<LOGN, S::PTS, S::TB>(z, T, lt);  // L conj(convolution): |.| = L |Y|, Y = DFT(A + i B)
            // |DFT A|^2 + |DFT B|^2 at bin k is (|Y[k]|^2 + |Y[n - k]|^2) / 2, exactly: no split is needed
#pragma unroll
            for (int j = 0; j < EPT; ++j) {
                const int e = e0 + ES * j;
                if (e <= half) {
                    const d2 v = zg[e], u = zg[e ? n - e : 0];
                    acc[j] += __builtin_fma(v.x, v.x, v.y * v.y) + __builtin_fma(u.x, u.x, u.y * u.y);
                }
            }
            __syncthreads();  // every bin has been read before the next pair is written
        }
        if (!live) return;
        const int F = half + 1;
        const double sc = 0.5 / ((double)N * (double)N);
        double* out = a.partial + (int64_t)blockIdx.y * F * a.tc + c;
#pragma unroll
        for (int j = 0; j < EPT; ++j) {
            const int e = e0 + ES * j;
            if (e <= half) out[(int64_t)e * a.tc] = acc[j] * sc;
        }
    }
}

// psd[f][c0 + c] = (sum over blocks, in order) * scale / nseg, one-sided bins doubled
__global__ void wp_finish_kernel(int64_t C, int64_t c0, int tc, int n, int nb, double mult, const double* partial,
                                 double* psd) {
    const int F = n / 2 + 1;
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x, tot = (int64_t)F * tc;
    if (i >= tot) return;
    const int f = (int)(i / tc), c = (int)(i % tc);
    double s = partial[i];
    for (int b = 1; b < nb; ++b) s += partial[b * tot + i];
    const bool twice = f > 0 && !(n % 2 == 0 && f == n / 2);
    psd[(int64_t)f * C + c0 + c] = s * (twice ? 2.0 * mult : mult);
}

template <int LOGN, bool CHIRP>
hipError_t wp_launch(const WpArgs& a, dim3 grid, hipStream_t st) {
    auto kern = wp_kernel<LOGN, CHIRP>;
    constexpr size_t lds = WpShape<LOGN>::lds_bytes;
    hipError_t e = hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(kern, grid, dim3(kThreads), lds, st, a);
    return hipSuccess;
}

template <bool CHIRP>
hipError_t wp_dispatch(int logL, const WpArgs& a, int nb, hipStream_t st) {
    const int G = std::max(1, kMinPts >> logL);
    const dim3 grid = CHIRP ? dim3(1) : dim3((unsigned)((a.tc + G - 1) / G), (unsigned)nb);
    switch (logL) {
        case 6: return wp_launch<6, CHIRP>(a, grid, st);
        case 7: return wp_launch<7, CHIRP>(a, grid, st);
        case 8: return wp_launch<8, CHIRP>(a, grid, st);
        case 9: return wp_launch<9, CHIRP>(a, grid, st);
        case 10: return wp_launch<10, CHIRP>(a, grid, st);
        case 11: return wp_launch<11, CHIRP>(a, grid, st);
        case 12: return wp_launch<12, CHIRP>(a, grid, st);
        default: return wp_launch<13, CHIRP>(a, grid, st);
    }
}

int wp_log_len(int n) {  // log2 L, L = max(64, nextpow2(2 n - 1))
    int l = kMinLogL;
    while ((1 << l) < 2 * n - 1) ++l;
    return l;
}

struct WpPlan {
    int logL, nseg, sb, nb, F;
    size_t tab, per_col;  // bytes of the tables, of one column's partial sums
};

// the segment blocks and the workspace layout: W_8192 | chirp w [n] (padded to 16 entries) | chirp spectrum [L] |
// partial [NB][F][tc]
WpPlan wp_plan(int64_t T, int n, int noverlap) {
    WpPlan p;
    p.logL = wp_log_len(n);
    p.nseg = (int)((T - n) / (n - noverlap) + 1);
    p.sb = 2 * ((p.nseg + 2 * kMaxBlocks - 1) / (2 * kMaxBlocks));  // whole pairs
    p.nb = (p.nseg + p.sb - 1) / p.sb;
    p.F = n / 2 + 1;
    p.tab = ((size_t)kTwG + (size_t)((n + 15) / 16 * 16) + ((size_t)1 << p.logL)) * sizeof(d2);
    p.per_col = (size_t)p.nb * p.F * sizeof(double);
    return p;
}

bool wp_shape_ok(int64_t C, int64_t T, int n, int noverlap) {
    // T - n < 2^31 steps of at least one sample: nseg fits an int
    return C > 0 && n >= 2 && n <= kMaxN && noverlap >= 0 && noverlap < n && T >= n && (T - n) / (n - noverlap) < INT32_MAX;
}

}  // namespace

size_t wc_welch_psd_workspace_size(int64_t C, int64_t T, int nperseg, int noverlap) {
    if (!wp_shape_ok(C, T, nperseg, noverlap)) return 0;
    const WpPlan p = wp_plan(T, nperseg, noverlap);
    return p.tab + p.per_col;
}

int wc_welch_psd(int64_t C, int64_t T, const double* x, int nperseg, int noverlap, const double* window, int detrend,
                 double scale, double* psd, void* workspace, size_t ws_bytes, void* stream) {
    wc_clear_err();
    char msg[200];
    const int n = nperseg;
    if (C <= 0) return wc_set_err(WC_EINVAL, "wc_welch_psd: C <= 0");
    if (n < 2) return wc_set_err(WC_EINVAL, "wc_welch_psd: nperseg < 2");
    if (noverlap < 0 || noverlap >= n) return wc_set_err(WC_EINVAL, "wc_welch_psd: noverlap outside 0 .. nperseg - 1");
    if (T < n) return wc_set_err(WC_EINVAL, "wc_welch_psd: T < nperseg");
    if (!x || !window || !psd) return wc_set_err(WC_EINVAL, "wc_welch_psd: x, window or psd is NULL");
    if (detrend != 0 && detrend != 1) return wc_set_err(WC_EINVAL, "wc_welch_psd: detrend must be 0 (none) or 1 (constant)");
    if (!(scale > 0.0) || !isfinite(scale)) return wc_set_err(WC_EINVAL, "wc_welch_psd: scale must be finite and positive");
    if ((T - n) / (n - noverlap) >= INT32_MAX) return wc_set_err(WC_EINVAL, "wc_welch_psd: 2^31 segments or more");
    const int F = n / 2 + 1;
    {
        const uintptr_t x0 = (uintptr_t)x, x1 = x0 + (size_t)T * C * 8, p0 = (uintptr_t)psd, p1 = p0 + (size_t)F * C * 8;
        if (p0 < x1 && x0 < p1) return wc_set_err(WC_EINVAL, "wc_welch_psd: psd must not alias x");
        if ((x0 & 7) || (p0 & 7) || ((uintptr_t)window & 7))
            return wc_set_err(WC_EINVAL, "wc_welch_psd: x, window and psd must be 8-byte aligned");
    }
    if (n > kMaxN) {
        snprintf(msg, sizeof msg, "wc_welch_psd: nperseg = %d > 4096 (the Bluestein FFT of 8192 points fills the LDS)", n);
        return wc_set_err(WC_EUNSUPPORTED, msg);
    }
    const WpPlan p = wp_plan(T, n, noverlap);
    if (!workspace || ws_bytes < p.tab + p.per_col) {
        snprintf(msg, sizeof msg, "wc_welch_psd: workspace < %zu bytes (wc_welch_psd_workspace_size)", p.tab + p.per_col);
        return wc_set_err(WC_EWORKSPACE, msg);
    }
    if ((uintptr_t)workspace & 15) return wc_set_err(WC_EINVAL, "wc_welch_psd: workspace must be 16-byte aligned");

    hipStream_t st = static_cast<hipStream_t>(stream);
    d2* Tw = static_cast<d2*>(workspace);
    d2* w = Tw + kTwG;
    d2* Bf = w + (n + 15) / 16 * 16;
    double* partial = reinterpret_cast<double*>(Bf + ((size_t)1 << p.logL));
    // columns per pass: what the workspace holds, and a grid of at most 2^20 column groups
    const int64_t tcmax = (int64_t)std::min<size_t>((ws_bytes - p.tab) / p.per_col, (size_t)std::min<int64_t>(C, 1 << 20));

    hipLaunchKernelGGL(wp_twiddle_kernel, dim3(kTwG / 256), dim3(256), 0, st, Tw);
    hipLaunchKernelGGL(wp_chirp_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, n, w);
    WpArgs a{C, 0, 1, n, n - noverlap, p.nseg, p.sb, detrend, x, window, Tw, w, Bf, partial};
    hipError_t e = wp_dispatch<true>(p.logL, a, 1, st);
    const double mult = scale / (double)p.nseg;
    for (int64_t c0 = 0; c0 < C && e == hipSuccess; c0 += tcmax) {
        a.c0 = c0;
        a.tc = (int)std::min<int64_t>(tcmax, C - c0);
        e = wp_dispatch<false>(p.logL, a, p.nb, st);
        const int64_t tot = (int64_t)p.F * a.tc;
        if (e == hipSuccess)
            hipLaunchKernelGGL(wp_finish_kernel, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, st, C, c0, a.tc, n,
                               p.nb, mult, partial, psd);
    }
    if (e != hipSuccess) {
        snprintf(wc_errbuf(), 512, "wc_welch_psd: %s", hipGetErrorString(e));
        return WC_EHIP;
    }
    return wc_hip_check("wc_welch_psd");
}

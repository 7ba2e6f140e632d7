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
// leading radix-2 stage for odd log2 L (wc_bluestein.h: the stages wc_hilbert.hip uses too, and the
// tables, shape, segment-pair transform, dispatch and argument checks that wc_csd.hip and
// wc_spectrogram.hip share with this file); twiddles come from a 768-entry
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
#include "wc_bluestein.h"

namespace {

constexpr int kMaxBlocks = 16;    // segment blocks per column

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

// workgroup (blockIdx.x = column group, blockIdx.y = segment block), item g = column
template <int LOGN>
__global__ void __launch_bounds__(kThreads) wp_kernel(const WpArgs a) {
    using S = BsShape<LOGN>;
    constexpr int N = S::N, G = S::G, NP = S::NP, ES = S::ES, EPT = S::EPT;
    d2* z = bs_lds();
    const int tid = threadIdx.x;
    const d2* T = bs_twiddles<LOGN>(z, a.T, tid);
    const int g = tid % G, e0 = tid / G;
    const int n = a.n;
    const int c = blockIdx.x * G + g;
    const bool live = c < a.tc;
    const int half = n / 2;
    double acc[EPT];
#pragma unroll
    for (int j = 0; j < EPT; ++j) acc[j] = 0.0;
    const int s0 = blockIdx.y * a.sb, s1 = min(a.nseg, s0 + a.sb);
    for (int s = s0; s < s1; s += 2) {
        // the thread index is made opaque per pair, so that no per-point address is kept in
        // registers across the loop (with them: 130 .. 169 VGPRs, and 63 spilled at L = 8192)
        int lt = tid;
        asm volatile("" : "+v"(lt));
        const int g = lt % G, e0 = lt / G;
        d2* zg = z + g * NP;
        const double* xc = a.x + a.c0 + blockIdx.x * G + g;
        bs_segment_pair<LOGN>(a, z, T, lt, xc, (int64_t)s * a.step, live, s + 1 < s1);
        // z = L conj(convolution): |.| = L |Y|, Y = DFT(A + i B), and
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

struct WpPlan {
    BsTables tab;  // the workspace's head
    int nseg, sb, nb, F;
    size_t per_col;  // bytes of one column's partial sums
};

// the segment blocks and the workspace layout: the tables | partial [NB][F][tc]
WpPlan wp_plan(int64_t T, int n, int noverlap, void* workspace) {
    WpPlan p;
    p.tab = bs_layout(n, workspace);
    p.nseg = (int)((T - n) / (n - noverlap) + 1);
    p.sb = 2 * ((p.nseg + 2 * kMaxBlocks - 1) / (2 * kMaxBlocks));  // whole pairs
    p.nb = (p.nseg + p.sb - 1) / p.sb;
    p.F = n / 2 + 1;
    p.per_col = (size_t)p.nb * p.F * sizeof(double);
    return p;
}

}  // namespace

size_t wc_welch_psd_workspace_size(int64_t C, int64_t T, int nperseg, int noverlap) {
    if (!bs_shape_ok(C, T, nperseg, noverlap)) return 0;
    const WpPlan p = wp_plan(T, nperseg, noverlap, nullptr);
    return p.tab.bytes + p.per_col;
}

int wc_welch_psd(int64_t C, int64_t T, const double* x, int nperseg, int noverlap, const double* window, int detrend,
                 double scale, double* psd, void* workspace, size_t ws_bytes, void* stream) {
    wc_clear_err();
    const char* fn = "wc_welch_psd";
    const int n = nperseg;
    if (int rc = bs_check_args(fn, "psd", C, T, x, n, noverlap, window, detrend, scale, psd, workspace)) return rc;
    const WpPlan p = wp_plan(T, n, noverlap, workspace);
    const WcSpan in = {"x", x, (size_t)T * C * 8, 8}, o = {"psd", psd, (size_t)p.F * C * 8, 8};
    if (int rc = wc_check_alias(fn, &o, 1, &in, 1)) return rc;
    if (int rc = wc_check_workspace(fn, "wc_welch_psd_workspace_size", workspace, ws_bytes, p.tab.bytes + p.per_col))
        return rc;

    hipStream_t st = static_cast<hipStream_t>(stream);
    double* partial = reinterpret_cast<double*>(p.tab.Bf + ((size_t)1 << p.tab.logL));
    // columns per pass: what the workspace holds, and a grid of at most 2^20 column groups
    const int64_t tcmax =
        (int64_t)std::min<size_t>((ws_bytes - p.tab.bytes) / p.per_col, (size_t)std::min<int64_t>(C, 1 << 20));

    int rc = bs_fill_tables(fn, p.tab, n, st);
    WpArgs a{C, 0, 1, n, n - noverlap, p.nseg, p.sb, detrend, x, window, p.tab.T, p.tab.w, p.tab.Bf, partial};
    const double mult = scale / (double)p.nseg;
    for (int64_t c0 = 0; c0 < C && rc == WC_OK; c0 += tcmax) {
        a.c0 = c0;
        a.tc = (int)std::min<int64_t>(tcmax, C - c0);
        rc = bs_dispatch(p.tab.logL, [&](auto I) {
            constexpr int LOGN = decltype(I)::value;
            return bs_launch<LOGN>(fn, wp_kernel<LOGN>, bs_grid(LOGN, a.tc, p.nb), st, a);
        });
        const int64_t tot = (int64_t)p.F * a.tc;
        if (rc == WC_OK)
            hipLaunchKernelGGL(wp_finish_kernel, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, st, C, c0, a.tc, n,
                               p.nb, mult, partial, psd);
    }
    return rc ? rc : wc_hip_check(fn);
}


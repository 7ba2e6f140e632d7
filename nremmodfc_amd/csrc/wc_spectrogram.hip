// wc_spectrogram.hip -- scipy.signal.spectrogram of every column of a time-major x [T][C] on the
// device (gfx950, fp64): the one-sided spectrum of every Welch segment, nothing averaged, any
// 2 <= nperseg <= 4096, as a PSD, complex, magnitude or angle.
//
// The transform (sp_kernel) is wc_csd.hip's cs_spec_kernel -- the same segmentation, window, constant
// detrend, chirp, tables and in-LDS Stockham FFT, and the same split: wc_bluestein.h's bs_segment_pair
// and bs_split, which both call.  A workgroup (512 threads) transforms one pair of segments
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
#include "wc_bluestein.h"

namespace {

constexpr int64_t kMaxC = 1 << 24;
constexpr int kMaxPairs = 32768;  // segment pairs per launch: gridDim.y

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

// workgroup (blockIdx.x = column group, blockIdx.y = segment pair of the launch), item g = column
template <int LOGN, int MODE>
__global__ void __launch_bounds__(kThreads) sp_kernel(const SpArgs a) {
    using S = BsShape<LOGN>;
    constexpr int N = S::N, G = S::G, NP = S::NP, ES = S::ES, EPT = S::EPT;
    d2* z = bs_lds();
    const int tid = threadIdx.x;
    const d2* T = bs_twiddles<LOGN>(z, a.T, tid);
    const int g = tid % G, e0 = tid / G;
    d2* zg = z + g * NP;
    const int n = a.n;
    const int64_t c = (int64_t)blockIdx.x * G + g;
    const bool live = c < a.C;
    const int half = n / 2;
    const int s = a.s0 + 2 * (int)blockIdx.y;
    const bool two = s + 1 < a.nseg;
    bs_segment_pair<LOGN>(a, z, T, tid, a.x + c, (int64_t)s * a.step, live, two);
    if (!live) return;
    const int F = half + 1;
    const double sc = 0.5 / (double)N;
    const int64_t seg = (int64_t)F * a.C;  // cells of one segment
    const int64_t o0 = (int64_t)s * seg + c;
#pragma unroll
    for (int j = 0; j < EPT; ++j) {
        const int e = e0 + ES * j;
        if (e <= half) {
            d2 XA, XB;
            bs_split(zg, a.w, n, e, sc, XA, XB);
            const bool twice = e > 0 && 2 * e != n;
            const int64_t cell = o0 + (int64_t)e * a.C;
            sp_store<MODE>(a.out, cell, XA, a.mul, twice);
            if (two) sp_store<MODE>(a.out, cell + seg, XB, a.mul, twice);
        }
    }
}

template <int MODE>
int sp_dispatch(int logL, const SpArgs& a, int pairs, hipStream_t st) {
    return bs_dispatch(logL, [&](auto I) {
        constexpr int LOGN = decltype(I)::value;
        return bs_launch<LOGN>("wc_spectrogram", sp_kernel<LOGN, MODE>, bs_grid(LOGN, a.C, pairs), st, a);
    });
}

int sp_dispatch_mode(int mode, int logL, const SpArgs& a, int pairs, hipStream_t st) {
    switch (mode) {
        case WC_SPEC_PSD: return sp_dispatch<WC_SPEC_PSD>(logL, a, pairs, st);
        case WC_SPEC_COMPLEX: return sp_dispatch<WC_SPEC_COMPLEX>(logL, a, pairs, st);
        case WC_SPEC_MAGNITUDE: return sp_dispatch<WC_SPEC_MAGNITUDE>(logL, a, pairs, st);
        default: return sp_dispatch<WC_SPEC_ANGLE>(logL, a, pairs, st);
    }
}

}  // namespace

size_t wc_spectrogram_workspace_size(int nperseg) {
    return (nperseg < 2 || nperseg > kMaxN) ? 0 : bs_layout(nperseg, nullptr).bytes;
}

int wc_spectrogram(int64_t C, int64_t T, const double* x, int nperseg, int noverlap, const double* window,
                   int detrend, double scale, int mode, double* out, void* workspace, size_t ws_bytes, void* stream) {
    wc_clear_err();
    const char* fn = "wc_spectrogram";
    const int n = nperseg;
    if (C > kMaxC) return wc_fail(WC_EINVAL, "wc_spectrogram: C > 2^24");
    if (int rc = bs_check_args(fn, "out", C, T, x, n, noverlap, window, detrend, scale, out, workspace)) return rc;
    if (mode < WC_SPEC_PSD || mode > WC_SPEC_ANGLE)
        return wc_fail(WC_EINVAL, "wc_spectrogram: unknown mode (WC_SPEC_PSD .. WC_SPEC_ANGLE)");
    const int F = n / 2 + 1;
    const int nseg = (int)((T - n) / (n - noverlap) + 1);
    {
        // S F C < 2^31 2^12 2^24 and T C < 2^63 2^24: sized in 128 bits
        const unsigned __int128 lim = (unsigned __int128)1 << 62;
        const unsigned __int128 xb = (unsigned __int128)T * (unsigned __int128)C * 8;
        const unsigned __int128 ob =
            (unsigned __int128)nseg * (unsigned)F * (unsigned __int128)C * (mode == WC_SPEC_COMPLEX ? 16 : 8);
        if (xb >= lim) return wc_fail(WC_EINVAL, "wc_spectrogram: x of 2^62 bytes or more");
        if (ob >= lim) return wc_fail(WC_EINVAL, "wc_spectrogram: an output of 2^62 bytes or more");
        const WcSpan in = {"x", x, (size_t)xb, 8}, o = {"out", out, (size_t)ob, 8};
        if (int rc = wc_check_alias(fn, &o, 1, &in, 1)) return rc;
    }
    const BsTables tab = bs_layout(n, workspace);
    if (int rc = wc_check_workspace(fn, "wc_spectrogram_workspace_size", workspace, ws_bytes, tab.bytes)) return rc;

    hipStream_t st = static_cast<hipStream_t>(stream);
    int rc = bs_fill_tables(fn, tab, n, st);
    const double mul = mode == WC_SPEC_PSD ? scale : sqrt(scale);
    SpArgs a{C, n, n - noverlap, nseg, 0, detrend, mul, x, window, tab.T, tab.w, tab.Bf, out};
    for (int64_t s0 = 0; s0 < nseg && rc == WC_OK; s0 += 2 * (int64_t)kMaxPairs) {
        const int segs = (int)std::min<int64_t>(2 * (int64_t)kMaxPairs, nseg - s0);
        a.s0 = (int)s0;
        rc = sp_dispatch_mode(mode, tab.logL, a, (segs + 1) / 2, st);
    }
    return rc ? rc : wc_hip_check(fn);
}

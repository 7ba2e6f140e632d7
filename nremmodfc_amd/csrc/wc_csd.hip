// wc_csd.hip -- cross-spectral density matrix and magnitude-squared coherence of the columns of a
// time-major x [T][C] on the device (gfx950, fp64): scipy.signal.csd / coherence with Welch's
// segmentation, any 2 <= nperseg <= 4096, P_xy = conj(X) Y averaged over the segments.
//
// Pass 1 (cs_spec_kernel) is wc_welch_psd.hip's segment transform -- the same segmentation, window,
// constant detrend, chirp, tables and in-LDS Stockham FFT: wc_bluestein.h's bs_segment_pair, which
// both call -- but it keeps the spectra.  A workgroup (512 threads) transforms one pair of
// segments (s, s + 1), s even, of G = 4096 / L neighbouring columns (one column at L = 8192) as
// A + i B in one complex Bluestein convolution.  The second FFT leaves z = L conj(convolution), so
//   Y[k] = DFT(A + i B)[k] = w[k] conj(z[k]) / L,      w[k] = exp(-i pi k^2 / n),
// and the two real segments' spectra are split out of it,
//   X_A[k] = (Y[k] + conj Y[n - k]) / 2,   X_B[k] = (Y[k] - conj Y[n - k]) / (2 i),
// the chirp factor applied to both terms before the split (w[n - k] is read from the table):
// wc_bluestein.h's bs_split, shared with wc_spectrogram.hip.  An
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
#include "wc_bluestein.h"

namespace {

constexpr int kMaxMatC = 1024;    // matrix modes: at most 528 tile pairs per bin
constexpr int64_t kMaxC = 1 << 24;
constexpr int kMaxChunkPairs = 32768;  // pass 1: gridDim.y
constexpr int kTile = 32;         // pass 2: columns per strip (kTile / 16 = 2 x 2 accumulators per thread)
constexpr int kKS = 16;           // pass 2: segments staged in LDS at a time
constexpr int kGramThreads = 256;

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

// workgroup (blockIdx.x = column group, blockIdx.y = segment pair of the chunk), item g = column
template <int LOGN>
__global__ void __launch_bounds__(kThreads) cs_spec_kernel(const CsArgs a) {
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
    d2* o = a.spec + (int64_t)(2 * blockIdx.y) * F * a.C + c;
#pragma unroll
    for (int j = 0; j < EPT; ++j) {
        const int e = e0 + ES * j;
        if (e <= half) {
            d2 XA, XB;
            bs_split(zg, a.w, n, e, sc, XA, XB);
            o[(int64_t)e * a.C] = XA;
            if (two) o[((int64_t)F + e) * a.C] = XB;
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

struct CsPlan {
    BsTables tab;  // the workspace's head
    int nseg, F;
    size_t aux, blk;  // bytes of aux [F][C] complex, of one segment pair's spectra
};

CsPlan cs_plan(int64_t C, int64_t T, int n, int noverlap, void* workspace) {
    CsPlan p;
    p.tab = bs_layout(n, workspace);
    p.nseg = (int)((T - n) / (n - noverlap) + 1);
    p.F = n / 2 + 1;
    p.aux = (size_t)p.F * (size_t)C * sizeof(d2);
    p.blk = 2 * p.aux;
    return p;
}

}  // namespace

size_t wc_csd_workspace_size(int64_t C, int64_t T, int nperseg, int noverlap) {
    if (C > kMaxC || !bs_shape_ok(C, T, nperseg, noverlap)) return 0;
    const CsPlan p = cs_plan(C, T, nperseg, noverlap, nullptr);
    return p.tab.bytes + p.aux + p.blk;
}

int wc_csd(int64_t C, int64_t T, const double* x, int nperseg, int noverlap, const double* window, int detrend,
           double scale, int mode, double* out, void* workspace, size_t ws_bytes, void* stream) {
    wc_clear_err();
    const char* fn = "wc_csd";
    const int n = nperseg;
    if (C > kMaxC) return wc_fail(WC_EINVAL, "wc_csd: C > 2^24");
    if (int rc = bs_check_args(fn, "out", C, T, x, n, noverlap, window, detrend, scale, out, workspace)) return rc;
    if (mode < WC_CSD_MATRIX || mode > WC_CSD_PAIR_COHERENCE)
        return wc_fail(WC_EINVAL, "wc_csd: unknown mode (WC_CSD_MATRIX .. WC_CSD_PAIR_COHERENCE)");
    const bool pairs = mode == WC_CSD_PAIRS || mode == WC_CSD_PAIR_COHERENCE;
    const bool coh = mode == WC_CSD_COHERENCE || mode == WC_CSD_PAIR_COHERENCE;
    if (pairs && (C & 1)) return wc_fail(WC_EINVAL, "wc_csd: a pair mode needs an even C (column i with i + C / 2)");
    if (!pairs && C > kMaxMatC)
        return wc_fail(WC_EUNSUPPORTED, "wc_csd: C = %lld > 1024 columns in a matrix mode", (long long)C);
    const CsPlan p = cs_plan(C, T, n, noverlap, workspace);
    const int F = p.F;
    const size_t cells = pairs ? (size_t)F * (size_t)(C / 2) : (size_t)F * (size_t)C * (size_t)C;
    const WcSpan in = {"x", x, (size_t)T * C * 8, 8}, o = {"out", out, cells * (coh ? 8 : 16), 8};
    if (int rc = wc_check_alias(fn, &o, 1, &in, 1)) return rc;
    const size_t need = p.tab.bytes + p.aux + p.blk;
    if (int rc = wc_check_workspace(fn, "wc_csd_workspace_size", workspace, ws_bytes, need)) return rc;

    hipStream_t st = static_cast<hipStream_t>(stream);
    double* aux = reinterpret_cast<double*>(p.tab.Bf + ((size_t)1 << p.tab.logL));
    d2* spec = reinterpret_cast<d2*>(aux) + (size_t)F * (size_t)C;
    // segment pairs per chunk: what the workspace holds
    const int64_t all_pairs = ((int64_t)p.nseg + 1) / 2;
    const int cpairs = (int)std::min<int64_t>(
        std::min<int64_t>((int64_t)((ws_bytes - p.tab.bytes - p.aux) / p.blk), all_pairs), kMaxChunkPairs);

    int rc = bs_fill_tables(fn, p.tab, n, st);
    CsArgs a{C, n, n - noverlap, p.nseg, 0, detrend, x, window, p.tab.T, p.tab.w, p.tab.Bf, spec};
    const double mult = scale / (double)p.nseg;
    const int nt = (int)((C + kTile - 1) / kTile);
    for (int64_t s0 = 0; s0 < p.nseg && rc == WC_OK; s0 += 2 * (int64_t)cpairs) {
        const int cs = (int)std::min<int64_t>(2 * (int64_t)cpairs, p.nseg - s0);
        const int first = s0 == 0, last = s0 + cs >= p.nseg;
        a.s0 = (int)s0;
        rc = bs_dispatch(p.tab.logL, [&](auto I) {
            constexpr int LOGN = decltype(I)::value;
            return bs_launch<LOGN>(fn, cs_spec_kernel<LOGN>, bs_grid(LOGN, C, (cs + 1) / 2), st, a);
        });
        if (rc) break;
        if (pairs) {
            const int64_t tot = (int64_t)F * (C / 2);
            hipLaunchKernelGGL(cs_pair_kernel, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, st, C, F, n, cs, first,
                               last, (int)coh, mult, spec, aux, out);
        } else {
            hipLaunchKernelGGL(cs_gram_kernel, dim3((unsigned)(nt * (nt + 1) / 2), (unsigned)F), dim3(kGramThreads), 0, st,
                               (int)C, F, n, cs, first, last, (int)coh, mult, spec, out);
        }
    }
    if (rc == WC_OK && mode == WC_CSD_COHERENCE) {
        const int64_t nd = (int64_t)F * C, tot = nd * C;
        hipLaunchKernelGGL(cs_diag_kernel, dim3((unsigned)((nd + 255) / 256)), dim3(256), 0, st, (int)C, F, out, aux);
        hipLaunchKernelGGL(cs_coherence_kernel, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, st, (int)C, F, aux,
                           out);
    }
    return rc ? rc : wc_hip_check(fn);
}


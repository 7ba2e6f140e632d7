// wc_hilbert.hip -- Hilbert phases and envelopes of long series (gfx950): utils.kuramoto's
// and utils.envelope's scipy.signal.hilbert(x, axis=0) for 2 <= M <= 524,288 samples per column.
//
// The analytic signal needs the exact length-M DFT (scipy pads nothing), and M is
// arbitrary (cortex_run.py's BOLD has 29,800 = 2^3 5^2 149 samples), so both DFTs
// are Bluestein convolutions over a power-of-two FFT of length
//   L = max(2^15, nextpow2(2 M - 1)):
//   X[k] = w[k] sum_n (x[n] w[n]) conj(w)[k - n],  w[k] = exp(-i pi k^2 / M),
// with k^2 reduced mod 2 M in integers before sincospi.  The inverse DFT is
// conj(DFT(conj(.))) / M, so one chirp and one chirp spectrum serve both.
//
// FFT_L is a four-step L = L1 L2 (n = L2 n1 + n2, k = k1 + L1 k2; L1, L2 <= 1024):
//   column pass: L1-point FFTs over n1 (stride L2), times W_L^(n2 k1)
//   row pass:    L2-point FFTs over n2 (contiguous)
// which leaves X[k1 + L1 k2] at position k1 L2 + k2.  A convolution does not care:
// the chirp spectrum is stored in the same order and the inverse runs the two
// passes backwards (rows, conjugate twiddle, columns) and lands in natural order.
// Passes that work on the same points are fused, so a column tile makes five trips
// through memory:
//   1. col  x w, zero padded -> FFT_L1, twiddle
//   2. row  FFT_L2, times the chirp spectrum, IFFT_L2, conjugate twiddle
//   3. col  IFFT_L1 -> conj(c) h / L (= conj(X h) w: the second DFT's input) -> FFT_L1, twiddle
//   4. row  as 2
//   5. col  IFFT_L1 -> conj(w) . = M times the analytic signal -> unit phasor, or modulus / M
// Work buffers are [L][tc] complex for a tile of tc columns (the columns of one
// point are contiguous), two of them, each pass reading one and writing the other.
// A workgroup (512 threads) owns 4096 points in LDS: G = 4096 / N sub-FFTs of length
// N, i.e. G neighbouring (n2, c) or (k1, c) items, whose points are G * 16
// contiguous bytes in memory.  The sub-FFT is an in-place Stockham (every read of a
// stage, barrier, every write, barrier), radix 4 with a leading radix-2 stage for
// odd log2 N (wc_bluestein.h's stages, shared with the Welch family and inlined here),
// twiddles from a 768-entry table of W_1024 in LDS; the inter-step
// twiddles are sincospi of the exact fraction (n2 k1 < L needs no reduction).
// No atomics, and a column's arithmetic does not depend on the tile it is in: the
// result is bit-identical for every workspace size and every C.
#define WC_BLUESTEIN_FFT_ONLY
#include "wc_bluestein.h"

namespace {

constexpr int64_t kMaxM = 524288;  // L = 2^20 = L1 L2 with L1 = L2 = 1024
constexpr int kMinLogL = 15;
constexpr int kPts = 4096;         // points per workgroup
constexpr int kTwN = 1024;         // sub-FFT twiddle base: T[j] = exp(-2 pi i j / 1024)
constexpr int kEpt = kPts / kThreads;  // points per thread on load / store

struct HlArgs {
    int64_t C, M, c0;  // columns of x, samples, first column of the tile
    int tc;            // columns of the tile
    int L, L2;         // FFT length, row length (L1 = L / L2)
    const double* x;   // [M][C]
    double* ph;        // [M][C][2] unit phasors, or [M][C] moduli (kColLastEnv)
    const d2* T;       // W_1024
    const d2* w;       // chirp [M]
    d2* Bf;            // chirp spectrum [L], position k1 L2 + k2
    const d2* src;     // [L][tc]
    d2* dst;           // [L][tc]
};

// scipy.signal.hilbert's spectral weights
__device__ __forceinline__ double hilbert_h(int64_t n, int64_t M) {
    if (n == 0 || (M % 2 == 0 && n == M / 2)) return 1.0;
    return n < (M + 1) / 2 ? 2.0 : 0.0;
}

__device__ __forceinline__ void load_tw(d2* T, const d2* Tg, int tid) {
    for (int j = tid; j < kTwLds; j += kThreads) T[j] = Tg[j];
}

enum { kColChirp = 0, kColFirst = 1, kColMid = 2, kColLast = 3, kColLastEnv = 4 };

// column pass: item q = n2 tc + c, points e = n1 (or k1) at n = e L2 + n2
template <int LOGN, int MODE>
__global__ void __launch_bounds__(kThreads) hl_col_kernel(const HlArgs a) {
    constexpr int N = 1 << LOGN, G = kPts / N, NP = N + 1, ES = kThreads / G;
    extern __shared__ __attribute__((aligned(16))) d2 hl_smem[];
    d2* z = hl_smem;
    d2* T = hl_smem + G * NP;
    const int tid = threadIdx.x;
    load_tw(T, a.T, tid);
    const int g = tid % G, e0 = tid / G;
    const int64_t q = (int64_t)blockIdx.x * G + g;
    const int n2 = (int)(q / a.tc), c = (int)(q % a.tc);
    d2* zg = z + g * NP;
#pragma unroll
    for (int j = 0; j < kEpt; ++j) {
        const int e = e0 + ES * j;
        const int64_t n = (int64_t)e * a.L2 + n2;
        d2 v = d2{0.0, 0.0};
        if constexpr (MODE == kColChirp) {  // conj(w) at n = m mod L, |m| < M
            const int64_t m = n < a.M ? n : (n > a.L - a.M ? a.L - n : -1);
            if (m >= 0) v = cconj(a.w[m]);
        } else if constexpr (MODE == kColFirst) {
            if (n < a.M) v = a.x[n * a.C + a.c0 + c] * a.w[n];
        } else {  // inverse sub-FFT as conj(FFT(conj(.)))
            v = cconj(a.src[n * a.tc + c]);
        }
        zg[e] = v;
    }
    __syncthreads();
    constexpr bool kLast = MODE == kColLast || MODE == kColLastEnv;
    if constexpr (MODE == kColMid || kLast) {
        fft_lds<LOGN, kPts, kTwN>(z, T, tid);  // F = conj(c) L, c = the circular convolution
        const double sc = 1.0 / (double)a.L;
#pragma unroll
        for (int j = 0; j < kEpt; ++j) {
            const int e = e0 + ES * j;
            const int64_t n = (int64_t)e * a.L2 + n2;
            const d2 F = zg[e];
            if constexpr (MODE == kColMid) {
                // X = w c; the next DFT's input conj(X h) w = conj(c) h (|w| = 1)
                zg[e] = n < a.M ? F * (sc * hilbert_h(n, a.M)) : d2{0.0, 0.0};
            } else if (n < a.M) {
                // analytic signal = conj(w c') / M, c' = conj(F) / L: phase of conj(w) F
                const d2 s = cmul(F, cconj(a.w[n])) * sc;
                // (sc is the second convolution's 1 / L; the inverse DFT's 1 / M is still owed)
                const double r = sqrt(s.x * s.x + s.y * s.y);
                if constexpr (MODE == kColLastEnv) {
                    a.ph[n * a.C + a.c0 + c] = r / (double)a.M;
                } else {
                    d2* o = reinterpret_cast<d2*>(a.ph) + n * a.C + a.c0 + c;
                    // numpy: angle(0) = 0; a NaN modulus is not 0 and gives a NaN phasor
                    *o = r == 0 ? d2{1.0, 0.0} : d2{s.x / r, s.y / r};
                }
            }
        }
        if constexpr (kLast) return;
        __syncthreads();
    }
    fft_lds<LOGN, kPts, kTwN>(z, T, tid);
#pragma unroll
    for (int j = 0; j < kEpt; ++j) {
        const int e = e0 + ES * j;
        const int64_t n = (int64_t)e * a.L2 + n2;
        double s, co;
        sincospi(2.0 * (double)((int64_t)n2 * e) / (double)a.L, &s, &co);  // W_L^(n2 k1), n2 k1 < L
        a.dst[n * a.tc + c] = cmul(zg[e], d2{co, -s});
    }
}

// row pass: item q = k1 tc + c, points e = n2 (or k2) at k1 L2 + e
template <int LOGN, bool CONV>
__global__ void __launch_bounds__(kThreads) hl_row_kernel(const HlArgs a) {
    constexpr int N = 1 << LOGN, G = kPts / N, NP = N + 1, ES = kThreads / G;
    extern __shared__ __attribute__((aligned(16))) d2 hl_smem[];
    d2* z = hl_smem;
    d2* T = hl_smem + G * NP;
    const int tid = threadIdx.x;
    load_tw(T, a.T, tid);
    const int g = tid % G, e0 = tid / G;
    const int64_t q = (int64_t)blockIdx.x * G + g;
    const int k1 = (int)(q / a.tc), c = (int)(q % a.tc);
    d2* zg = z + g * NP;
    const int64_t row = (int64_t)k1 * N;
#pragma unroll
    for (int j = 0; j < kEpt; ++j) {
        const int e = e0 + ES * j;
        zg[e] = a.src[(row + e) * a.tc + c];
    }
    __syncthreads();
    fft_lds<LOGN, kPts, kTwN>(z, T, tid);
    if constexpr (!CONV) {  // the chirp spectrum (tc = 1)
#pragma unroll
        for (int j = 0; j < kEpt; ++j) {
            const int e = e0 + ES * j;
            a.Bf[row + e] = zg[e];
        }
    } else {
#pragma unroll
        for (int j = 0; j < kEpt; ++j) {
            const int e = e0 + ES * j;
            zg[e] = cconj(cmul(zg[e], a.Bf[row + e]));
        }
        __syncthreads();
        fft_lds<LOGN, kPts, kTwN>(z, T, tid);
#pragma unroll
        for (int j = 0; j < kEpt; ++j) {
            const int e = e0 + ES * j;
            double s, co;
            sincospi(2.0 * (double)((int64_t)k1 * e) / (double)a.L, &s, &co);  // conj(W_L^(k1 n2))
            a.dst[(row + e) * a.tc + c] = cconj(cmul(zg[e], d2{co, -s}));
        }
    }
}

template <int N> constexpr size_t hl_lds_bytes() { return ((size_t)kPts + kPts / N + kTwLds) * sizeof(d2); }

// who names the entry point in messages, here and below
template <int LOGN, int MODE>
int launch_col(const char* who, const HlArgs& a, int64_t items, hipStream_t st) {
    constexpr int N = 1 << LOGN;
    auto kern = hl_col_kernel<LOGN, MODE>;
    if (int rc = wc_raise_lds(who, kern, hl_lds_bytes<N>())) return rc;
    hipLaunchKernelGGL(kern, dim3((unsigned)(items / (kPts / N))), dim3(kThreads), hl_lds_bytes<N>(), st, a);
    return WC_OK;
}
template <int LOGN, bool CONV>
int launch_row(const char* who, const HlArgs& a, int64_t items, hipStream_t st) {
    constexpr int N = 1 << LOGN;
    auto kern = hl_row_kernel<LOGN, CONV>;
    if (int rc = wc_raise_lds(who, kern, hl_lds_bytes<N>())) return rc;
    hipLaunchKernelGGL(kern, dim3((unsigned)(items / (kPts / N))), dim3(kThreads), hl_lds_bytes<N>(), st, a);
    return WC_OK;
}

template <int MODE>
int col_pass(const char* who, int log1, const HlArgs& a, hipStream_t st) {
    const int64_t items = (int64_t)a.L2 * a.tc;  // a multiple of G: L2 >= 128 >= G
    switch (log1) {
        case 8: return launch_col<8, MODE>(who, a, items, st);
        case 9: return launch_col<9, MODE>(who, a, items, st);
        default: return launch_col<10, MODE>(who, a, items, st);
    }
}
template <bool CONV>
int row_pass(const char* who, int log2, const HlArgs& a, hipStream_t st) {
    const int64_t items = (int64_t)(a.L / a.L2) * a.tc;
    switch (log2) {
        case 7: return launch_row<7, CONV>(who, a, items, st);
        case 8: return launch_row<8, CONV>(who, a, items, st);
        case 9: return launch_row<9, CONV>(who, a, items, st);
        default: return launch_row<10, CONV>(who, a, items, st);
    }
}

int hl_log_len(int64_t M) {  // log2 L, L = max(2^15, nextpow2(2 M - 1))
    int l = kMinLogL;
    while (((int64_t)1 << l) < 2 * M - 1) ++l;
    return l;
}
// workspace: W_1024 | chirp w [M] (padded to a 256-B multiple) | chirp spectrum [L] | 2 x [L][tc]
size_t hl_chirp_elems(int64_t M) { return (size_t)((M + 15) / 16 * 16); }
size_t hl_table_bytes(int64_t M, int64_t L) { return ((size_t)kTwN + hl_chirp_elems(M) + (size_t)L) * sizeof(d2); }

}  // namespace

size_t wc_hilbert_long_workspace_size(int64_t C, int64_t M) {
    if (C <= 0 || M < 2 || M > kMaxM) return 0;
    const int64_t L = (int64_t)1 << hl_log_len(M);
    return hl_table_bytes(M, L) + 2 * (size_t)L * sizeof(d2);
}

// the five passes over column tiles, for both outputs: out is phasor [M][C][2] (16-byte aligned) or,
// with envelope, env [M][C]; `who` names the entry point in messages
static int hl_run(const char* who, bool envelope, int64_t C, int64_t M, const double* x, double* out, void* workspace,
                  size_t ws_bytes, void* stream) {
    const int logL = hl_log_len(M), log1 = (logL + 1) / 2, log2 = logL / 2;  // 8..10, 7..10
    const int64_t L = (int64_t)1 << logL;
    const size_t tab = hl_table_bytes(M, L), per_col = 2 * (size_t)L * sizeof(d2);
    const char* size_fn = envelope ? "wc_hilbert_envelope_workspace_size" : "wc_hilbert_long_workspace_size";
    if (int rc = wc_check_workspace(who, size_fn, workspace, ws_bytes, tab + per_col)) return rc;
    const WcSpan al[2] = {{"workspace", workspace, 0, 16},  // d2 stores; env: doubles
                          {envelope ? "env" : "phasor", out, 0, envelope ? 8 : 16}};
    if (int rc = wc_check_align(who, al, 2)) return rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    d2* T = static_cast<d2*>(workspace);
    d2* w = T + kTwN;
    d2* Bf = w + hl_chirp_elems(M);
    d2* buf0 = Bf + L;
    const int64_t tcmax = (int64_t)std::min<size_t>((ws_bytes - tab) / per_col, (size_t)std::min<int64_t>(C, 1 << 20));

    hipLaunchKernelGGL(bs_twiddle_kernel<kTwN>, dim3(kTwN / 256), dim3(256), 0, st, T);
    hipLaunchKernelGGL(bs_chirp_kernel<int64_t>, dim3((unsigned)((M + 255) / 256)), dim3(256), 0, st, M, w);
    HlArgs a{C, M, 0, 1, (int)L, 1 << log2, x, out, T, w, Bf, nullptr, buf0};
    int rc = col_pass<kColChirp>(who, log1, a, st);
    a.src = buf0;
    if (rc == WC_OK) rc = row_pass<false>(who, log2, a, st);
    for (int64_t c0 = 0; c0 < C && rc == WC_OK; c0 += tcmax) {
        a.c0 = c0;
        a.tc = (int)std::min<int64_t>(tcmax, C - c0);
        d2* buf1 = buf0 + (size_t)L * a.tc;
        a.src = nullptr, a.dst = buf0;
        rc = col_pass<kColFirst>(who, log1, a, st);
        a.src = buf0, a.dst = buf1;
        if (rc == WC_OK) rc = row_pass<true>(who, log2, a, st);
        a.src = buf1, a.dst = buf0;
        if (rc == WC_OK) rc = col_pass<kColMid>(who, log1, a, st);
        a.src = buf0, a.dst = buf1;
        if (rc == WC_OK) rc = row_pass<true>(who, log2, a, st);
        a.src = buf1, a.dst = nullptr;
        if (rc == WC_OK) rc = envelope ? col_pass<kColLastEnv>(who, log1, a, st) : col_pass<kColLast>(who, log1, a, st);
    }
    return rc ? rc : wc_hip_check(who);
}

int wc_hilbert_phase_long(int64_t C, int64_t M, const double* x, double* phasor, void* workspace, size_t ws_bytes,
                          void* stream) {
    wc_clear_err();
    if (C <= 0 || M < 2 || !x || !phasor) return wc_fail(WC_EINVAL, "wc_hilbert_phase_long: bad arguments");
    if (M > kMaxM)
        return wc_fail(WC_EUNSUPPORTED, "wc_hilbert_phase_long: M > 524288 (the FFT length 2^20 = 1024 x 1024)");
    return hl_run("wc_hilbert_phase_long", false, C, M, x, phasor, workspace, ws_bytes, stream);
}

// wc_hilbert_envelope's long method (the entry point, its validation and the dispatch: wc_signal.hip)
int wc_hilbert_envelope_long(int64_t C, int64_t M, const double* x, double* env, void* workspace, size_t ws_bytes,
                             void* stream) {
    return hl_run("wc_hilbert_envelope", true, C, M, x, env, workspace, ws_bytes, stream);
}

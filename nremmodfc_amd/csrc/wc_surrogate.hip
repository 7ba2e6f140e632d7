// wc_surrogate.hip -- surrogate-tested functional connectivity for a batch of simulations on gfx950:
// the reference's probabilistic_thresholding (graph_utils.py:220-265) without a surrogate time series
// and without an inverse FFT.  The definitions, the phase stream included, are in include/wcsde.h and
// restated in numpy in tests/surrogate_reference.py.
//
// The real part of the inverse FFT of Y exp(i r), r the phases stacked over their own reverse, is the
// inverse FFT of the product's Hermitian part: with h = L/2 the surrogate of column n has the spectrum
//     X_n(k) = Y_n(k) (exp(i rv[k][n]) + exp(-i rv[k-1][n])) / 2   (1 <= k <= h - 1),
//     X_n(h) = Y_n(h) cos(rv[h-1][n]),
// and by Parseval its correlation matrix is the normalised Gram matrix of the L - 1 real rows
// sqrt(2) Re X(k), sqrt(2) Im X(k), X(h).  Y comes from wc_spectrogram (nperseg = L, one segment).
//
//   surrogate_fc_kernel    one workgroup per (simulation, surrogate), the S surrogates of a simulation
//                          next to each other in the grid so that its spectrum (216 KB at L = 298,
//                          N = 90) is read from HBM once and S - 1 times from L2.  kBins bins at a
//                          time: the phases of kBins + 1 rows of rv (one Philox block gives four
//                          nodes; cospi and sinpi of w 2^-31), the rotated rows into LDS, then the
//                          N x N products on v_mfma_f64_16x16x4_f64: the 16 x 16 tiles of the upper
//                          triangle (21 at N = 90) dealt to the four waves, four rows an instruction,
//                          both operands one double a lane from LDS.  The inner dimension is tiled
//                          (32 rows of at most 96 doubles), never whole.  (The register-blocked VALU
//                          form of wc_fcd.hip's window_pattern, 21 cells a thread, measured slower here:
//                          13.4 against 12.2 ms for 100,000 matrices of 90 nodes, docs/CHANGELOG.md.  It
//                          reads 12 doubles from LDS per 21 multiply-adds; a tile's MFMA reads two per 16.)
//   surrogate_test_kernel  one workgroup per matrix: mean and deviation over the surrogates per pair
//                          (two passes), p = 1 - Phi(z), then Benjamini-Hochberg in LDS: a bitonic
//                          sort of the p-values with 16-bit pair indices, p (P / rank), the running
//                          minimum from the top by doubling steps, the values put back by index, and
//                          the two symmetric matrices written row by row.
// Every sum has one fixed order and there are no atomics: a (simulation, surrogate) pair and a matrix
// give the same bits alone and anywhere in any batch.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include "wc_common.h"
#include "wc_device.h"

namespace {

constexpr int kMaxN = 96;
constexpr int kMaxL = 4096;
constexpr int kThreads = 256;      // surrogate_fc_kernel
constexpr int kTile = 16;          // side of a tile of the Gram matrix (v_mfma_f64_16x16x4_f64)
constexpr int kBins = 16;          // bins of the spectrum in LDS at a time: 2 kBins rows of the Gram product
constexpr int kTestThreads = 1024; // surrogate_test_kernel
constexpr int kPerThread = 8;      // sort entries a thread of it holds: 8192 >= nextpow2(4560)

// ---- wc_surrogate_fc: one workgroup per (simulation, surrogate) ----
template <int R>
__global__ void __launch_bounds__(kThreads) surrogate_fc_kernel(int N, int h, int S, size_t C,
                                                                const double2* __restrict__ spec,
                                                                const uint64_t* __restrict__ seeds,
                                                                double* __restrict__ sfc) {
    constexpr int Np = R * kTile;
    __shared__ double rows[2 * kBins][Np];            // the rotated bins: (re, im) of bin k0 + kk in rows 2 kk, 2 kk + 1
    __shared__ double cs[kBins + 1][Np], sn[kBins + 1][Np];  // cos, sin of rv[k0 - 1 + kk][n]
    __shared__ double isd[Np];                        // 1 / sqrt(g_nn)
    const int tid = threadIdx.x;
    const int b = blockIdx.x / S, s = blockIdx.x % S;
    const uint64_t seed = seeds[s];
    const double2* y = spec + (size_t)b * N;          // bin k of node n at y[k C + n]

    // tile q of the upper triangle, rows first, belongs to wave q % 4; a lane holds D[(lane >> 4) + 4 r][lane & 15]
    constexpr int T = R * (R + 1) / 2, M = (T + 3) / 4;   // tiles; tiles a wave at most
    const int wave = tid / 64, lane = tid % 64;
    int ti[M], tj[M];
    wcdev::f64x4 acc[M];
#pragma unroll
    for (int m = 0; m < M; ++m) {
        int q = min(wave + 4 * m, T - 1), i = 0;
        while (q >= R - i) {
            q -= R - i;
            ++i;
        }
        ti[m] = i;
        tj[m] = i + q;
        acc[m] = wcdev::f64x4{0.0, 0.0, 0.0, 0.0};
    }

    for (int k0 = 1; k0 <= h; k0 += kBins) {
        const int nb = min(kBins, h - k0 + 1);        // bins k0 .. k0 + nb - 1
        // rows k0 - 1 .. k0 + nb - 1 of rv, none past h - 1; one Philox block is four nodes
        const int np = min(nb + 1, h - k0 + 1);
        for (int task = tid; task < np * (Np / 4); task += kThreads) {
            const int kk = task / (Np / 4), q = task % (Np / 4);
            uint32_t w[4];
            wcdev::philox_ctr((uint64_t)(k0 - 1 + kk), (uint32_t)q, seed, w);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                double sv, cv;
                sincospi((double)w[j] * 4.656612873077392578125e-10, &sv, &cv);  // w 2^-31: 2 pi w 2^-32 = pi (w 2^-31)
                cs[kk][4 * q + j] = cv;
                sn[kk][4 * q + j] = sv;
            }
        }
        __syncthreads();
        for (int idx = tid; idx < nb * Np; idx += kThreads) {
            const int kk = idx / Np, n = idx % Np, k = k0 + kk;
            double2 v = make_double2(0.0, 0.0);
            if (n < N) v = y[(size_t)k * C + n];
            double re, im;
            if (k < h) {
                // (exp(i rv[k]) + exp(-i rv[k-1])) / 2; rv[k] is row kk + 1 of cs, sn
                const double cr = 0.5 * (cs[kk + 1][n] + cs[kk][n]), ci = 0.5 * (sn[kk + 1][n] - sn[kk][n]);
                re = M_SQRT2 * (v.x * cr - v.y * ci);
                im = M_SQRT2 * (v.x * ci + v.y * cr);
            } else {
                re = v.x * cs[kk][n];                 // Y(h) is real; rv[h - 1]
                im = 0.0;
            }
            rows[2 * kk][n] = re;
            rows[2 * kk + 1][n] = im;
        }
        if (nb & 1)                                   // whole groups of four rows: A[i][k] = rows[k][i], four k an MFMA
            for (int n = tid; n < 2 * Np; n += kThreads) rows[2 * nb + n / Np][n % Np] = 0.0;
        __syncthreads();
        for (int t0 = 0; t0 < 2 * nb; t0 += 4) {
            const double* r = rows[t0 + (lane >> 4)];
#pragma unroll
            for (int m = 0; m < M; ++m)
                if (wave + 4 * m < T)
                    acc[m] = __builtin_amdgcn_mfma_f64_16x16x4f64(r[16 * ti[m] + (lane & 15)], r[16 * tj[m] + (lane & 15)],
                                                                  acc[m], 0, 0, 0);
        }
        __syncthreads();
    }
#pragma unroll
    for (int m = 0; m < M; ++m)
        if (wave + 4 * m < T && ti[m] == tj[m]) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int row = (lane >> 4) + 4 * r;
                if (row == (lane & 15) && 16 * ti[m] + row < N) isd[16 * ti[m] + row] = 1.0 / sqrt(acc[m][r]);
            }
        }
    __syncthreads();
    double* out = sfc + (size_t)blockIdx.x * ((size_t)N * (N - 1) / 2);
#pragma unroll
    for (int m = 0; m < M; ++m)
        if (wave + 4 * m < T) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int i = 16 * ti[m] + (lane >> 4) + 4 * r, j = 16 * tj[m] + (lane & 15);
                if (i < j && j < N) out[i * N - i * (i + 1) / 2 + j - i - 1] = clip1(acc[m][r] * isd[i] * isd[j]);
            }
        }
}

// ---- wc_surrogate_test: one workgroup per matrix ----
// stats.norm.cdf's evaluation (Cephes ndtr)
__device__ __forceinline__ double norm_cdf(double z) {
    const double t = z * M_SQRT1_2, a = fabs(t);
    if (a < 1.0) return 0.5 + 0.5 * erf(t);
    const double y = 0.5 * erfc(a);
    return t > 0.0 ? 1.0 - y : y;
}

__device__ __forceinline__ int pair_index(int N, int i, int j) { return i * N - i * (i + 1) / 2 + j - i - 1; }

__global__ void __launch_bounds__(kTestThreads) surrogate_test_kernel(int N, int S, int n2, const double* __restrict__ fc,
                                                                     const double* __restrict__ sfc, double alpha,
                                                                     double* __restrict__ p_adj, double* __restrict__ fc_adj,
                                                                     double* __restrict__ mu_out, double* __restrict__ sd_out,
                                                                     double* __restrict__ p_out) {
    extern __shared__ __attribute__((aligned(16))) double lds[];
    double* key = lds;                                               // [n2] the p-values, sorted, adjusted, put back
    uint16_t* idx = reinterpret_cast<uint16_t*>(key + n2);           // [n2] the pair a sorted value belongs to
    uint8_t* row = reinterpret_cast<uint8_t*>(idx + n2);             // [P]  i of pair q
    __shared__ int bad;
    const int tid = threadIdx.x, b = blockIdx.x;
    const int P = N * (N - 1) / 2;
    const double* f = fc + (size_t)b * N * N;
    const double* sf = sfc + (size_t)b * S * P;

    if (tid == 0) bad = 0;
    for (int e = tid; e < N * N; e += kTestThreads) {
        const int i = e / N, j = e % N;
        if (i < j) row[pair_index(N, i, j)] = (uint8_t)i;
    }
    __syncthreads();
    for (int q = tid; q < n2; q += kTestThreads) {
        double p = INFINITY;                                         // the padding sorts last
        if (q < P) {
            const int i = row[q], j = q - pair_index(N, i, i + 1) + i + 1;
            double sum = 0.0;
            for (int s = 0; s < S; ++s) sum += sf[(size_t)s * P + q];
            const double mu = sum / S;
            double ss = 0.0;
            for (int s = 0; s < S; ++s) {
                const double d = sf[(size_t)s * P + q] - mu;
                ss = fma(d, d, ss);
            }
            const double sd = sqrt(ss / S);
            p = sd > 0.0 ? 1.0 - norm_cdf((f[i * N + j] - mu) / sd) : NAN;
            if (!isfinite(p)) bad = 1;
            if (mu_out) mu_out[(size_t)b * P + q] = mu;
            if (sd_out) sd_out[(size_t)b * P + q] = sd;
            if (p_out) p_out[(size_t)b * P + q] = p;
        }
        key[q] = p;
        idx[q] = (uint16_t)q;
    }
    __syncthreads();
    double* pa = p_adj + (size_t)b * N * N;
    double* fa = fc_adj + (size_t)b * N * N;
    if (bad) {                                                       // the same for every thread
        for (int e = tid; e < N * N; e += kTestThreads) {
            pa[e] = NAN;
            fa[e] = NAN;
        }
        return;
    }
    // bitonic sort, ascending; equal keys may come out in any order: they get equal results below
    for (int k = 2; k <= n2; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int t = tid; t < n2 / 2; t += kTestThreads) {
                const int lo = ((t & ~(j - 1)) << 1) | (t & (j - 1)), hi = lo + j;
                const double a = key[lo], c = key[hi];
                if ((a > c) == ((lo & k) == 0)) {
                    key[lo] = c;
                    key[hi] = a;
                    const uint16_t u = idx[lo];
                    idx[lo] = idx[hi];
                    idx[hi] = u;
                }
            }
            __syncthreads();
        }
    for (int r = tid; r < P; r += kTestThreads) key[r] *= (double)P / (double)(r + 1);
    __syncthreads();
    // key[r] = min over r' >= r by doubling steps (min is exact: the order does not matter)
    for (int d = 1; d < n2; d <<= 1) {
        double v[kPerThread];
#pragma unroll
        for (int m = 0; m < kPerThread; ++m) {
            const int e = tid + kTestThreads * m;
            v[m] = e + d < n2 ? key[e + d] : INFINITY;
        }
        __syncthreads();
#pragma unroll
        for (int m = 0; m < kPerThread; ++m) {
            const int e = tid + kTestThreads * m;
            if (e < n2) key[e] = fmin(key[e], v[m]);
        }
        __syncthreads();
    }
    {   // back in place: key[q] of pair q
        double v[kPerThread];
        int q[kPerThread];
#pragma unroll
        for (int m = 0; m < kPerThread; ++m) {
            const int e = tid + kTestThreads * m;
            v[m] = e < P ? fmin(key[e], 1.0) : 0.0;
            q[m] = e < P ? idx[e] : -1;
        }
        __syncthreads();
#pragma unroll
        for (int m = 0; m < kPerThread; ++m)
            if (q[m] >= 0) key[q[m]] = v[m];
        __syncthreads();
    }
    for (int e = tid; e < N * N; e += kTestThreads) {
        const int i = e / N, j = e % N;
        double pv = 0.0, fv = 0.0;
        if (i != j) {
            const int lo = min(i, j), hi = max(i, j);
            pv = key[pair_index(N, lo, hi)];
            fv = f[lo * N + hi] * (pv < alpha ? 1.0 : 0.0);
        }
        pa[e] = pv;
        fa[e] = fv;
    }
}

size_t test_lds_bytes(int n2, int P) { return (size_t)n2 * 10 + (((size_t)P + 15) & ~(size_t)15); }

// S >= 2, B S < 2^31 and the shapes both entries share; 0: fine
int check_shape(const char* fn, int B, int N, int S) {
    if (B < 1) return wc_fail(WC_EINVAL, "%s: B < 1", fn);
    if (N < 2) return wc_fail(WC_EINVAL, "%s: N < 2", fn);
    if (N > kMaxN) return wc_fail(WC_EUNSUPPORTED, "%s: N = %d > 96 (the products of one matrix per workgroup, in registers)", fn, N);
    if (S < 2) return wc_fail(WC_EINVAL, "%s: S = %d, needs at least 2 surrogates", fn, S);
    if ((int64_t)B * S > INT32_MAX) return wc_fail(WC_EINVAL, "%s: 2^31 surrogates or more (B times S)", fn);
    return WC_OK;
}

}  // namespace

extern "C" {

int wc_surrogate_fc(int B, int N, int L, int S, const double* spec, const uint64_t* seeds, double* sfc, void* stream) {
    wc_clear_err();
    const char* fn = "wc_surrogate_fc";
    if (int rc = check_shape(fn, B, N, S)) return rc;
    if (L < 4) return wc_fail(WC_EINVAL, "%s: L = %d < 4", fn, L);
    if (L & 1) return wc_fail(WC_EINVAL, "%s: L = %d is odd (the reference's stacked phases need an even length)", fn, L);
    if (L > kMaxL) return wc_fail(WC_EUNSUPPORTED, "%s: L = %d > 4096 (wc_spectrogram's longest segment)", fn, L);
    if (!spec || !seeds || !sfc) return wc_fail(WC_EINVAL, "%s: spec, seeds or sfc is NULL", fn);
    const size_t b = B, n = N, s = S, P = n * (n - 1) / 2, C = b * n;
    const WcSpan ins[2] = {{"spec", spec, (size_t)(L / 2 + 1) * C * 16, 16}, {"seeds", seeds, s * 8, 8}};
    const WcSpan outs[1] = {{"sfc", sfc, b * s * P * 8, 8}};
    if (int rc = wc_check_spans(fn, ins, 2, outs, 1)) return rc;
    const dim3 grid((unsigned)(B * S)), block(kThreads);
    hipStream_t st = static_cast<hipStream_t>(stream);
    const double2* y = reinterpret_cast<const double2*>(spec);
#define WC_SURR_LAUNCH(R) hipLaunchKernelGGL(surrogate_fc_kernel<R>, grid, block, 0, st, N, L / 2, S, C, y, seeds, sfc)
    switch ((N + kTile - 1) / kTile) {
        case 1: WC_SURR_LAUNCH(1); break;
        case 2: WC_SURR_LAUNCH(2); break;
        case 3: WC_SURR_LAUNCH(3); break;
        case 4: WC_SURR_LAUNCH(4); break;
        case 5: WC_SURR_LAUNCH(5); break;
        default: WC_SURR_LAUNCH(6); break;
    }
#undef WC_SURR_LAUNCH
    return wc_hip_check(fn);
}

int wc_surrogate_test(int B, int N, int S, const double* fc, const double* sfc, double alpha, double* p_adj,
                      double* fc_adj, double* mu, double* sd, double* p, void* stream) {
    wc_clear_err();
    const char* fn = "wc_surrogate_test";
    if (int rc = check_shape(fn, B, N, S)) return rc;
    if (!(alpha > 0.0 && alpha < 1.0)) return wc_fail(WC_EINVAL, "%s: alpha = %g, must lie in (0, 1)", fn, alpha);
    if (!fc || !sfc || !p_adj || !fc_adj) return wc_fail(WC_EINVAL, "%s: fc, sfc, p_adj or fc_adj is NULL", fn);
    const size_t b = B, n = N, s = S, P = n * (n - 1) / 2;
    const WcSpan ins[2] = {{"fc", fc, b * n * n * 8, 8}, {"sfc", sfc, b * s * P * 8, 8}};
    const WcSpan outs[5] = {{"p_adj", p_adj, b * n * n * 8, 8}, {"fc_adj", fc_adj, b * n * n * 8, 8},
                            {"mu", mu, b * P * 8, 8}, {"sd", sd, b * P * 8, 8}, {"p", p, b * P * 8, 8}};
    if (int rc = wc_check_spans(fn, ins, 2, outs, 5)) return rc;
    int n2 = 2;
    while (n2 < (int)P) n2 <<= 1;
    const size_t lds = test_lds_bytes(n2, (int)P);
    if (int rc = wc_raise_lds(fn, surrogate_test_kernel, lds)) return rc;
    hipLaunchKernelGGL(surrogate_test_kernel, dim3((unsigned)B), dim3(kTestThreads), lds, static_cast<hipStream_t>(stream),
                       N, S, n2, fc, sfc, alpha, p_adj, fc_adj, mu, sd, p);
    return wc_hip_check(fn);
}

}  // extern "C"

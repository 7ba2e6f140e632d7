// wc_leida.hip -- LEiDA (Leading Eigenvector Dynamics Analysis, Cabral et al. 2017) of a batch of
// simulations on gfx950: the leading eigenvector of every instantaneous phase-coherence matrix, k-means
// over the eigenvectors (assignment and centroid update), and the statistics of the resulting state
// sequences (occupancy, dwell time, transition matrix).  Nothing in the reference computes any of it;
// the definitions are in include/wcsde.h and restated in numpy in tests/leida_reference.py.
//
// wc_leida_eigvec   dPC(t) = c c^T + s s^T has rank <= 2: its non-zero eigenvalues are those of the 2 x 2
//                   Gram matrix [[cc, cs], [cs, ss]], in closed form, and its leading eigenvector is
//                   w0 c + w1 s for the Gram matrix's (w0, w1).  16 lanes per row up to N = 128 (four
//                   rows a wave), a wave per row beyond; lane l the nodes l, l + 16 (64), ..: the row is
//                   read once into registers (16 bytes a lane, contiguous over the row's lanes) and serves
//                   the three dot products, the norm and the output.  No LDS.
// wc_kmeans_assign  one workgroup per 64 rows; rows and centroids through LDS 32 nodes at a time (the n0
//                   loop of wc_fcd.hip's phase_kernel); wave g of the four keeps, for its lane's row, the
//                   centroids k = g, g + 4, ..; the distances meet in LDS and thread r scans them in k order.
// wc_kmeans_update  partial sums of every (block of 256 rows, k, node) into the workspace, one wave per
//                   (block, 64 nodes), its rows in order; then every (k, node) adds the blocks in index
//                   order.  Under the cosine metric a first kernel leaves every row's norm in the workspace.
// wc_state_stats    one workgroup per simulation, integer counters in LDS (integer atomics: the counts do
//                   not depend on their order), one division per output.
// Every floating-point sum has one fixed order that depends on the shape alone: a lane's nodes in
// ascending order, then the xor butterfly over the row's lanes (both operands of each stage commute, so
// every lane holds the same bits); a block's rows in order, then the blocks in order.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include "wc_common.h"

namespace {

constexpr int kMaxN = 1024;
constexpr int kMaxK = 32;
constexpr int kThreads = 256;
constexpr int kWave = 64;
constexpr int kEigRows = kThreads / kWave;   // rows of a workgroup of norms_kernel: a wave each
constexpr int kEigNarrow = 16;               // lanes a row of eigvec_kernel up to kEigNarrowN nodes (a wave beyond)
constexpr int kEigNarrowN = 8 * kEigNarrow;  // 128
constexpr int kAsgRows = 64;                 // rows of a workgroup of assign_kernel
constexpr int kAsgNc = 32;                   // nodes of its rows and centroids in LDS at a time
constexpr int kAsgKper = kMaxK / (kThreads / kWave);  // centroids a thread keeps: 8
constexpr int kUpdRows = WC_KMEANS_UPDATE_BLOCK;      // rows of a partial sum: 256
constexpr int64_t kLaunchBlocks = (int64_t)1 << 22;   // workgroups of one launch (chunks beyond it)

// Sum over aligned groups of LANES lanes of the wave, the same bits in every lane of a group.
template <int LANES>
__device__ __forceinline__ double group_sum(double v) {
#pragma unroll
    for (int o = LANES / 2; o > 0; o >>= 1) v += __shfl_xor(v, o, kWave);
    return v;
}
__device__ __forceinline__ double wave_sum(double v) { return group_sum<kWave>(v); }

// ---- wc_leida_eigvec: LANES lanes of a wave per row, PER = nodes a lane holds ----
// No lane leaves before the end, so every shuffle finds its partner; a degenerate row is a select at the store.
template <int LANES, int PER>
__global__ void __launch_bounds__(kThreads) eigvec_kernel(int64_t row0, int64_t rows, int N,
                                                          const double2* __restrict__ phasor,
                                                          double* __restrict__ vec, double* __restrict__ share) {
    const int lane = threadIdx.x % LANES;                 // within the row's lanes
    const int shift = (threadIdx.x % kWave) / LANES * LANES;  // where they begin in the wave
    const int64_t local = (int64_t)blockIdx.x * (kThreads / LANES) + threadIdx.x / LANES;
    const bool live = local < rows;
    const int64_t row = row0 + (live ? local : 0);
    const double2* z = phasor + row * N;
    double c[PER], s[PER];
    double cc = 0.0, ss = 0.0, cs = 0.0;
#pragma unroll
    for (int j = 0; j < PER; ++j) {
        const int n = lane + LANES * j;
        c[j] = s[j] = 0.0;  // past N: zeros, which add nothing to a sum
        if (live && n < N) {
            const double2 q = z[n];
            c[j] = q.x;
            s[j] = q.y;
        }
        cc = fma(c[j], c[j], cc);
        ss = fma(s[j], s[j], ss);
        cs = fma(c[j], s[j], cs);
    }
    cc = group_sum<LANES>(cc);
    ss = group_sum<LANES>(ss);
    cs = group_sum<LANES>(cs);
    const double tot = cc + ss;  // lambda1 + lambda2
    const double h = 0.5 * (cc - ss), r = hypot(h, cs);
    // a NaN or an infinity in the row (or squares that overflow), and lambda1 = lambda2: no leading vector
    const bool finite = tot < INFINITY, none = !finite || r == 0.0;
    // the Gram matrix's leading eigenvector, the form whose first or second entry does not cancel
    const double w0 = h >= 0.0 ? h + r : cs, w1 = h >= 0.0 ? cs : r - h;
    double nn = 0.0;
#pragma unroll
    for (int j = 0; j < PER; ++j) {
        c[j] = fma(w0, c[j], w1 * s[j]);
        nn = fma(c[j], c[j], nn);
    }
    const double norm = sqrt(group_sum<LANES>(nn));
    const uint64_t mine = (LANES == kWave ? ~0ull : ((1ull << (LANES % kWave)) - 1)) << shift;
    double sum = 0.0;
    int pos = 0;
#pragma unroll
    for (int j = 0; j < PER; ++j) {
        c[j] /= norm;
        sum += c[j];
        pos += __popcll(__ballot(c[j] > 0.0) & mine);  // padding is 0: never counted
    }
    sum = group_sum<LANES>(sum);
    // Cabral's rule: most entries negative; a draw decided by the sum
    const bool flip = 2 * pos > N || (2 * pos == N && sum > 0.0);
    if (!live) return;
    double* out = vec + row * N;
#pragma unroll
    for (int j = 0; j < PER; ++j)
        if (lane + LANES * j < N) out[lane + LANES * j] = none ? NAN : (flip ? -c[j] : c[j]);
    if (lane == 0) share[row] = none ? ((finite && tot > 0.0) ? 0.5 : NAN) : (0.5 * tot + r) / tot;
}

// ---- wc_kmeans_assign: one workgroup per kAsgRows rows ----
template <int METRIC>
__global__ void __launch_bounds__(kThreads) assign_kernel(int64_t row0, int64_t rows, int N, int K,
                                                          const double* __restrict__ x,
                                                          const double* __restrict__ cent,
                                                          int32_t* __restrict__ labels, double* __restrict__ dist) {
    __shared__ double xs[kAsgRows][kAsgNc + 1];
    __shared__ double cs[kMaxK][kAsgNc + 1];
    __shared__ double ds[kAsgRows][kMaxK + 1];
    const int tid = threadIdx.x, r = tid % kWave, g = tid / kWave;
    const int64_t first = (int64_t)blockIdx.x * kAsgRows;  // within the launch
    double acc[kAsgKper], cq[kAsgKper], xx = 0.0;
#pragma unroll
    for (int a = 0; a < kAsgKper; ++a) acc[a] = cq[a] = 0.0;
    for (int n0 = 0; n0 < N; n0 += kAsgNc) {
#pragma unroll
        for (int m = 0; m < kAsgRows * kAsgNc / kThreads; ++m) {
            const int idx = tid + kThreads * m, rr = idx / kAsgNc, nn = idx % kAsgNc, n = n0 + nn;
            // past N or the last row: zeros, which add nothing to a sum
            xs[rr][nn] = (n < N && first + rr < rows) ? x[(size_t)(row0 + first + rr) * N + n] : 0.0;
        }
#pragma unroll
        for (int m = 0; m < kMaxK * kAsgNc / kThreads; ++m) {
            const int idx = tid + kThreads * m, k = idx / kAsgNc, nn = idx % kAsgNc, n = n0 + nn;
            cs[k][nn] = (n < N && k < K) ? cent[(size_t)k * N + n] : 0.0;
        }
        __syncthreads();
#pragma unroll 4
        for (int nn = 0; nn < kAsgNc; ++nn) {
            const double xv = xs[r][nn];
            xx = fma(xv, xv, xx);
#pragma unroll
            for (int a = 0; a < kAsgKper; ++a) {
                const int k = g + (kThreads / kWave) * a;  // the same for the whole wave
                if (k < K) {
                    const double cv = cs[k][nn];
                    cq[a] = fma(cv, cv, cq[a]);
                    if (METRIC == WC_KMEANS_SQEUCLIDEAN) {
                        const double d = xv - cv;
                        acc[a] = fma(d, d, acc[a]);
                    } else {
                        acc[a] = fma(xv, cv, acc[a]);
                    }
                }
            }
        }
        __syncthreads();
    }
#pragma unroll
    for (int a = 0; a < kAsgKper; ++a) {
        const int k = g + (kThreads / kWave) * a;
        if (k < K) {
            // a centroid with a NaN or an infinity, or without a direction under cosine: NaN, never chosen
            const bool ok = cq[a] < INFINITY && (METRIC == WC_KMEANS_SQEUCLIDEAN || cq[a] > 0.0);
            const double d = METRIC == WC_KMEANS_SQEUCLIDEAN ? acc[a] : 1.0 - acc[a] / (sqrt(xx) * sqrt(cq[a]));
            ds[r][k] = ok ? d : NAN;
        }
    }
    __syncthreads();
    if (g == 0 && first + r < rows) {
        const bool ok = xx < INFINITY && (METRIC == WC_KMEANS_SQEUCLIDEAN || xx > 0.0);
        int lab = -1;
        double best = NAN;
        if (ok)
            for (int k = 0; k < K; ++k) {
                const double d = ds[r][k];
                if (d == d && (lab < 0 || d < best)) {  // strictly smaller: a tie stays with the lower k
                    lab = k;
                    best = d;
                }
            }
        labels[row0 + first + r] = lab;
        dist[row0 + first + r] = best;
    }
}

// ---- wc_kmeans_update under cosine, first: every row's norm, one wave per row ----
__global__ void __launch_bounds__(kThreads) norms_kernel(int64_t row0, int64_t rows, int N,
                                                         const double* __restrict__ x, double* __restrict__ norms) {
    const int lane = threadIdx.x % kWave;
    const int64_t local = (int64_t)blockIdx.x * kEigRows + threadIdx.x / kWave;
    if (local >= rows) return;
    const double* xr = x + (size_t)(row0 + local) * N;
    double q = 0.0;
    for (int n = lane; n < N; n += kWave) q = fma(xr[n], xr[n], q);
    q = sqrt(wave_sum(q));
    if (lane == 0) norms[row0 + local] = q;
}

// ---- wc_kmeans_update: one wave per (block of kUpdRows rows, 64 nodes); KB >= K accumulators ----
template <int KB>
__global__ void __launch_bounds__(kWave) update_partial_kernel(int64_t blk0, int tiles, int64_t R, int N, int K,
                                                               const double* __restrict__ x,
                                                               const int32_t* __restrict__ labels,
                                                               const double* __restrict__ norms,
                                                               double* __restrict__ part, int64_t* __restrict__ cnt) {
    const int lane = threadIdx.x, tile = blockIdx.x % tiles, n = tile * kWave + lane;
    const int64_t blk = blk0 + blockIdx.x / tiles;
    const int64_t r0 = blk * kUpdRows, r1 = r0 + kUpdRows < R ? r0 + kUpdRows : R;
    double acc[KB];
#pragma unroll
    for (int k = 0; k < KB; ++k) acc[k] = 0.0;
    int64_t members = 0;  // of cluster `lane`
#pragma unroll 8
    for (int64_t r = r0; r < r1; ++r) {  // loads ahead of the adds, which stay in order
        const int lab = labels[r];
        double v = n < N ? x[(size_t)r * N + n] : 0.0;
        if (norms) v /= norms[r];
        // the row goes to its own cluster and 0 to the others: adding 0 changes no bit, and a NaN of the
        // row stays out of the clusters it does not belong to
#pragma unroll
        for (int k = 0; k < KB; ++k) acc[k] += lab == k ? v : 0.0;
        members += lab == lane;
    }
    if (n < N) {
#pragma unroll
        for (int k = 0; k < KB; ++k)
            if (k < K) part[((size_t)blk * K + k) * N + n] = acc[k];
    }
    if (tile == 0 && lane < K) cnt[(size_t)blk * K + lane] = members;
}

// ---- wc_kmeans_update, last: the blocks in index order, one thread per (k, node) ----
__global__ void __launch_bounds__(kThreads) update_final_kernel(int64_t nblk, int N, int K,
                                                                const double* __restrict__ part,
                                                                const int64_t* __restrict__ cnt,
                                                                const double* __restrict__ prev,
                                                                double* __restrict__ cent, int64_t* __restrict__ count) {
    const int idx = blockIdx.x * kThreads + threadIdx.x;
    if (idx >= K * N) return;
    const int k = idx / N;
    int64_t c = 0;
    double s = 0.0;
#pragma unroll 8
    for (int64_t b = 0; b < nblk; ++b) {
        c += cnt[(size_t)b * K + k];
        s += part[(size_t)b * K * N + idx];
    }
    cent[idx] = c ? s / (double)c : prev[idx];  // an empty cluster keeps its centroid
    if (idx % N == 0) count[k] = c;
}

// ---- wc_state_stats: one workgroup per simulation ----
__global__ void __launch_bounds__(kThreads) state_stats_kernel(int b0, int B, int M, int K,
                                                               const int32_t* __restrict__ labels,
                                                               double* __restrict__ occupancy, double* __restrict__ dwell,
                                                               double* __restrict__ trans) {
    __shared__ int occ[kMaxK], runs[kMaxK], tr[kMaxK * kMaxK];
    const int tid = threadIdx.x, b = b0 + blockIdx.x;
    for (int i = tid; i < K * K; i += kThreads) tr[i] = 0;
    if (tid < K) occ[tid] = runs[tid] = 0;
    __syncthreads();
    auto label = [&](int t) {
        const int v = labels[(size_t)t * B + b];
        return (v < 0 || v >= K) ? -1 : v;  // anything but a state counts as -1 (include/wcsde.h)
    };
    for (int t = tid; t < M; t += kThreads) {
        const int l = label(t);
        if (l < 0) continue;
        atomicAdd(&occ[l], 1);
        if (t == 0 || label(t - 1) != l) atomicAdd(&runs[l], 1);  // a maximal run begins here
        if (t + 1 < M) {
            const int nx = label(t + 1);
            if (nx >= 0) atomicAdd(&tr[l * K + nx], 1);
        }
    }
    __syncthreads();
    for (int i = tid; i < K * K; i += kThreads) {
        int from = 0;
        for (int j = 0; j < K; ++j) from += tr[(i / K) * K + j];
        trans[(size_t)b * K * K + i] = from ? (double)tr[i] / (double)from : NAN;
    }
    if (tid < K) {
        int valid = 0;
        for (int j = 0; j < K; ++j) valid += occ[j];
        occupancy[(size_t)b * K + tid] = valid ? (double)occ[tid] / (double)valid : NAN;
        dwell[(size_t)b * K + tid] = occ[tid] ? (double)occ[tid] / (double)runs[tid] : NAN;
    }
}

// Shapes and limits of the k-means entry points; what == nullptr: no message (the workspace query).
int check_kmeans(const char* what, int64_t R, int N, int K, int metric) {
    const char* fmt = what ? "%s: %s" : nullptr;
    if (R < 1) return wc_fail(WC_EINVAL, fmt, what, "R < 1");
    if (R > WC_LEIDA_MAX_ROWS) return wc_fail(WC_EUNSUPPORTED, fmt, what, "R > WC_LEIDA_MAX_ROWS = 2^40 rows");
    if (N < 2) return wc_fail(WC_EINVAL, fmt, what, "N < 2");
    if (N > kMaxN) return wc_fail(WC_EUNSUPPORTED, fmt, what, "N > 1024");
    if (K < 1) return wc_fail(WC_EINVAL, fmt, what, "K < 1");
    if (K > kMaxK) return wc_fail(WC_EUNSUPPORTED, fmt, what, "K > 32");
    if (metric != WC_KMEANS_SQEUCLIDEAN && metric != WC_KMEANS_COSINE)
        return wc_fail(WC_EINVAL, fmt, what, "unknown metric (WC_KMEANS_SQEUCLIDEAN or WC_KMEANS_COSINE)");
    return WC_OK;
}

struct UpdateLayout {
    int64_t nblk;
    size_t part_bytes, cnt_bytes, norm_bytes;
};

UpdateLayout update_layout(int64_t R, int N, int K, int metric) {
    UpdateLayout u;
    u.nblk = (R + kUpdRows - 1) / kUpdRows;
    u.part_bytes = sizeof(double) * (size_t)u.nblk * K * N;
    u.cnt_bytes = sizeof(int64_t) * (size_t)u.nblk * K;
    u.norm_bytes = metric == WC_KMEANS_COSINE ? sizeof(double) * (size_t)R : 0;
    return u;
}

}  // namespace

extern "C" {

int wc_leida_eigvec(int64_t R, int N, const double* phasor, double* vec, double* share, void* stream) {
    wc_clear_err();
    if (R < 1) return wc_fail(WC_EINVAL, "wc_leida_eigvec: R < 1");
    if (R > WC_LEIDA_MAX_ROWS) return wc_fail(WC_EUNSUPPORTED, "wc_leida_eigvec: R > WC_LEIDA_MAX_ROWS = 2^40 rows");
    if (N < 2) return wc_fail(WC_EINVAL, "wc_leida_eigvec: N < 2");
    if (N > kMaxN) return wc_fail(WC_EUNSUPPORTED, "wc_leida_eigvec: N > 1024 (a row in one wave's registers)");
    if (!phasor || !vec || !share) return wc_fail(WC_EINVAL, "wc_leida_eigvec: phasor, vec or share is NULL");
    const size_t r = (size_t)R, n = (size_t)N;
    const WcSpan ins[1] = {{"phasor", phasor, r * n * 16, 16}};
    const WcSpan outs[2] = {{"vec", vec, r * n * 8, 8}, {"share", share, r * 8, 8}};
    if (int rc = wc_check_spans("wc_leida_eigvec", ins, 1, outs, 2)) return rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const double2* z = reinterpret_cast<const double2*>(phasor);
    // N <= 128: 16 lanes a row, four rows a wave (shorter butterflies, four rows' loads in flight a wave)
    const int lanes = N <= kEigNarrowN ? kEigNarrow : kWave, rows_wg = kThreads / lanes;
    const int per = (N + lanes - 1) / lanes;
    const int64_t per_launch = kLaunchBlocks * rows_wg;
    wc_chunks(R, per_launch, [&](int64_t r0, int64_t nr) {
        const dim3 grid((unsigned)((nr + rows_wg - 1) / rows_wg)), block(kThreads);
#define WC_EIG(L, P) hipLaunchKernelGGL((eigvec_kernel<L, P>), grid, block, 0, st, r0, nr, N, z, vec, share)
        if (lanes == kEigNarrow) {
            if (per <= 1) WC_EIG(kEigNarrow, 1);
            else if (per <= 2) WC_EIG(kEigNarrow, 2);
            else if (per <= 4) WC_EIG(kEigNarrow, 4);
            else if (per <= 6) WC_EIG(kEigNarrow, 6);
            else WC_EIG(kEigNarrow, 8);
        } else {
            if (per <= 4) WC_EIG(kWave, 4);
            else if (per <= 8) WC_EIG(kWave, 8);
            else WC_EIG(kWave, 16);
        }
#undef WC_EIG
    });
    return wc_hip_check("wc_leida_eigvec");
}

int wc_kmeans_assign(int64_t R, int N, int K, const double* x, const double* cent, int metric, int32_t* labels,
                     double* dist, void* stream) {
    wc_clear_err();
    if (int rc = check_kmeans("wc_kmeans_assign", R, N, K, metric)) return rc;
    if (!x || !cent || !labels || !dist)
        return wc_fail(WC_EINVAL, "wc_kmeans_assign: x, cent, labels or dist is NULL");
    const size_t r = (size_t)R, n = (size_t)N, k = (size_t)K;
    const WcSpan ins[2] = {{"x", x, r * n * 8, 8}, {"cent", cent, k * n * 8, 8}};
    const WcSpan outs[2] = {{"labels", labels, r * 4, 4}, {"dist", dist, r * 8, 8}};
    if (int rc = wc_check_spans("wc_kmeans_assign", ins, 2, outs, 2)) return rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    wc_chunks(R, kLaunchBlocks * kAsgRows, [&](int64_t r0, int64_t nr) {
        const dim3 grid((unsigned)((nr + kAsgRows - 1) / kAsgRows)), block(kThreads);
        if (metric == WC_KMEANS_SQEUCLIDEAN)
            hipLaunchKernelGGL(assign_kernel<WC_KMEANS_SQEUCLIDEAN>, grid, block, 0, st, r0, nr, N, K, x, cent, labels,
                               dist);
        else
            hipLaunchKernelGGL(assign_kernel<WC_KMEANS_COSINE>, grid, block, 0, st, r0, nr, N, K, x, cent, labels, dist);
    });
    return wc_hip_check("wc_kmeans_assign");
}

size_t wc_kmeans_workspace_size(int64_t R, int N, int K, int metric) {
    if (check_kmeans(nullptr, R, N, K, metric)) return 0;
    const UpdateLayout u = update_layout(R, N, K, metric);
    return u.part_bytes + u.cnt_bytes + u.norm_bytes;
}

int wc_kmeans_update(int64_t R, int N, int K, const double* x, const int32_t* labels, const double* cent_prev,
                     int metric, double* cent, int64_t* count, void* workspace, size_t ws_bytes, void* stream) {
    wc_clear_err();
    if (int rc = check_kmeans("wc_kmeans_update", R, N, K, metric)) return rc;
    if (!x || !labels || !cent_prev || !cent || !count)
        return wc_fail(WC_EINVAL, "wc_kmeans_update: x, labels, cent_prev, cent or count is NULL");
    const char* fn = "wc_kmeans_update";
    const size_t r = (size_t)R, n = (size_t)N, k = (size_t)K;
    const WcSpan ins[3] = {{"x", x, r * n * 8, 8}, {"labels", labels, r * 4, 4}, {"cent_prev", cent_prev, k * n * 8, 8}};
    const WcSpan outs[2] = {{"cent", cent, k * n * 8, 8}, {"count", count, k * 8, 8}};
    const WcSpan ws = {"workspace", workspace, ws_bytes, 8};
    if (int rc = wc_check_align(fn, &ws, 1)) return rc;
    if (int rc = wc_check_spans(fn, ins, 3, outs, 2)) return rc;
    const UpdateLayout u = update_layout(R, N, K, metric);
    const size_t need = u.part_bytes + u.cnt_bytes + u.norm_bytes;
    if (int rc = wc_check_workspace(fn, "wc_kmeans_workspace_size", workspace, ws_bytes, need)) return rc;
    if (int rc = wc_check_alias(fn, &ws, 1, ins, 3)) return rc;
    if (int rc = wc_check_alias(fn, &ws, 1, outs, 2)) return rc;
    // the minimum is all that is ever used: the result cannot depend on what lies beyond it
    double* part = static_cast<double*>(workspace);
    int64_t* cnt = reinterpret_cast<int64_t*>(static_cast<char*>(workspace) + u.part_bytes);
    double* norms = u.norm_bytes ? reinterpret_cast<double*>(static_cast<char*>(workspace) + u.part_bytes + u.cnt_bytes)
                                 : nullptr;
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (norms)
        wc_chunks(R, kLaunchBlocks * kEigRows, [&](int64_t r0, int64_t nr) {
            hipLaunchKernelGGL(norms_kernel, dim3((unsigned)((nr + kEigRows - 1) / kEigRows)), dim3(kThreads), 0, st, r0,
                               nr, N, x, norms);
        });
    const int tiles = (N + kWave - 1) / kWave;  // <= 16
    wc_chunks(u.nblk, kLaunchBlocks / 16, [&](int64_t b0, int64_t nbk) {
        const dim3 grid((unsigned)(nbk * tiles)), block(kWave);
        if (K <= 4)
            hipLaunchKernelGGL(update_partial_kernel<4>, grid, block, 0, st, b0, tiles, R, N, K, x, labels, norms, part, cnt);
        else if (K <= 8)
            hipLaunchKernelGGL(update_partial_kernel<8>, grid, block, 0, st, b0, tiles, R, N, K, x, labels, norms, part, cnt);
        else if (K <= 16)
            hipLaunchKernelGGL(update_partial_kernel<16>, grid, block, 0, st, b0, tiles, R, N, K, x, labels, norms, part,
                               cnt);
        else
            hipLaunchKernelGGL(update_partial_kernel<32>, grid, block, 0, st, b0, tiles, R, N, K, x, labels, norms, part,
                               cnt);
    });
    hipLaunchKernelGGL(update_final_kernel, dim3((unsigned)((K * N + kThreads - 1) / kThreads)), dim3(kThreads), 0, st,
                       u.nblk, N, K, part, cnt, cent_prev, cent, count);
    return wc_hip_check("wc_kmeans_update");
}

int wc_state_stats(int B, int M, int K, const int32_t* labels, double* occupancy, double* dwell, double* trans,
                   void* stream) {
    wc_clear_err();
    if (B < 1) return wc_fail(WC_EINVAL, "wc_state_stats: B < 1");
    if (M < 1) return wc_fail(WC_EINVAL, "wc_state_stats: M < 1");
    if (K < 1) return wc_fail(WC_EINVAL, "wc_state_stats: K < 1");
    if (K > kMaxK) return wc_fail(WC_EUNSUPPORTED, "wc_state_stats: K > 32");
    if (!labels || !occupancy || !dwell || !trans)
        return wc_fail(WC_EINVAL, "wc_state_stats: labels, occupancy, dwell or trans is NULL");
    const size_t b = (size_t)B, m = (size_t)M, k = (size_t)K;
    const WcSpan ins[1] = {{"labels", labels, m * b * 4, 4}};
    const WcSpan outs[3] = {{"occupancy", occupancy, b * k * 8, 8}, {"dwell", dwell, b * k * 8, 8},
                            {"trans", trans, b * k * k * 8, 8}};
    if (int rc = wc_check_spans("wc_state_stats", ins, 1, outs, 3)) return rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    wc_chunks(B, kLaunchBlocks, [&](int64_t b0, int64_t nb) {
        hipLaunchKernelGGL(state_stats_kernel, dim3((unsigned)nb), dim3(kThreads), 0, st, (int)b0, B, M, K, labels,
                           occupancy, dwell, trans);
    });
    return wc_hip_check("wc_state_stats");
}

}  // extern "C"

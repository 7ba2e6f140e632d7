/*
 * wcsde.h -- C ABI of libwcsde.so, the MI355X (gfx950) Wilson-Cowan SDE sweep
 * engine.  Plain pointers and sizes only; no torch types cross this boundary.
 *
 * The reference (vandal-uv/NREMmodFC) has no FFI: its boundary is the Python
 * module surface of netwWilsonCowanPlastic.  Each entry point
 * below replaces one piece of that surface; the Python mirror in
 * nremmodfc_amd/ (netwWilsonCowanPlastic.py, utils.py, sweep.py) binds them
 * with ctypes (INTEGRATION.md shows the binding).
 *
 * Conventions
 *  - every array argument is DEVICE memory owned by the caller (e.g. a
 *    torch.cuda tensor's data_ptr()), contiguous, batch-major unless stated;
 *  - no allocation inside a call; work is enqueued on `stream` (a hipStream_t,
 *    NULL = default stream) and the call returns without host synchronisation
 *    (the one call that waits for the stream is wc_integrate_status, whose
 *    result is a host value);
 *  - return 0 on success or a negative WC_E* code; wc_last_error() gives a
 *    thread-local message for the last failure on the calling thread;
 *  - reentrant: no global mutable state.
 */
#ifndef WCSDE_H
#define WCSDE_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define WCSDE_ABI_VERSION 7

/* Noise stream (the reference's numba RNG is seeded from os.urandom and never
 * reproducible; the build defines its own): Philox4x32-10 with
 * key (WC_PHILOX_KEY0, WC_PHILOX_KEY1) and counter
 *   (step & 0xffffffff, ((step >> 32) << 16) | quad, simkey lo32, simkey hi32)
 * for global Euler step `step` (< 2^48), node quad `quad` = node / 4 (< 2^16)
 * and the 64-bit per-simulation key; outputs x0..x3 ->
 *   u = (2*(x >> 9) + 1) * 2^-24,
 *   z[4q+0,1] = sqrt(-2 ln u0) (cos, sin)(2 pi u1),  z[4q+2,3] likewise from u2, u3,
 * and the noise of wc:80 is sqdtD * z. */
#define WC_PHILOX_KEY0 0x243F6A88u
#define WC_PHILOX_KEY1 0x85A308D3u

enum wc_precision { WC_F32 = 0, WC_F64 = 1 };

enum wc_error {
    WC_OK = 0,
    WC_EINVAL = -1,     /* bad shape / argument */
    WC_EUNSUPPORTED = -2, /* size outside what the kernels support */
    WC_EWORKSPACE = -3, /* workspace NULL or too small */
    WC_EHIP = -4        /* a HIP runtime call failed */
};

/* Node/model constants of netwWilsonCowanPlastic.py:20-57 (drivers override P
 * and rhoE, whole_sweep_both.py:39-40).  sqdtD = D/sqrt(dtSim) is the std of
 * the per-step noise drawn inside the E sigmoid (wc:55-57, wc:80-81). */
typedef struct wc_params {
    double a_ee, a_ei, a_ii;
    double tauE, tauI;
    double P, rhoE;
    double rE, rI, mu, sigmaI;
    double sqdtD;
    double dtSim;
} wc_params;

int wcsde_abi_version(void);
const char* wc_last_error(void);

/* Bytes of device workspace wc_integrate needs for B simulations of an N-node
 * connectome.  N <= 96: the connectome's MFMA A-operand image only (state stays
 * in registers for the whole call).  N > 96: the A-operand image plus the
 * tile-major state image and the double-buffered E operand (32 B per
 * node-simulation in fp32, padded to multiples of 64 nodes and simulations). */
size_t wc_workspace_size(int B, int N, int precision);

/*
 * Advance B independent simulations by `nsteps` Euler-Maruyama steps of the
 * plastic Wilson-Cowan network.  Replaces the per-step work of
 * netwWilsonCowanPlastic.wilsonCowan (wc:77-83) and the three Euler loops of
 * run() (wc:101-135); the host calls it once per phase/chunk with that
 * phase's tau_ip (0.05, 1, 2: wc:95,110,118).
 *
 *  sc        [N][N] fp64     structural connectome CM (row i = target node)
 *  G,sigmaE  [B][N] fp64     per-simulation, per-node coupling and E slope
 *                            (homogeneous sweeps repeat one value per row;
 *                            maps mode G_i = G + dG*m_i, whole_sweep_both_maps.py:104-108)
 *  keys      [B]    uint64   Philox4x32-10 key of each simulation's noise stream
 *  E,I,A     [B][N] fp64     state (E, I, a_ie), read at entry, written at exit
 *  step0                     global step index of the first step (Philox counter)
 *  rec_every >0: store the state BEFORE the update of every local step s with
 *            s % rec_every == 0 (wc:124-125) as record k = s/rec_every in
 *            recE/recI/recA, element type float (WC_F32) or double (WC_F64);
 *            recI/recA may be NULL.  rec_every == 0: no recording.
 *  rec_ld    0: records time-major [n_rec][B][N] (Y_t[:, k, :] of run());
 *            > 0: node-major, record k of column c = b*N + n at c*rec_ld + k
 *            (a slot of the sweep pipeline's E ring, read by BOLD and Welch).
 *  precision WC_F32: E, I, sigmoids in fp32; coupling CM.E on the fp16 MFMA:
 *            CM*sA and E*2^10 each split into two fp16 parts (hi + lo, 22
 *            significant bits), three cross terms (lo.hi, hi.lo, hi.hi) with
 *            fp32 accumulation, 1/(2^10 sA) folded into G; a_ie as a
 *            compensated fp32 pair;
 *            WC_F64: everything fp64 (the parity mode).
 *  N <= 96   one launch integrates all nsteps with the state in registers;
 *  N > 96    fp32, nsteps > 1 (the default): ONE persistent cooperative launch
 *            (wc_sde_large.hip persist_kernel) -- one workgroup per CU owns 128
 *            nodes x 80 simulations with their state in registers for all nsteps;
 *            the 8 node blocks of a simulation block exchange the E operand image
 *            through the workspace every step (bounded waits).  If the grid cannot
 *            be made co-resident (cooperative launch refused: too many blocks, or
 *            the CUs are shared) or WCSDE_PERSISTENT=0, and for fp64: one
 *            GEMM-shaped launch per Euler step (step_kernel), the state in the
 *            workspace between steps.  Both give the same bits.  Every wait of
 *            the persistent path is bounded: one that times out sets the
 *            workspace's status word and poisons E, I, A with NaN (carried by
 *            every later call on that state); wc_integrate_status reports it.
 *            Same noise stream on every path.
 */
int wc_integrate(const wc_params* p, int precision, int B, int N,
                 const double* sc, const double* G, const double* sigmaE,
                 const uint64_t* keys, double* E, double* I, double* A,
                 int64_t step0, int64_t nsteps, double tau_ip,
                 int64_t rec_every, int64_t rec_ld, void* recE, void* recI, void* recA,
                 void* workspace, size_t ws_bytes, void* stream);

/* Status of the last wc_integrate call on `workspace` (same B, N, precision):
 * waits for `stream`, then returns WC_EHIP if that call's persistent N > 96
 * integrator had an inter-workgroup wait time out (its E, I, A are NaN), else 0.
 * The one wc_integrate-side call that synchronises; call it when the results are
 * needed anyway (the sweep pipeline: once per batch).  A timed-out call's NaN
 * state propagates through every later call, so a check at the end of a batch
 * also covers its earlier calls (the NaN state or this word).  N <= 96: waits
 * for the stream and returns 0. */
int wc_integrate_status(const void* workspace, int B, int N, int precision, void* stream);

/* Standard normals the integrator draws at global step `step`: out [B][N]
 * (float or double per precision).  Test hook for the noise stream. */
int wc_noise(int precision, int B, int N, const uint64_t* keys, int64_t step,
             void* out, void* stream);

/* One evaluation of netwWilsonCowanPlastic.wilsonCowan(t, X, sigmaE, mu, tau_ip, G)
 * (wc:77-83), fp64, for B simulations: X [B][3][N] rows (E, I, a_ie) -> out
 * [B][3][N] = (dE/dt, dI/dt, da_ie/dt).  The noise of wc:80 is sqdtD times the
 * normals of Philox step `step` of each key (the integrator's normals at that
 * global step); p->mu is the call's mu.  G, sigmaE [B][N]; sc [N][N]. */
int wc_rhs(const wc_params* p, int B, int N, const double* sc, const double* G,
           const double* sigmaE, const uint64_t* keys, int64_t step, double tau_ip,
           const double* X, double* out, void* stream);

/* ------------------------------------------------------------------------
 * simBOLD (netwWilsonCowanPlastic.py:140-158), streamed.
 * Columns c = b*N + n.  The caller allocates wc_bold_state_doubles() doubles
 * of device state, calls wc_bold_init once, wc_bold_chunk for consecutive
 * sample ranges [t0, t0+Tc) of the E trajectory (any chunking), and
 * wc_bold_finish once every sample 0..n_total-1 has been fed: out [M][C] is
 * filtfilt(b, a, BOLD[neq:], axis=0)[::dec], M = ceil((n_total-neq)/dec).
 * BOLD = Balloon-Windkessel of E at step dt (assumed form of the missing
 * BOLDModel.BD.Sim). */
typedef struct wc_bold_cfg {
    double dt;        /* BOLD Euler step: dt*downsamp = 0.04 (wc:144, wc:148) */
    int64_t neq;      /* leading samples dropped (Neq = 2000, wc:145) */
    int64_t n_total;  /* samples of E_t (len(wc.time) = 300000) */
    int64_t dec;      /* BOLD_downsamp (1000; cortex_run.py uses 10) */
    double b[5], a[5]; /* band-pass, a[0] = 1: bessel(2, [2*.01*dt, 2*.1*dt], 'bandpass') (wc:152) */
    double zi[4];     /* scipy.signal.lfilter_zi(b, a) */
} wc_bold_cfg;

int64_t wc_bold_blocks(const wc_bold_cfg* cfg);
size_t wc_bold_state_doubles(const wc_bold_cfg* cfg, int64_t C);
int wc_bold_init(const wc_bold_cfg* cfg, int64_t C, double* state, void* stream);
/* E: float (e_f64 = 0) or double; e_ld == 0: time-major [Tc][C]; e_ld > 0:
 * node-major, sample tt of column c at E[c*e_ld + tt].
 * copy (optional, fp32 time-major E only): the chunk is also written
 * node-major, sample tt of column c at copy[c*copy_ld + tt] (copy_ld >= Tc;
 * 16-B row stores when copy is 16-B aligned and copy_ld % 4 == 0) -- the
 * transposition the Welch stage needs, done in the same pass as the BOLD
 * stream through an LDS tile with full-line stores.
 * NULL: no copy. */
int wc_bold_chunk(const wc_bold_cfg* cfg, int64_t C, const void* E, int e_f64, int64_t e_ld,
                  int64_t t0, int64_t Tc, double* state, void* copy, int64_t copy_ld, void* stream);
int wc_bold_finish(const wc_bold_cfg* cfg, int64_t C, const double* state, double* out, void* stream);

/* Hierarchical module analysis of B FC matrices, batched (run_many_seeds.py:
 * 130-133 over HMA.Functional_HP / Balance / nodal_measures, HMA.py:30-203).
 * fc [B][N][N] fp64 (N <= 96): read, then clipped in place (FC[FC < 0] = 0,
 * as HMA.py:55 does to the caller's matrix).  Outputs: hin[B], hse[B]
 * (Balance), hin_node[B][N], hse_node[B][N] (nodal_measures); optional
 * clus_num [B][N-1] int32 (Functional_HP's Clus_num) and sv [B][N] (singular
 * values of the symmetrised positive part, descending).  Eigen-decomposition
 * by cyclic Jacobi in LDS, one workgroup per matrix.
 * Non-finite entries: the clip comes first, so -Inf becomes 0 and a NaN stays.  A
 * matrix that then holds a NaN or +Inf gets NaN in hin, hse, hin_node, hse_node
 * and sv and -1 in every clus_num; its NaN and +Inf entries stay in fc.  The other
 * matrices of the batch are not affected. */
int wc_hma(int B, int N, double* fc, double* hin, double* hse, double* hin_node, double* hse_node,
           int* clus_num, double* sv, void* stream);

/* The same outputs for any N >= 3 (N > 96: the matrix does not fit the Jacobi's
 * LDS) from the eigensystem of F = (max(FC,0) + max(FC,0)^T)/2 computed by the
 * caller on the device: lam [B][N] eigenvalues (any order), vt [B][N][N] with row
 * j the eigenvector of lam[j].  Ranks |lam| (stable, descending), walks the
 * levels (HMA.py:62-101), Balance and nodal_measures as wc_hma.  N <= 4096
 * (the label arrays take 40 B per node of the 160 KB LDS; larger N returns
 * WC_EUNSUPPORTED).  A matrix with a NaN or infinite value in lam gets NaN in
 * every floating output and -1 in every clus_num, without a ranking (vt is not
 * read): a caller marks a matrix that is not finite this way and keeps it from
 * its eigensolver. */
int wc_hma_modes(int B, int N, const double* lam, const double* vt, double* hin, double* hse,
                 double* hin_node, double* hse_node, int* clus_num, double* sv, void* stream);

/* ------------------------------------------------------------------------
 * SC optimiser (optimize_SC_Hopf.py:47-104), SURVEY.md 8f rank 4.
 * The Hopf (Stuart-Landau) network of Hopf_model_multi.py:46-156, batched over
 * simulations (random seeds):
 *   x' = (a - x^2 - y^2) x - w y + sum_j (G M_ij / norm) (x_j - x_i)
 *   y' = (a - x^2 - y^2) y + w x + sum_j (G M_ij / norm) (y_j - y_i)
 *   state += f dt + beta z sqrt(dt)    (Euler-Maruyama, :143-144)
 * fp64.  Noise: the Philox stream above with the simulation key; node i's
 * (x, y) normals are the Box-Muller pair (2i, 2i+1), i.e. quad i/2.
 * x, y [B][N] in/out; when rec_every > 0, x BEFORE every local step s with
 * s % rec_every == 0 is stored at rec[s / rec_every][B][N] (and y at rec_y,
 * which may be NULL): a run recorded from its first step gives the
 * reference's results[k] = state after k*downsamp steps (:140-149).  M is N x N
 * (row i = inputs of node i); workspace >= wc_hopf_workspace_size(B, N): the
 * weight image and one segment (512 steps) of pre-generated normals. */
typedef struct wc_hopf_params {
    double a;     /* bifurcation parameter (Hopf_model_multi.py:22) */
    double w;     /* angular frequency, 0.05 * 2 pi (:23) */
    double beta;  /* noise scale (:25) */
    double dt;    /* Euler step (:28) */
    double G;     /* global coupling (:38; optimize_SC_Hopf.py:39) */
    double norm;  /* mean column sum of M (:37, optimize_SC_Hopf.py:30,101) */
} wc_hopf_params;

size_t wc_hopf_workspace_size(int B, int N);
int wc_hopf_integrate(const wc_hopf_params* p, int B, int N, const double* M, const uint64_t* keys,
                      double* x, double* y, int64_t step0, int64_t nsteps, int64_t rec_every,
                      double* rec, double* rec_y, void* workspace, size_t ws_bytes, void* stream);

/* scipy.signal.filtfilt(b, a, x, axis=0) of every column of x [T][C] fp64 ->
 * y [T][C] (y must not alias x): odd extension of padlen = 3 (order + 1),
 * lfilter_zi initial conditions zi[order] (host, from the caller), DF2T in
 * scipy's association order.  1 <= order <= 8 (utils.envelope's low-pass is
 * order 3); T must exceed padlen; b, a, zi are HOST arrays of order + 1,
 * order + 1 and order doubles, a[0] == 1.
 * (optimize_SC_Hopf.py:63-66, utils.py:145-154; also any simBOLD-style band-pass.) */
int wc_filtfilt(int order, const double* b, const double* a, const double* zi, int64_t T, int64_t C,
                const double* x, double* y, void* stream);

/* Unit phasors exp(i angle(hilbert(x, axis=0))) of every column of x [M][C]
 * (utils.kuramoto, utils.py:35-37): phasor [M][C][2] (cos, sin).  workspace:
 * >= M doubles.  Range: 2 <= M <= 8192.  It is a direct circulant convolution,
 * O(M^2) per column, with the length-M Hilbert kernel in LDS (M * 8 bytes of a
 * 64 KB launch); longer series return WC_EUNSUPPORTED: use wc_hilbert_phase_long.
 * A sample whose analytic signal is exactly 0 has the phasor (1, 0) (numpy's
 * angle(0) = 0).  A NaN or infinite sample makes phasors of its column NaN (every
 * one of them for a NaN), never (1, 0), and touches no other column. */
int wc_hilbert_phase(int64_t C, int M, const double* x, double* phasor, void* workspace,
                     size_t ws_bytes, void* stream);

/* The same phasors for long series, 2 <= M <= 524288, in O(M log M): the exact
 * length-M DFT and its inverse (scipy.signal.hilbert pads nothing) as Bluestein
 * convolutions over a power-of-two FFT of length L = max(2^15, nextpow2(2 M - 1))
 * (wc_hilbert.hip).  phasor [M][C][2] as above (16-byte aligned, as workspace).
 * wc_hilbert_long_workspace_size is the minimum: the tables (W_1024, the chirp
 * and its spectrum) and two [L] complex buffers for one column; every further
 * 32 L bytes let one more column be in flight per pass (up to C), and the result
 * is bit-identical for every workspace size and every C.  0 for C <= 0, M < 2 or
 * M > 524288 (wc_hilbert_phase_long then returns WC_EINVAL / WC_EUNSUPPORTED).
 * Zero, NaN and infinite samples as wc_hilbert_phase. */
size_t wc_hilbert_long_workspace_size(int64_t C, int64_t M);
int wc_hilbert_phase_long(int64_t C, int64_t M, const double* x, double* phasor, void* workspace,
                          size_t ws_bytes, void* stream);

/* |scipy.signal.hilbert(x, axis=0)| of every column of x [M][C] fp64 -> env
 * [M][C] fp64 (utils.envelope, utils.py:149), 2 <= M <= 524288.  method: 1 =
 * the direct convolution of wc_hilbert_phase (M <= 8192, else WC_EUNSUPPORTED;
 * workspace M doubles), 2 = the Bluestein pipeline of wc_hilbert_phase_long
 * (workspace as wc_hilbert_long_workspace_size: the returned minimum holds one
 * column, every further 32 L bytes one more in flight, 16-byte aligned, result
 * bit-identical for every workspace size and every C), 0 = whichever is
 * faster: direct below M = 2048, long from there on.  env must not alias x.
 * The size function returns 0 where the call would not return WC_OK or
 * WC_EWORKSPACE. */
size_t wc_hilbert_envelope_workspace_size(int64_t C, int64_t M, int method);
int wc_hilbert_envelope(int64_t C, int64_t M, const double* x, double* env, int method,
                        void* workspace, size_t ws_bytes, void* stream);

/* Per simulation b of bold [M][B][N] (the filtered, decimated BOLD; or, with
 * bold == NULL, of the given fc_in [B][N][N]):
 *   fc_out [B][N][N]  np.corrcoef(BOLD.T)                (may be NULL)
 *   metrics [B][K][4] utils.get_all_metrics(sFC, empfc[k], data_range) = corr, euc, ssim, new_metric
 *   extra [B][3]      np.mean(sFC), kuramoto sync, meta (sync/meta 0 if phasor NULL)
 * N >= 7 (the SSIM window).  N <= 96: one workgroup per simulation with the FC in
 * LDS, no workspace (may be NULL).  N > 96 (config 5, N = 1000): the FC is tiled
 * through global memory (wc_fc_large.hip) and workspace must hold
 * wc_fc_metrics_workspace_size(B, N, M, K, fc_out != NULL) bytes (it includes
 * the B N^2 doubles of FC when fc_out is NULL).  Deterministic for every N.
 * Non-finite values, as numpy: a constant column (0 / 0), a NaN
 * or an infinite sample make that column's row and column of the FC NaN, diagonal
 * included; an FC with a NaN (fc_in too) gives NaN in mean(sFC) and in the
 * metrics that read it; NaN phasors give NaN sync and meta.  The other
 * simulations of the batch are not affected. */
size_t wc_fc_metrics_workspace_size(int B, int N, int M, int K, int want_fc);
int wc_fc_metrics(int B, int N, int M, const double* bold, const double* fc_in, const double* empfc,
                  int K, double data_range, const double* phasor, double* fc_out, double* metrics,
                  double* extra, void* workspace, size_t ws_bytes, void* stream);

/* np.corrcoef(x[:, b, :].T) for every simulation b of a long time-major series
 * x [M][B][N] (the SC optimiser's FC, optimize_SC_Hopf.py:67-69: 6000 samples),
 * split over time blocks so a small batch still fills the GPU; fc [B][N][N],
 * clipped to [-1, 1] (a NaN stays: a constant column, a NaN or an infinite sample
 * make that column's row and column NaN, as numpy).  N >= 2, M >= 2 (N > 96: 64 x 64 covariance tiles in
 * global memory, wc_fc_large.hip).  Deterministic (fixed blocks, fixed combine
 * order).  workspace: wc_corrcoef_workspace_size(B, N, M) bytes. */
size_t wc_corrcoef_workspace_size(int B, int N, int M);
int wc_corrcoef(int B, int N, int M, const double* x, double* fc, void* workspace, size_t ws_bytes,
                void* stream);

/* utils.kuramoto (utils.py:34-40) from unit phasors [M][B][N][2] (wc_hilbert_phase):
 * out [B][2] = (mean_t R(t), std_t R(t)), R(t) = |mean_n exp(i theta_n(t))|; NaN
 * for a simulation with a NaN phasor. */
int wc_kuramoto(int B, int N, int M, const double* phasor, double* out, void* stream);

/* ------------------------------------------------------------------------
 * Welch peak frequency (whole_sweep_both.py:90-95): signal.welch(E_t.T, fs,
 * nperseg=4000), node-mean PSD, first argmax.  wc_welch_prepare fills the
 * twiddle workspace once; wc_welch_accumulate adds nseg (1, 2 or 4) consecutive segments
 * [seg0 + 2000 k, seg0 + 2000 k + 4000), k < nseg, of every column to acc [B][2001] (fp64, zero it
 * first; the ring must hold the nseg segments' span, 4000 + 2000 (nseg - 1) samples);
 * E is node-major: sample t of column c at
 *   c*ld + ((t / slot) % nslots) * slot + t % slot   (a ring of nslots slots);
 * wc_welch_peak turns acc (nseg segments) into peak [B] (Hz) and optionally
 * the node-mean density PSD psd [B][2001]. */
size_t wc_welch_workspace_size(void);
int wc_welch_bins(void);
int wc_welch_prepare(void* workspace, size_t ws_bytes, void* stream);
int wc_welch_accumulate(int B, int N, const void* E, int e_f64, int64_t ld, int64_t slot,
                        int64_t nslots, int64_t seg0, int nseg, const void* workspace, double* acc,
                        void* stream);
int wc_welch_peak(int B, int N, int nseg, double fs, const double* acc, double* peak, double* psd,
                  void* stream);

/* scipy.signal.welch(x, axis=0) of every column of a time-major x [T][C] fp64 ->
 * psd [nperseg/2 + 1][C] fp64 (cortex_run.py:203-209), for return_onesided=True,
 * average='mean', nfft=None: segments of nperseg samples every
 * step = nperseg - noverlap, nseg = (T - nperseg) / step + 1 of them (trailing
 * samples are ignored); per segment the mean is subtracted (detrend 1) or not
 * (detrend 0), the segment is multiplied by window [nperseg] (DEVICE, fp64) and
 * |DFT|^2 taken at bins 0 .. nperseg/2; the mean over segments times scale (the
 * caller's 1 / (fs sum w^2) for a density, 1 / (sum w)^2 for a spectrum) is
 * doubled at every bin but 0 and, for even nperseg, nperseg/2.
 * 2 <= nperseg <= 4096 (any value: the exact DFT is a Bluestein convolution over
 * an FFT of max(64, nextpow2(2 nperseg - 1)) points in one workgroup's LDS,
 * wc_welch_psd.hip; larger returns WC_EUNSUPPORTED), 0 <= noverlap < nperseg,
 * T >= nperseg, C >= 1; psd must not alias x; x, window, psd 8-byte and the
 * workspace 16-byte aligned.  wc_welch_psd_workspace_size is the minimum: the
 * tables (W_8192, the chirp and its spectrum) and the per-block sums of one
 * column, NB (nperseg/2 + 1) doubles with NB <= 16 segment blocks fixed by
 * (T, nperseg, noverlap); every further such slice lets one more column be in
 * flight per pass (up to C).  No atomics: a column's PSD is bit-identical for
 * every C, every position of the column and every workspace size.  The size
 * function returns 0 where the call would not return WC_OK or WC_EWORKSPACE. */
size_t wc_welch_psd_workspace_size(int64_t C, int64_t T, int nperseg, int noverlap);
int wc_welch_psd(int64_t C, int64_t T, const double* x, int nperseg, int noverlap,
                 const double* window, int detrend, double scale, double* psd,
                 void* workspace, size_t ws_bytes, void* stream);

/* scipy.signal.csd / coherence between the columns of a time-major x [T][C] fp64
 * (wc_csd.hip): wc_welch_psd's segments, window, detrend, scale and one-sided
 * doubling, P_ij[f] = mean over segments of conj(X_i[f]) X_j[f] (SciPy's sign),
 * F = nperseg/2 + 1 bins.  mode selects the output:
 *   WC_CSD_MATRIX          out [F][C][C] complex, interleaved (re, im): exactly
 *                          Hermitian, the diagonal (the columns' PSDs) exactly real;
 *   WC_CSD_COHERENCE       out [F][C][C] real, |P_ij|^2 / (P_ii P_jj): exactly
 *                          symmetric (scale is validated but cancels);
 *   WC_CSD_PAIRS           out [F][C/2] complex, column i against column i + C/2
 *                          (csd(x, y) of equally shaped x and y, stacked [x | y]);
 *   WC_CSD_PAIR_COHERENCE  out [F][C/2] real, the pairs' coherence.
 * Plain IEEE division: a column without power gives NaN coherence, as SciPy.
 * 2 <= nperseg <= 4096 (larger: WC_EUNSUPPORTED), 0 <= noverlap < nperseg,
 * T >= nperseg, 1 <= C <= 2^24; the matrix modes take C <= 1024 (more:
 * WC_EUNSUPPORTED), the pair modes an even C; out must not alias x; x, window, out
 * 8-byte and the workspace 16-byte aligned.
 * wc_csd_workspace_size is the minimum, whatever the mode: the tables of
 * wc_welch_psd, F C 16 bytes of running sums, and the complex spectra of one
 * segment block (two segments, the pair that shares a transform) of all C columns,
 * 2 F C 16 bytes; every further segment block lets two more segments go through the
 * two passes at a time (up to all).  No atomics: the segments are added in one
 * order fixed by (T, nperseg, noverlap), a later chunk continues the running sum,
 * and the result is bit-identical for every workspace size and from run to run; an
 * entry depends on the samples of its own two columns only.  The size function
 * returns 0 for a shape the call rejects (the mode's own limits apart). */
#define WC_CSD_MATRIX 0
#define WC_CSD_COHERENCE 1
#define WC_CSD_PAIRS 2
#define WC_CSD_PAIR_COHERENCE 3
size_t wc_csd_workspace_size(int64_t C, int64_t T, int nperseg, int noverlap);
int wc_csd(int64_t C, int64_t T, const double* x, int nperseg, int noverlap,
           const double* window, int detrend, double scale, int mode, double* out,
           void* workspace, size_t ws_bytes, void* stream);

/* scipy.signal.spectrogram(x, axis=0) of every column of a time-major x [T][C] fp64
 * (wc_spectrogram.hip): wc_welch_psd's / wc_csd's segments, window, detrend and scale,
 * S = (T - nperseg) / (nperseg - noverlap) + 1 segments and F = nperseg/2 + 1 bins,
 * nothing averaged.  X is the DFT of the windowed (detrend 1: mean-free) segment;
 * mode selects what is written of it:
 *   WC_SPEC_PSD        out [S][F][C] real, |X|^2 scale, doubled at every bin but 0
 *                      and (even nperseg) nperseg/2;
 *   WC_SPEC_COMPLEX    out [S][F][C] complex, interleaved (re, im): X sqrt(scale), no
 *                      doubling (SciPy's mode='stft' scaling); the imaginary part at
 *                      bins 0 and (even nperseg) nperseg/2 is exactly 0;
 *   WC_SPEC_MAGNITUDE  out [S][F][C] real, |X| sqrt(scale);
 *   WC_SPEC_ANGLE      out [S][F][C] real, atan2(im, re) of X in [-pi, pi]; a bin
 *                      that is exactly zero gives 0.
 * The layout is segment-major (a transform workgroup holds neighbouring columns of a
 * bin, which it writes contiguously); SciPy's [F][C][S] is the permuted view.
 * 2 <= nperseg <= 4096 (larger: WC_EUNSUPPORTED), 0 <= noverlap < nperseg,
 * T >= nperseg, 1 <= C <= 2^24, x and out below 2^62 bytes each; out must not alias x
 * (over the mode's own size, S F C cells of 8 or 16 bytes); x, window, out 8-byte and
 * the workspace 16-byte aligned.  Every argument is validated before any device work.
 * The workspace holds the tables only (W_8192, the chirp padded to 16 entries and its
 * spectrum [L], L = max(64, nextpow2(2 nperseg - 1))): (8192 + ceil(nperseg/16) 16 + L)
 * 16 bytes, whatever C and T; the size function returns 0 for nperseg < 2 or > 4096.
 * No atomics, nothing accumulated: a cell depends on its column's samples in its
 * segment pair only (segments 2k and 2k + 1 share a transform), and the result is
 * bit-identical for every C, every position of the column and from run to run. */
#define WC_SPEC_PSD 0
#define WC_SPEC_COMPLEX 1
#define WC_SPEC_MAGNITUDE 2
#define WC_SPEC_ANGLE 3
size_t wc_spectrogram_workspace_size(int nperseg);
int wc_spectrogram(int64_t C, int64_t T, const double* x, int nperseg, int noverlap,
                   const double* window, int detrend, double scale, int mode, double* out,
                   void* workspace, size_t ws_bytes, void* stream);

/* Phase and envelope connectivity between the columns of every simulation
 * (wc_phaseconn.hip), from the unit phasors phasor [M][B][N][2] = (cos, sin) of
 * wc_hilbert_phase / wc_hilbert_phase_long (B = 1, N = C for a plain [T][C] array;
 * taken as given) and the envelopes amp [M][B][N] of wc_hilbert_envelope.  For
 * columns i != j of one simulation, with u the phasors and a the envelopes,
 *   c(t) = u_i.x u_j.x + u_i.y u_j.y
 *   s(t) = u_i.y u_j.x - u_i.x u_j.y      (two rounded products and one subtraction,
 *                                          never an FMA: identical columns give 0)
 *   WC_CONN_PLV       sqrt((sum_t c)^2 + (sum_t s)^2) / M               diagonal 1
 *   WC_CONN_PLI       |sum_t sign(s)| / M, sign(0) = 0                  diagonal 0
 *   WC_CONN_WPLI      |sum_t a_i a_j s| / sum_t |a_i a_j s|             diagonal 0
 *   WC_CONN_AEC_ORTH  (corr_t(a_i |s|, a_j) + corr_t(a_j |s|, a_i)) / 2 diagonal 0
 * (corr: Pearson's coefficient; the envelope of one column orthogonal to the other's
 * phase, Hipp et al. 2012, no logarithm, no absolute value).  A zero denominator
 * gives NaN: wpli and aec_orth of two identical columns, aec_orth with a constant
 * envelope.  measures is a non-empty set of the bits; out holds one [B][N][N] matrix
 * per set bit, in ascending bit order, each exactly symmetric.  amp may be NULL
 * exactly when neither WC_CONN_WPLI nor WC_CONN_AEC_ORTH is set.  (The plain
 * amplitude-envelope correlation is wc_corrcoef of the envelopes.)
 * B >= 1, 1 <= N <= 1024 (more: WC_EUNSUPPORTED), 2 <= M <= 524288 (more:
 * WC_EUNSUPPORTED); out must not alias phasor or amp; phasor, amp, out 8-byte and the
 * workspace 16-byte aligned.  Every argument is validated before any device work.
 * The sums run over time blocks of 4096 samples and 32 x 32 column tiles; with
 * nt = ceil(N / 32), nblk = ceil(M / 4096), the workspace holds the blocks' partial
 * sums, B nt (nt + 1) / 2 nblk K 8192 bytes with K = 8 if an amplitude bit is set
 * and 3 otherwise, plus B nblk N 16 bytes (rounded up to 16) for WC_CONN_AEC_ORTH;
 * more is not used.  The size function returns 0 where the call would return
 * neither WC_OK nor WC_EWORKSPACE.  No atomics: an entry depends on the samples of
 * its own two columns, M and the measure only -- not on N, B, its position, the
 * workspace size, the other measures asked for or the run. */
#define WC_CONN_PLV 1
#define WC_CONN_PLI 2
#define WC_CONN_WPLI 4
#define WC_CONN_AEC_ORTH 8
size_t wc_phase_conn_workspace_size(int B, int N, int64_t M, int measures);
int wc_phase_conn(int B, int N, int64_t M, const double* phasor, const double* amp, int measures,
                  double* out, void* workspace, size_t ws_bytes, void* stream);

/* Weighted graph measures of B matrices w [B][N][N] fp64, batched (wc_graph.hip; the reference's
 * graph_utils.py, after Rubinov & Sporns): the companions of wc_hma's integration and segregation
 * on the matrix side.  No symmetry is assumed: every expression is evaluated as the reference
 * writes it, so a directed matrix gives what the reference gives.  One workgroup per matrix (per
 * matrix and node for the local efficiency), everything in LDS, no workspace.
 *
 * Common to the three: B >= 1, 2 <= N <= 96 (more: WC_EUNSUPPORTED), w not NULL, at least one output
 * not NULL (every output is optional on its own), no output overlapping w, every pointer 8-byte
 * aligned (the int32 outputs too); all of it checked before any device work.
 *
 * wc_graph_paths: distance_wei (graph_utils.py:1462-1529) and charpath (:1533-1591) of every matrix.
 *   w holds weights (lengths == 0: the connection lengths are L = 1/w where w != 0, as invert,
 *   :68-90) or the lengths themselves (lengths != 0).  D starts as 0 on the diagonal, L where
 *   L != 0 and +inf elsewhere; Floyd-Warshall gives the shortest paths.
 *     dist  [B][N][N]  D: +inf for an unreachable pair, 0 on the diagonal
 *     hops  [B][N][N]  int32, edges of the shortest path (the reference's B): 1 on an edge,
 *                      h[i][k] + h[k][j] wherever D[i][k] + D[k][j] < D[i][j] strictly; 0 on the
 *                      diagonal and for an unreachable pair
 *     stats [B][4]     lambda = mean D, efficiency = mean 1/D, radius = min ecc, diameter = max ecc
 *     ecc   [B][N]     row maxima of D
 *   all over the off-diagonal entries, the infinite ones included (include_infinite != 0: one
 *   unreachable pair makes lambda +inf and adds 0 to the efficiency, which then equals
 *   efficiency_wei(local=False), :597-690) or dropped (include_infinite == 0; a row with nothing
 *   left has ecc NaN and is passed over by radius and diameter, no entry at all gives lambda and
 *   efficiency NaN).
 *   A matrix with a negative or NaN entry (the reference is undefined there) gets NaN in every
 *   fp64 output and -1 in hops; the other matrices of the batch are not affected.
 *
 * wc_graph_local_efficiency: efficiency_wei(local=True) (:667-685).  eloc [B][N]; for node u, with
 *   V the nodes v where w[u][v] != 0 or w[v][u] != 0 and D the shortest paths within V,
 *     e = 1/D (0 on the diagonal), se = cuberoot(e) + cuberoot(e^T),
 *     sw = cuberoot(w[u][V]) + cuberoot(w[V][u]),  sa = (w[u][V] != 0) + (w[V][u] != 0),
 *     E[u] = (sum_ij sw_i sw_j se_ij / 2) / ((sum sa)^2 - sum sa^2), and 0 where the numerator is 0
 *   (no neighbour, or one).  cuberoot(x) = sign(x) |x|^(1/3) (:38-43).  Negative or NaN entries as
 *   for wc_graph_paths: eloc of that matrix is NaN.  B N < 2^31.
 *
 * wc_graph_clustering: with ws = cuberoot(w), cyc3_i = sum_j (ws ws)_ij ws_ji and K_i the
 *   non-zeros of row i,
 *     clustering   [B][N]  cyc3_i / (K_i (K_i - 1)), exactly 0 where cyc3_i == 0 (clustering_coef_wu,
 *                          :1305-1323)
 *     transitivity [B]     sum cyc3 / sum K (K - 1)                     (transitivity_wu, :1673-1689)
 *     strengths    [B][N]  column sums                                   (strengths_und, :1766-1778)
 *     degrees      [B][N]  int32, non-zeros of a column                  (degrees_und, :1721-1737)
 *   Negative weights are legal here: the cube root carries the sign. */
int wc_graph_paths(int B, int N, const double* w, int lengths, int include_infinite, double* dist,
                   int* hops, double* stats, double* ecc, void* stream);
int wc_graph_local_efficiency(int B, int N, const double* w, double* eloc, void* stream);
int wc_graph_clustering(int B, int N, const double* w, double* clustering, double* transitivity,
                        double* strengths, int* degrees, void* stream);

/* Node measures of the same batch (wc_graph.hip): which nodes are hubs, and of what kind.  The
 * argument checks are those of the three entry points above, before any device work.
 *
 * wc_graph_betweenness: betweenness_wei (graph_utils.py:1983-2052) of every matrix, Brandes'
 *   algorithm with one wave per source.  w holds weights (lengths == 0: L = 1/w where w != 0) or the
 *   lengths themselves (lengths != 0, what betweenness_wei takes); a zero is no edge and the diagonal
 *   is ignored.  bc [B][N].  Ordered pairs are counted, so an undirected graph has twice the textbook
 *   value, as in the reference.  A candidate path length is the single fp64 sum D[v] + L[v][w]; a
 *   shorter one replaces the predecessors and the number of paths, an equal one adds to them; all
 *   unsettled nodes at the minimum distance are settled together: ties resolve as in the reference.
 *   With unique shortest paths every value is an integer and exact.  betweenness_bin (:1929-1980) is
 *   the same on the lengths (w != 0), to rounding.  A matrix with a negative or NaN entry gets NaN in
 *   its row of bc; the others are not affected.  No atomics: a matrix gives the same bits alone as
 *   inside a batch.
 *
 * wc_graph_modules: measures of a given partition ci [B][N] int32, labels in [0, K), 1 <= K <= N; ci
 *   4-byte aligned and overlapping no output.  Each of part, z, q may be NULL (not all three).
 *     part [B][N]  participation_coef (:271-307): 1 - sum_m (sum_{j in m} W_ij)^2 / (sum_j W_ij)^2,
 *                  exactly 0 where the strength is 0; degree 0: rows (undirected, out), 1: the
 *                  transpose (in)
 *     z    [B][N]  module_degree_zscore (:2103-2140): (k_i - mean) / std of the within-module degrees
 *                  k_i = sum_{j in m(i)} A_ij over the node's own module, population std; A = W
 *                  (zflag 0, 1), W^T (2), W + W^T (3).  A NaN quotient (0/0: a single-member module,
 *                  equal degrees) is 0, as in the reference, which therefore also hides a NaN of w
 *     q    [B]     (1/s) sum_ij (W_ij - gamma k_i^out k_j^in / s) delta(ci_i, ci_j), s = sum W: the
 *                  modularity of the partition (Newman; Leicht & Newman for a directed matrix)
 *   Negative weights are legal: they are summed.  A matrix with a label outside [0, K) gets NaN in
 *   part, z and q, and nothing is indexed by that label; the others are not affected. */
int wc_graph_betweenness(int B, int N, const double* w, int lengths, double* bc, void* stream);
int wc_graph_modules(int B, int N, int K, const double* w, const int32_t* ci, int degree, int zflag,
                     double gamma, double* part, double* z, double* q, void* stream);

/* Partition search on the same batch (wc_louvain.hip): the ci that wc_graph_modules takes.  Every
 * argument is checked before any device work: B, R >= 1, 2 <= N <= 96 (more: WC_EUNSUPPORTED),
 * B R < 2^31; fp64 and uint64 arrays 8-byte, int32 arrays 4-byte aligned; no output overlapping an
 * input or another output.
 *
 * wc_graph_louvain: community_louvain (graph_utils.py:958-1122) from the objective matrix on, for
 *   every pair of a matrix and a seed.  obj [B][N][N] is the reference's B after :1032-1052 (the
 *   modularity matrix W - gamma k_out k_in^T / s, the Potts matrix, or any other), norm [B] its s;
 *   ci0 NULL (every node its own module) or [B][N] int32 starting labels in [0, N), relabelled as
 *   np.unique does; seeds [R] uint64.
 *     ci   [B][R][N]  int32, labels 0 .. K-1: the reference's final labelling minus 1
 *     q    [B][R]     the objective of that partition, trace of the pooled matrix / s
 *     info [B][R][2]  int32, levels (passes of the outer loop) and node sweeps in all; may be NULL
 *   Per level, sweeps over the current nodes until none moves; node u of module ma has
 *   dQ = Hnm[u,:] - Hnm[u,ma] + obj[u,u], dQ[ma] = 0, and moves where max dQ > 1e-10 to the lowest
 *   index that attains the maximum (np.argmax), an empty module included.  Between levels the
 *   modules are relabelled as np.unique does and obj is pooled over module pairs, the upper triangle
 *   computed and mirrored; levels go on while q - q0 > 1e-10.  No symmetry is assumed.
 *   The visiting order is the engine's own, as numpy's permutation cannot be drawn here: sweeps
 *   are numbered t = 0, 1, 2, ... over all levels of a run, and sweep t visits n nodes in the stable
 *   argsort of n 32-bit keys, key i = word i % 4 of the Philox block above with step = t,
 *   quad = i / 4, simkey = seed; ties go to the lower index.  It depends on seed and t only.
 *   A matrix whose obj or norm holds NaN or inf, or whose ci0 holds a label outside [0, N), gets
 *   ci = -1, q = NaN and info = 0 in all its runs; a run whose level has not settled after 1000
 *   sweeps (the reference raises) gets ci = -1 and q = NaN; nothing else is affected.  Fixed
 *   summation order and no atomics: a (matrix, seed) pair gives the same bits alone as in any batch.
 *
 * wc_graph_agreement: agreement (:890-932).  ci [B][R][N] int32, R partitions of every matrix.
 *     D [B][N][N]  the number of the R partitions in which i and j share a label, exact; 0 on the
 *                  diagonal
 *   A negative label anywhere in a matrix's partitions (a run that wc_graph_louvain refused) makes
 *   its D NaN; the others are not affected. */
int wc_graph_louvain(int B, int R, int N, const double* obj, const double* norm, const int32_t* ci0,
                     const uint64_t* seeds, int32_t* ci, double* q, int32_t* info, void* stream);
int wc_graph_agreement(int B, int R, int N, const int32_t* ci, double* D, void* stream);

/* Partition search on matrices with weights of both signs (wc_louvain_sign.hip).
 *
 * wc_graph_louvain_sign: modularity_louvain_und_sign (graph_utils.py:697-855; Rubinov & Sporns 2011)
 *   for every pair of a matrix and a seed.  w [B][N][N] fp64, any signs; seeds [R] uint64; gamma
 *   finite; qtype 0 "sta", 1 "pos", 2 "smp", 3 "gja", 4 "neg".
 *     ci   [B][R][N]  int32, labels 0 .. K-1: the reference's final labelling minus 1
 *     q    [B][R]     the modularity of the last level
 *     info [B][R][2]  int32, levels (passes of the outer loop) and node sweeps in all; may be NULL
 *   W0 = W (W > 0), W1 = -W (W < 0); kn0, kn1 their column sums and s0, s1 the sums of those, all
 *   taken in ascending index order; (d0, d1) = (1/s0, 1/(s0+s1)) sta, (1/s0, 0) pos, (1/s0, 1/s1)
 *   smp, (1/(s0+s1), 1/(s0+s1)) gja, (0, 1/s1) neg; then s0 == 0 gives s0 = 1, d0 = 0 and s1 == 0
 *   gives s1 = 1, d1 = 0.  Per level, sweeps over the current nodes until none moves; node u of module
 *   ma has, one rounding per operation and no fma, as numpy evaluates the reference's line,
 *     dQ0 = ((knm0[u,m] + W0[u,u]) - knm0[u,ma]) - ((gamma kn0[u]) ((km0[m] + kn0[u]) - km0[ma])) / s0,
 *     dQ1 the same on W1, dQ = d0 dQ0 - d1 dQ1 (both products rounded), dQ[ma] = 0,
 *   and moves where max dQ > 1e-10 to the lowest index that attains the maximum, an empty module
 *   included.  Between levels the modules are relabelled as np.unique does and W0, W1 are pooled
 *   over module pairs, the upper triangle computed and mirrored; the level's modularity is
 *   q = d0 (tr W0 - sum(W0 W0) / s0) - d1 (tr W1 - sum(W1 W1) / s1), the sum over all entries of the
 *   matrix product taken as the sum of the squared column sums (the pooled matrix is symmetric);
 *   levels go on while q - q before > 1e-10, from q = -1, 0, and the last level's ci and q are
 *   returned whether it improved or not.  An all-zero matrix gives N singletons and q = 0.
 *   The visiting order is wc_graph_louvain's: sweeps numbered t = 0, 1, 2, ... over all levels of a
 *   run, the same Philox keys.
 *   A matrix with a NaN or inf gets ci = -1, q = NaN and info = 0 in all its runs; a run whose level
 *   has not settled after 1000 sweeps, or that would start a 301st level (the reference raises in
 *   both cases) gets ci = -1 and q = NaN; nothing else is affected.
 *   Workspace: W0 and W1 of the pooled levels lie in global memory, one slot of 16 N^2 bytes per
 *   workgroup; the grid is min(B R, ws_bytes / slot) workgroups, which stride over the problems.
 *   ws_bytes below one slot: WC_EINVAL.  Fixed summation order, no atomics: a (matrix, seed) pair gives
 *   the same bits alone, in any batch and with any ws_bytes.
 *   Checked before any device work: B, R >= 1, 2 <= N <= 96 (more: WC_EUNSUPPORTED), B R < 2^31, qtype
 *   in 0 .. 4, gamma finite; w, seeds, ci, q, workspace not NULL; fp64 and uint64 arrays and the
 *   workspace 8-byte, int32 arrays 4-byte aligned; no output, the used part of the workspace
 *   included, overlapping an input or another output. */
int wc_graph_louvain_sign(int B, int R, int N, const double* w, double gamma, int qtype,
                          const uint64_t* seeds, int32_t* ci, double* q, int32_t* info,
                          void* workspace, size_t ws_bytes, void* stream);

/* Dynamic functional connectivity (wc_fcd.hip): sliding-window FC with its FCD matrix (Hansen et al.
 * 2015) and the phase-coherence FCD (Deco & Kringelbach 2016).  The reference computes neither; these
 * definitions are the contract (tests/fcd_reference.py restates them in numpy).
 *
 * wc_fcd: x [M][B][N] fp64, time-major (wc_fc_metrics' layout), window length win, step step.
 *   nw = (M - win) / step + 1 windows; window k is rows k step .. k step + win - 1; trailing rows that
 *   fit no window are not read.  FC_k = np.corrcoef(x[k step : k step + win, b, :].T) (each window
 *   centred on its own column means before the products, clipped to [-1, 1]); its pattern v_k is the
 *   strict upper triangle, row-major (utils.flat_FC's order), P = N (N - 1) / 2 entries.
 *     fcd   [B][nw][nw]  fcd[b][k][l] = Pearson correlation of v_k and v_l (two passes, clipped to
 *                        [-1, 1]): one triangle computed and mirrored, so exactly symmetric; the
 *                        diagonal exactly 1 where defined
 *     winfc [B][nw][P]   the patterns v_k, or NULL
 *   A column that is constant within a window (its centred values all exactly 0) makes the entries
 *   of v_k that involve it NaN (0 / 0, as numpy); row and column k of fcd, the diagonal included, are
 *   then NaN, as for a pattern without variance.  No other window and no other simulation changes.
 *   3 <= N <= 96 (more: WC_EUNSUPPORTED), 2 <= win <= M, step >= 1, nw <= WC_FCD_MAX_WINDOWS (more:
 *   WC_EUNSUPPORTED); x, fcd and the workspace not NULL, every pointer 8-byte aligned, nothing
 *   overlapping; all of it checked before any device work.
 *   Workspace: wc_fcd_workspace_size() bytes (0: bad shape) hold the centred patterns and norms of
 *   min(B, 8) simulations, (nw P + nw) doubles each; the batch goes through it in chunks, a larger
 *   workspace takes more simulations a chunk.  Less: WC_EWORKSPACE.
 *   Every output of simulation b depends on that simulation's data, M, win and step only, bit for
 *   bit: not on B, on b, or on ws_bytes.  Every sum has one fixed order; no atomics.
 *
 * wc_fcd_phase: phasor [M][B][N][2] fp64, wc_hilbert_phase's unit phasors (c, s).  With
 *   d_t[i][j] = cos(theta_i(t) - theta_j(t)) = c_i c_j + s_i s_j,
 *     fcd [B][M][M]  the cosine similarity of the strict upper triangles of d_t and d_u, clipped to
 *                    [-1, 1]; exactly symmetric, the diagonal exactly 1, NaN in row and column t
 *                    (diagonal included) where the norm of d_t is 0 or not finite
 *   2 <= N <= 96 (more: WC_EUNSUPPORTED), 1 <= M <= WC_FCD_PHASE_MAX_M (more: WC_EUNSUPPORTED);
 *   pointers not NULL, 8-byte aligned, not overlapping.  No workspace; bits as for wc_fcd. */
#define WC_FCD_MAX_WINDOWS 4096  /* wc_fcd: windows (fcd is nw x nw a simulation) */
#define WC_FCD_PHASE_MAX_M 4096  /* wc_fcd_phase: samples (fcd is M x M a simulation) */
size_t wc_fcd_workspace_size(int B, int N, int M, int win, int step);
int wc_fcd(int B, int N, int M, const double* x, int win, int step, double* fcd, double* winfc,
           void* workspace, size_t ws_bytes, void* stream);
int wc_fcd_phase(int B, int N, int M, const double* phasor, double* fcd, void* stream);

/* LEiDA, Leading Eigenvector Dynamics Analysis (Cabral et al. 2017), and the state statistics a sweep is
 * fitted on (Deco et al. 2019), in wc_leida.hip.  The reference computes none of it; these definitions
 * are the contract (tests/leida_reference.py restates them in numpy).  Everything fp64; every
 * floating-point sum has one fixed order that depends on the shape alone; no floating-point atomics; all
 * arguments are checked before any device work.  1 <= R <= WC_LEIDA_MAX_ROWS (more: WC_EUNSUPPORTED),
 * 2 <= N <= 1024 and 1 <= K <= 32 (more: WC_EUNSUPPORTED); pointers not NULL, doubles and int64 8-byte
 * aligned, int32 4-byte aligned, nothing overlapping.
 *
 * wc_leida_eigvec: phasor [R][N][2] fp64, 16-byte aligned: wc_hilbert_phase's [M][B][N][2] seen flat,
 *   R = M B (unit modulus is not required).  With c = phasor[r][.][0], s = phasor[r][.][1] the phase
 *   coherence matrix is A = c c^T + s s^T, whose non-zero eigenvalues are those of [[cc, cs], [cs, ss]],
 *   cc = sum c^2, ss = sum s^2, cs = sum c s: with h = (cc - ss) / 2 and r = hypot(h, cs),
 *   lambda1,2 = (cc + ss) / 2 +- r, w = (h + r, cs) if h >= 0, else (cs, r - h), and
 *     vec   [R][N]  v = (w0 c + w1 s) / its norm, negated if p = #{v_i > 0} has 2 p > N, or 2 p = N and
 *                   sum v > 0 (most entries negative; the sum in the kernel's own order)
 *     share [R]     lambda1 / (lambda1 + lambda2)
 *   r = 0 exactly (lambda1 = lambda2): the row of vec NaN, share 0.5, NaN for an all-zero row.  A NaN
 *   or an infinity in a row, or squares that overflow: that row of vec and its share NaN, nothing else.
 *   A row's bits depend on that row and N only.
 *
 * wc_kmeans_assign: x [R][N], cent [K][N], metric WC_KMEANS_SQEUCLIDEAN: sum (x - c)^2, summed as it
 *   stands, or WC_KMEANS_COSINE: 1 - x.c / (|x| |c|).
 *     labels [R] int32  the centroid of smallest distance, a tie to the lowest k
 *     dist   [R]        that distance
 *   A row with a NaN or an infinity, or of norm 0 under cosine: label -1, dist NaN.  A centroid with a
 *   NaN or an infinity, or of norm 0 under cosine, is never chosen; none left: label -1, dist NaN.
 *
 * wc_kmeans_update: x [R][N], labels [R] int32, cent_prev [K][N] ->
 *     cent  [K][N]      the mean of the rows labelled k (cosine: of the rows divided by their norms; a
 *                       member of norm 0 makes its centroid NaN, as numpy); cent_prev[k] where there are none
 *     count [K] int64   the rows labelled k
 *   Labels outside 0 .. K-1 (-1 among them) belong to nobody.  A NaN in a row reaches its own cluster only.
 *   Workspace: wc_kmeans_workspace_size() bytes (0: bad shape): the partial sums of every block of
 *   WC_KMEANS_UPDATE_BLOCK rows, K N doubles and K int64 a block, and R norms under cosine; blocks are
 *   added in index order.  Less: WC_EWORKSPACE; more is never touched, so the bits of cent depend on
 *   (R, N, K), the metric and the data only.
 *
 * wc_state_stats: labels [M][B] int32, time-major (what assigning [M][B][N] eigenvectors yields), K
 *   states, B >= 1, M >= 1.  With V = the times whose label is in 0 .. K-1,
 *     occupancy [B][K]     #{t in V: l_t = k} / #V; all NaN if V is empty
 *     dwell     [B][K]     the mean length in samples of the maximal runs of k (runs that touch either
 *                          end count; any other label ends a run); NaN if k never occurs
 *     trans     [B][K][K]  #{t: l_t = i, l_t+1 = j} / #{t: l_t = i, l_t+1 in V}, self-transitions
 *                          included, rows summing to 1; a row NaN if i has no successor
 *   counted in integers and divided once.  A label outside -1 .. K-1 counts as -1: the status path for
 *   device-side findings, wc_integrate_status, reads a word of wc_integrate's workspace, and
 *   wc_state_stats has none. */
#define WC_LEIDA_MAX_ROWS ((int64_t)1 << 40)
#define WC_KMEANS_UPDATE_BLOCK 256  /* wc_kmeans_update: rows of a partial sum */
enum wc_kmeans_metric { WC_KMEANS_SQEUCLIDEAN = 0, WC_KMEANS_COSINE = 1 };
int wc_leida_eigvec(int64_t R, int N, const double* phasor, double* vec, double* share, void* stream);
int wc_kmeans_assign(int64_t R, int N, int K, const double* x, const double* cent, int metric,
                     int32_t* labels, double* dist, void* stream);
size_t wc_kmeans_workspace_size(int64_t R, int N, int K, int metric);
int wc_kmeans_update(int64_t R, int N, int K, const double* x, const int32_t* labels,
                     const double* cent_prev, int metric, double* cent, int64_t* count, void* workspace,
                     size_t ws_bytes, void* stream);
int wc_state_stats(int B, int M, int K, const int32_t* labels, double* occupancy, double* dwell,
                   double* trans, void* stream);

/* Surrogate-tested functional connectivity (wc_surrogate.hip): the reference's
 * probabilistic_thresholding (graph_utils.py:220-265) for a batch.  It multiplies the FFT of the
 * mean-free series y [L][N] by exp(i r), r [L] the random phases rv [L/2][N] stacked over their own
 * reverse, and correlates the real part of the inverse FFT.  That real part is the inverse FFT of
 * the Hermitian part of the product, so with h = L/2 the spectrum of surrogate column n is
 *     X_n(k) = Y_n(k) (exp(i rv[k][n]) + exp(-i rv[k-1][n])) / 2    for 1 <= k <= h - 1,
 *     X_n(h) = Y_n(h) cos(rv[h-1][n]),
 * bin 0 being removed by the correlation's own centring, and by Parseval the surrogate's correlation
 * matrix is the Gram matrix, normalised by its diagonal, of the real rows
 *     sqrt(2) Re X(k), sqrt(2) Im X(k) (k = 1 .. h - 1), X(h):    L - 1 rows, no inverse transform.
 * The amplitude spectrum is not preserved: that is the reference's surrogate and is reproduced.
 *
 * Phases.  The phases are the engine's: rv[k][n] of a surrogate with seed s is 2 pi w 2^-32, w the
 * word n & 3 of the Philox4x32-10 block with counter (k lo32, (k hi16 << 16) | n >> 2, s lo32,
 * s hi32) and key (WC_PHILOX_KEY0, WC_PHILOX_KEY1): the block wc_graph_louvain's visiting order
 * draws with (t, i >> 2, seed).  They depend on the seed, k and n only, not on the simulation, as
 * the reference's np.random.seed(i + 1) gives every series the same random_vector.  The kernel
 * takes cos and sin of 2 pi w 2^-32 as cospi and sinpi of w 2^-31, which is exact in its argument.
 *
 * wc_surrogate_fc: spec [L/2 + 1][B N] complex, interleaved (re, im): the DFT at bins 0 .. L/2 of
 *   the mean-free columns of x [L][B][N], which wc_spectrogram gives with nperseg = L, noverlap = 0,
 *   a window of ones, detrend 1, scale 1 and WC_SPEC_COMPLEX; seeds [S] uint64.
 *     sfc [B][S][P]  the strict upper triangle, row-major, P = N (N - 1) / 2, of the correlation
 *                    matrix of surrogate s of simulation b: the Gram product in fp64, the rows taken
 *                    four at a time in the order k = 1 .. h, real before imaginary (one
 *                    v_mfma_f64_16x16x4_f64 per 16 x 16 tile), g_ij (1 / sqrt g_ii) (1 / sqrt g_jj)
 *                    clipped to [-1, 1] as wc_corrcoef; a column without power (a constant series)
 *                    or with a NaN or an infinity gives NaN in its pairs (0 inf, as numpy's 0 / 0).
 *   No atomics, one fixed order: a (simulation, surrogate) pair gives the same bits alone and at any
 *   position of any batch.
 *
 * wc_surrogate_test: fc [B][N][N] the FC of the series themselves (wc_corrcoef), of which the
 *   strict upper triangle is read; sfc as above; 0 < alpha < 1.  Per pair q = (i, j), i < j:
 *     mu = (sum_s sfc[b][s][q]) / S, sd = sqrt((sum_s (sfc[b][s][q] - mu)^2) / S), both sums in the
 *     order of s (two passes; the population deviation, as stats.norm.fit), z = (fc[b][i][j] - mu) / sd,
 *     p = 1 - Phi(z), evaluated as the reference's 1 - stats.norm.cdf: with t = z / sqrt 2,
 *     Phi = 1/2 + erf(t) / 2 where |t| < 1, else erfc(|t|) / 2 or, for t > 0, 1 minus that; so p
 *     saturates to exactly 0 from z of about 8.3 on, as the reference's.  sd > 0 false: p = NaN (SciPy
 *     refuses a scale of 0).
 *   Per matrix the Benjamini-Hochberg adjustment over its P values, as
 *   scipy.stats.false_discovery_control(p, method='bh'): sorted ascending, p_(r) (P / r) for rank r =
 *   1 .. P (the quotient first), the running minimum from the top, at most 1, back in place.  Equal
 *   p-values get equal results in any order.
 *     p_adj  [B][N][N]  the adjusted p-values, symmetric, diagonal 0 (the reference's matrix_recon)
 *     fc_adj [B][N][N]  fc[b][i][j] (p_adj < alpha ? 1 : 0) at (i, j) and (j, i), diagonal 0
 *     mu, sd, p [B][P]  the pairs' statistics and unadjusted p-values; each may be NULL
 *   A matrix with a p that is not finite (a constant or non-finite column, a pair whose surrogate
 *   values all coincide, a NaN in fc) has p_adj and fc_adj NaN throughout, the diagonal included;
 *   mu, sd and p are written as computed; no other matrix is touched.
 *
 * Both: B >= 1, 2 <= N <= 96 (more: WC_EUNSUPPORTED), S >= 2, B S < 2^31; wc_surrogate_fc: L even
 * (odd: WC_EINVAL, the reference raises there), 4 <= L <= 4096 (more: WC_EUNSUPPORTED); pointers
 * not NULL (mu, sd, p apart), spec 16-byte and every other array 8-byte aligned, no output
 * overlapping an input or another output; all of it checked before any device work. */
int wc_surrogate_fc(int B, int N, int L, int S, const double* spec, const uint64_t* seeds,
                    double* sfc, void* stream);
int wc_surrogate_test(int B, int N, int S, const double* fc, const double* sfc, double alpha,
                      double* p_adj, double* fc_adj, double* mu, double* sd, double* p, void* stream);

/* Degree- and strength-preserving null models of signed undirected matrices (wc_nullmodel.hip): the
 * reference's randmio_und_signed (graph_utils.py:2165-2217) and null_model_und_sign (:2219-2338;
 * Rubinov & Sporns 2011), for every pair of a matrix and a seed.  tests/nullmodel_reference.py
 * restates this text in numpy.
 *
 * Both: w [B][N][N] fp64, any signs, exactly symmetric; the diagonal is not used: it is cleared
 * (:2264).  seeds [R] uint64.  info [B][R][3] int32: the effective rewirings eff, the draws consumed
 * (modulo 2^32), and a status: 0, or 1 to 3 as below; may be NULL.
 *
 * Rewiring.  itr = bin_swaps (N (N - 1) / 2) iterations; bin_swaps = 0 rewires nothing.  An iteration
 *   makes at most A = round(N / 2) + 1 attempts, the rounding half to even as np.round (N = 5: 2,
 *   N = 7: 4).  An attempt takes four distinct nodes (a, b, c, d) and, with signs in {-, 0, +}, swaps
 *   where sign(ab) == sign(cd), sign(ad) == sign(cb) and sign(ab) != sign(ad): (ad, da) <- ab,
 *   (ab, ba) <- ad, (cb, bc) <- cd, (cd, dc) <- cb, the old values; that ends the iteration and counts
 *   in eff.  The nodes are the engine's: the draws of a run are numbered d = 0, 1, 2, ... over all its
 *   iterations, draw d is the Philox block above with step = d, quad = 0x8000, simkey = seed, and
 *   (a, b, c, d) = (x[k] N) >> 32 for its words k = 0 .. 3.  A draw whose four values are not distinct
 *   is passed over without counting as an attempt (the reference's recursion).  The partition
 *   searches and the surrogates use quads below 24, the shuffles below 0x4000 .. 0x410f: the streams
 *   of one seed do not meet.
 *
 * wc_graph_rewire: randmio_und_signed.
 *     wr [B][R][N][N]  the matrix after the run, its weights moved with their signs; diagonal 0
 *
 * wc_graph_null_model: null_model_und_sign.  The matrix is rewired as above where fewer than
 *   N (N - 1) off-diagonal entries are positive (:2268); else eff = 0 and no draw is consumed.  Of
 *   the rewired matrix only the signs are used.  Then, once per sign s, the positive first
 *   (pass 0, 1): Acur and A_rcur the sign-s entries of w and of the rewired matrix;
 *     S   [N]  the column sums of w Acur, in ascending row order;
 *     Wv       the sign-s weights of the strict upper triangle of w, sorted ascending, wsize of them;
 *     the live list: the sign-s places (i, j), i < j, of the rewired matrix, row-major; wsize too;
 *     P[i][j] = S[i] S[j].
 *   neg_mode says what the negative pass takes for w: 0, the reference's code as written, takes w
 *   itself, so S and Wv are negative, Wv begins with the largest magnitude, and the value written,
 *   -Wv, is POSITIVE: on a matrix with negative weights the reference returns a w0 without any, and
 *   r[1] = NaN.  This is the reference's behaviour, pinned to its own outputs, not the definition.
 *   1, the definition (BCT's null_model_und_sign.m), takes -w: S and Wv positive, the value written,
 *   -Wv, negative.  The positive pass does not depend on it.
 *   period = round(1 / wei_freq), 0 .. 64 (more: WC_EUNSUPPORTED).  period 0 (wei_freq 0): one sort,
 *   the place of rank x receives Wv[x].  Else for m = wsize, wsize - period, ... while m > 0, period
 *   number p = 0, 1, ...:
 *     1. Oind: the m live places ordered by (P[i][j], place in the live list), < on the doubles, -0.0
 *        equal to 0.0: np.argsort's result wherever no two live keys are equal, the stable one else;
 *     2. R[0 .. k), k = min(m, period): the first k values of a Fisher-Yates shuffle of 0 .. m-1:
 *        for q = 0 .. k-1, j = q + ((word_q (m - q)) >> 32), swap places q and j, R[q] = place q;
 *        word_q is word q & 3 of the Philox block with step = p, quad = 0x4000 + 0x100 pass + (q >> 2);
 *     3. for q in order, with o = Oind[R[q]] at (i, j) and v = Wv[R[q]]: w0[i][j] = w0[j][i] = v in
 *        pass 0, -v in pass 1; fi = 1 - v / S[i], fj = 1 - v / S[j]; P[i][:] *= fi, then P[:][i] *= fi
 *        (P[i][i] twice), then the same with j and fj (P[i][j] takes fi before fj); S[i] -= v,
 *        S[j] -= v.  One rounding per operation, no fma;
 *     4. the k places leave the live list and the k weights leave Wv, the order of the rest kept.
 *   S[i] or S[j] equal to 0 at step 3 (the reference divides by zero): the run stops with status 1,
 *   w0 and r NaN, eff and draws as counted.
 *     w0 [B][R][N][N]  the null model, symmetric, diagonal 0
 *     r  [B][R][2]     the Pearson correlation of the positive strengths of w and of w0 (column sums
 *                      of the positive entries), and of the negative ones; clipped to [-1, 1]; NaN
 *                      where a sequence is constant (0 / 0, as np.corrcoef).  May be NULL.
 *
 * Both: a matrix with a NaN or an infinity anywhere, the diagonal included, has status 3; else one
 * with w[i][j] != w[j][i] somewhere has status 2; wr, w0 and r are NaN and eff and draws 0 in all its
 * runs, and no other matrix is affected.
 * Workspace: the sorted weights lie in global memory, one slot of wc_graph_null_model_slot_bytes(N) =
 * 4 N (N - 1) bytes per workgroup (0 for an N outside 4 .. 96); the grid is min(B R, ws_bytes / slot)
 * workgroups, which stride over the problems; wc_graph_rewire takes the same workspace.  ws_bytes
 * below one slot: WC_EINVAL.  Fixed order, no atomics: a (matrix, seed) pair gives the same bits
 * alone, in any batch and with any ws_bytes.
 * Checked before any device work: B, R >= 1, 4 <= N <= 96 (less: WC_EINVAL, four distinct nodes do
 * not exist; more: WC_EUNSUPPORTED), B R < 2^31, bin_swaps >= 0 and itr A < 2^31, period and neg_mode
 * in range; w, seeds, wr or w0 and the workspace not NULL; fp64 and uint64 arrays and the workspace
 * 8-byte, info 4-byte aligned; no output, the used part of the workspace included, overlapping an
 * input or another output. */
size_t wc_graph_null_model_slot_bytes(int N);
int wc_graph_rewire(int B, int R, int N, const double* w, int bin_swaps, const uint64_t* seeds,
                    double* wr, int32_t* info, void* workspace, size_t ws_bytes, void* stream);
int wc_graph_null_model(int B, int R, int N, const double* w, int bin_swaps, int period, int neg_mode,
                        const uint64_t* seeds, double* w0, double* r, int32_t* info,
                        void* workspace, size_t ws_bytes, void* stream);

/* Hub organisation of B matrices (wc_hubs.hip): the reference's rich_club_wu (graph_utils.py:2528-2570),
 * rich_club_wd (:2482-2525), rich_club_bu (:2440-2479), rich_club_bd (:2396-2437), assortativity_wei
 * (:1869-1926), assortativity_bin (:1808-1866) and score_wu (:2573-2609).  tests/hubs_reference.py
 * restates this text in numpy.
 *
 * All three: w [B][N][N] fp64, 2 <= N <= 96, one workgroup per matrix.  No symmetry is assumed and
 * the diagonal is taken as given: the expressions are evaluated as the reference writes them.  A
 * matrix with a NaN or an infinity anywhere has NaN in its fp64 outputs and -1 in its int32 outputs;
 * no other matrix is affected.  Fixed order, no atomics: a matrix gives the same bits alone as in any
 * batch.  Every output may be NULL, but not all of them.
 *
 * wc_graph_rich_club.  deg_j = the non-zeros of column j (directed == 0: rich_club_wu, degrees_und), plus
 *   the non-zeros of row j (directed != 0: rich_club_wd, degrees_dir's deg).  K levels are written,
 *   1 <= K <= N (directed == 0) or 2 N (directed != 0); level index k = 0 .. K-1 stands for the degree
 *   l = k + 1.
 *     maxdeg [B]    int32  max_j deg_j, the reference's default klevel
 *     rw     [B][K] the weighted coefficient: NaN where no node has deg < l (the reference's
 *                   `continue`); else, over the nodes with deg >= l, Wr = the sum of every entry of the
 *                   kept submatrix, both triangles and the diagonal, Er = the number of its non-zero
 *                   entries, and rw = Wr / (the sum of the Er largest of all N^2 entries of w): the first
 *                   Er of np.sort(w.flat)[::-1], in which zeros and negative entries take their place.
 *                   No node kept, or none of its entries non-zero: 0 / 0 = NaN.
 *     rb     [B][K] the binary coefficient ek / (nk (nk - 1)) as IEEE gives it (nk = 0: NaN; nk = 1:
 *                   NaN or +-inf), over the nodes with deg > l (the reference removes deg <= k + 1)
 *     nk     [B][K] int32  the number of those nodes
 *     ek     [B][K] the sum of their submatrix of w as given; the reference does not binarise it
 *   Sums: with the nodes in descending order of degree, ties by ascending index, the kept nodes are the
 *   first n; node a's shell, w[a][b] then w[b][a] for the b before it and then w[a][a], is added up
 *   over b in the order a + 1, a + 2, ... modulo N, the shells in order of a.  The sorted entries
 *   are added in blocks of 64 (a tree over xor distances 32 .. 1), the blocks and then the rest in order.
 *
 * wc_graph_assortativity.  flag 0 takes the edges i < j with w[i][j] > 0 (np.triu(w, 1) > 0), flags 1 .. 4
 *   every (i, j) with w[i][j] > 0; other flags: WC_EINVAL.  With in = column, out = row, the values a
 *   of the edge's i and b of its j are
 *     r_bin [B]  the non-zeros: flag 0 in/in (degrees_und), 1 out/in, 2 in/out, 3 out/out, 4 in/in;
 *     r_wei [B]  the sums: flag 0 in/in (strengths_und), 1 out/in, 2 in/out, 3 out/out, and flag 4
 *                in/out, THE SAME AS FLAG 2: the reference's assortativity_wei reads ist[i], ost[j]
 *                there although its docstring says in/in.  Done as written, and pinned by a test.
 *   and with E the number of edges
 *     term1 = sum(a b) / E, term2 = (sum((a + b) / 2) / E)^2, term3 = sum((a^2 + b^2) / 2) / E,
 *     r = (term1 - term2) / (term3 - term2),
 *   one rounding per operation in this order; the sums run over j within a row, then over the rows.
 *   The degree sums are exact, so r_bin is the reference's bits and a regular graph gives its exact
 *   0 / 0 = NaN.  E = 0: NaN.
 *
 * wc_graph_score.  s [B][S] fp64 levels, S >= 1, B S < 2^31.  Per (matrix, level) score_wu's loop:
 *   the strengths are the column sums of the current matrix, a column added up in row order
 *   0 .. N-1 (np.sum(axis=0) of a C-ordered matrix); all nodes with 0 < str < s are peeled together,
 *   their rows and columns going to zero; repeated until no node is peeled.
 *     member [B][S][N] int32  1 where the node was not peeled
 *     sn     [B][S]    int32  the nodes with str > 0 at the end
 *     rounds [B][S]    int32  the passes that peeled a node or more
 *   The core matrix is w with the rows and columns of the peeled nodes cleared.
 *
 * Checked before any device work: B >= 1, 2 <= N <= 96 (more: WC_EUNSUPPORTED), w not NULL, an output
 * given, K, flag and S in range, s not NULL; fp64 arrays 8-byte, int32 arrays 4-byte aligned; no output
 * overlapping an input or another output. */
int wc_graph_rich_club(int B, int N, const double* w, int directed, int K, double* rw, double* rb,
                       int32_t* nk, double* ek, int32_t* maxdeg, void* stream);
int wc_graph_assortativity(int B, int N, const double* w, int flag, double* r_wei, double* r_bin,
                           void* stream);
int wc_graph_score(int B, int N, int S, const double* w, const double* s, int32_t* member, int32_t* sn,
                   int32_t* rounds, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* WCSDE_H */

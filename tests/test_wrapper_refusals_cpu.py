"""What the Python wrappers (sigchain, utils, graph_utils; partition, nullmodel, surrogate and their numpy
facades) refuse, and their public surface, as literals recorded from the commit before their argument
handling moved into nremmodfc_amd/_args.py: the first three modules before _args.py existed, the other
six before its number gates and seeded-run helpers did (no GPU: every row is refused before the device
is touched, so CPU tensors and numpy arrays are enough).

ROWS: one row per `raise` statement of the three modules, as (id, call, exception class, exact
message), plus rows that show a shared helper under each wrapper's name.  At the recorded commit the
modules hold 89 (sigchain), 39 (utils) and 15 (graph_utils) `raise` statements, and every one of them
has a row: none needs device work to be reached.  Three are reached in an unusual way.  BoldStream.feed
and BoldStream.finish are called on a plain namespace, since a real BoldStream initialises its state on
the device; graph_module_measures' "same device" refusal takes a ci on torch's meta device; and
utils.kuramoto uploads before it looks at the shape, so its row runs with utils.device = "cpu".

The seeded modules, at their recorded commit: partition 7 `raise` statements, nullmodel 11, surrogate 7,
all with a row, most with one per way of failing the test (a bool, a float, a bound), and the shared
helpers (seeds, the matrix stack, the series) under each wrapper's name.  nullmodel_np has 11: 7 have
rows, the 3 of _refused, which reads a status the device wrote, are called directly, and "a null model
was refused" comes after device work and has none.  partition_np's 2 (consensus_und's non-finite D and
its missing consensus) both come after device work and have none; its rows show graph_utils._matrices
under its names.  surrogate_np's 2 have rows, and surrogate._test_args shows under its name.

PTR_ROWS: calls in which a CPU tensor passes every check of the wrapper and _lib.ptr refuses it.  A
wrapper that asks for the stream first (graph_measures) shows torch's own error instead, which is not a
refusal of this package and has no row.

DOUBLE_ROWS: calls that are wrong in two ways, which pin the order of the checks.  The SciPy facades
disagree among themselves (utils.welch and utils.spectrogram look at nfft before complex input,
utils.csd and utils.coherence the other way round); each keeps its own order.  utils.coherence has no
return_onesided parameter, so its second row is Python's own TypeError.  Every public wrapper of
partition, nullmodel and surrogate has a chain of rows, each wrong in its k-th and (k+1)-th check.

Then the clamped-nperseg UserWarning of welch, csd, coherence and spectrogram, which must name the
caller's file, and inspect.signature of every public callable and the value of every public constant.
graph_louvain's symmetrising warning fires after device work and is tested in test_wrapper_calls_gpu.py.
"""
import inspect
import types

import numpy as np
import pytest
import torch

from nremmodfc_amd import (_lib, graph_utils as gu, nullmodel as nm, nullmodel_np as nmn, partition as pt,
                          partition_np as ptn, sigchain as sc, surrogate as sg, surrogate_np as sgn, utils as ut)

WCSDEError = _lib.WCSDEError


def f64(*shape):
    return torch.zeros(shape, dtype=torch.float64)


def f32(*shape):
    return torch.zeros(shape, dtype=torch.float32)


def i32(*shape):
    return torch.zeros(shape, dtype=torch.int32)


def i64(*shape):
    return torch.zeros(shape, dtype=torch.int64)


def full(value, *shape):
    return torch.full(shape, value, dtype=torch.float64)


def on_cpu(fn, *args, **kw):
    """fn with utils.device = "cpu": a facade that uploads before it checks."""
    saved, ut.device = ut.device, "cpu"
    try:
        return fn(*args, **kw)
    finally:
        ut.device = saved


ns = types.SimpleNamespace
GM = "['dist', 'hops', 'charpath', 'efficiency', 'ecc', 'radius', 'diameter', 'local_efficiency', 'clustering', " \
     "'transitivity', 'strengths', 'degrees']"
GPM = "['dist', 'hops', 'charpath', 'efficiency', 'ecc', 'radius', 'diameter']"
GMM = "['participation', 'zscore', 'modularity']"
CM = "['plv', 'pli', 'wpli', 'aec', 'aec_orth']"
STACK = "w must be a [B][N][N] or [N][N] fp64 device tensor"
STACK_N = "needs B >= 1 and 2 <= N <= 96 (one matrix per workgroup, in LDS)"
X64, Z64, ONES3 = np.zeros(64), np.zeros(64, dtype=complex), np.ones((3, 3))
QT = "['sta', 'pos', 'smp', 'gja', 'neg']"
SEEDS = "seeds must be an int or a non-empty sequence of ints in [0, 2^64), got "
SERIES = "x must be a [L][N] or time-major [L][B][N] fp64 device tensor"
EVEN_L = "needs an even number of samples, at least 4 (the reference's stacked phases need an even length)"
LAB4 = [0, 0, 1, 1]

ROWS = [
    # ---- sigchain ----
    ("ptr_at", lambda: sc._ptr_at(f64(2, 2)), WCSDEError, "libwcsde takes contiguous device tensors only"),
    ("bold_short", lambda: sc.BoldStream(2, 2015), ValueError,
     "simBOLD needs at least neq + 16 samples (filtfilt padlen 15)"),
    ("bold_feed_dtype", lambda: sc.BoldStream.feed(ns(), i32(4, 2)), TypeError, "E must be float32 or float64"),
    ("bold_finish_early", lambda: sc.BoldStream.finish(ns(t=1, n_total=2)), RuntimeError,
     "BoldStream fed 1 of 2 samples"),
    ("hilbert_long_M", lambda: sc.hilbert_phase_long(f64(1, 2)), WCSDEError,
     "hilbert_phase: M = 1 outside 2 .. 524288 (or no columns)"),
    ("hilbert_env_M", lambda: sc.hilbert_envelope(f64(1, 2)), WCSDEError,
     "hilbert_envelope: M = 1 outside 2 .. 524288 (8192 for method 1), no columns or method = 0 not 0, 1, 2"),
    ("hilbert_env_method", lambda: sc.hilbert_envelope(f64(8, 2), method=3), WCSDEError,
     "hilbert_envelope: M = 8 outside 2 .. 524288 (8192 for method 1), no columns or method = 3 not 0, 1, 2"),
    ("filtfilt_ba", lambda: sc.filtfilt([1.0, 2.0], [1.0], f64(30, 2)), ValueError,
     "filtfilt: b and a must be 1-D arrays of the same length"),
    ("filtfilt_x", lambda: sc.filtfilt([1.0, 0.5], [1.0, 0.2], f32(30, 2)), TypeError,
     "filtfilt: x must be a [T][C] or [T][B][N] fp64 device tensor"),
    ("filtfilt_x_1d", lambda: sc.filtfilt([1.0, 0.5], [1.0, 0.2], f64(30)), TypeError,
     "filtfilt: x must be a [T][C] or [T][B][N] fp64 device tensor"),
    ("hma_dtype", lambda: sc.hma(f32(2, 3, 3)), WCSDEError,
     "hma: fc must be a contiguous fp64 device tensor (it is clipped in place)"),
    ("hma_strided", lambda: sc.hma(f64(2, 3, 6)[:, :, ::2]), WCSDEError,
     "hma: fc must be a contiguous fp64 device tensor (it is clipped in place)"),
    ("hma_N", lambda: sc.hma(torch.empty((1, 4097, 4097), dtype=torch.float64)), WCSDEError,
     "hma: N = 4097 > 4096 (wc_hma_modes keeps 40 B of labels per node in LDS)"),
    ("gm_unknown", lambda: sc.graph_measures(f64(3, 3), "nope"), ValueError,
     "graph_measures: unknown measure 'nope', must be one of " + GM),
    ("gm_unknown_in_list", lambda: sc.graph_measures(f64(3, 3), ["dist", "nope"]), ValueError,
     "graph_measures: unknown measure 'nope', must be one of " + GM),
    ("gm_none", lambda: sc.graph_measures(f64(3, 3), ()), ValueError,
     "graph_measures: no measure asked for, choose from " + GM),
    ("gm_lengths", lambda: sc.graph_measures(f64(3, 3), ("dist", "degrees"), lengths=True), ValueError,
     "graph_measures: lengths=True goes with the path measures " + GPM + " only, the others are defined on weights"),
    ("gm_dtype", lambda: sc.graph_measures(f32(3, 3)), TypeError, "graph_measures: " + STACK),
    ("gm_numpy", lambda: sc.graph_measures(np.zeros((3, 3))), TypeError, "graph_measures: " + STACK),
    ("gm_dim", lambda: sc.graph_measures(f64(3)), TypeError, "graph_measures: " + STACK),
    ("gm_square", lambda: sc.graph_measures(f64(2, 3, 4)), TypeError, "graph_measures: " + STACK),
    ("gm_N1", lambda: sc.graph_measures(f64(1, 1)), ValueError, "graph_measures: N = 1, B = 1: " + STACK_N),
    ("gm_N97", lambda: sc.graph_measures(f64(2, 97, 97)), ValueError, "graph_measures: N = 97, B = 2: " + STACK_N),
    ("gm_B0", lambda: sc.graph_measures(f64(0, 3, 3)), ValueError, "graph_measures: N = 3, B = 0: " + STACK_N),
    ("gb_dtype", lambda: sc.graph_betweenness(f32(3, 3)), TypeError, "graph_betweenness: " + STACK),
    ("gb_N97", lambda: sc.graph_betweenness(f64(97, 97)), ValueError, "graph_betweenness: N = 97, B = 1: " + STACK_N),
    ("gmm_unknown", lambda: sc.graph_module_measures(f64(3, 3), i32(3), "nope"), ValueError,
     "graph_module_measures: unknown measure 'nope', must be one of " + GMM),
    ("gmm_none", lambda: sc.graph_module_measures(f64(3, 3), i32(3), []), ValueError,
     "graph_module_measures: no measure asked for, choose from " + GMM),
    ("gmm_degree", lambda: sc.graph_module_measures(f64(3, 3), i32(3), degree="both"), ValueError,
     "graph_module_measures: degree 'both', must be one of ['undirected', 'out', 'in']"),
    ("gmm_zflag", lambda: sc.graph_module_measures(f64(3, 3), i32(3), zflag=4), ValueError,
     "graph_module_measures: zflag 4, must be 0, 1, 2 or 3"),
    ("gmm_zflag_bool", lambda: sc.graph_module_measures(f64(3, 3), i32(3), zflag=True), ValueError,
     "graph_module_measures: zflag True, must be 0, 1, 2 or 3"),
    ("gmm_w", lambda: sc.graph_module_measures(f32(3, 3), i32(3)), TypeError, "graph_module_measures: " + STACK),
    ("gmm_w_N", lambda: sc.graph_module_measures(f64(1, 1), i32(1)), ValueError,
     "graph_module_measures: N = 1, B = 1: " + STACK_N),
    ("gmm_ci_dtype", lambda: sc.graph_module_measures(f64(3, 3), i64(3)), TypeError,
     "graph_module_measures: ci must be an int32 device tensor [N] or [B][N] with N = 3, B = 1"),
    ("gmm_ci_shape", lambda: sc.graph_module_measures(f64(2, 3, 3), i32(3, 3)), TypeError,
     "graph_module_measures: ci must be an int32 device tensor [N] or [B][N] with N = 3, B = 2"),
    ("gmm_n_modules", lambda: sc.graph_module_measures(f64(3, 3), i32(3), n_modules=0), ValueError,
     "graph_module_measures: n_modules = 0, must be in [1, N = 3]"),
    ("gmm_device", lambda: sc.graph_module_measures(f64(3, 3), torch.zeros(3, dtype=torch.int32, device="meta")),
     ValueError, "graph_module_measures: ci and w must be on the same device"),
    ("gl_seeds", lambda: sc.graph_louvain(f64(3, 3), seeds=-1), ValueError,
     "graph_louvain: seeds must be an int or a non-empty sequence of ints in [0, 2^64), got -1"),
    ("gl_seeds_empty", lambda: sc.graph_louvain(f64(3, 3), seeds=[]), ValueError,
     "graph_louvain: seeds must be an int or a non-empty sequence of ints in [0, 2^64), got []"),
    ("gl_ci", lambda: sc.graph_louvain(f64(3, 3), ci=i32(4)), TypeError,
     "graph_louvain: ci must hold integer labels, [N] or [B][N] with N = 3, B = 1"),
    ("gl_ci_float", lambda: sc.graph_louvain(f64(3, 3), ci=[0.5, 1.0, 2.0]), TypeError,
     "graph_louvain: ci must hold integer labels, [N] or [B][N] with N = 3, B = 1"),
    ("gl_objective", lambda: sc.graph_louvain(f64(3, 3), objective="nope"), ValueError,
     "graph_louvain: objective 'nope', must be one of ['modularity', 'potts'] or a [N][N] / [B][N][N] fp64 device "
     "tensor (negative_sym and negative_asym are not built: the reference refuses negative weights before it "
     "reaches them)"),
    ("gl_objective_tensor", lambda: sc.graph_louvain(f64(3, 3), objective=f32(3, 3)), TypeError,
     "graph_louvain: an objective tensor must be fp64 [N][N] or [B][N][N] on w's device, N = 3, B = 1"),
    ("gl_w", lambda: sc.graph_louvain(f32(3, 3)), TypeError, "graph_louvain: " + STACK),
    ("gl_negative", lambda: sc.graph_louvain(full(-1.0, 3, 3)), ValueError,
     "graph_louvain: w must not contain negative weights (an entry below -1e-10)"),
    ("gl_potts", lambda: sc.graph_louvain(full(0.5, 3, 3), objective="potts"), ValueError,
     "graph_louvain: the Potts objective requires a binary w"),
    ("ga_dtype", lambda: sc.graph_agreement(i64(2, 3)), TypeError,
     "graph_agreement: ci must be an int32 device tensor [B][R][N] or [R][N]"),
    ("ga_dim", lambda: sc.graph_agreement(i32(3)), TypeError,
     "graph_agreement: ci must be an int32 device tensor [B][R][N] or [R][N]"),
    ("ga_N", lambda: sc.graph_agreement(i32(2, 1)), ValueError,
     "graph_agreement: N = 1, R = 2, B = 1: needs B, R >= 1 and 2 <= N <= 96"),
    ("gc_reps", lambda: sc.graph_consensus_matrix(f64(3, 3), reps=0), ValueError,
     "graph_consensus_matrix: reps = 0, must be a positive int"),
    ("gc_seeds", lambda: sc.graph_consensus_matrix(f64(3, 3), reps=2, seeds=[1]), ValueError,
     "graph_consensus_matrix: seeds must be a sequence of length reps, or None"),
    ("gc_w", lambda: sc.graph_consensus_matrix(f32(3, 3), reps=2), TypeError, "graph_louvain: " + STACK),
    ("fcd_method", lambda: sc.fcd(f64(12, 3), 4, method="nope"), ValueError,
     "fcd: unknown method 'nope', must be one of ['corr', 'phase']"),
    ("fcd_dtype", lambda: sc.fcd(f32(12, 3), 4), TypeError, "fcd: x must be a [M][C] or [M][B][N] fp64 device tensor"),
    ("fcd_dim", lambda: sc.fcd(f64(12), 4), TypeError, "fcd: x must be a [M][C] or [M][B][N] fp64 device tensor"),
    ("fcd_N97", lambda: sc.fcd(f64(12, 97), 4), ValueError,
     "fcd: N = 97, B = 1: needs B >= 1 and N <= 96 (one window's correlation matrix, a tile's phasors per "
     "workgroup)"),
    ("fcd_phase_window", lambda: sc.fcd(f64(12, 3), window=4, method="phase"), ValueError,
     "fcd: method='phase' has no windows: window and step must be left None"),
    ("fcd_phase_windows", lambda: sc.fcd(f64(12, 3), method="phase", want_windows=True), ValueError,
     "fcd: method='phase' takes neither want_windows nor ws_bytes"),
    ("fcd_phase_trim", lambda: sc.fcd(f64(12, 3), method="phase", trim=6), ValueError,
     "fcd: method='phase' needs N >= 2, trim >= 0 and 1 <= M - 2 trim <= 4096 (N = 3, M = 12, trim = 6)"),
    ("fcd_corr_trim", lambda: sc.fcd(f64(12, 3), 4, trim=1), ValueError,
     "fcd: method='corr' takes no trim (it goes with method='phase')"),
    ("fcd_corr_window", lambda: sc.fcd(f64(12, 3)), ValueError, "fcd: method='corr' needs a window length"),
    ("fcd_corr_N", lambda: sc.fcd(f64(12, 2), 4), ValueError,
     "fcd: method='corr' needs N >= 3, 2 <= window <= M and step >= 1 (N = 2, M = 12, window = 4, step = 1)"),
    ("fcd_corr_nw", lambda: sc.fcd(f64(5000, 3), 2), ValueError, "fcd: 4999 windows > 4096: take a larger step"),
    ("fcdp_shape", lambda: sc.fcd_from_phasors(f64(4, 3, 3)), TypeError,
     "fcd_from_phasors: phasor must be a [M][C][2] or [M][B][N][2] fp64 device tensor"),
    ("fcdp_N", lambda: sc.fcd_from_phasors(f64(4, 1, 2)), ValueError,
     "fcd_from_phasors: N = 1, B = 1, M = 4: needs B >= 1, 2 <= N <= 96 and 1 <= M <= 4096"),
    ("fcdks_dtype", lambda: sc.fcd_ks(f32(3, 3), [0.1]), TypeError,
     "fcd_ks: fcd must be a [B][nw][nw] or [nw][nw] fp64 device tensor"),
    ("fcdks_lag", lambda: sc.fcd_ks(f64(3, 3), [0.1], lag=3), ValueError, "fcd_ks: lag = 3 must be in 1 .. nw - 1 = 2"),
    ("fcdks_emp", lambda: sc.fcd_ks(f64(3, 3), []), ValueError,
     "fcd_ks: emp_values must be a 1-D sample without NaN, not empty"),
    ("leida_dtype", lambda: sc.leida(f32(4, 3)), TypeError, "leida: x must be a [M][C] or [M][B][N] fp64 device tensor"),
    ("leida_N", lambda: sc.leida(f64(4, 1)), ValueError,
     "leida: needs B >= 1, 2 <= N <= 1024, trim >= 0, M >= 2 and M - 2 trim >= 1 (N = 1, B = 1, M = 4, trim = 0)"),
    ("leidap_shape", lambda: sc.leida_from_phasors(f64(4, 3, 3)), TypeError,
     "leida_from_phasors: phasor must be a [M][N][2] or [M][B][N][2] fp64 device tensor"),
    ("leidap_N", lambda: sc.leida_from_phasors(f64(4, 1, 2)), ValueError,
     "leida_from_phasors: N = 1, 4 rows: needs at least one row and 2 <= N <= 1024"),
    ("ka_metric", lambda: sc.kmeans_assign(f64(4, 2), f64(2, 2), "nope"), ValueError,
     "kmeans_assign: unknown metric 'nope', must be one of ['sqeuclidean', 'cosine']"),
    ("ka_x", lambda: sc.kmeans_assign(f32(4, 2), f64(2, 2)), TypeError,
     "kmeans_assign: x must be a [R][N] or [M][B][N] fp64 device tensor"),
    ("ka_centroids", lambda: sc.kmeans_assign(f64(4, 2), f64(2)), TypeError,
     "kmeans_assign: centroids must be a [K][N] fp64 device tensor"),
    ("ka_nodes", lambda: sc.kmeans_assign(f64(4, 2), f64(2, 3)), ValueError,
     "kmeans_assign: centroids have 3 nodes, x has N = 2"),
    ("ka_N", lambda: sc.kmeans_assign(f64(4, 1), f64(2, 1)), ValueError,
     "kmeans_assign: N = 1: needs at least one row and 2 <= N <= 1024"),
    ("ka_K", lambda: sc.kmeans_assign(f64(4, 2), f64(33, 2)), ValueError, "kmeans_assign: K = 33: needs 1 <= K <= 32"),
    ("ku_x", lambda: sc.kmeans_update(f32(4, 2), i32(4), f64(2, 2)), TypeError,
     "kmeans_update: x must be a [R][N] or [M][B][N] fp64 device tensor"),
    ("ku_labels", lambda: sc.kmeans_update(f64(4, 2), i64(4), f64(2, 2)), TypeError,
     "kmeans_update: labels must be an int32 device tensor shaped as x without its last axis"),
    ("ku_labels_shape", lambda: sc.kmeans_update(f64(4, 2), i32(3), f64(2, 2)), TypeError,
     "kmeans_update: labels must be an int32 device tensor shaped as x without its last axis"),
    ("ls_centroids", lambda: sc.leida_states(f64(4, 2), f32(2, 2)), TypeError,
     "leida_states: centroids must be a [K][N] fp64 device tensor"),
    ("km_init_n_init", lambda: sc.kmeans(f64(4, 2), f64(2, 2), n_init=2), ValueError,
     "kmeans: explicit initial centroids go with n_init = 1"),
    ("km_init_nodes", lambda: sc.kmeans(f64(4, 2), f64(2, 3)), ValueError,
     "kmeans: centroids have 3 nodes, x has N = 2"),
    ("km_k_type", lambda: sc.kmeans(f64(4, 2), 2.5), TypeError,
     "kmeans: k_or_init must be an integer k or initial centroids, a [K][N] fp64 device tensor"),
    ("km_k_bool", lambda: sc.kmeans(f64(4, 2), True), TypeError,
     "kmeans: k_or_init must be an integer k or initial centroids, a [K][N] fp64 device tensor"),
    ("km_K", lambda: sc.kmeans(f64(4, 2), 0), ValueError, "kmeans: K = 0: needs 1 <= K <= 32"),
    ("km_n_init", lambda: sc.kmeans(f64(4, 2), 2, n_init=0), ValueError, "kmeans: n_init = 0 < 1"),
    ("km_max_iter", lambda: sc.kmeans(f64(4, 2), 2, max_iter=-1), ValueError, "kmeans: max_iter = -1 < 0"),
    ("km_x", lambda: sc.kmeans(f32(4, 2), 2), TypeError, "kmeans: x must be a [R][N] or [M][B][N] fp64 device tensor"),
    ("km_pool", lambda: sc.kmeans(full(float("nan"), 1, 2), 1), ValueError,
     "kmeans: 0 rows without NaN or infinity, fewer than k = 1"),
    ("ss_dtype", lambda: sc.state_stats(i64(20), 2), TypeError,
     "state_stats: labels must be a [M][B] or [M] int32 device tensor"),
    ("ss_K", lambda: sc.state_stats(i32(20), 40), ValueError,
     "state_stats: M = 20, B = 1, K = 40: needs M >= 1, B >= 1 and 1 <= K <= 32"),
    ("skl_p", lambda: sc.state_kl(f32(3), [0.2, 0.3, 0.5]), TypeError, "state_kl: p must be a [B][K] or [K] fp64 tensor"),
    ("skl_q", lambda: sc.state_kl(f64(3), [0.5, 0.5]), ValueError, "state_kl: q must be one row of K = 3 entries"),
    ("welch_detrend", lambda: sc.welch(f64(64, 2), detrend="linear"), NotImplementedError,
     "welch: detrend = 'linear' (only 'constant' and False run on the device)"),
    ("csd_detrend", lambda: sc.csd(f64(64, 2), detrend="linear"), NotImplementedError,
     "csd: detrend = 'linear' (only 'constant' and False run on the device)"),
    ("coherence_detrend", lambda: sc.coherence(f64(64, 2), detrend="linear"), NotImplementedError,
     "coherence: detrend = 'linear' (only 'constant' and False run on the device)"),
    ("spectrogram_detrend", lambda: sc.spectrogram(f64(64, 2), detrend="linear"), NotImplementedError,
     "spectrogram: detrend = 'linear' (only 'constant' and False run on the device)"),
    ("welch_scaling", lambda: sc.welch(f64(64, 2), scaling="nope"), ValueError, "Unknown scaling: 'nope'"),
    ("welch_nperseg", lambda: sc.welch(f64(64, 2), nperseg=0), ValueError, "nperseg must be a positive integer"),
    ("welch_window_2d", lambda: sc.welch(f64(64, 2), window=np.ones((2, 2))), ValueError, "window must be 1-D"),
    ("welch_window_long", lambda: sc.welch(f64(64, 2), window=np.ones(65)), ValueError,
     "window is longer than input signal"),
    ("welch_window_nperseg", lambda: sc.welch(f64(64, 2), window=np.ones(8), nperseg=4), ValueError,
     "value specified for nperseg is different from length of window"),
    ("welch_noverlap", lambda: sc.welch(f64(64, 2), nperseg=8, noverlap=8), ValueError,
     "noverlap must be less than nperseg."),
    ("welch_x", lambda: sc.welch(f32(64, 2)), TypeError, "welch: x must be a [T][C] or [T][B][N] fp64 device tensor"),
    ("welch_x_1d", lambda: sc.welch(f64(64)), TypeError, "welch: x must be a [T][C] or [T][B][N] fp64 device tensor"),
    ("csd_x", lambda: sc.csd(f64(64, 2, 2)), TypeError, "csd: x must be a [T][C] fp64 device tensor"),
    ("coherence_x", lambda: sc.coherence(f32(64, 2)), TypeError, "coherence: x must be a [T][C] fp64 device tensor"),
    ("csd_y", lambda: sc.csd(f64(64, 2), f64(64, 3)), TypeError,
     "csd: y must be an fp64 tensor of x's shape on x's device"),
    ("coherence_y", lambda: sc.coherence(f64(64, 2), f32(64, 2)), TypeError,
     "coherence: y must be an fp64 tensor of x's shape on x's device"),
    ("spectrogram_phase", lambda: sc.spectrogram(f64(64, 2), mode="phase"), NotImplementedError,
     "spectrogram: mode = 'phase' (unwrapped angles) does not run on the device; utils.spectrogram unwraps the "
     "device's angles on the host"),
    ("spectrogram_mode", lambda: sc.spectrogram(f64(64, 2), mode="nope"), ValueError,
     "unknown value for mode nope, must be one of ['psd', 'complex', 'magnitude', 'angle', 'phase']"),
    ("spectrogram_x", lambda: sc.spectrogram(f32(64, 2)), TypeError,
     "spectrogram: x must be a [T][C] or [T][B][N] fp64 device tensor"),
    ("pcf_unknown", lambda: sc.phase_connectivity_from(f64(8, 3, 2), measures="nope"), ValueError,
     "phase_connectivity_from: unknown measure 'nope', must be one of " + CM),
    ("pcf_none", lambda: sc.phase_connectivity_from(f64(8, 3, 2), measures=()), ValueError,
     "phase_connectivity_from: no measure asked for, choose from " + CM),
    ("pc_unknown", lambda: sc.phase_connectivity(f64(8, 3), ("plv", "nope")), ValueError,
     "phase_connectivity: unknown measure 'nope', must be one of " + CM),
    ("pcf_phasor", lambda: sc.phase_connectivity_from(f64(8, 3)), TypeError,
     "phase_connectivity_from: phasor must be a [T][C][2] or [T][B][N][2] fp64 device tensor"),
    ("pcf_amp", lambda: sc.phase_connectivity_from(f64(8, 3, 2)), TypeError,
     "phase_connectivity_from: wpli, aec and aec_orth need amp, an fp64 tensor of the phasors' [T][C] or [T][B][N] "
     "on their device"),
    ("pcf_amp_shape", lambda: sc.phase_connectivity_from(f64(8, 3, 2), f64(8, 4), "aec"), TypeError,
     "phase_connectivity_from: wpli, aec and aec_orth need amp, an fp64 tensor of the phasors' [T][C] or [T][B][N] "
     "on their device"),
    ("pc_x", lambda: sc.phase_connectivity(f32(8, 3)), TypeError,
     "phase_connectivity: x must be a [T][C] or [T][B][N] fp64 device tensor"),
    # ---- utils ----
    ("u_envelope", lambda: ut.envelope(np.zeros((4, 2, 2))), ValueError, "series must be (time,) or (time, rois)"),
    ("u_welch_nfft", lambda: ut.welch(X64, nperseg=8, nfft=16), NotImplementedError,
     "welch: nfft other than nperseg (zero padding) does not run on the device"),
    ("u_welch_nfft_clamped", lambda: ut.welch(X64, nperseg=128, nfft=128), NotImplementedError,
     "welch: nfft other than nperseg (zero padding) does not run on the device"),
    ("u_welch_onesided", lambda: ut.welch(X64, return_onesided=False), NotImplementedError,
     "welch: return_onesided=False does not run on the device"),
    ("u_welch_average", lambda: ut.welch(X64, average="median"), NotImplementedError,
     "welch: average = 'median' (only 'mean' runs on the device)"),
    ("u_welch_detrend", lambda: ut.welch(X64, detrend="linear"), NotImplementedError,
     "welch: detrend = 'linear' (only 'constant' and False run on the device)"),
    ("u_welch_complex", lambda: ut.welch(Z64), NotImplementedError, "welch: complex input x does not run on the device"),
    ("u_welch_empty", lambda: ut.welch(np.zeros(0)), ValueError, "welch: x must have at least one sample"),
    ("u_spec_mode", lambda: ut.spectrogram(X64, mode="nope"), ValueError,
     "unknown value for mode nope, must be one of ['psd', 'complex', 'magnitude', 'angle', 'phase']"),
    ("u_spec_nfft", lambda: ut.spectrogram(X64, nperseg=8, nfft=16), NotImplementedError,
     "spectrogram: nfft other than nperseg (zero padding) does not run on the device"),
    ("u_spec_onesided", lambda: ut.spectrogram(X64, return_onesided=False), NotImplementedError,
     "spectrogram: return_onesided=False does not run on the device"),
    ("u_spec_detrend", lambda: ut.spectrogram(X64, detrend="linear"), NotImplementedError,
     "spectrogram: detrend = 'linear' (only 'constant' and False run on the device)"),
    ("u_spec_complex", lambda: ut.spectrogram(Z64), NotImplementedError,
     "spectrogram: complex input x does not run on the device"),
    ("u_spec_empty", lambda: ut.spectrogram(np.zeros(0)), ValueError, "spectrogram: x must have at least one sample"),
    ("u_csd_complex", lambda: ut.csd(X64, Z64), NotImplementedError, "csd: complex input does not run on the device"),
    ("u_coh_complex", lambda: ut.coherence(Z64, X64), NotImplementedError,
     "coherence: complex input does not run on the device"),
    ("u_csd_shapes", lambda: ut.csd(X64, np.zeros(32)), NotImplementedError,
     "csd: x and y of different shapes or lengths (broadcasting, zero padding of the shorter) do not run on the "
     "device"),
    ("u_coh_shapes", lambda: ut.coherence(X64, np.zeros(32)), NotImplementedError,
     "coherence: x and y of different shapes or lengths (broadcasting, zero padding of the shorter) do not run on "
     "the device"),
    ("u_csd_empty", lambda: ut.csd(np.zeros(0), np.zeros(0)), ValueError, "csd: x must have at least one sample"),
    ("u_coh_empty", lambda: ut.coherence(np.zeros(0), np.zeros(0)), ValueError,
     "coherence: x must have at least one sample"),
    ("u_csd_nfft", lambda: ut.csd(X64, X64, nperseg=8, nfft=16), NotImplementedError,
     "csd: nfft other than nperseg (zero padding) does not run on the device"),
    ("u_coh_nfft", lambda: ut.coherence(X64, X64, window=np.ones(8), nfft=16), NotImplementedError,
     "coherence: nfft other than nperseg (zero padding) does not run on the device"),
    ("u_csd_onesided", lambda: ut.csd(X64, X64, return_onesided=False), NotImplementedError,
     "csd: return_onesided=False does not run on the device"),
    ("u_csd_average", lambda: ut.csd(X64, X64, average="median"), NotImplementedError,
     "csd: average = 'median' (only 'mean' runs on the device)"),
    ("u_csd_detrend", lambda: ut.csd(X64, X64, detrend="linear"), NotImplementedError,
     "csd: detrend = 'linear' (only 'constant' and False run on the device)"),
    ("u_coh_detrend", lambda: ut.coherence(X64, X64, detrend=True), NotImplementedError,
     "coherence: detrend = True (only 'constant' and False run on the device)"),
    ("u_csdm_complex", lambda: ut.csd_matrix(np.zeros((64, 2), dtype=complex)), NotImplementedError,
     "csd_matrix: complex input does not run on the device"),
    ("u_cohm_complex", lambda: ut.coherence_matrix(np.zeros((64, 2), dtype=complex)), NotImplementedError,
     "coherence_matrix: complex input does not run on the device"),
    ("u_csdm_detrend", lambda: ut.csd_matrix(np.zeros((64, 2)), detrend="linear"), NotImplementedError,
     "csd_matrix: detrend = 'linear' (only 'constant' and False run on the device)"),
    ("u_cohm_detrend", lambda: ut.coherence_matrix(np.zeros((64, 2)), detrend="linear"), NotImplementedError,
     "coherence_matrix: detrend = 'linear' (only 'constant' and False run on the device)"),
    ("u_csdm_shape", lambda: ut.csd_matrix(X64), ValueError, "csd_matrix: x must be (time, rois)"),
    ("u_cohm_shape", lambda: ut.coherence_matrix(np.zeros((0, 2))), ValueError, "coherence_matrix: x must be (time, rois)"),
    ("u_conn_measures", lambda: ut.connectivity(np.zeros((30, 3)), measures="nope"), ValueError,
     "connectivity: unknown measure 'nope', must be one of " + CM),
    ("u_conn_none", lambda: ut.connectivity(np.zeros((30, 3)), measures=[]), ValueError,
     "connectivity: no measure asked for, choose from " + CM),
    ("u_conn_dtype", lambda: ut.connectivity(np.zeros((30, 3), dtype=complex)), TypeError,
     "connectivity: series must be real numbers, not complex128"),
    ("u_conn_shape", lambda: ut.connectivity(np.zeros(30)), ValueError, "series must be (time, rois) or (time, B, N)"),
    ("u_conn_freqs", lambda: ut.connectivity(np.zeros((30, 3)), freqs=[8]), ValueError,
     "freqs must be [fmin, fmax] or None"),
    ("u_fcd_dtype", lambda: ut.fcd(np.zeros((30, 3), dtype=complex)), TypeError,
     "fcd: series must be real numbers, not complex128"),
    ("u_fcd_shape", lambda: ut.fcd(np.zeros((0, 3))), ValueError, "series must be (time, rois) or (time, B, N)"),
    ("u_fcd_method", lambda: ut.fcd(np.zeros((30, 3)), method="nope"), ValueError,
     "fcd: unknown method 'nope', must be one of ['corr', 'phase']"),
    ("u_leida_dtype", lambda: ut.leida(np.zeros((30, 3), dtype="U1"), 0.002, None), TypeError,
     "leida: series must be real numbers, not <U1"),
    ("u_leida_shape", lambda: ut.leida(np.zeros(30), 0.002, None), ValueError,
     "series must be (time, rois) or (time, B, N)"),
    ("u_leida_freqs", lambda: ut.leida(np.zeros((30, 3)), 0.002, [8, 13, 20]), ValueError,
     "freqs must be [fmin, fmax] or None"),
    ("u_leida_metric", lambda: ut.leida(np.zeros((30, 3)), 0.002, None, metric="nope"), ValueError,
     "leida: unknown metric 'nope', must be one of ['sqeuclidean', 'cosine']"),
    ("u_leida_both", lambda: ut.leida(np.zeros((30, 3)), 0.002, None, centroids=np.zeros((2, 3)), k=2), ValueError,
     "leida: give centroids or k, not both"),
    ("u_leida_k", lambda: ut.leida(np.zeros((30, 3)), 0.002, None, k=33), ValueError,
     "leida: K = 33: needs 1 <= K <= 32"),
    ("u_leida_centroids", lambda: ut.leida(np.zeros((30, 3)), 0.002, None, centroids=np.zeros((2, 4))), ValueError,
     "leida: centroids must be (K, N = 3) with 1 <= K <= 32"),
    ("u_leida_N", lambda: ut.leida(np.zeros((8, 1)), 0.002, None), ValueError,
     "leida: needs 2 <= N <= 1024, trim >= 0 and time - 2 trim >= 1 (N = 1, time = 8, trim = 0)"),
    ("u_kuramoto", lambda: on_cpu(ut.kuramoto, np.zeros(5)), ValueError, "sign must be (time, nodes)"),
    ("u_metrics", lambda: ut.get_all_metrics(np.zeros((3, 3)), np.zeros((4, 4))), ValueError,
     "sFC and empFC must be square matrices of the same shape"),
    # ---- graph_utils ----
    ("g_thresholding", lambda: gu.thresholding(np.zeros((3, 3)), direct="x"), ValueError,
     "Invalid type of matrix -> direct options: undirected or directed"),
    ("g_N", lambda: gu.clustering_coef_wu(np.zeros((1, 1))), ValueError,
     "clustering_coef_wu: N = 1, the device kernels take 2 <= N <= 96"),
    ("g_N97", lambda: gu.betweenness_bin(np.zeros((2, 97, 97))), ValueError,
     "betweenness_bin: N = 97, the device kernels take 2 <= N <= 96"),
    ("g_negative", lambda: gu.distance_wei(-ONES3), ValueError,
     "distance_wei: negative or NaN entries (the shortest paths are undefined)"),
    ("g_nan", lambda: gu.efficiency_wei(ONES3 * np.nan), ValueError,
     "efficiency_wei: negative or NaN entries (the shortest paths are undefined)"),
    ("g_betweenness_negative", lambda: gu.betweenness_wei(-ONES3), ValueError,
     "betweenness_wei: negative or NaN entries (the shortest paths are undefined)"),
    ("g_labels", lambda: gu.participation_coef(ONES3, [0, 1]), ValueError,
     "participation_coef: ci needs one label per node, [N] or [B, N] with a stack, got shape (2,) for matrices of "
     "shape (3, 3)"),
    ("g_labels_zscore", lambda: gu.module_degree_zscore(ONES3, np.zeros((2, 3))), ValueError,
     "module_degree_zscore: ci needs one label per node, [N] or [B, N] with a stack, got shape (2, 3) for matrices "
     "of shape (3, 3)"),
    ("g_degree", lambda: gu.participation_coef(ONES3, [0, 1, 1], degree="both"), ValueError,
     "participation_coef: degree 'both', must be 'undirected', 'in' or 'out'"),
    ("g_flag", lambda: gu.module_degree_zscore(ONES3, [0, 1, 1], flag=4), ValueError,
     "module_degree_zscore: flag 4, must be 0, 1, 2 or 3"),
    ("g_louvain_negative", lambda: gu.community_louvain(-ONES3), ValueError,
     "community_louvain: adjmat must not contain negative weights"),
    ("g_louvain_negative_sym", lambda: gu.community_louvain(ONES3, B="negative_sym"), ValueError,
     "community_louvain: B = 'negative_sym' is not built: the reference refuses negative weights before it reaches "
     "that objective"),
    ("g_louvain_unknown", lambda: gu.community_louvain(ONES3, B="nope"), ValueError,
     "community_louvain: unknown objective function type 'nope', must be 'modularity', 'potts' or a matrix"),
    ("g_louvain_potts", lambda: gu.community_louvain(0.5 * ONES3, B="potts"), ValueError,
     "community_louvain: Potts hamiltonian requires binary input matrix"),
    ("g_louvain_matrix", lambda: gu.community_louvain(ONES3, B=np.zeros((2, 2))), ValueError,
     "community_louvain: objective function matrix does not match size of adjacency matrix"),
    ("g_louvain_labels", lambda: gu.community_louvain(ONES3, ci=[0, 1]), ValueError,
     "community_louvain: ci needs one label per node, [N] or [B, N] with a stack, got shape (2,) for matrices of "
     "shape (3, 3)"),
    ("g_consensus_negative", lambda: gu.get_agreement_matrix(-ONES3), ValueError,
     "get_agreement_matrix: adjmat must not contain negative weights"),
    ("g_agreement_shape", lambda: gu.agreement(np.zeros(3)), ValueError,
     "agreement: ci needs [vertex x partition], or a [B, N, M] stack, got shape (3,)"),
    ("g_agreement_N", lambda: gu.agreement(np.zeros((1, 2))), ValueError,
     "agreement: N = 1, the device kernels take 2 <= N <= 96"),
    ("g_consensus_seeds", lambda: gu.get_agreement_matrix(ONES3, reps=2, seeds=[1]), ValueError,
     "get_agreement_matrix: seeds must be an array of length equal to reps, or None"),
    # ---- partition ----
    ("pt_sign_qtype", lambda: pt.graph_louvain_sign(f64(3, 3), qtype="nope"), ValueError,
     "graph_louvain_sign: modularity type unknown: qtype 'nope', must be one of " + QT),
    ("pt_sign_qtype_int", lambda: pt.graph_louvain_sign(f64(3, 3), qtype=0), ValueError,
     "graph_louvain_sign: modularity type unknown: qtype 0, must be one of " + QT),
    ("pt_sign_gamma_inf", lambda: pt.graph_louvain_sign(f64(3, 3), gamma=float("inf")), ValueError,
     "graph_louvain_sign: gamma = inf, must be a finite number"),
    ("pt_sign_gamma_bool", lambda: pt.graph_louvain_sign(f64(3, 3), gamma=True), ValueError,
     "graph_louvain_sign: gamma = True, must be a finite number"),
    ("pt_sign_gamma_str", lambda: pt.graph_louvain_sign(f64(3, 3), gamma="1"), ValueError,
     "graph_louvain_sign: gamma = '1', must be a finite number"),
    ("pt_sign_seeds", lambda: pt.graph_louvain_sign(f64(3, 3), seeds=-1), ValueError, "graph_louvain_sign: " + SEEDS + "-1"),
    ("pt_sign_seeds_empty", lambda: pt.graph_louvain_sign(f64(3, 3), seeds=[]), ValueError,
     "graph_louvain_sign: " + SEEDS + "[]"),
    ("pt_sign_seeds_bool", lambda: pt.graph_louvain_sign(f64(3, 3), seeds=[0, True]), ValueError,
     "graph_louvain_sign: " + SEEDS + "[0, True]"),
    ("pt_sign_seeds_2_64", lambda: pt.graph_louvain_sign(f64(3, 3), seeds=[1 << 64]), ValueError,
     "graph_louvain_sign: " + SEEDS + "[18446744073709551616]"),
    ("pt_sign_seeds_set", lambda: pt.graph_louvain_sign(f64(3, 3), seeds={1}), ValueError,
     "graph_louvain_sign: " + SEEDS + "{1}"),
    ("pt_sign_w", lambda: pt.graph_louvain_sign(f32(3, 3)), TypeError, "graph_louvain_sign: " + STACK),
    ("pt_sign_N97", lambda: pt.graph_louvain_sign(f64(2, 97, 97)), ValueError,
     "graph_louvain_sign: N = 97, B = 2: " + STACK_N),
    ("pt_sign_ws", lambda: pt.graph_louvain_sign(f64(3, 3), ws_bytes=143), ValueError,
     "graph_louvain_sign: ws_bytes = 143, needs at least one slot of 16 N^2 = 144 bytes"),
    ("pt_sign_ws_bool", lambda: pt.graph_louvain_sign(f64(3, 3), ws_bytes=True), ValueError,
     "graph_louvain_sign: ws_bytes = True, needs at least one slot of 16 N^2 = 144 bytes"),
    ("pt_sign_ws_float", lambda: pt.graph_louvain_sign(f64(3, 3), ws_bytes=144.0), ValueError,
     "graph_louvain_sign: ws_bytes = 144.0, needs at least one slot of 16 N^2 = 144 bytes"),
    ("pt_consensus_reps", lambda: pt.graph_consensus(f64(3, 3), 0.5, reps=0), ValueError,
     "graph_consensus: reps = 0, must be a positive int"),
    ("pt_consensus_reps_float", lambda: pt.graph_consensus(f64(3, 3), 0.5, reps=2.0), ValueError,
     "graph_consensus: reps = 2.0, must be a positive int"),
    ("pt_consensus_max_iter", lambda: pt.graph_consensus(f64(3, 3), 0.5, reps=2, max_iter=0), ValueError,
     "graph_consensus: max_iter = 0, must be a positive int"),
    ("pt_consensus_max_iter_bool", lambda: pt.graph_consensus(f64(3, 3), 0.5, reps=2, max_iter=True), ValueError,
     "graph_consensus: max_iter = True, must be a positive int"),
    ("pt_consensus_tau", lambda: pt.graph_consensus(f64(3, 3), float("nan"), reps=2), ValueError,
     "graph_consensus: tau = nan, must be a finite number"),
    ("pt_consensus_tau_none", lambda: pt.graph_consensus(f64(3, 3), None, reps=2), ValueError,
     "graph_consensus: tau = None, must be a finite number"),
    ("pt_consensus_seeds_len", lambda: pt.graph_consensus(f64(3, 3), 0.5, reps=2, seeds=[1]), ValueError,
     "graph_consensus: seeds must be a sequence of length reps = 2, or None"),
    ("pt_consensus_seeds_int", lambda: pt.graph_consensus(f64(3, 3), 0.5, reps=2, seeds=3), ValueError,
     "graph_consensus: seeds must be a sequence of length reps = 2, or None"),
    ("pt_consensus_seeds_value", lambda: pt.graph_consensus(f64(3, 3), 0.5, reps=2, seeds=[-1, 0]), ValueError,
     "graph_consensus: " + SEEDS + "[-1, 0]"),
    ("pt_consensus_D", lambda: pt.graph_consensus(f32(3, 3), 0.5, reps=2), TypeError, "graph_consensus: " + STACK),
    # ---- nullmodel ----
    ("nm_rewire_N", lambda: nm.graph_rewire(f64(3, 3)), ValueError,
     "graph_rewire: N = 3, a rewiring takes four distinct nodes: needs N >= 4"),
    ("nm_rewire_w", lambda: nm.graph_rewire(f32(4, 4)), TypeError, "graph_rewire: " + STACK),
    ("nm_rewire_N97", lambda: nm.graph_rewire(f64(97, 97)), ValueError, "graph_rewire: N = 97, B = 1: " + STACK_N),
    ("nm_rewire_seeds", lambda: nm.graph_rewire(f64(4, 4), seeds=1.0), ValueError, "graph_rewire: " + SEEDS + "1.0"),
    ("nm_rewire_swaps", lambda: nm.graph_rewire(f64(4, 4), bin_swaps=-1), ValueError,
     "graph_rewire: bin_swaps = -1, must be an int >= 0"),
    ("nm_rewire_swaps_bool", lambda: nm.graph_rewire(f64(4, 4), bin_swaps=True), ValueError,
     "graph_rewire: bin_swaps = True, must be an int >= 0"),
    ("nm_rewire_swaps_float", lambda: nm.graph_rewire(f64(4, 4), bin_swaps=1.0), ValueError,
     "graph_rewire: bin_swaps = 1.0, must be an int >= 0"),
    ("nm_rewire_swaps_2_31", lambda: nm.graph_rewire(f64(4, 4), bin_swaps=119304648), ValueError,
     "graph_rewire: bin_swaps = 119304648: its iterations times 3 attempts reach 2^31"),
    ("nm_rewire_swaps_2_31_odd", lambda: nm.graph_rewire(f64(5, 5), bin_swaps=71582789), ValueError,
     "graph_rewire: bin_swaps = 71582789: its iterations times 3 attempts reach 2^31"),
    ("nm_rewire_ws", lambda: nm.graph_rewire(f64(4, 4), ws_bytes=47), ValueError,
     "graph_rewire: ws_bytes = 47, needs at least one slot of 4 N (N - 1) = 48 bytes"),
    ("nm_rewire_ws_bool", lambda: nm.graph_rewire(f64(4, 4), ws_bytes=True), ValueError,
     "graph_rewire: ws_bytes = True, needs at least one slot of 4 N (N - 1) = 48 bytes"),
    ("nm_null_negative", lambda: nm.graph_null_model(f64(4, 4), negative="nope"), ValueError,
     "graph_null_model: negative = 'nope', must be one of ['reference', 'bct']"),
    ("nm_null_wei_freq", lambda: nm.graph_null_model(f64(4, 4), wei_freq=2), ValueError,
     "graph_null_model: wei_freq = 2, must be a number in [0, 1]"),
    ("nm_null_wei_freq_bool", lambda: nm.graph_null_model(f64(4, 4), wei_freq=True), ValueError,
     "graph_null_model: wei_freq = True, must be a number in [0, 1]"),
    ("nm_null_wei_freq_nan", lambda: nm.graph_null_model(f64(4, 4), wei_freq=float("nan")), ValueError,
     "graph_null_model: wei_freq = nan, must be a number in [0, 1]"),
    ("nm_null_period", lambda: nm.graph_null_model(f64(4, 4), wei_freq=0.01), ValueError,
     "graph_null_model: wei_freq = 0.01 is a period of 100 > 64; 0 sorts once"),
    ("nm_null_seeds", lambda: nm.graph_null_model(f64(4, 4), seeds="1"), ValueError, "graph_null_model: " + SEEDS + "'1'"),
    ("nm_null_N", lambda: nm.graph_null_model(f64(2, 3, 3)), ValueError,
     "graph_null_model: N = 3, a rewiring takes four distinct nodes: needs N >= 4"),
    ("nm_null_swaps", lambda: nm.graph_null_model(f64(4, 4), bin_swaps=-1), ValueError,
     "graph_null_model: bin_swaps = -1, must be an int >= 0"),
    ("nm_null_ws", lambda: nm.graph_null_model(f64(5, 5), ws_bytes=79), ValueError,
     "graph_null_model: ws_bytes = 79, needs at least one slot of 4 N (N - 1) = 80 bytes"),
    ("nm_pnorm_reps", lambda: nm.participation_norm(f64(4, 4), LAB4, reps=0), ValueError,
     "participation_norm: reps = 0, must be a positive int"),
    ("nm_pnorm_reps_bool", lambda: nm.participation_norm(f64(4, 4), LAB4, reps=True), ValueError,
     "participation_norm: reps = True, must be a positive int"),
    ("nm_pnorm_max_bytes", lambda: nm.participation_norm(f64(4, 4), LAB4, reps=2, max_bytes=0), ValueError,
     "participation_norm: max_bytes = 0, must be a positive int"),
    ("nm_pnorm_max_bytes_float", lambda: nm.participation_norm(f64(4, 4), LAB4, reps=2, max_bytes=1e6), ValueError,
     "participation_norm: max_bytes = 1000000.0, must be a positive int"),
    ("nm_pnorm_seeds_len", lambda: nm.participation_norm(f64(4, 4), LAB4, reps=2, seeds=[1]), ValueError,
     "participation_norm: seeds must be a sequence of length reps = 2, or None"),
    ("nm_pnorm_seeds_int", lambda: nm.participation_norm(f64(4, 4), LAB4, reps=2, seeds=7), ValueError,
     "participation_norm: seeds must be a sequence of length reps = 2, or None"),
    ("nm_pnorm_seeds_value", lambda: nm.participation_norm(f64(4, 4), LAB4, reps=2, seeds=[0, -1]), ValueError,
     "participation_norm: " + SEEDS + "[0, -1]"),
    ("nm_pnorm_negative", lambda: nm.participation_norm(f64(4, 4), LAB4, reps=2, negative=1), ValueError,
     "participation_norm: negative = 1, must be one of ['reference', 'bct']"),
    ("nm_pnorm_wei_freq", lambda: nm.participation_norm(f64(4, 4), LAB4, reps=2, wei_freq=-0.1), ValueError,
     "participation_norm: wei_freq = -0.1, must be a number in [0, 1]"),
    ("nm_pnorm_N", lambda: nm.participation_norm(f64(3, 3), [0, 0, 1], reps=2), ValueError,
     "participation_norm: N = 3, a rewiring takes four distinct nodes: needs N >= 4"),
    ("nm_pnorm_swaps", lambda: nm.participation_norm(f64(4, 4), LAB4, reps=2, bin_swaps=None), ValueError,
     "participation_norm: bin_swaps = None, must be an int >= 0"),
    ("nm_pnorm_labels", lambda: nm.participation_norm(f64(4, 4), [0, 0, 1], reps=2), TypeError,
     "participation_norm: ci must hold integer labels, [N] or [B][N] with N = 4, B = 1"),
    # ---- surrogate ----
    ("sg_fc_x", lambda: sg.surrogate_fc(f32(4, 2), [1, 2]), TypeError, "surrogate_fc: " + SERIES),
    ("sg_fc_L_odd", lambda: sg.surrogate_fc(f64(5, 2), [1, 2]), ValueError, "surrogate_fc: L = 5, " + EVEN_L),
    ("sg_fc_L_2", lambda: sg.surrogate_fc(f64(2, 2), [1, 2]), ValueError, "surrogate_fc: L = 2, " + EVEN_L),
    ("sg_fc_L_max", lambda: sg.surrogate_fc(f64(4098, 2), [1, 2]), ValueError,
     "surrogate_fc: L = 4098 > 4096 (one transform per workgroup, in LDS)"),
    ("sg_fc_N", lambda: sg.surrogate_fc(f64(4, 1), [1, 2]), ValueError,
     "surrogate_fc: N = 1, B = 1: needs B >= 1 and 2 <= N <= 96 (the result feeds the graph kernels)"),
    ("sg_fc_B", lambda: sg.surrogate_fc(f64(4, 0, 2), [1, 2]), ValueError,
     "surrogate_fc: N = 2, B = 0: needs B >= 1 and 2 <= N <= 96 (the result feeds the graph kernels)"),
    ("sg_fc_seeds_one", lambda: sg.surrogate_fc(f64(4, 2), [1]), ValueError,
     "surrogate_fc: seeds must be a sequence of at least 2 ints in [0, 2^64), got [1]"),
    ("sg_fc_seeds_int", lambda: sg.surrogate_fc(f64(4, 2), 5), ValueError,
     "surrogate_fc: seeds must be a sequence of at least 2 ints in [0, 2^64), got 5"),
    ("sg_fc_seeds_value", lambda: sg.surrogate_fc(f64(4, 2), [1, -2]), ValueError, "surrogate_fc: " + SEEDS + "[1, -2]"),
    ("sg_test_surr_number", lambda: sg.fc_surrogate_test(f64(4, 2), surr_number=1), ValueError,
     "fc_surrogate_test: surr_number = 1, must be an int of at least 2"),
    ("sg_test_surr_number_float", lambda: sg.fc_surrogate_test(f64(4, 2), surr_number=2.0), ValueError,
     "fc_surrogate_test: surr_number = 2.0, must be an int of at least 2"),
    ("sg_test_alpha_1", lambda: sg.fc_surrogate_test(f64(4, 2), surr_number=2, alpha=1), ValueError,
     "fc_surrogate_test: alpha = 1, must lie in (0, 1)"),
    ("sg_test_alpha_0", lambda: sg.fc_surrogate_test(f64(4, 2), surr_number=2, alpha=0.0), ValueError,
     "fc_surrogate_test: alpha = 0.0, must lie in (0, 1)"),
    ("sg_test_alpha_bool", lambda: sg.fc_surrogate_test(f64(4, 2), surr_number=2, alpha=False), ValueError,
     "fc_surrogate_test: alpha = False, must lie in (0, 1)"),
    ("sg_test_seeds_len", lambda: sg.fc_surrogate_test(f64(4, 2), surr_number=2, seeds=[1, 2, 3]), ValueError,
     "fc_surrogate_test: seeds must be a sequence of surr_number = 2 ints in [0, 2^64), got [1, 2, 3]"),
    ("sg_test_seeds_int", lambda: sg.fc_surrogate_test(f64(4, 2), surr_number=2, seeds=4), ValueError,
     "fc_surrogate_test: seeds must be a sequence of surr_number = 2 ints in [0, 2^64), got 4"),
    ("sg_test_seeds_value", lambda: sg.fc_surrogate_test(f64(4, 2), surr_number=2, seeds=[1, 2.0]), ValueError,
     "fc_surrogate_test: " + SEEDS + "[1, 2.0]"),
    ("sg_test_L", lambda: sg.fc_surrogate_test(f64(7, 2), surr_number=2), ValueError, "fc_surrogate_test: L = 7, " + EVEN_L),
    ("sg_test_ws", lambda: sg.fc_surrogate_test(f64(4, 3), surr_number=2, ws_bytes=47), ValueError,
     "fc_surrogate_test: ws_bytes = 47, needs at least one simulation's slab of 8 S P = 48 bytes"),
    ("sg_test_ws_bool", lambda: sg.fc_surrogate_test(f64(4, 3), surr_number=2, ws_bytes=True), ValueError,
     "fc_surrogate_test: ws_bytes = True, needs at least one simulation's slab of 8 S P = 48 bytes"),
    # ---- partition_np, nullmodel_np, surrogate_np ----
    ("ptn_sign_shape", lambda: ptn.modularity_louvain_und_sign(np.zeros(3)), ValueError,
     "modularity_louvain_und_sign: needs an N x N matrix or a [B, N, N] stack, got shape (3,)"),
    ("ptn_consensus_N", lambda: ptn.consensus_und(np.zeros((1, 1)), 0.5), ValueError,
     "consensus_und: N = 1, the device kernels take 2 <= N <= 96"),
    ("nmn_shape", lambda: nmn.randmio_und_signed(np.zeros(3), 1), ValueError,
     "randmio_und_signed: needs an N x N matrix, got shape (3,)"),
    ("nmn_N", lambda: nmn.null_model_und_sign(np.zeros((3, 3))), ValueError,
     "null_model_und_sign: N = 3, the device kernel takes 4 <= N <= 96"),
    ("nmn_N97", lambda: nmn.participation_coef_norm(np.zeros((97, 97)), np.zeros(97)), ValueError,
     "participation_coef_norm: N = 97, the device kernel takes 4 <= N <= 96"),
    ("nmn_itr", lambda: nmn.randmio_und_signed(np.zeros((4, 4)), -1), ValueError,
     "randmio_und_signed: itr = -1, must be an int >= 0"),
    ("nmn_itr_bool", lambda: nmn.randmio_und_signed(np.zeros((4, 4)), True), ValueError,
     "randmio_und_signed: itr = True, must be an int >= 0"),
    ("nmn_itr_fraction", lambda: nmn.randmio_und_signed(np.zeros((4, 4)), 1.5), ValueError,
     "randmio_und_signed: itr = 1.5, must be an int >= 0"),
    ("nmn_null_directed", lambda: nmn.null_model_und_sign(np.triu(np.ones((4, 4)), 1)), TypeError,
     "Input must be undirected"),
    ("nmn_pnorm_degree", lambda: nmn.participation_coef_norm(np.zeros((4, 4)), LAB4, degree="both"), ValueError,
     "participation_coef_norm: degree 'both', must be 'undirected', 'in' or 'out'"),
    ("nmn_pnorm_directed", lambda: nmn.participation_coef_norm(np.triu(np.ones((4, 4)), 1), LAB4), TypeError,
     "Input must be undirected"),
    ("nmn_pnorm_labels", lambda: nmn.participation_coef_norm(np.zeros((4, 4)), [0, 1]), ValueError,
     "participation_coef_norm: ci needs one label per node, got shape (2,)"),
    ("nmn_status_3", lambda: nmn._refused("randmio_und_signed", None, 3), ValueError,
     "randmio_und_signed: the matrix holds NaN or inf"),
    ("nmn_status_2", lambda: nmn._refused("null_model_und_sign", None, 2), TypeError, "Input must be undirected"),
    ("nmn_status_1", lambda: nmn._refused("null_model_und_sign", None, 1), ZeroDivisionError,
     "null_model_und_sign: a strength reached exactly 0 where the reference divides by it"),
    ("sgn_conn", lambda: sgn.probabilistic_thresholding(np.zeros((4, 2)), conn="plv"), KeyError,
     "'invalid connectivity metric'"),
    ("sgn_y", lambda: sgn.probabilistic_thresholding(np.zeros(3)), TypeError,
     "probabilistic_thresholding: y must be a real [L, N] array or a [B, L, N] stack, got shape (3,), dtype float64"),
    ("sgn_y_complex", lambda: sgn.probabilistic_thresholding(np.zeros((4, 2), dtype=complex)), TypeError,
     "probabilistic_thresholding: y must be a real [L, N] array or a [B, L, N] stack, got shape (4, 2), dtype "
     "complex128"),
    ("sgn_surr_number", lambda: sgn.probabilistic_thresholding(np.zeros((4, 2)), surr_number=1), ValueError,
     "probabilistic_thresholding: surr_number = 1, must be an int of at least 2"),
    ("sgn_alpha", lambda: sgn.probabilistic_thresholding(np.zeros((4, 2)), alpha=2), ValueError,
     "probabilistic_thresholding: alpha = 2, must lie in (0, 1)"),
    ("sgn_L", lambda: sgn.probabilistic_thresholding(np.zeros((2, 5, 3))), ValueError,
     "probabilistic_thresholding: L = 5, " + EVEN_L),
]
ROWS += [("g_shape_" + n, (lambda f: lambda: f(np.zeros(3)))(getattr(gu, n)), ValueError,
          n + ": needs an N x N matrix or a [B, N, N] stack, got shape (3,)")
         for n in ("distance_wei", "efficiency_wei", "clustering_coef_wu", "transitivity_wu", "strengths_und",
                   "degrees_und", "betweenness_wei", "betweenness_bin")]
ROWS += [("g_shape_" + n, (lambda f: lambda: f(np.zeros((0, 3, 3)), [0, 1, 1]))(getattr(gu, n)), ValueError,
          n + ": needs an N x N matrix or a [B, N, N] stack, got shape (0, 3, 3)")
         for n in ("participation_coef", "module_degree_zscore")]
ROWS += [("g_shape_" + n, (lambda f: lambda: f(np.zeros((3, 4))))(getattr(gu, n)), ValueError,
          n + ": needs an N x N matrix or a [B, N, N] stack, got shape (3, 4)")
         for n in ("community_louvain", "get_agreement_matrix")]

DEVICE_ONLY = "libwcsde takes device tensors only"
PTR_ROWS = [(name, call, WCSDEError, DEVICE_ONLY) for name, call in [
    ("hilbert_phase", lambda: sc.hilbert_phase(f64(8, 2))),
    ("hilbert_phase_long", lambda: sc.hilbert_phase_long(f64(8, 2))),
    ("hilbert_envelope", lambda: sc.hilbert_envelope(f64(8, 2))),
    ("filtfilt", lambda: sc.filtfilt([1.0, 0.5], [1.0, 0.2], f64(30, 2))),
    ("kuramoto", lambda: sc.kuramoto(f64(8, 2))),
    ("fc_metrics", lambda: sc.fc_metrics(f64(8, 6), 2, 3)),
    ("hma", lambda: sc.hma(f64(2, 3, 3))),
    ("graph_betweenness", lambda: sc.graph_betweenness(f64(3, 3))),
    ("graph_module_measures", lambda: sc.graph_module_measures(f64(3, 3), i32(3))),
    ("graph_louvain", lambda: sc.graph_louvain(full(1.0, 3, 3))),
    ("graph_agreement", lambda: sc.graph_agreement(i32(2, 3))),
    ("fcd", lambda: sc.fcd(f64(12, 3), 4)),
    ("fcd_from_phasors", lambda: sc.fcd_from_phasors(f64(4, 3, 2))),
    ("leida", lambda: sc.leida(f64(8, 3))),
    ("leida_from_phasors", lambda: sc.leida_from_phasors(f64(4, 3, 2))),
    ("kmeans_assign", lambda: sc.kmeans_assign(f64(4, 2), f64(2, 2))),
    ("kmeans_update", lambda: sc.kmeans_update(f64(4, 2), i32(4), f64(2, 2))),
    ("kmeans", lambda: sc.kmeans(full(1.0, 4, 2), 2)),
    ("leida_states", lambda: sc.leida_states(f64(4, 2), f64(2, 2))),
    ("state_stats", lambda: sc.state_stats(i32(20), 2)),
    ("welch", lambda: sc.welch(f64(64, 2), nperseg=8)),
    ("csd", lambda: sc.csd(f64(64, 2), nperseg=8)),
    ("coherence", lambda: sc.coherence(f64(64, 2), f64(64, 2), nperseg=8)),
    ("spectrogram", lambda: sc.spectrogram(f64(64, 2), nperseg=8)),
    ("phase_connectivity_from", lambda: sc.phase_connectivity_from(f64(8, 3, 2), measures="plv")),
    ("phase_connectivity", lambda: sc.phase_connectivity(f64(8, 3), "plv")),
    ("corrcoef", lambda: sc.corrcoef(f64(8, 1, 3), 1, 3)),
    ("sim_bold", lambda: sc.sim_bold(f64(2016, 2))),
    ("welch_accumulator", lambda: sc.WelchAccumulator(1, 1, "cpu")),
    ("welch_peak", lambda: sc.welch_peak(f64(8000, 1, 1))),
    ("utils_kuramoto", lambda: on_cpu(ut.kuramoto, np.zeros((8, 2)))),
    ("utils_envelope", lambda: on_cpu(ut.envelope, np.zeros((30, 2)))),
    ("utils_welch", lambda: on_cpu(ut.welch, X64, nperseg=8)),
    ("utils_get_all_metrics", lambda: on_cpu(ut.get_all_metrics, np.eye(3), np.eye(3))),
    ("graph_louvain_sign", lambda: pt.graph_louvain_sign(f64(3, 3))),
    ("graph_louvain_sign_seeds_ws", lambda: pt.graph_louvain_sign(f64(2, 3, 3), seeds=[0, (1 << 64) - 1], ws_bytes=144)),
    ("graph_consensus", lambda: pt.graph_consensus(f64(3, 3), 0.5, reps=2)),
    ("graph_rewire", lambda: nm.graph_rewire(f64(4, 4))),
    ("graph_null_model", lambda: nm.graph_null_model(f64(4, 4), seeds=[1, 2], ws_bytes=48)),
    ("participation_norm", lambda: nm.participation_norm(f64(4, 4), LAB4, reps=2)),
    ("surrogate_fc", lambda: sg.surrogate_fc(f64(4, 2), [1, 2])),
    ("fc_surrogate_test", lambda: sg.fc_surrogate_test(f64(4, 2), surr_number=2)),
]]

Z3 = np.zeros(64, dtype=complex)
DOUBLE_ROWS = [
    ("welch_nfft_complex", lambda: ut.welch(Z3, nperseg=8, nfft=16), NotImplementedError,
     "welch: nfft other than nperseg (zero padding) does not run on the device"),
    ("welch_detrend_onesided", lambda: ut.welch(X64, detrend="linear", return_onesided=False), NotImplementedError,
     "welch: return_onesided=False does not run on the device"),
    ("spectrogram_nfft_complex", lambda: ut.spectrogram(Z3, nperseg=8, nfft=16), NotImplementedError,
     "spectrogram: nfft other than nperseg (zero padding) does not run on the device"),
    ("spectrogram_detrend_onesided", lambda: ut.spectrogram(X64, detrend="linear", return_onesided=False),
     NotImplementedError, "spectrogram: return_onesided=False does not run on the device"),
    ("csd_nfft_complex", lambda: ut.csd(Z3, Z3, nperseg=8, nfft=16), NotImplementedError,
     "csd: complex input does not run on the device"),
    ("csd_detrend_onesided", lambda: ut.csd(X64, X64, detrend="linear", return_onesided=False), NotImplementedError,
     "csd: return_onesided=False does not run on the device"),
    ("coherence_nfft_complex", lambda: ut.coherence(Z3, Z3, nperseg=8, nfft=16), NotImplementedError,
     "coherence: complex input does not run on the device"),
    ("coherence_detrend_onesided", lambda: ut.coherence(X64, X64, detrend="linear", return_onesided=False), TypeError,
     "coherence() got an unexpected keyword argument 'return_onesided'"),
    ("welch_average_detrend", lambda: ut.welch(X64, detrend="linear", average="median"), NotImplementedError,
     "welch: average = 'median' (only 'mean' runs on the device)"),
    ("csd_shapes_nfft", lambda: ut.csd(X64, np.zeros(32), nperseg=8, nfft=16), NotImplementedError,
     "csd: x and y of different shapes or lengths (broadcasting, zero padding of the shorter) do not run on the "
     "device"),
    ("csd_matrix_complex_detrend", lambda: ut.csd_matrix(np.zeros((64, 2), dtype=complex), detrend="linear"),
     NotImplementedError, "csd_matrix: complex input does not run on the device"),
    ("csd_matrix_detrend_shape", lambda: ut.csd_matrix(X64, detrend="linear"), NotImplementedError,
     "csd_matrix: detrend = 'linear' (only 'constant' and False run on the device)"),
    ("connectivity_measures_dtype", lambda: ut.connectivity(np.zeros((30, 3), dtype=complex), measures="nope"),
     ValueError, "connectivity: unknown measure 'nope', must be one of " + CM),
    ("utils_fcd_dtype_method", lambda: ut.fcd(np.zeros((30, 3), dtype=complex), method="nope"), TypeError,
     "fcd: series must be real numbers, not complex128"),
    ("utils_leida_freqs_metric", lambda: ut.leida(np.zeros((30, 3)), 0.002, [8], metric="nope"), ValueError,
     "freqs must be [fmin, fmax] or None"),
    ("graph_measures_name_dtype", lambda: sc.graph_measures(f32(3, 3), "nope"), ValueError,
     "graph_measures: unknown measure 'nope', must be one of " + GM),
    ("graph_measures_lengths_dtype", lambda: sc.graph_measures(f32(3, 3), "degrees", lengths=True), ValueError,
     "graph_measures: lengths=True goes with the path measures " + GPM + " only, the others are defined on weights"),
    ("graph_module_measures_degree_zflag", lambda: sc.graph_module_measures(f64(3, 3), i32(3), degree="both", zflag=9),
     ValueError, "graph_module_measures: degree 'both', must be one of ['undirected', 'out', 'in']"),
    ("graph_module_measures_zflag_w", lambda: sc.graph_module_measures(f32(3, 3), i32(3), zflag=9), ValueError,
     "graph_module_measures: zflag 9, must be 0, 1, 2 or 3"),
    ("graph_louvain_objective_seeds", lambda: sc.graph_louvain(f32(3, 3), seeds=-1, objective="nope"), ValueError,
     "graph_louvain: objective 'nope', must be one of ['modularity', 'potts'] or a [N][N] / [B][N][N] fp64 device "
     "tensor (negative_sym and negative_asym are not built: the reference refuses negative weights before it "
     "reaches them)"),
    ("graph_louvain_seeds_w", lambda: sc.graph_louvain(f32(3, 3), seeds=-1), ValueError,
     "graph_louvain: seeds must be an int or a non-empty sequence of ints in [0, 2^64), got -1"),
    ("fcd_method_dtype", lambda: sc.fcd(f32(12, 3), 4, method="nope"), ValueError,
     "fcd: unknown method 'nope', must be one of ['corr', 'phase']"),
    ("kmeans_metric_K_int", lambda: sc.kmeans(f64(4, 2), 0, metric="nope"), ValueError,
     "kmeans: K = 0: needs 1 <= K <= 32"),
    ("kmeans_metric_K_init", lambda: sc.kmeans(f64(4, 2), f64(33, 2), metric="nope"), ValueError,
     "kmeans: unknown metric 'nope', must be one of ['sqeuclidean', 'cosine']"),
    ("kmeans_assign_metric_K", lambda: sc.kmeans_assign(f64(4, 2), f64(33, 2), metric="nope"), ValueError,
     "kmeans_assign: unknown metric 'nope', must be one of ['sqeuclidean', 'cosine']"),
    ("state_stats_dtype_K", lambda: sc.state_stats(i64(20), 40), TypeError,
     "state_stats: labels must be a [M][B] or [M] int32 device tensor"),
    ("phase_connectivity_from_names_phasor", lambda: sc.phase_connectivity_from(f64(8, 3), measures="nope"),
     ValueError, "phase_connectivity_from: unknown measure 'nope', must be one of " + CM),
    ("spectrogram_mode_x", lambda: sc.spectrogram(f32(64, 2), mode="phase"), NotImplementedError,
     "spectrogram: mode = 'phase' (unwrapped angles) does not run on the device; utils.spectrogram unwraps the "
     "device's angles on the host"),
    ("welch_x_detrend", lambda: sc.welch(f32(64, 2), detrend="linear"), TypeError,
     "welch: x must be a [T][C] or [T][B][N] fp64 device tensor"),
    ("welch_detrend_scaling", lambda: sc.welch(f64(64, 2), detrend="linear", scaling="nope"), NotImplementedError,
     "welch: detrend = 'linear' (only 'constant' and False run on the device)"),
    ("louvain_sign_qtype_gamma", lambda: pt.graph_louvain_sign(f32(3, 3), seeds=-1, gamma=None, qtype="nope"), ValueError,
     "graph_louvain_sign: modularity type unknown: qtype 'nope', must be one of " + QT),
    ("louvain_sign_gamma_seeds", lambda: pt.graph_louvain_sign(f32(3, 3), seeds=-1, gamma=None), ValueError,
     "graph_louvain_sign: gamma = None, must be a finite number"),
    ("louvain_sign_seeds_w", lambda: pt.graph_louvain_sign(f32(3, 3), seeds=-1, ws_bytes=1), ValueError,
     "graph_louvain_sign: " + SEEDS + "-1"),
    ("louvain_sign_w_ws", lambda: pt.graph_louvain_sign(f32(3, 3), ws_bytes=1), TypeError, "graph_louvain_sign: " + STACK),
    ("consensus_reps_max_iter", lambda: pt.graph_consensus(f32(3, 3), None, reps=0, seeds=[1], max_iter=0), ValueError,
     "graph_consensus: reps = 0, must be a positive int"),
    ("consensus_max_iter_tau", lambda: pt.graph_consensus(f32(3, 3), None, reps=2, seeds=[1], max_iter=0), ValueError,
     "graph_consensus: max_iter = 0, must be a positive int"),
    ("consensus_tau_seeds", lambda: pt.graph_consensus(f32(3, 3), None, reps=2, seeds=[1]), ValueError,
     "graph_consensus: tau = None, must be a finite number"),
    ("consensus_seeds_value_len", lambda: pt.graph_consensus(f32(3, 3), 0.5, reps=2, seeds=[-1]), ValueError,
     "graph_consensus: " + SEEDS + "[-1]"),
    ("consensus_seeds_D", lambda: pt.graph_consensus(f32(3, 3), 0.5, reps=2, seeds=[1]), ValueError,
     "graph_consensus: seeds must be a sequence of length reps = 2, or None"),
    ("rewire_seeds_N", lambda: nm.graph_rewire(f64(3, 3), bin_swaps=-1, seeds=-1), ValueError, "graph_rewire: " + SEEDS + "-1"),
    ("rewire_N_swaps", lambda: nm.graph_rewire(f64(3, 3), bin_swaps=-1, ws_bytes=1), ValueError,
     "graph_rewire: N = 3, a rewiring takes four distinct nodes: needs N >= 4"),
    ("rewire_swaps_ws", lambda: nm.graph_rewire(f64(4, 4), bin_swaps=-1, ws_bytes=1), ValueError,
     "graph_rewire: bin_swaps = -1, must be an int >= 0"),
    ("null_model_negative_wei_freq", lambda: nm.graph_null_model(f64(3, 3), seeds=-1, wei_freq=2, negative="nope"),
     ValueError, "graph_null_model: negative = 'nope', must be one of ['reference', 'bct']"),
    ("null_model_wei_freq_seeds", lambda: nm.graph_null_model(f64(3, 3), seeds=-1, wei_freq=2), ValueError,
     "graph_null_model: wei_freq = 2, must be a number in [0, 1]"),
    ("null_model_seeds_N", lambda: nm.graph_null_model(f64(3, 3), seeds=-1), ValueError, "graph_null_model: " + SEEDS + "-1"),
    ("null_model_N_swaps", lambda: nm.graph_null_model(f64(3, 3), bin_swaps=-1), ValueError,
     "graph_null_model: N = 3, a rewiring takes four distinct nodes: needs N >= 4"),
    ("null_model_swaps_ws", lambda: nm.graph_null_model(f64(4, 4), bin_swaps=-1, ws_bytes=1), ValueError,
     "graph_null_model: bin_swaps = -1, must be an int >= 0"),
    ("pnorm_reps_max_bytes", lambda: nm.participation_norm(f64(3, 3), LAB4, reps=0, max_bytes=0), ValueError,
     "participation_norm: reps = 0, must be a positive int"),
    ("pnorm_max_bytes_seeds", lambda: nm.participation_norm(f64(3, 3), LAB4, reps=2, seeds=[1], max_bytes=0), ValueError,
     "participation_norm: max_bytes = 0, must be a positive int"),
    ("pnorm_seeds_negative", lambda: nm.participation_norm(f64(3, 3), LAB4, reps=2, seeds=[1], negative="nope"), ValueError,
     "participation_norm: seeds must be a sequence of length reps = 2, or None"),
    ("pnorm_negative_wei_freq", lambda: nm.participation_norm(f64(3, 3), LAB4, reps=2, wei_freq=2, negative="nope"),
     ValueError, "participation_norm: negative = 'nope', must be one of ['reference', 'bct']"),
    ("pnorm_wei_freq_N", lambda: nm.participation_norm(f64(3, 3), LAB4, reps=2, wei_freq=2), ValueError,
     "participation_norm: wei_freq = 2, must be a number in [0, 1]"),
    ("pnorm_N_swaps", lambda: nm.participation_norm(f64(3, 3), LAB4, reps=2, bin_swaps=-1), ValueError,
     "participation_norm: N = 3, a rewiring takes four distinct nodes: needs N >= 4"),
    ("pnorm_swaps_labels", lambda: nm.participation_norm(f64(4, 4), [0], reps=2, bin_swaps=-1), ValueError,
     "participation_norm: bin_swaps = -1, must be an int >= 0"),
    ("surrogate_fc_x_seeds", lambda: sg.surrogate_fc(f64(5, 2), [1]), ValueError, "surrogate_fc: L = 5, " + EVEN_L),
    ("surrogate_test_surr_number_alpha", lambda: sg.fc_surrogate_test(f64(5, 2), surr_number=1, alpha=2, seeds=[1]),
     ValueError, "fc_surrogate_test: surr_number = 1, must be an int of at least 2"),
    ("surrogate_test_alpha_seeds", lambda: sg.fc_surrogate_test(f64(5, 2), surr_number=2, alpha=2, seeds=[1]), ValueError,
     "fc_surrogate_test: alpha = 2, must lie in (0, 1)"),
    ("surrogate_test_seeds_x", lambda: sg.fc_surrogate_test(f64(5, 2), surr_number=2, seeds=[1], ws_bytes=1), ValueError,
     "fc_surrogate_test: seeds must be a sequence of surr_number = 2 ints in [0, 2^64), got [1]"),
    ("surrogate_test_x_ws", lambda: sg.fc_surrogate_test(f64(5, 2), surr_number=2, ws_bytes=1), ValueError,
     "fc_surrogate_test: L = 5, " + EVEN_L),
    ("randmio_N_itr", lambda: nmn.randmio_und_signed(np.zeros((3, 3)), -1), ValueError,
     "randmio_und_signed: N = 3, the device kernel takes 4 <= N <= 96"),
    ("pcn_degree_N", lambda: nmn.participation_coef_norm(np.zeros((3, 3)), [0], degree="both"), ValueError,
     "participation_coef_norm: degree 'both', must be 'undirected', 'in' or 'out'"),
    ("probabilistic_thresholding_conn_y", lambda: sgn.probabilistic_thresholding(np.zeros(3), conn="plv"), KeyError,
     "'invalid connectivity metric'"),
]


def _ids(rows):
    return [r[0] for r in rows]


def _refused(call, cls, message):
    with pytest.raises(Exception) as err:
        call()
    assert type(err.value) is cls, f"{type(err.value).__name__}: {err.value}"
    assert str(err.value) == message


@pytest.mark.parametrize("call, cls, message", [r[1:] for r in ROWS], ids=_ids(ROWS))
def test_refusal(call, cls, message):
    _refused(call, cls, message)


@pytest.mark.parametrize("call, cls, message", [r[1:] for r in PTR_ROWS], ids=_ids(PTR_ROWS))
def test_cpu_tensor_reaches_ptr(call, cls, message):
    _refused(call, cls, message)


@pytest.mark.parametrize("call, cls, message", [r[1:] for r in DOUBLE_ROWS], ids=_ids(DOUBLE_ROWS))
def test_first_refusal_wins(call, cls, message):
    _refused(call, cls, message)


def test_row_ids_are_unique():
    ids = _ids(ROWS + PTR_ROWS + DOUBLE_ROWS)
    assert len(ids) == len(set(ids))


@pytest.mark.parametrize("fn", [sc.welch, sc.csd, sc.coherence, sc.spectrogram], ids=lambda f: f.__name__)
def test_clamped_nperseg_warning_names_the_caller(fn):
    """nperseg > T with a named window: SciPy's UserWarning, attributed to the file that called the
    public function (the call then goes on and stops at _lib.ptr, on this CPU tensor)."""
    with pytest.warns(UserWarning) as caught, pytest.raises(WCSDEError, match=DEVICE_ONLY):
        fn(f64(4, 2), nperseg=8)
    assert len(caught) == 1
    assert caught[0].category is UserWarning
    assert str(caught[0].message) == "nperseg = 8 is greater than input length  = 4, using nperseg = 4"
    assert caught[0].filename == __file__


SIGNATURES = {
    "sigchain": {
        "BoldStream": "(C, n_total, neq=2000, dec=1000, bold_dt=0.04, device='cuda')",
        "BoldStream.feed": "(self, E, Tc=None, e_ld=0, offset=0, copy=None, copy_ld=0, copy_offset=0)",
        "BoldStream.finish": "(self)",
        "hilbert_phase": "(x)",
        "hilbert_phase_long": "(x, out=None, ws_bytes=None)",
        "hilbert_envelope": "(x, method=0, ws_bytes=None)",
        "filtfilt": "(b, a, x)",
        "envelope_filters": "(dt, fmin, fmax, fcut)",
        "envelope": "(x, dt=0.002, freqs=(8, 13), fcut=None)",
        "fc_metrics": "(bold=None, B=None, N=None, empfc=None, fc_in=None, kuramoto=True, want_fc=False, "
                      "data_range=1.0)",
        "kuramoto": "(x, B=1, N=None)",
        "hma": "(fc, want_clus_num=False)",
        "WelchAccumulator": "(B, N, device='cuda')",
        "WelchAccumulator.accumulate": "(self, E, ld, slot, nslots, seg0, nseg=1)",
        "WelchAccumulator.peak": "(self, fs=500.0, want_psd=False)",
        "graph_measures": "(w, measures=('dist', 'hops', 'charpath', 'efficiency', 'ecc', 'radius', 'diameter', "
                          "'local_efficiency', 'clustering', 'transitivity', 'strengths', 'degrees'), lengths=False, "
                          "include_infinite=True)",
        "graph_betweenness": "(w, lengths=False)",
        "graph_module_measures": "(w, ci, measures=('participation', 'zscore', 'modularity'), degree='undirected', "
                                 "zflag=0, gamma=1.0, n_modules=None)",
        "graph_louvain": "(w, seeds=0, gamma=1.0, ci=None, objective='modularity', want_info=False)",
        "graph_agreement": "(ci)",
        "graph_consensus_matrix": "(w, reps=100, tau=0.5, gamma=1.0, ci=None, objective='modularity', seeds=None)",
        "fcd": "(x, window=None, step=None, method='corr', want_windows=False, trim=0, ws_bytes=None)",
        "fcd_from_phasors": "(phasor)",
        "fcd_ks": "(fcd, emp_values, lag=1)",
        "leida": "(x, trim=0)",
        "leida_from_phasors": "(phasor)",
        "kmeans_assign": "(x, centroids, metric='cosine')",
        "kmeans_update": "(x, labels, centroids, metric='cosine', ws_bytes=None)",
        "kmeans": "(x, k_or_init, metric='cosine', max_iter=100, n_init=1, seed=0)",
        "state_stats": "(labels, k)",
        "leida_states": "(vec, centroids, metric='cosine')",
        "state_kl": "(p, q)",
        "welch_peak": "(E_t, fs=500.0, want_psd=False)",
        "welch": "(x, fs=1.0, window='hann', nperseg=None, noverlap=None, detrend='constant', scaling='density', "
                 "ws_bytes=None)",
        "csd": "(x, y=None, fs=1.0, window='hann', nperseg=None, noverlap=None, detrend='constant', "
               "scaling='density', ws_bytes=None)",
        "coherence": "(x, y=None, fs=1.0, window='hann', nperseg=None, noverlap=None, detrend='constant', "
                     "ws_bytes=None)",
        "spectrogram": "(x, fs=1.0, window=('tukey', 0.25), nperseg=None, noverlap=None, detrend='constant', "
                       "scaling='density', mode='psd')",
        "phase_connectivity_from": "(phasor, amp=None, measures=('plv', 'pli', 'wpli', 'aec', 'aec_orth'), "
                                   "ws_bytes=None)",
        "phase_connectivity": "(x, measures=('plv', 'pli', 'wpli', 'aec', 'aec_orth'))",
        "sim_bold": "(E_t, bold_downsamp=1000, neq=2000, bold_dt=0.04)",
        "corrcoef": "(x, B, N)",
    },
    "utils": {
        "cohen_d": "(x, y)",
        "flat_FC": "(FC)",
        "new_metric": "(flat1, flat2)",
        "sub_weight": "(struct, prop=1)",
        "cortex_mat": "(mat90)",
        "scale_mat": "(struct, G, subG)",
        "envelope": "(series, dt=0.002, freqs=[8, 13], fcut=None)",
        "welch": "(x, fs=1.0, window='hann', nperseg=None, noverlap=None, nfft=None, detrend='constant', "
                 "return_onesided=True, scaling='density', axis=-1, average='mean')",
        "spectrogram": "(x, fs=1.0, window=('tukey', 0.25), nperseg=None, noverlap=None, nfft=None, "
                       "detrend='constant', return_onesided=True, scaling='density', axis=-1, mode='psd')",
        "csd": "(x, y, fs=1.0, window='hann', nperseg=None, noverlap=None, nfft=None, detrend='constant', "
               "return_onesided=True, scaling='density', axis=-1, average='mean')",
        "coherence": "(x, y, fs=1.0, window='hann', nperseg=None, noverlap=None, nfft=None, detrend='constant', "
                     "axis=-1)",
        "csd_matrix": "(x, fs=1.0, window='hann', nperseg=None, noverlap=None, detrend='constant', "
                      "scaling='density')",
        "coherence_matrix": "(x, fs=1.0, window='hann', nperseg=None, noverlap=None, detrend='constant')",
        "connectivity": "(series, dt=0.002, freqs=[8, 13], measures=('plv', 'pli', 'wpli', 'aec', 'aec_orth'), "
                        "device='cuda')",
        "fcd": "(series, window=30, step=1, method='corr', trim=0, device='cuda')",
        "leida": "(series, dt, freqs, centroids=None, k=None, trim=0, metric='cosine', device='cuda')",
        "kuramoto": "(sign)",
        "get_all_metrics": "(sFC, empFC, data_range=1)",
    },
    "graph_utils": {
        "get_uptri": "(x)",
        "matrix_recon": "(x)",
        "thresholding": "(x, threshold=0.2, zero_diag=True, direct='undirected')",
        "cuberoot": "(x)",
        "invert": "(W, copy=True)",
        "distance_wei": "(G)",
        "charpath": "(D, include_diagonal=False, include_infinite=True)",
        "efficiency_wei": "(Gw, local=False)",
        "clustering_coef_wu": "(W)",
        "transitivity_wu": "(W)",
        "strengths_und": "(CIJ)",
        "degrees_und": "(CIJ)",
        "betweenness_wei": "(G)",
        "betweenness_bin": "(G)",
        "participation_coef": "(W, ci, degree='undirected')",
        "module_degree_zscore": "(W, ci, flag=0)",
        "community_louvain": "(W, gamma=1, ci=None, B='modularity', seed=None)",
        "agreement": "(ci, buffsz=1000)",
        "get_agreement_matrix": "(W, reps=100, tau=0.5, gamma=1, ci=None, B='modularity', seeds=None)",
    },
    "partition": {
        "louvain_sign_slot_bytes": "(N)",
        "graph_louvain_sign": "(w, seeds=0, gamma=1.0, qtype='sta', want_info=False, ws_bytes=None)",
        "graph_consensus": "(D, tau, reps=1000, seeds=None, max_iter=100)",
    },
    "nullmodel": {
        "null_model_slot_bytes": "(N)",
        "period_of": "(name, wei_freq)",
        "graph_rewire": "(w, bin_swaps=5, seeds=0, want_info=False, ws_bytes=None)",
        "graph_null_model": "(w, seeds=0, bin_swaps=5, wei_freq=0.1, negative='bct', want_stats=False, ws_bytes=None)",
        "participation_norm": "(w, ci, reps=100, seeds=None, bin_swaps=5, wei_freq=0.1, negative='bct', "
                              "max_bytes=268435456)",
    },
    "surrogate": {
        "surrogate_slab_bytes": "(N, S)",
        "surrogate_fc": "(x, seeds)",
        "fc_surrogate_test": "(x, surr_number=50, alpha=0.05, seeds=None, want_stats=False, ws_bytes=None)",
    },
    "partition_np": {
        "modularity_louvain_und_sign": "(W, gamma=1, qtype='sta', seed=None)",
        "consensus_und": "(D, tau, reps=1000)",
    },
    "nullmodel_np": {
        "randmio_und_signed": "(R, itr, seed=None)",
        "null_model_und_sign": "(W, bin_swaps=5, wei_freq=0.1, seed=None)",
        "participation_coef_norm": "(W, ci, degree='undirected', BA_iters=100)",
    },
    "surrogate_np": {
        "probabilistic_thresholding": "(y, surr_number=50, alpha=0.05, conn='corr')",
    },
}

CONSTANTS = {
    "sigchain": {
        "NEQ": 2000,
        "WELCH_NPERSEG": 4000,
        "WELCH_HOP": 2000,
        "HILBERT_DIRECT_MAX_M": 8192,
        "HILBERT_LONG_WS_CAP": 1073741824,
        "HMA_JACOBI_MAX_N": 96,
        "HMA_MODES_MAX_N": 4096,
        "HMA_EIGH_BATCH": 64,
        "GRAPH_MAX_N": 96,
        "GRAPH_PATH_MEASURES": ("dist", "hops", "charpath", "efficiency", "ecc", "radius", "diameter"),
        "GRAPH_CLUSTER_MEASURES": ("clustering", "transitivity", "strengths", "degrees"),
        "GRAPH_MEASURES": ("dist", "hops", "charpath", "efficiency", "ecc", "radius", "diameter", "local_efficiency",
                           "clustering", "transitivity", "strengths", "degrees"),
        "GRAPH_MODULE_MEASURES": ("participation", "zscore", "modularity"),
        "GRAPH_MODULE_DEGREES": {"undirected": 0, "out": 0, "in": 1},
        "GRAPH_LOUVAIN_OBJECTIVES": ("modularity", "potts"),
        "GRAPH_PARTITION_SEARCH": ("graph_louvain", "graph_agreement", "graph_consensus_matrix"),
        "GRAPH_LOUVAIN_MIN_WEIGHT": -1e-10,
        "FCD_MAX_N": 96,
        "FCD_MAX_WINDOWS": 4096,
        "FCD_PHASE_MAX_M": 4096,
        "FCD_WS_CAP": 1073741824,
        "FCD_METHODS": ("corr", "phase"),
        "FCD_KS_CHUNK": 256,
        "LEIDA_MAX_N": 1024,
        "KMEANS_MAX_K": 32,
        "KMEANS_METRICS": {"sqeuclidean": 0, "cosine": 1},
        "KMEANS_UPDATE_BLOCK": 256,
        "WELCH_PSD_WS_CAP": 1073741824,
        "CSD_WS_CAP": 1073741824,
        "CSD_MATRIX": 0,
        "CSD_COHERENCE": 1,
        "CSD_PAIRS": 2,
        "CSD_PAIR_COHERENCE": 3,
        "SPEC_MODES": {"psd": 0, "complex": 1, "magnitude": 2, "angle": 3},
        "CONN_BITS": {"plv": 1, "pli": 2, "wpli": 4, "aec_orth": 8},
        "CONN_MEASURES": ("plv", "pli", "wpli", "aec", "aec_orth"),
        "AEC_GROUP": 48,
    },
    "utils": {
        "device": "cuda",
        "thal": [38, 51],
        "not_thal": [i for i in range(90) if i not in (38, 51)],
        "subL": [35, 36, 37, 38],
        "subR": [51, 52, 53, 54],
        "sub": [35, 36, 37, 38, 51, 52, 53, 54],
        "cortex": [i for i in range(90) if i not in (35, 36, 37, 38, 51, 52, 53, 54)],
    },
    "graph_utils": {
        "GRAPH_MAX_N": 96,
    },
    "partition": {
        "LOUVAIN_SIGN_QTYPES": ("sta", "pos", "smp", "gja", "neg"),
        "LOUVAIN_SIGN_SLOTS": 2048,
    },
    "nullmodel": {
        "NULL_MODEL_MIN_N": 4,
        "NULL_MODEL_SLOTS": 4096,
        "NULL_MODEL_MAX_PERIOD": 64,
        "NEGATIVE_MODES": ("reference", "bct"),
        "PARTICIPATION_NORM_BYTES": 268435456,
    },
    "surrogate": {
        "SURROGATE_MAX_L": 4096,
        "SURROGATE_WS_CAP": 1073741824,
    },
    "partition_np": {
        "CONSENSUS_MAX_ITER": 100,
    },
    "nullmodel_np": {
        "NULL_MODEL_MIN_N": 4,
        "NULL_MODEL_MAX_N": 96,
    },
    "surrogate_np": {},
}

MODULES = {"sigchain": sc, "utils": ut, "graph_utils": gu, "partition": pt, "nullmodel": nm, "surrogate": sg,
           "partition_np": ptn, "nullmodel_np": nmn, "surrogate_np": sgn}


def _public(mod):
    """(signatures, constants) of the names without a leading underscore that mod itself defines."""
    sigs, consts = {}, {}
    for name, v in vars(mod).items():
        if name.startswith("_") or inspect.ismodule(v):
            continue
        if inspect.isclass(v):
            if v.__module__ == mod.__name__:
                sigs[name] = str(inspect.signature(v))
                sigs.update({f"{name}.{m}": str(inspect.signature(f)) for m, f in vars(v).items()
                             if not m.startswith("_") and callable(f)})
        elif callable(v):
            if getattr(v, "__module__", None) == mod.__name__:
                sigs[name] = str(inspect.signature(v))
        elif isinstance(v, (int, float, str, tuple, list, dict)):
            consts[name] = v
    return sigs, consts


@pytest.mark.parametrize("module", list(MODULES))
def test_public_signatures(module):
    assert _public(MODULES[module])[0] == SIGNATURES[module]


@pytest.mark.parametrize("module", list(MODULES))
def test_public_constants(module):
    consts = _public(MODULES[module])[1]
    assert consts == CONSTANTS[module]
    assert {n: type(v) for n, v in consts.items()} == {n: type(v) for n, v in CONSTANTS[module].items()}
    for name in ("GRAPH_MODULE_DEGREES", "KMEANS_METRICS", "SPEC_MODES", "CONN_BITS"):  # their order is in messages
        if name in consts:
            assert list(consts[name]) == list(CONSTANTS[module][name])

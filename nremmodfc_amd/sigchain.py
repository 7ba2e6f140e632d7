"""Device-side signal chain: BOLD + band-pass filtfilt + decimation, FC and
goodness of fit, Kuramoto, Welch peak, band-limited amplitude envelopes, Welch
spectra per column, cross spectra and coherence between columns, spectrograms
per column, phase and envelope connectivity between columns, sliding-window FC
and FCD, HMA and the weighted graph measures of the FC matrices -- thin wrappers
over libwcsde.so.

References: simBOLD netwWilsonCowanPlastic.py:140-158; np.corrcoef
whole_sweep_both.py:81; utils.get_all_metrics / kuramoto utils.py:34-50; Welch
peak whole_sweep_both.py:90-95; utils.envelope utils.py:145-154; signal.welch
cortex_run.py:203-209.  Every array
stays on the device; columns are c = b*N + n.
"""
from __future__ import annotations

import ctypes
import functools
import warnings

import numpy as np
import torch

from . import _args, _lib
from .filters import bold_band, lfilter_zi

NEQ = 2000          # wc:145
WELCH_NPERSEG = 4000  # whole_sweep_both.py:90
WELCH_HOP = WELCH_NPERSEG // 2


_FROM_2D = range(2, 65)   # [T][C], [T][B][N] and beyond: the columns are whatever follows the time axis


def _ptr_at(t, offset_elems=0):
    """Device pointer to element `offset_elems` of a contiguous tensor."""
    if not t.is_cuda or not t.is_contiguous():
        raise _lib.WCSDEError("libwcsde takes contiguous device tensors only")
    return ctypes.c_void_p(t.data_ptr() + offset_elems * t.element_size())


class BoldStream:
    """simBOLD for C columns fed in consecutive sample chunks (any chunking).

    n_total = number of E samples per column (len(wc.time)); output after
    finish(): [M][C] fp64 = filtfilt(b, a, BOLD[neq:], axis=0)[::dec].
    """

    def __init__(self, C, n_total, neq=NEQ, dec=1000, bold_dt=0.04, device="cuda"):
        b, a = bold_band(bold_dt)
        zi = lfilter_zi(b, a)
        self.cfg = _lib.WCBoldCfgC(bold_dt, neq, n_total, dec, (ctypes.c_double * 5)(*b),
                                   (ctypes.c_double * 5)(*a), (ctypes.c_double * 4)(*zi))
        L = _lib.lib()
        self.C, self.n_total, self.device = int(C), int(n_total), torch.device(device)
        if n_total - neq < 16:
            raise ValueError("simBOLD needs at least neq + 16 samples (filtfilt padlen 15)")
        self.M = int(L.wc_bold_blocks(ctypes.byref(self.cfg)))
        nd = L.wc_bold_state_doubles(ctypes.byref(self.cfg), self.C)
        self.state = torch.empty(nd, dtype=torch.float64, device=self.device)
        _lib.check(L.wc_bold_init(ctypes.byref(self.cfg), self.C, _lib.ptr(self.state), _lib.stream_handle()),
                   "wc_bold_init")
        self.t = 0

    def feed(self, E, Tc=None, e_ld=0, offset=0, copy=None, copy_ld=0, copy_offset=0):
        """Feed the next Tc samples.  E time-major [Tc][C] (e_ld=0), or a node-major
        buffer with sample tt of column c at flat index offset + c*e_ld + tt.
        copy (fp32 time-major E only): also write the chunk node-major into
        copy at flat index copy_offset + c*copy_ld + tt (the Welch ring)."""
        if Tc is None:
            Tc = E.shape[0]
        f64 = E.dtype == torch.float64
        if not f64 and E.dtype != torch.float32:
            raise TypeError("E must be float32 or float64")
        cp = _ptr_at(copy, copy_offset) if copy is not None else None
        rc = _lib.lib().wc_bold_chunk(ctypes.byref(self.cfg), self.C, _ptr_at(E, offset), int(f64), e_ld, self.t,
                                      Tc, _lib.ptr(self.state), cp, copy_ld, _lib.stream_handle())
        _lib.check(rc, "wc_bold_chunk")
        self.t += Tc

    def finish(self):
        if self.t != self.n_total:
            raise RuntimeError(f"BoldStream fed {self.t} of {self.n_total} samples")
        out = torch.empty((self.M, self.C), dtype=torch.float64, device=self.device)
        _lib.check(_lib.lib().wc_bold_finish(ctypes.byref(self.cfg), self.C, _lib.ptr(self.state), _lib.ptr(out),
                                             _lib.stream_handle()), "wc_bold_finish")
        return out


HILBERT_DIRECT_MAX_M = 8192       # wc_hilbert_phase: M * 8 bytes of LDS in a 64 KB launch
HILBERT_LONG_WS_CAP = 1 << 30     # wc_hilbert_phase_long: workspace ceiling (column tiles beyond it)


def hilbert_phase(x):
    """Unit phasors of hilbert(x, axis=0) for x [M][C] fp64 -> [M][C][2].

    M <= 8192 (HILBERT_DIRECT_MAX_M) takes wc_hilbert_phase, the direct O(M^2)
    convolution; longer series, up to M = 524288, take wc_hilbert_phase_long
    (Bluestein over a power-of-two FFT, O(M log M)) with a workspace for as many
    columns in flight as HILBERT_LONG_WS_CAP allows.  M > 524288 raises."""
    M, C = x.shape
    ph = torch.empty((M, C, 2), dtype=torch.float64, device=x.device)
    if M <= HILBERT_DIRECT_MAX_M:
        ws = _args.workspace(M * 8, x.device)
        _lib.check(_lib.lib().wc_hilbert_phase(C, M, _lib.ptr(x.contiguous()), _lib.ptr(ph), _lib.ptr(ws), M * 8,
                                               _lib.stream_handle()), "wc_hilbert_phase")
        return ph
    return hilbert_phase_long(x, ph)


def _hilbert_long_ws(need, C, M, ws_bytes):
    """ws_bytes of the Bluestein path: the caller's, or by default what all C columns want."""
    if ws_bytes is not None:
        return ws_bytes
    fft_len = max(1 << 15, 1 << (2 * M - 2).bit_length())  # max(2^15, nextpow2(2 M - 1))
    return _args.ws_default(need, need + (C - 1) * 32 * fft_len, HILBERT_LONG_WS_CAP)


def hilbert_phase_long(x, out=None, ws_bytes=None):
    """wc_hilbert_phase_long for x [M][C] fp64, any 2 <= M <= 524288 -> [M][C][2].

    ws_bytes: workspace size (default: what all C columns want, at most
    HILBERT_LONG_WS_CAP, never below the minimum); the result does not depend on it."""
    L = _lib.lib()
    M, C = x.shape
    need = L.wc_hilbert_long_workspace_size(C, M)
    if need == 0:
        raise _lib.WCSDEError(f"hilbert_phase: M = {M} outside 2 .. 524288 (or no columns)")
    ws_bytes = _hilbert_long_ws(need, C, M, ws_bytes)
    ph = torch.empty((M, C, 2), dtype=torch.float64, device=x.device) if out is None else out
    ws = _args.workspace(ws_bytes, x.device)
    _lib.check(L.wc_hilbert_phase_long(C, M, _lib.ptr(x.contiguous()), _lib.ptr(ph), _lib.ptr(ws), ws_bytes,
                                       _lib.stream_handle()), "wc_hilbert_phase_long")
    return ph


def hilbert_envelope(x, method=0, ws_bytes=None):
    """|hilbert(x, axis=0)| for x [M][C] fp64, 2 <= M <= 524288 -> [M][C] (wc_hilbert_envelope).

    method: 0 = the faster of the two (direct below M = 2048, long from there on), 1 = the direct
    convolution (M <= 8192), 2 = the Bluestein FFT.  ws_bytes (long method only): workspace size
    (default: what all C columns want, at most HILBERT_LONG_WS_CAP, never below the minimum); the
    result does not depend on it."""
    L = _lib.lib()
    M, C = x.shape
    need = L.wc_hilbert_envelope_workspace_size(C, M, method)
    if need == 0:
        raise _lib.WCSDEError(f"hilbert_envelope: M = {M} outside 2 .. 524288 (8192 for method 1), no columns "
                              f"or method = {method} not 0, 1, 2")
    # the direct method: q[0..M), nothing to gain from more
    ws_bytes = need if need == M * 8 else _hilbert_long_ws(need, C, M, ws_bytes)
    x = x.contiguous()
    env = torch.empty((M, C), dtype=torch.float64, device=x.device)
    ws = _args.workspace(ws_bytes, x.device)
    _lib.check(L.wc_hilbert_envelope(C, M, _lib.ptr(x), _lib.ptr(env), method, _lib.ptr(ws), ws_bytes,
                                     _lib.stream_handle()), "wc_hilbert_envelope")
    return env


def filtfilt(b, a, x):
    """scipy.signal.filtfilt(b, a, x, axis=0) for a device [T][C] or [T][B][N] fp64 tensor
    (wc_filtfilt: orders 1 .. 8, default padlen 3 (order + 1) < T, lfilter_zi initial conditions);
    b, a host coefficient arrays of equal length, a[0] == 1.  Returns a new tensor of x's shape."""
    b = np.asarray(b, dtype=np.float64)
    a = np.asarray(a, dtype=np.float64)
    if b.ndim != 1 or b.shape != a.shape:
        raise ValueError("filtfilt: b and a must be 1-D arrays of the same length")
    _args.tensor("filtfilt", "x must be a [T][C] or [T][B][N] fp64 device tensor", x, torch.float64, _FROM_2D)
    zi = lfilter_zi(b, a)
    x = x.contiguous()
    y = torch.empty_like(x)
    T = x.shape[0]
    dp = lambda v: (ctypes.c_double * len(v))(*[float(t) for t in v])  # noqa: E731
    _lib.check(_lib.lib().wc_filtfilt(len(a) - 1, dp(b), dp(a), dp(zi), T, x.numel() // T, _lib.ptr(x), _lib.ptr(y),
                                      _lib.stream_handle()), "wc_filtfilt")
    return y


@functools.lru_cache(maxsize=16)
def envelope_filters(dt, fmin, fmax, fcut):
    """utils.envelope's two designs (utils.py:147, 151): signal.bessel(3, [2 dt fmin, 2 dt fmax],
    'bandpass') and, for a truthy fcut, signal.bessel(3, [2 dt fcut], 'low') (else None), as (b, a)
    pairs.  SciPy's own design routines, as optimize_sc.band and for its reason: in (b, a) form the
    last bits of the coefficients matter (a restated design moved the envelope by 2e-8 .. 4e-7 of
    its scale)."""
    from scipy import signal
    bp = signal.bessel(3, [2 * dt * fmin, 2 * dt * fmax], btype="bandpass")
    lp = signal.bessel(3, [2 * dt * fcut], btype="low") if fcut else None
    return bp, lp


def envelope(x, dt=0.002, freqs=(8, 13), fcut=None):
    """utils.envelope (utils.py:145-154) on the device: Bessel order-3 band-pass filtfilt over
    freqs (Hz, at sampling step dt), |hilbert| along time and, for a truthy fcut, a Bessel order-3
    low-pass filtfilt at fcut Hz.  x [T][C] or [T][B][N] fp64 -> a tensor of x's shape."""
    fmin, fmax = freqs
    (bb, ba), lp = envelope_filters(float(dt), float(fmin), float(fmax), float(fcut) if fcut else None)
    T = x.shape[0]
    env = hilbert_envelope(filtfilt(bb, ba, x).reshape(T, -1)).reshape(x.shape)
    return filtfilt(lp[0], lp[1], env) if lp is not None else env


def fc_metrics(bold=None, B=None, N=None, empfc=None, fc_in=None, kuramoto=True, want_fc=False, data_range=1.0):
    """Per simulation: FC (np.corrcoef(BOLD.T)), get_all_metrics vs each empfc,
    mean(FC), Kuramoto sync/meta.

    bold [M][B*N] or [M][B][N] fp64, or fc_in [B][N][N] instead.  empfc: [K][N][N]
    tensor/array or None.  Returns (fc [B][N][N] | None, metrics [B][K][4], extra [B][3]).
    """
    L = _lib.lib()
    if bold is not None:
        M = bold.shape[0]
        bold = bold.reshape(M, B * N).contiguous()
        dev = bold.device
    else:
        fc_in = fc_in.contiguous()
        B, N = fc_in.shape[0], fc_in.shape[1]
        M, dev = 2, fc_in.device
        kuramoto = False
    K = 0 if empfc is None else int(empfc.shape[0])
    emp = None if empfc is None else torch.as_tensor(np.asarray(empfc, dtype=np.float64)).to(dev).contiguous()
    metrics = torch.empty((B, max(K, 1), 4), dtype=torch.float64, device=dev)
    extra = torch.empty((B, 3), dtype=torch.float64, device=dev)
    fc = torch.empty((B, N, N), dtype=torch.float64, device=dev) if want_fc else None
    ph = hilbert_phase(bold) if kuramoto else None
    nws = L.wc_fc_metrics_workspace_size(B, N, M, K, int(want_fc))  # 0 for N <= 96
    ws = _args.workspace(nws, dev) if nws else None
    rc = L.wc_fc_metrics(B, N, M, _lib.ptr(bold) if bold is not None else None, _lib.ptr(fc_in), _lib.ptr(emp), K,
                         float(data_range), _lib.ptr(ph), _lib.ptr(fc), _lib.ptr(metrics), _lib.ptr(extra),
                         _lib.ptr(ws), nws, _lib.stream_handle())
    _lib.check(rc, "wc_fc_metrics")
    return fc, metrics[:, :K], extra


def kuramoto(x, B=1, N=None):
    """utils.kuramoto of x [M][B*N] (or [M][N]) fp64 on the device -> [B][2] (sync, meta)."""
    M = x.shape[0]
    x = x.reshape(M, -1).contiguous()
    N = x.shape[1] // B if N is None else N
    ph = hilbert_phase(x)
    out = torch.empty((B, 2), dtype=torch.float64, device=x.device)
    _lib.check(_lib.lib().wc_kuramoto(B, N, M, _lib.ptr(ph), _lib.ptr(out), _lib.stream_handle()), "wc_kuramoto")
    return out


HMA_JACOBI_MAX_N = 96   # wc_hma: F and V (2 N^2 fp64) in one workgroup's LDS
HMA_MODES_MAX_N = 4096  # wc_hma_modes: 2 N fp64 + 6 N int32 label arrays (40 N B) in 160 KB of LDS
HMA_EIGH_BATCH = 64     # N > 96: matrices per eigensolver call (bounds the V buffers)


def hma(fc, want_clus_num=False):
    """HMA integration / segregation of B FC matrices on the device (HMA.py:30-203
    as run_many_seeds.py:130-133 uses it).

    fc [B][N][N] (or [N][N]) fp64 device tensor, clipped in place (FC < 0 -> 0,
    as HMA.py:55).  Returns a dict of device tensors: hin [B], hse [B],
    hin_node [B][N], hse_node [B][N], sv [B][N] (+ clus_num [B][N-1] int32).
    A matrix that holds a NaN or +Inf after the clip has NaN in all of them (clus_num:
    -1) and keeps those entries; the other matrices of the batch are not affected.
    """
    L = _lib.lib()
    if fc.dim() == 2:
        fc = fc.unsqueeze(0)
    if fc.dtype != torch.float64 or not fc.is_contiguous():
        raise _lib.WCSDEError("hma: fc must be a contiguous fp64 device tensor (it is clipped in place)")
    B, N = fc.shape[0], fc.shape[1]
    dev = fc.device
    out = {k: torch.empty(s, dtype=torch.float64, device=dev)
           for k, s in (("hin", (B,)), ("hse", (B,)), ("hin_node", (B, N)), ("hse_node", (B, N)), ("sv", (B, N)))}
    cn = torch.empty((B, N - 1), dtype=torch.int32, device=dev) if want_clus_num else None
    res = dict(out, clus_num=cn) if want_clus_num else out
    if N <= HMA_JACOBI_MAX_N:
        rc = L.wc_hma(B, N, _lib.ptr(fc), _lib.ptr(out["hin"]), _lib.ptr(out["hse"]), _lib.ptr(out["hin_node"]),
                      _lib.ptr(out["hse_node"]), _lib.ptr(cn), _lib.ptr(out["sv"]), _lib.stream_handle())
        _lib.check(rc, "wc_hma")
        return res
    if N > HMA_MODES_MAX_N:  # fail before the eigensolver, not in wc_hma_modes
        raise _lib.WCSDEError(f"hma: N = {N} > {HMA_MODES_MAX_N} (wc_hma_modes keeps 40 B of labels per node in LDS)")
    # N > 96: F and V no longer fit one workgroup's LDS.  The eigensystem of the symmetrised
    # positive part comes from the batched device eigensolver (rocSOLVER through torch.linalg.eigh),
    # everything after it -- ranks, module levels, Balance, nodal measures -- from wc_hma_modes.
    fc.clamp_(min=0.0)  # HMA.py:55: the caller's FC is clipped in place (-Inf -> 0, a NaN stays)
    for b0 in range(0, B, HMA_EIGH_BATCH):
        b1 = min(B, b0 + HMA_EIGH_BATCH)
        f = fc[b0:b1]
        sym = (f + f.transpose(1, 2)) / 2
        # a matrix that holds a NaN or +Inf never reaches the eigensolver (it raises for the whole batch or
        # returns what it likes): zeros go in its place, and a NaN spectrum tells wc_hma_modes to write NaN
        bad = ~torch.isfinite(sym).all(dim=2).all(dim=1)
        lam, V = torch.linalg.eigh(torch.where(bad[:, None, None], torch.zeros_like(sym), sym))
        lam = torch.where(bad[:, None], torch.full_like(lam, float("nan")), lam)
        vt = V.transpose(1, 2).contiguous()  # row j = eigenvector j (coalesced rows per level)
        sl = {k: v[b0:b1] for k, v in out.items()}
        rc = L.wc_hma_modes(b1 - b0, N, _lib.ptr(lam.contiguous()), _lib.ptr(vt), _lib.ptr(sl["hin"]),
                            _lib.ptr(sl["hse"]), _lib.ptr(sl["hin_node"]), _lib.ptr(sl["hse_node"]),
                            _lib.ptr(cn[b0:b1] if cn is not None else None), _lib.ptr(sl["sv"]),
                            _lib.stream_handle())
        _lib.check(rc, "wc_hma_modes")
        del lam, V, vt
    return res


class WelchAccumulator:
    """Running node-summed |FFT|^2 of 4000-sample Hann segments (welch, nperseg=4000)."""

    def __init__(self, B, N, device="cuda"):
        L = _lib.lib()
        self.B, self.N, self.device = B, N, torch.device(device)
        self.bins = L.wc_welch_bins()
        self.ws = torch.empty(L.wc_welch_workspace_size() // 8, dtype=torch.float64, device=self.device)
        _lib.check(L.wc_welch_prepare(_lib.ptr(self.ws), self.ws.numel() * 8, _lib.stream_handle()),
                   "wc_welch_prepare")
        self.acc = torch.zeros((B, self.bins), dtype=torch.float64, device=self.device)
        self.nseg = 0

    def accumulate(self, E, ld, slot, nslots, seg0, nseg=1):
        """Add segments [seg0 + 2000 k, seg0 + 2000 k + 4000), k < nseg (1, 2 or 4), of every column of
        the node-major ring E (segments in one launch read their shared halves once from HBM)."""
        f64 = E.dtype == torch.float64
        rc = _lib.lib().wc_welch_accumulate(self.B, self.N, _ptr_at(E), int(f64), ld, slot, nslots, seg0, nseg,
                                            _lib.ptr(self.ws), _lib.ptr(self.acc), _lib.stream_handle())
        _lib.check(rc, "wc_welch_accumulate")
        self.nseg += nseg

    def peak(self, fs=500.0, want_psd=False):
        peak = torch.empty(self.B, dtype=torch.float64, device=self.device)
        psd = torch.empty((self.B, self.bins), dtype=torch.float64, device=self.device) if want_psd else None
        _lib.check(_lib.lib().wc_welch_peak(self.B, self.N, self.nseg, fs, _lib.ptr(self.acc), _lib.ptr(peak),
                                            _lib.ptr(psd), _lib.stream_handle()), "wc_welch_peak")
        return peak, psd


GRAPH_MAX_N = 96    # wc_graph_*: one matrix per workgroup, in LDS
GRAPH_PATH_MEASURES = ("dist", "hops", "charpath", "efficiency", "ecc", "radius", "diameter")  # wc_graph_paths
GRAPH_CLUSTER_MEASURES = ("clustering", "transitivity", "strengths", "degrees")                # wc_graph_clustering
GRAPH_MEASURES = GRAPH_PATH_MEASURES + ("local_efficiency",) + GRAPH_CLUSTER_MEASURES
_GRAPH_STATS = {"charpath": 0, "efficiency": 1, "radius": 2, "diameter": 3}  # columns of wc_graph_paths' stats


def graph_measures(w, measures=GRAPH_MEASURES, lengths=False, include_infinite=True):
    """Weighted graph measures of B matrices on the device (the reference's graph_utils.py, after
    Rubinov & Sporns): w [B][N][N] or [N][N] fp64 device tensor, 2 <= N <= 96 -> a dict from measure
    name to a device tensor ([B] leading, or without it for a single matrix).  No symmetry is assumed.

    From wc_graph_paths (distance_wei + charpath): "dist" [N][N] shortest weighted paths over the
    lengths 1/w (w itself with lengths=True), +inf where there is none; "hops" [N][N] int32, their
    edges; "charpath" and "efficiency", the means of D and 1/D off the diagonal (the latter is
    efficiency_wei(local=False)); "ecc" [N], "radius", "diameter".  include_infinite=False leaves the
    infinite distances out of those means and maxima.  "local_efficiency" [N] from
    wc_graph_local_efficiency (efficiency_wei(local=True)).  From wc_graph_clustering: "clustering" [N]
    (clustering_coef_wu), "transitivity" (transitivity_wu), "strengths" [N] (strengths_und), "degrees"
    [N] int32 (degrees_und).  Only the kernels that the asked measures need are launched.  A matrix with
    a negative or NaN entry has NaN (hops: -1) in the path measures and the local efficiency.
    lengths=True goes with the path measures only: the others are defined on weights.

    Composes with fc_metrics(..., want_fc=True) and hma: both leave FC matrices of this layout."""
    names = _args.names("graph_measures", measures, GRAPH_MEASURES)
    if lengths and any(m not in GRAPH_PATH_MEASURES for m in names):
        raise ValueError(f"graph_measures: lengths=True goes with the path measures {list(GRAPH_PATH_MEASURES)} "
                         "only, the others are defined on weights")
    w, single, B, N = _graph_stack("graph_measures", w)
    L = _lib.lib()
    dev, st = w.device, _lib.stream_handle()
    want = set(names)

    def new(key, *shape, dtype=torch.float64):
        return torch.empty((B,) + shape, dtype=dtype, device=dev) if want & set(key) else None

    res = {}
    if want & set(GRAPH_PATH_MEASURES):
        dist, hops = new(("dist",), N, N), new(("hops",), N, N, dtype=torch.int32)
        stats, ecc = new(tuple(_GRAPH_STATS), 4), new(("ecc",), N)
        _lib.check(L.wc_graph_paths(B, N, _lib.ptr(w), int(bool(lengths)), int(bool(include_infinite)), _lib.ptr(dist),
                                    _lib.ptr(hops), _lib.ptr(stats), _lib.ptr(ecc), st), "wc_graph_paths")
        res.update(dist=dist, hops=hops, ecc=ecc)
        if stats is not None:
            res.update({m: stats[:, k] for m, k in _GRAPH_STATS.items()})
    if "local_efficiency" in want:
        res["local_efficiency"] = new(("local_efficiency",), N)
        _lib.check(L.wc_graph_local_efficiency(B, N, _lib.ptr(w), _lib.ptr(res["local_efficiency"]), st),
                   "wc_graph_local_efficiency")
    if want & set(GRAPH_CLUSTER_MEASURES):
        clus, trans = new(("clustering",), N), new(("transitivity",))
        stre, deg = new(("strengths",), N), new(("degrees",), N, dtype=torch.int32)
        _lib.check(L.wc_graph_clustering(B, N, _lib.ptr(w), _lib.ptr(clus), _lib.ptr(trans), _lib.ptr(stre),
                                         _lib.ptr(deg), st), "wc_graph_clustering")
        res.update(clustering=clus, transitivity=trans, strengths=stre, degrees=deg)
    return _args.unbatch(single, {m: res[m] for m in names})


def _graph_stack(name, w):
    """(w contiguous, single, B, N) of a [B][N][N] or [N][N] fp64 tensor, refused before the device is touched."""
    w, single, B, N = _args.stack(name, "w must be a [B][N][N] or [N][N] fp64 device tensor", w, square=True)
    if N < 2 or N > GRAPH_MAX_N or B < 1:
        raise ValueError(f"{name}: N = {N}, B = {B}: needs B >= 1 and 2 <= N <= {GRAPH_MAX_N} "
                         "(one matrix per workgroup, in LDS)")
    return w, single, B, N


def graph_betweenness(w, lengths=False):
    """Node betweenness centrality of B matrices on the device (wc_graph_betweenness; the reference's
    betweenness_wei): w [B][N][N] or [N][N] fp64 device tensor, 2 <= N <= 96 -> [B][N], or [N] for a
    single matrix.  w holds weights, with the connection lengths 1/w where w != 0, or, with
    lengths=True, the lengths themselves; a zero is no edge, the diagonal is ignored, no symmetry is
    assumed.  Ordered pairs are counted: an undirected graph has twice the textbook value, as in the
    reference; divide by (N - 1)(N - 2) for the range [0, 1].  Ties between shortest paths resolve as
    in the reference; with unique shortest paths every value is an exact integer.  A matrix with a
    negative or NaN entry has NaN in its row.  The same matrix gives the same bits in any batch.

    Composes with fc_metrics(..., want_fc=True) and hma, like graph_measures."""
    w, single, B, N = _graph_stack("graph_betweenness", w)
    bc = torch.empty((B, N), dtype=torch.float64, device=w.device)
    _lib.check(_lib.lib().wc_graph_betweenness(B, N, _lib.ptr(w), int(bool(lengths)), _lib.ptr(bc),
                                               _lib.stream_handle()), "wc_graph_betweenness")
    return _args.unbatch(single, bc)


GRAPH_MODULE_MEASURES = ("participation", "zscore", "modularity")
GRAPH_MODULE_DEGREES = {"undirected": 0, "out": 0, "in": 1}


def graph_module_measures(w, ci, measures=GRAPH_MODULE_MEASURES, degree="undirected", zflag=0, gamma=1.0,
                          n_modules=None):
    """Measures of a given partition of B matrices on the device (wc_graph_modules): w [B][N][N] or
    [N][N] fp64 device tensor, 2 <= N <= 96; ci int32 device tensor of module labels, [B][N] or [N]
    shared by every matrix, labels in [0, n_modules) (n_modules=None: [0, N)) -> a dict from measure
    name to a device tensor.

    "participation" [N]: the participation coefficient (the reference's participation_coef),
    1 - sum_m (sum_{j in m} W_ij)^2 / (sum_j W_ij)^2, 0 where the strength is 0; degree "undirected" or
    "out" uses rows, "in" the transpose.  "zscore" [N]: the within-module degree z-score
    (module_degree_zscore) with the reference's flag as zflag: 0 undirected, 1 W, 2 W^T, 3 W + W^T;
    population standard deviation; where the reference's NaN rule gives 0 (a single-member module, a
    module of equal degrees) this gives 0, and like the reference it therefore cannot tell a NaN in w
    from such a case: a NaN entry shows as 0 in the z-scores of its module.  "modularity": Q =
    (1/s) sum_ij (W_ij - gamma k_i^out k_j^in / s) delta(ci_i, ci_j), s = sum W (Newman; Leicht &
    Newman for a directed matrix).  Negative weights are summed as they are.  Only the outputs asked
    for are allocated.  A matrix with a label out of range has NaN in every measure; no label is read
    back to the host."""
    names = _args.names("graph_module_measures", measures, GRAPH_MODULE_MEASURES)
    if degree not in GRAPH_MODULE_DEGREES:
        raise ValueError(f"graph_module_measures: degree {degree!r}, must be one of {list(GRAPH_MODULE_DEGREES)}")
    if isinstance(zflag, bool) or not isinstance(zflag, int) or not 0 <= zflag <= 3:
        raise ValueError(f"graph_module_measures: zflag {zflag!r}, must be 0, 1, 2 or 3")
    w, single, B, N = _graph_stack("graph_module_measures", w)
    _args.tensor("graph_module_measures", f"ci must be an int32 device tensor [N] or [B][N] with N = {N}, B = {B}", ci,
                 torch.int32, shapes=((N,), (B, N)))
    K = N if n_modules is None else int(n_modules)
    if K < 1 or K > N:
        raise ValueError(f"graph_module_measures: n_modules = {n_modules}, must be in [1, N = {N}]")
    if ci.device != w.device:
        raise ValueError("graph_module_measures: ci and w must be on the same device")
    ci = (ci.expand(B, N) if ci.dim() == 1 else ci).contiguous()

    def new(m, *shape):
        return torch.empty((B,) + shape, dtype=torch.float64, device=w.device) if m in names else None

    res = {"participation": new("participation", N), "zscore": new("zscore", N), "modularity": new("modularity")}
    _lib.check(_lib.lib().wc_graph_modules(B, N, K, _lib.ptr(w), _lib.ptr(ci), GRAPH_MODULE_DEGREES[degree], zflag,
                                           float(gamma), _lib.ptr(res["participation"]), _lib.ptr(res["zscore"]),
                                           _lib.ptr(res["modularity"]), _lib.stream_handle()), "wc_graph_modules")
    return _args.unbatch(single, {m: res[m] for m in names})


GRAPH_LOUVAIN_OBJECTIVES = ("modularity", "potts")    # graph_louvain's built-in objectives; or a tensor
GRAPH_PARTITION_SEARCH = ("graph_louvain", "graph_agreement", "graph_consensus_matrix")  # wc_louvain.hip
GRAPH_LOUVAIN_MIN_WEIGHT = -1e-10                     # graph_utils.py:999: anything below is refused


def _louvain_labels(name, ci, B, N, dev):
    """Starting labels [N] or [B][N] (any integers) -> int32 [B][N] in [0, N), dense in the order of
    the sorted distinct values of each row (np.unique's inverse), on the device and without a sync."""
    if not isinstance(ci, torch.Tensor):
        ci = torch.from_numpy(np.ascontiguousarray(np.asarray(ci)))
    if ci.dtype not in (torch.int32, torch.int64, torch.int16, torch.int8, torch.uint8) or ci.dim() not in (1, 2) \
            or ci.shape[-1] != N or (ci.dim() == 2 and ci.shape[0] != B):
        raise TypeError(f"{name}: ci must hold integer labels, [N] or [B][N] with N = {N}, B = {B}")
    ci = ci.to(dev).long()
    ci = ci.expand(B, N) if ci.dim() == 1 else ci
    srt, idx = ci.sort(dim=1, stable=True)
    rank = torch.zeros_like(srt)
    rank[:, 1:] = (srt[:, 1:] != srt[:, :-1]).cumsum(1)
    return torch.empty_like(rank).scatter_(1, idx, rank).int().contiguous()


def _halving_sum(x):
    """Sum over the last axis by halving it with elementwise adds: torch's own reductions choose their
    order by the shape, so a matrix would sum to other bits alone than inside a batch."""
    n = x.shape[-1]
    while n > 1:
        h = (n + 1) // 2
        top = x[..., :n - h] + x[..., h:n]
        x = top if n == 2 * h else torch.cat([top, x[..., n - h:h]], dim=-1)
        n = h
    return x[..., 0]


def graph_louvain(w, seeds=0, gamma=1.0, ci=None, objective="modularity", want_info=False):
    """Louvain community search on the device (wc_graph_louvain; the reference's community_louvain):
    w [B][N][N] or [N][N] fp64 device tensor, 2 <= N <= 96 -> (ci int32, q fp64), ci [B][R][N] with
    labels 0 .. K-1 (the reference's minus 1) and q [B][R] the objective reached.  seeds is an int or
    a sequence of R ints; an int gives no R axis, as an [N][N] input gives no batch axis.  Every
    (matrix, seed) pair is an independent run in one launch.

    objective "modularity": obj = W - gamma outer(rowsum, colsum) / s, s = sum W (Newman; Leicht &
    Newman for a directed W); "potts": W - gamma (W == 0), W must be binary; or a [N][N] / [B][N][N]
    fp64 tensor, used as it is (gamma is ignored) and symmetrised as (B + B^T) / 2, with a warning,
    where it is not symmetric.  obj is built with torch ops on the device.  ci is None (every node its
    own module) or starting labels, any integers, [N] for all matrices or [B][N].  A W with an entry
    below -1e-10 raises ValueError, as the reference refuses it (this check and the Potts one read
    one flag back from the device).

    The algorithm is the reference's, decision for decision.  The visiting order is not numpy's:
    sweep t of a run visits the nodes in the stable argsort of Philox4x32-10 words keyed by
    (seed, t) (include/wcsde.h), so a seed does not reproduce the partition numpy gives for that
    seed, only the reference's algorithm under that order; the same seed gives the same bits in
    every call and every batch.  A matrix with a NaN or inf in obj or s has ci = -1 and q = NaN (so
    has an empty graph under "modularity": s = 0; the reference returns the starting partition with
    q = NaN there); so has a run that does not settle within 1000 sweeps of a level, where the
    reference raises.  That happens on directed matrices at gamma > 1 (a node's gain is taken from its
    row alone, and nodes then move in and out of modules without end); emptied modules keep rounding
    residues of 1e-17 in Hnm there, between which a node may choose, so on a directed matrix at
    gamma > 1 the device, which sums in another order than numpy, may take other turns than the
    reference; everywhere else the tests find the reference's partition exactly.  want_info=True adds info int32 [B][R][2]: levels and node sweeps in all."""
    name = "graph_louvain"
    custom = isinstance(objective, torch.Tensor)
    if not custom and (not isinstance(objective, str) or objective not in GRAPH_LOUVAIN_OBJECTIVES):
        raise ValueError(f"{name}: objective {objective!r}, must be one of {list(GRAPH_LOUVAIN_OBJECTIVES)} or a "
                         "[N][N] / [B][N][N] fp64 device tensor (negative_sym and negative_asym are not built: "
                         "the reference refuses negative weights before it reaches them)")
    seed_arr, scalar = _args.seeds(name, seeds)
    w, single, B, N = _graph_stack(name, w)
    wb = w.reshape(B, N, N)
    dev = w.device
    if custom:
        _args.tensor(name, f"an objective tensor must be fp64 [N][N] or [B][N][N] on w's device, N = {N}, B = {B}",
                     objective, torch.float64, shapes=((N, N), (B, N, N)), device=dev)
    ci0 = None if ci is None else _louvain_labels(name, ci, B, N, dev)
    refuse = wb.min() < GRAPH_LOUVAIN_MIN_WEIGHT
    if not custom and objective == "potts":
        refuse = torch.stack([refuse, ~((wb == 0) | (wb == 1) | wb.isnan()).all()])
    refuse = refuse.reshape(-1).tolist()
    if refuse[0]:
        raise ValueError(f"{name}: w must not contain negative weights (an entry below -1e-10)")
    if len(refuse) > 1 and refuse[1]:
        raise ValueError(f"{name}: the Potts objective requires a binary w")
    ko, ki = _halving_sum(wb), _halving_sum(wb.transpose(1, 2))     # row and column sums, [B][N]
    s = _halving_sum(ko)
    if custom:
        obj = objective.expand(B, N, N)
        close = torch.isclose(obj, obj.transpose(1, 2)).all(dim=2).all(dim=1)
        if not bool(close.all()):
            warnings.warn(f"{name}: objective function matrix not symmetric, symmetrizing", stacklevel=2)
            obj = torch.where(close[:, None, None], obj, (obj + obj.transpose(1, 2)) / 2)
    elif objective == "modularity":
        obj = wb - float(gamma) * (ko[:, :, None] * ki[:, None, :]) / s[:, None, None]
    else:
        obj = wb - float(gamma) * (wb == 0).to(torch.float64)
    obj = obj.contiguous()
    R = len(seed_arr)
    seeds_dev = _args.upload_seeds(seed_arr, dev)
    out = torch.empty((B, R, N), dtype=torch.int32, device=dev)
    q = torch.empty((B, R), dtype=torch.float64, device=dev)
    info = torch.empty((B, R, 2), dtype=torch.int32, device=dev) if want_info else None
    _lib.check(_lib.lib().wc_graph_louvain(B, R, N, _lib.ptr(obj), _lib.ptr(s), _lib.ptr(ci0), _lib.ptr(seeds_dev),
                                           _lib.ptr(out), _lib.ptr(q), _lib.ptr(info), _lib.stream_handle()),
               "wc_graph_louvain")
    return _args.unrun(scalar, single, (out, q) + ((info,) if want_info else ()))


def graph_agreement(ci):
    """Agreement matrix of R partitions on the device (wc_graph_agreement; the reference's agreement):
    ci int32 device tensor [B][R][N] or [R][N] (graph_louvain's layout) -> D fp64 [B][N][N] or [N][N],
    the number of the R partitions in which i and j share a label, exact, 0 on the diagonal.  A
    negative label (a run that graph_louvain refused) makes its matrix's D NaN."""
    ci, single, B, N = _args.stack("graph_agreement", "ci must be an int32 device tensor [B][R][N] or [R][N]", ci,
                                   torch.int32)
    R = ci.shape[-2]
    if N < 2 or N > GRAPH_MAX_N or B < 1 or R < 1:
        raise ValueError(f"graph_agreement: N = {N}, R = {R}, B = {B}: needs B, R >= 1 and 2 <= N <= {GRAPH_MAX_N}")
    D = torch.empty((B, N, N), dtype=torch.float64, device=ci.device)
    _lib.check(_lib.lib().wc_graph_agreement(B, R, N, _lib.ptr(ci), _lib.ptr(D), _lib.stream_handle()),
               "wc_graph_agreement")
    return _args.unbatch(single, D)


def graph_consensus_matrix(w, reps=100, tau=0.5, gamma=1.0, ci=None, objective="modularity", seeds=None):
    """Thresholded agreement of reps Louvain runs on the device (the reference's get_agreement_matrix):
    graph_louvain with seeds 0 .. reps-1 (or the reps seeds given), graph_agreement, D / reps, entries
    below tau set to 0, the diagonal 0 -> [B][N][N] or [N][N].  One Louvain launch and one agreement
    launch serve the whole stack.  A matrix that graph_louvain refuses is NaN throughout."""
    _args.integer("graph_consensus_matrix", f"reps = {reps!r}, must be a positive int", reps, 1)
    if seeds is None:
        seeds = range(int(reps))
    elif isinstance(seeds, (int, np.integer)) or len(seeds) != reps:
        raise ValueError("graph_consensus_matrix: seeds must be a sequence of length reps, or None")
    part, _ = graph_louvain(w, seeds=list(seeds), gamma=gamma, ci=ci, objective=objective)
    D = graph_agreement(part) / int(reps)
    return torch.where(D < float(tau), torch.zeros_like(D), D)


FCD_MAX_N = 96           # wc_fcd, wc_fcd_phase: one window's correlation matrix, a tile's phasors per workgroup
FCD_MAX_WINDOWS = 4096    # WC_FCD_MAX_WINDOWS
FCD_PHASE_MAX_M = 4096    # WC_FCD_PHASE_MAX_M
FCD_WS_CAP = 1 << 30      # wc_fcd: workspace ceiling (chunks of simulations beyond it)
FCD_METHODS = ("corr", "phase")


def fcd(x, window=None, step=None, method="corr", want_windows=False, trim=0, ws_bytes=None):
    """Functional connectivity dynamics of B simulations on the device: x [M][C] (one simulation)
    or [M][B][N] fp64 device tensor, time-major.

    method="corr" (wc_fcd; Hansen et al. 2015): sliding windows of `window` samples every `step`
    (default 1), nw = (M - window) // step + 1 of them; FC_k = np.corrcoef of window k, its pattern the
    strict upper triangle (utils.flat_FC's order, P = N (N - 1) / 2 entries); fcd[b][k][l] the Pearson
    correlation of patterns k and l -> fcd [B][nw][nw] ([nw][nw] for 2-D input), exactly symmetric
    with a unit diagonal; with want_windows also the patterns, (fcd, windows [B][nw][P]).  A column
    that is constant within a window makes row and column k of fcd NaN, nothing else.  3 <= N <= 96,
    2 <= window <= M, nw <= FCD_MAX_WINDOWS = 4096.  ws_bytes: workspace size (default: what all B
    simulations want, at most FCD_WS_CAP, never below the minimum, 8 simulations' patterns); the result
    does not depend on it.

    method="phase" (wc_fcd_phase; Deco & Kringelbach 2016): x must be band-limited already; from
    hilbert_phase's phasors, less `trim` samples at either end (the transform's edge effects),
    d_t[i][j] = cos(theta_i(t) - theta_j(t)) and fcd[b][t][u] the cosine similarity of the strict upper
    triangles of d_t and d_u -> [B][M - 2 trim][M - 2 trim].  2 <= N <= 96, M - 2 trim <=
    FCD_PHASE_MAX_M = 4096.  window and step have no meaning here and must be left None."""
    if method not in FCD_METHODS:
        raise ValueError(f"fcd: unknown method {method!r}, must be one of {list(FCD_METHODS)}")
    x, single, B, N = _args.stack("fcd", "x must be a [M][C] or [M][B][N] fp64 device tensor", x, batch=1)
    M = x.shape[0]
    if B < 1 or N > FCD_MAX_N:
        raise ValueError(f"fcd: N = {N}, B = {B}: needs B >= 1 and N <= {FCD_MAX_N} (one window's correlation "
                         "matrix, a tile's phasors per workgroup)")
    L = _lib.lib()
    if method == "phase":
        if window is not None or step is not None:
            raise ValueError("fcd: method='phase' has no windows: window and step must be left None")
        if want_windows or ws_bytes is not None:
            raise ValueError("fcd: method='phase' takes neither want_windows nor ws_bytes")
        trim = int(trim)
        Mt = M - 2 * trim
        if trim < 0 or N < 2 or M < 2 or Mt < 1 or Mt > FCD_PHASE_MAX_M:
            raise ValueError(f"fcd: method='phase' needs N >= 2, trim >= 0 and 1 <= M - 2 trim <= {FCD_PHASE_MAX_M} "
                             f"(N = {N}, M = {M}, trim = {trim})")
        ph = hilbert_phase(x.reshape(M, B * N))[trim:M - trim].view(Mt, B, N, 2)
        return _args.unbatch(single, fcd_from_phasors(ph))
    if trim:
        raise ValueError("fcd: method='corr' takes no trim (it goes with method='phase')")
    if window is None:
        raise ValueError("fcd: method='corr' needs a window length")
    window, step = int(window), (1 if step is None else int(step))
    if N < 3 or window < 2 or window > M or step < 1:
        raise ValueError(f"fcd: method='corr' needs N >= 3, 2 <= window <= M and step >= 1 (N = {N}, M = {M}, "
                         f"window = {window}, step = {step})")
    nw = (M - window) // step + 1
    if nw > FCD_MAX_WINDOWS:
        raise ValueError(f"fcd: {nw} windows > {FCD_MAX_WINDOWS}: take a larger step")
    P = N * (N - 1) // 2
    need = L.wc_fcd_workspace_size(B, N, M, window, step)
    nbytes = _args.ws_default(need, (nw * P + nw) * 8 * B, FCD_WS_CAP) if ws_bytes is None else int(ws_bytes)
    out = torch.empty((B, nw, nw), dtype=torch.float64, device=x.device)
    pats = torch.empty((B, nw, P), dtype=torch.float64, device=x.device) if want_windows else None
    ws = _args.workspace(nbytes, x.device)
    _lib.check(L.wc_fcd(B, N, M, _lib.ptr(x), window, step, _lib.ptr(out), _lib.ptr(pats), _lib.ptr(ws), nbytes,
                        _lib.stream_handle()), "wc_fcd")
    return _args.unbatch(single, (out, pats) if want_windows else out)


def fcd_from_phasors(phasor):
    """The phase-coherence FCD (wc_fcd_phase) of unit phasors the caller already holds: phasor
    [M][C][2] or [M][B][N][2] fp64 (hilbert_phase's output, trimmed as wanted) -> [M][M] or [B][M][M];
    see fcd(method="phase").  2 <= N <= 96, M <= FCD_PHASE_MAX_M = 4096."""
    phasor, single, B, N = _args.stack("fcd_from_phasors", "phasor must be a [M][C][2] or [M][B][N][2] fp64 device "
                                       "tensor", phasor, ndim=4, batch=1, last=2)
    M = phasor.shape[0]
    if B < 1 or N < 2 or N > FCD_MAX_N or M < 1 or M > FCD_PHASE_MAX_M:
        raise ValueError(f"fcd_from_phasors: N = {N}, B = {B}, M = {M}: needs B >= 1, 2 <= N <= {FCD_MAX_N} and "
                         f"1 <= M <= {FCD_PHASE_MAX_M}")
    out = torch.empty((B, M, M), dtype=torch.float64, device=phasor.device)
    _lib.check(_lib.lib().wc_fcd_phase(B, N, M, _lib.ptr(phasor), _lib.ptr(out), _lib.stream_handle()),
               "wc_fcd_phase")
    return _args.unbatch(single, out)


FCD_KS_CHUNK = 256        # fcd_ks: simulations a pass (bounds the sorted copies)


def fcd_ks(fcd, emp_values, lag=1):
    """Two-sample Kolmogorov-Smirnov statistic, per simulation, between the entries fcd[b][k][l] with
    l - k >= lag and the 1-D sample emp_values (an empirical FCD's entries): the usual distance a sweep is
    fitted on.  fcd [B][nw][nw] or [nw][nw] fp64 device tensor -> [B] (a scalar tensor for one matrix);
    a simulation with a NaN among its selected entries gets NaN.  Plain torch (sort, searchsorted) on the
    device, FCD_KS_CHUNK simulations at a time."""
    f, single, _, _ = _args.stack("fcd_ks", "fcd must be a [B][nw][nw] or [nw][nw] fp64 device tensor", fcd, square=True)
    f = f[None] if single else f
    nw, lag = f.shape[-1], int(lag)
    if lag < 1 or lag >= nw:
        raise ValueError(f"fcd_ks: lag = {lag} must be in 1 .. nw - 1 = {nw - 1}")
    emp = torch.as_tensor(np.asarray(emp_values.cpu() if isinstance(emp_values, torch.Tensor) else emp_values,
                                     dtype=np.float64))
    if emp.dim() != 1 or emp.numel() == 0 or bool(torch.isnan(emp).any()):
        raise ValueError("fcd_ks: emp_values must be a 1-D sample without NaN, not empty")
    emp = emp.to(f.device).sort().values
    mask = torch.ones((nw, nw), dtype=torch.bool, device=f.device).triu(lag)
    na, ne = int(mask.sum()), emp.numel()
    out = torch.empty(f.shape[0], dtype=torch.float64, device=f.device)
    for b0 in range(0, f.shape[0], FCD_KS_CHUNK):
        a = f[b0:b0 + FCD_KS_CHUNK][:, mask]                   # [b][na]
        bad = torch.isnan(a).any(dim=1)
        a = a.nan_to_num(nan=0.0).sort(dim=1).values
        pooled = torch.cat((a, emp.expand(a.shape[0], ne)), dim=1).contiguous()
        cdf_a = torch.searchsorted(a, pooled, right=True).double() / na
        cdf_e = torch.searchsorted(emp, pooled, right=True).double() / ne
        d = (cdf_a - cdf_e).abs().amax(dim=1)
        out[b0:b0 + FCD_KS_CHUNK] = torch.where(bad, torch.full_like(d, float("nan")), d)
    return _args.unbatch(single, out)


LEIDA_MAX_N = 1024        # wc_leida_eigvec, wc_kmeans_*: a row in one wave's registers
KMEANS_MAX_K = 32         # wc_kmeans_*, wc_state_stats
KMEANS_METRICS = {"sqeuclidean": 0, "cosine": 1}   # WC_KMEANS_SQEUCLIDEAN, WC_KMEANS_COSINE
KMEANS_UPDATE_BLOCK = 256  # WC_KMEANS_UPDATE_BLOCK: rows of a partial sum of wc_kmeans_update


def leida(x, trim=0):
    """LEiDA's first stage (Cabral et al. 2017) on the device: x [M][C] (one simulation) or [M][B][N] fp64
    device tensor, time-major and band-limited already.  From hilbert_phase's phasors, less `trim`
    samples at either end (the transform's edge effects, as fcd(method="phase")), the leading eigenvector
    of every instantaneous phase-coherence matrix dPC(t)[i][j] = cos(theta_i(t) - theta_j(t))
    (leida_from_phasors) -> (vec [M - 2 trim][B][N], share [M - 2 trim][B]), without B for 2-D input.
    2 <= N <= LEIDA_MAX_N = 1024."""
    x, single, B, N = _args.stack("leida", "x must be a [M][C] or [M][B][N] fp64 device tensor", x, batch=1)
    M = x.shape[0]
    trim = int(trim)
    Mt = M - 2 * trim
    if B < 1 or N < 2 or N > LEIDA_MAX_N or trim < 0 or M < 2 or Mt < 1:
        raise ValueError(f"leida: needs B >= 1, 2 <= N <= {LEIDA_MAX_N}, trim >= 0, M >= 2 and M - 2 trim >= 1 "
                         f"(N = {N}, B = {B}, M = {M}, trim = {trim})")
    ph = hilbert_phase(x.reshape(M, B * N))[trim:M - trim]
    return leida_from_phasors(ph if single else ph.view(Mt, B, N, 2))


def leida_from_phasors(phasor):
    """The leading eigenvector of every phase-coherence matrix (wc_leida_eigvec) of phasors the caller
    already holds: phasor [M][N][2] or [M][B][N][2] fp64 (hilbert_phase's output, trimmed as wanted; unit
    modulus is not required) -> (vec, share): vec [M][N] or [M][B][N], unit vectors, most of their
    entries negative (Cabral's sign rule); share [M] or [M][B] = lambda1 / (lambda1 + lambda2), the part
    of dPC's variance that the vector carries.  dPC = c c^T + s s^T has rank <= 2, so the vector comes
    from the closed-form eigenvector of a 2 x 2 Gram matrix: three dot products a row, nothing N x N.
    A row with lambda1 = lambda2 exactly, or with a NaN or an infinity, is NaN.  2 <= N <= 1024."""
    _args.tensor("leida_from_phasors", "phasor must be a [M][N][2] or [M][B][N][2] fp64 device tensor", phasor,
                 torch.float64, (3, 4), last=2)
    N, lead = phasor.shape[-2], tuple(phasor.shape[:-2])
    R = int(np.prod(lead))
    if R < 1 or N < 2 or N > LEIDA_MAX_N:
        raise ValueError(f"leida_from_phasors: N = {N}, {R} rows: needs at least one row and 2 <= N <= {LEIDA_MAX_N}")
    phasor = phasor.contiguous()
    if phasor.data_ptr() % 16:
        phasor = phasor.clone()
    vec = torch.empty(lead + (N,), dtype=torch.float64, device=phasor.device)
    share = torch.empty(lead, dtype=torch.float64, device=phasor.device)
    _lib.check(_lib.lib().wc_leida_eigvec(R, N, _lib.ptr(phasor), _lib.ptr(vec), _lib.ptr(share),
                                          _lib.stream_handle()), "wc_leida_eigvec")
    return vec, share


def _kmeans_rows(name, x):
    return _args.tensor(name, "x must be a [R][N] or [M][B][N] fp64 device tensor", x, torch.float64, (2, 3))


def _kmeans_args(name, x, centroids, metric):
    """What the k-means functions refuse before they touch the device -> (x as [R][N], centroids
    [K][N], metric code, the leading shape of x)."""
    if metric not in KMEANS_METRICS:
        raise ValueError(f"{name}: unknown metric {metric!r}, must be one of {list(KMEANS_METRICS)}")
    _kmeans_rows(name, x)
    _args.tensor(name, "centroids must be a [K][N] fp64 device tensor", centroids, torch.float64, (2,))
    N, K = x.shape[-1], centroids.shape[0]
    if centroids.shape[1] != N:
        raise ValueError(f"{name}: centroids have {centroids.shape[1]} nodes, x has N = {N}")
    if x.numel() == 0 or N < 2 or N > LEIDA_MAX_N:
        raise ValueError(f"{name}: N = {N}: needs at least one row and 2 <= N <= {LEIDA_MAX_N}")
    if K < 1 or K > KMEANS_MAX_K:
        raise ValueError(f"{name}: K = {K}: needs 1 <= K <= {KMEANS_MAX_K}")
    return x.reshape(-1, N).contiguous(), centroids.contiguous(), KMEANS_METRICS[metric], tuple(x.shape[:-1])


def _assign(x2, cent, code):
    R, N = x2.shape
    labels = torch.empty(R, dtype=torch.int32, device=x2.device)
    dist = torch.empty(R, dtype=torch.float64, device=x2.device)
    _lib.check(_lib.lib().wc_kmeans_assign(R, N, cent.shape[0], _lib.ptr(x2), _lib.ptr(cent), code, _lib.ptr(labels),
                                           _lib.ptr(dist), _lib.stream_handle()), "wc_kmeans_assign")
    return labels, dist


def _update(x2, labels, cent, code, ws_bytes=None):
    L = _lib.lib()
    (R, N), K = x2.shape, cent.shape[0]
    nbytes = L.wc_kmeans_workspace_size(R, N, K, code) if ws_bytes is None else int(ws_bytes)
    ws = _args.workspace(nbytes, x2.device)
    new = torch.empty_like(cent)
    count = torch.empty(K, dtype=torch.int64, device=x2.device)
    _lib.check(L.wc_kmeans_update(R, N, K, _lib.ptr(x2), _lib.ptr(labels), _lib.ptr(cent), code, _lib.ptr(new),
                                  _lib.ptr(count), _lib.ptr(ws), nbytes, _lib.stream_handle()), "wc_kmeans_update")
    return new, count


def kmeans_assign(x, centroids, metric="cosine"):
    """The nearest centroid of every row (wc_kmeans_assign): x [R][N] or [M][B][N], centroids [K][N], fp64
    device tensors -> (labels int32, dist), shaped as x without its last axis.  metric "sqeuclidean":
    sum (x - c)^2; "cosine": 1 - x.c / (|x| |c|).  The smallest distance wins, a tie goes to the lowest
    k.  A row with a NaN (or an infinity, or without a direction under cosine) gets label -1 and dist NaN;
    a centroid like that is never chosen.  1 <= K <= 32, 2 <= N <= 1024."""
    x2, cent, code, lead = _kmeans_args("kmeans_assign", x, centroids, metric)
    labels, dist = _assign(x2, cent, code)
    return labels.view(lead), dist.view(lead)


def kmeans_update(x, labels, centroids, metric="cosine", ws_bytes=None):
    """Centroids from labels (wc_kmeans_update): x [R][N] or [M][B][N], labels int32 shaped as x without
    its last axis, centroids [K][N] the previous ones -> (centroids [K][N], count [K] int64).  Centroid
    k is the mean of the rows labelled k (cosine: of the rows divided by their norms); rows labelled -1
    belong to nobody; an empty cluster keeps its previous centroid, count 0.  Partial sums over blocks of
    KMEANS_UPDATE_BLOCK = 256 rows, added in index order: the bits depend on the shape and the data
    only, not on ws_bytes (default and minimum: wc_kmeans_workspace_size)."""
    x2, cent, code, lead = _kmeans_args("kmeans_update", x, centroids, metric)
    _args.tensor("kmeans_update", "labels must be an int32 device tensor shaped as x without its last axis", labels,
                 torch.int32, shapes=(lead,))
    return _update(x2, labels.reshape(-1).contiguous(), cent, code, ws_bytes)


def kmeans(x, k_or_init, metric="cosine", max_iter=100, n_init=1, seed=0):
    """Lloyd's k-means around wc_kmeans_assign and wc_kmeans_update: x [R][N] or [M][B][N] fp64 device
    tensor (the latter pooled over simulations and times: how empirical states are made) ->
    (centroids [K][N], labels int32 shaped as x without its last axis, inertia, n_iter).

    k_or_init: initial centroids [K][N], or an integer k: k distinct rows without NaN or infinity,
    picked by np.random.default_rng(seed); with n_init > 1 as many such draws from the one generator,
    the run of lowest inertia kept (the first among equals).  Each run: assign; stop if the labels repeat
    the previous assignment's or after max_iter updates; else update and assign again.  n_iter counts
    the updates, labels are those of the returned centroids, inertia the sum of their distances over the
    rows with a label.  No k-means++ seeding, no choice of k."""
    if isinstance(k_or_init, torch.Tensor):
        if int(n_init) != 1:
            raise ValueError("kmeans: explicit initial centroids go with n_init = 1")
        inits = [k_or_init]
        x2, _, code, lead = _kmeans_args("kmeans", x, k_or_init, metric)
    elif not isinstance(k_or_init, (int, np.integer)) or isinstance(k_or_init, bool):
        raise TypeError("kmeans: k_or_init must be an integer k or initial centroids, a [K][N] fp64 device tensor")
    else:
        k = int(k_or_init)
        if k < 1 or k > KMEANS_MAX_K:
            raise ValueError(f"kmeans: K = {k}: needs 1 <= K <= {KMEANS_MAX_K}")
        if int(n_init) < 1:
            raise ValueError(f"kmeans: n_init = {n_init} < 1")
        inits = None
    max_iter = int(max_iter)
    if max_iter < 0:
        raise ValueError(f"kmeans: max_iter = {max_iter} < 0")
    if inits is None:
        _kmeans_rows("kmeans", x)
        x2, _, code, lead = _kmeans_args("kmeans", x, x.reshape(-1, x.shape[-1])[:1], metric)
        pool = torch.nonzero(torch.isfinite(x2).all(dim=1)).reshape(-1).cpu().numpy()
        if pool.size < k:
            raise ValueError(f"kmeans: {pool.size} rows without NaN or infinity, fewer than k = {k}")
        rng = np.random.default_rng(seed)
        inits = [x2[torch.as_tensor(np.sort(rng.choice(pool, size=k, replace=False)), device=x2.device)]
                 for _ in range(int(n_init))]
    best = None
    for init in inits:
        cent, prev, n_iter = init.contiguous().clone(), None, 0
        while True:
            labels, dist = _assign(x2, cent, code)
            if (prev is not None and torch.equal(labels, prev)) or n_iter >= max_iter:
                break
            cent, _ = _update(x2, labels, cent, code)
            prev, n_iter = labels, n_iter + 1
        inertia = float(torch.nansum(dist))
        if best is None or inertia < best[2]:
            best = (cent, labels.view(lead), inertia, n_iter)
    return best


def state_stats(labels, k):
    """What a sweep is fitted on (wc_state_stats): labels [M][B] or [M] int32 device tensor, time-major,
    k states -> a dict of "occupancy" [B][k] (the share of the labelled times spent in each state),
    "dwell" [B][k] (the mean length in samples of the maximal runs of a state; a -1 ends a run) and
    "trans" [B][k][k] (the transition probabilities between consecutive labelled times, self-transitions
    included), without B for 1-D labels.  Counted in integers, divided once; NaN where there is nothing
    to divide by.  A label outside -1 .. k - 1 counts as -1."""
    labels, single, B, _ = _args.stack("state_stats", "labels must be a [M][B] or [M] int32 device tensor", labels,
                                       torch.int32, ndim=2, batch=1)
    k, M = int(k), labels.shape[0]
    if M < 1 or B < 1 or k < 1 or k > KMEANS_MAX_K:
        raise ValueError(f"state_stats: M = {M}, B = {B}, K = {k}: needs M >= 1, B >= 1 and 1 <= K <= {KMEANS_MAX_K}")
    f64 = dict(dtype=torch.float64, device=labels.device)
    occ, dwell, trans = torch.empty((B, k), **f64), torch.empty((B, k), **f64), torch.empty((B, k, k), **f64)
    _lib.check(_lib.lib().wc_state_stats(B, M, k, _lib.ptr(labels), _lib.ptr(occ), _lib.ptr(dwell), _lib.ptr(trans),
                                         _lib.stream_handle()), "wc_state_stats")
    return _args.unbatch(single, dict(occupancy=occ, dwell=dwell, trans=trans))


def leida_states(vec, centroids, metric="cosine"):
    """LEiDA's third stage: vec [M][B][N] or [M][N] (leida's eigenvectors), centroids [K][N] (kmeans of
    empirical or pooled eigenvectors) -> a dict of "labels" [M][B] int32 (kmeans_assign; -1 for a NaN
    eigenvector) and state_stats' "occupancy" [B][K], "dwell" [B][K], "trans" [B][K][K], without B for a
    2-D vec."""
    x2, cent, code, lead = _kmeans_args("leida_states", vec, centroids, metric)
    labels = _assign(x2, cent, code)[0].view(lead)
    return dict(labels=labels, **state_stats(labels, cent.shape[0]))


def state_kl(p, q):
    """The symmetrised Kullback-Leibler divergence 0.5 (KL(p||q) + KL(q||p)) between occupancy rows
    p [B][K] or [K] and an empirical one q [K] -> [B] (a scalar tensor for one row): the distance a
    sweep is fitted on after LEiDA (Deco et al. 2019).  0 log 0 = 0; an entry that is 0 on one side only
    gives +inf; a row with a NaN gives NaN.  Plain torch, like fcd_ks."""
    _args.tensor("state_kl", "p must be a [B][K] or [K] fp64 tensor", p, torch.float64, (1, 2))
    q = torch.as_tensor(np.asarray(q.cpu() if isinstance(q, torch.Tensor) else q, dtype=np.float64)).to(p.device)
    if q.dim() != 1 or q.shape[0] != p.shape[-1] or q.numel() == 0:
        raise ValueError(f"state_kl: q must be one row of K = {p.shape[-1]} entries")
    q = q.expand_as(p)

    def kl(a, b):
        t = torch.where(a > 0, a * (torch.log(a) - torch.log(b)), torch.zeros_like(a))
        return torch.where(torch.isnan(a) | torch.isnan(b), torch.full_like(a, float("nan")), t).sum(dim=-1)

    return 0.5 * (kl(p, q) + kl(q, p))


def welch_peak(E_t, fs=500.0, want_psd=False):
    """whole_sweep_both.py:90-95 for E [T][B][N] (time-major): peak frequency per
    simulation (and the node-mean PSD)."""
    T, B, N = E_t.shape
    nodemajor = E_t.reshape(T, B * N).t().contiguous()  # [C][T]
    wa = WelchAccumulator(B, N, E_t.device)
    nseg = (T - WELCH_NPERSEG) // WELCH_HOP + 1
    for s in range(nseg):
        wa.accumulate(nodemajor, T, T, 1, s * WELCH_HOP)
    return wa.peak(fs, want_psd)


WELCH_PSD_WS_CAP = 1 << 30     # wc_welch_psd: workspace ceiling (column tiles beyond it)


@functools.lru_cache(maxsize=16)
def _welch_window(window, nperseg, device):
    """scipy.signal.get_window(window, nperseg) (periodic, as signal.welch's) on the device, with the
    host sums the scalings need: (tensor [nperseg], sum w^2, (sum w)^2).  window: a name or a
    (name, parameter, ...) tuple."""
    from scipy import signal
    return _welch_window_upload(signal.get_window(window, nperseg), device)


def _welch_window_upload(win, device):
    win = np.ascontiguousarray(win, dtype=np.float64)
    return torch.as_tensor(win).to(device), float((win * win).sum()), float(win.sum() ** 2)


def _welch_args(name, T, device, fs, window, nperseg, noverlap, detrend, scaling, stacklevel=3):
    """SciPy's coercion of the arguments welch, csd and coherence share, for a series of T samples ->
    (detrend flag, window tensor [nperseg], nperseg, noverlap, scale, freqs); name prefixes the
    messages; stacklevel makes the clamped-nperseg warning point at the public function's caller."""
    from scipy import fft as sp_fft
    if detrend == "constant":
        det = 1
    elif detrend is False:
        det = 0
    else:
        raise NotImplementedError(f"{name}: detrend = {detrend!r} (only 'constant' and False run on the device)")
    if scaling not in ("density", "spectrum"):
        raise ValueError(f"Unknown scaling: {scaling!r}")
    if nperseg is not None:
        nperseg = int(nperseg)
        if nperseg < 1:
            raise ValueError("nperseg must be a positive integer")
    if isinstance(window, (str, tuple)):
        if nperseg is None:
            nperseg = 256
        if nperseg > T:
            warnings.warn(f"nperseg = {nperseg:d} is greater than input length  = {T:d}, using nperseg = {T:d}",
                          stacklevel=stacklevel)
            nperseg = T
        win, sw2, s2w = _welch_window(window, nperseg, str(device))
    else:
        w = np.asarray(window)
        if w.ndim != 1:
            raise ValueError("window must be 1-D")
        if T < w.shape[0]:
            raise ValueError("window is longer than input signal")
        if nperseg is None:
            nperseg = w.shape[0]
        elif nperseg != w.shape[0]:
            raise ValueError("value specified for nperseg is different from length of window")
        win, sw2, s2w = _welch_window_upload(w, device)
    noverlap = nperseg // 2 if noverlap is None else int(noverlap)
    if noverlap >= nperseg:
        raise ValueError("noverlap must be less than nperseg.")
    scale = 1.0 / (fs * sw2) if scaling == "density" else 1.0 / s2w
    return det, win, nperseg, noverlap, scale, sp_fft.rfftfreq(nperseg, 1 / fs)


def welch(x, fs=1.0, window="hann", nperseg=None, noverlap=None, detrend="constant", scaling="density",
          ws_bytes=None):
    """scipy.signal.welch(x, fs, window, nperseg, noverlap, detrend=detrend, scaling=scaling, axis=0)
    of a device tensor x [T][C] or [T][B][N] fp64 (wc_welch_psd: one-sided, mean over segments,
    2 <= nperseg <= 4096) -> (freqs, psd): freqs a numpy array [F], F = nperseg // 2 + 1, psd a
    device tensor [F][C] or [F][B][N].

    window: a SciPy window name or (name, parameter) tuple, or an array of nperseg weights.
    SciPy's defaults and coercions: nperseg None -> 256 (an array window: its length), noverlap
    None -> nperseg // 2, both through int(); a named window with nperseg > T is clamped to T with
    SciPy's UserWarning.  detrend: "constant" or False.  scaling: "density" or "spectrum".
    ws_bytes: workspace size (default: what all columns want, at most WELCH_PSD_WS_CAP, never
    below the minimum); the result does not depend on it."""
    _args.tensor("welch", "x must be a [T][C] or [T][B][N] fp64 device tensor", x, torch.float64, _FROM_2D)
    T = x.shape[0]
    det, win, nperseg, noverlap, scale, freqs = _welch_args("welch", T, x.device, fs, window, nperseg, noverlap,
                                                            detrend, scaling)

    L = _lib.lib()
    x2 = x.reshape(T, -1).contiguous()
    C = x2.shape[1]
    F = nperseg // 2 + 1
    need = L.wc_welch_psd_workspace_size(C, T, nperseg, noverlap)
    if ws_bytes is None and need:
        nseg = (T - nperseg) // (nperseg - noverlap) + 1
        sb = 2 * -(-nseg // 32)                   # segments per block; -(-nseg // sb) blocks of F doubles a column
        ws_bytes = _args.ws_default(need, need + (C - 1) * -(-nseg // sb) * F * 8, WELCH_PSD_WS_CAP)
    ws_bytes = ws_bytes or 16                     # need == 0: the call says why
    psd = torch.empty((F, C), dtype=torch.float64, device=x.device)
    ws = _args.workspace(ws_bytes, x.device)
    _lib.check(L.wc_welch_psd(C, T, _lib.ptr(x2), nperseg, noverlap, _lib.ptr(win), det, scale, _lib.ptr(psd),
                              _lib.ptr(ws), ws_bytes, _lib.stream_handle()), "wc_welch_psd")
    return freqs, psd.reshape((F,) + tuple(x.shape[1:]))


CSD_WS_CAP = 1 << 30           # wc_csd: workspace ceiling (segment chunks beyond it)
CSD_MATRIX, CSD_COHERENCE, CSD_PAIRS, CSD_PAIR_COHERENCE = 0, 1, 2, 3


def _csd(name, coh, x, y, fs, window, nperseg, noverlap, detrend, scaling, ws_bytes):
    _args.tensor(name, "x must be a [T][C] fp64 device tensor", x, torch.float64, (2,))
    if y is not None:
        _args.tensor(name, "y must be an fp64 tensor of x's shape on x's device", y, torch.float64,
                     shapes=(tuple(x.shape),), device=x.device)
    T = x.shape[0]
    det, win, nperseg, noverlap, scale, freqs = _welch_args(name, T, x.device, fs, window, nperseg, noverlap,
                                                            detrend, scaling, stacklevel=4)
    L = _lib.lib()
    x2 = (x if y is None else torch.cat((x, y), dim=1)).contiguous()  # pairs: column i with i + C
    C = x2.shape[1]
    F = nperseg // 2 + 1
    mode = (CSD_COHERENCE if coh else CSD_MATRIX) if y is None else (CSD_PAIR_COHERENCE if coh else CSD_PAIRS)
    need = L.wc_csd_workspace_size(C, T, nperseg, noverlap)
    if ws_bytes is None and need:
        nseg = (T - nperseg) // (nperseg - noverlap) + 1
        ws_bytes = _args.ws_default(need, need + (-(-nseg // 2) - 1) * 2 * F * C * 16, CSD_WS_CAP)  # all segment pairs
    ws_bytes = ws_bytes or 16                     # need == 0: the call says why
    shape = (F, x.shape[1], x.shape[1]) if y is None else (F, x.shape[1])
    out = torch.empty(shape, dtype=torch.float64 if coh else torch.complex128, device=x.device)
    ws = _args.workspace(ws_bytes, x.device)
    _lib.check(L.wc_csd(C, T, _lib.ptr(x2), nperseg, noverlap, _lib.ptr(win), det, scale, mode, _lib.ptr(out),
                        _lib.ptr(ws), ws_bytes, _lib.stream_handle()), "wc_csd")
    return freqs, out


def csd(x, y=None, fs=1.0, window="hann", nperseg=None, noverlap=None, detrend="constant", scaling="density",
        ws_bytes=None):
    """Cross-spectral density (wc_csd) of a device tensor x [T][C] fp64 with welch's arguments and
    coercions -> (freqs, P), P complex128 on the device.  y None: the matrix between x's columns,
    P [F][C][C] with P[f][i][j] = scipy.signal.csd(x[:, i], x[:, j])[1][f] (C <= 1024; exactly
    Hermitian, the diagonal welch's PSDs).  y of x's shape: columnwise, P [F][C] =
    scipy.signal.csd(x, y, axis=0).  ws_bytes: workspace size (default: what all segments want, at
    most CSD_WS_CAP, never below the minimum); the result does not depend on it."""
    return _csd("csd", False, x, y, fs, window, nperseg, noverlap, detrend, scaling, ws_bytes)


def coherence(x, y=None, fs=1.0, window="hann", nperseg=None, noverlap=None, detrend="constant", ws_bytes=None):
    """Magnitude-squared coherence |P_xy|^2 / (P_xx P_yy) (wc_csd), arguments and shapes as csd's,
    real fp64 on the device: [F][C][C] between x's columns (y None), [F][C] =
    scipy.signal.coherence(x, y, axis=0) otherwise.  A column without power gives NaN, as SciPy."""
    return _csd("coherence", True, x, y, fs, window, nperseg, noverlap, detrend, "density", ws_bytes)


SPEC_MODES = {"psd": 0, "complex": 1, "magnitude": 2, "angle": 3}  # WC_SPEC_*


def spectrogram(x, fs=1.0, window=("tukey", 0.25), nperseg=None, noverlap=None, detrend="constant",
                scaling="density", mode="psd"):
    """scipy.signal.spectrogram(x, fs, window, nperseg, noverlap, detrend=detrend, scaling=scaling,
    axis=0, mode=mode) of a device tensor x [T][C] or [T][B][N] fp64 (wc_spectrogram: one-sided,
    2 <= nperseg <= 4096) -> (freqs, times, Sxx): freqs [F], F = nperseg // 2 + 1, and times [S],
    the segments' centres, numpy arrays equal to SciPy's; Sxx a device tensor of SciPy's shape,
    [F][C][S] or [F][B][N][S], float64 (mode "complex": complex128).

    Sxx is a permuted view, without a copy, of the segment-major [S][F][C] buffer the kernel
    writes (SciPy's own result is a non-contiguous view too): call .contiguous() where a consumer
    needs the segments adjacent in memory.

    window, nperseg, detrend and scaling are welch's, with SciPy's spectrogram defaults: a Tukey
    (0.25) window, nperseg None -> 256 (an array window: its length), noverlap None -> nperseg // 8
    of the nperseg in use (after a named window's nperseg > T is clamped to T with SciPy's
    UserWarning).  mode: "psd", "complex" (the segments' spectra, SciPy's stft scaling),
    "magnitude" or "angle" (in [-pi, pi]; an exactly zero bin gives 0).  "phase" is an unwrapping of
    the angles that the device does not do (utils.spectrogram does it on the host):
    NotImplementedError."""
    if mode == "phase":
        raise NotImplementedError("spectrogram: mode = 'phase' (unwrapped angles) does not run on the device; "
                                  "utils.spectrogram unwraps the device's angles on the host")
    if mode not in SPEC_MODES:
        raise ValueError(f"unknown value for mode {mode}, must be one of {list(SPEC_MODES) + ['phase']}")
    _args.tensor("spectrogram", "x must be a [T][C] or [T][B][N] fp64 device tensor", x, torch.float64, _FROM_2D)
    T = x.shape[0]
    det, win, nperseg, nov, scale, freqs = _welch_args("spectrogram", T, x.device, fs, window, nperseg, noverlap,
                                                       detrend, scaling)
    if noverlap is None:
        nov = nperseg // 8                        # of the clamped nperseg, as SciPy
    step = nperseg - nov
    times = np.arange(nperseg / 2, T - nperseg / 2 + 1, step) / float(fs)

    L = _lib.lib()
    x2 = x.reshape(T, -1).contiguous()
    C = x2.shape[1]
    F = nperseg // 2 + 1
    S = (T - nperseg) // step + 1 if T >= nperseg else 0
    ws_bytes = L.wc_spectrogram_workspace_size(nperseg) or 16  # 0: the call says why
    out = torch.empty((S, F, C), dtype=torch.complex128 if mode == "complex" else torch.float64, device=x.device)
    ws = _args.workspace(ws_bytes, x.device)
    _lib.check(L.wc_spectrogram(C, T, _lib.ptr(x2), nperseg, nov, _lib.ptr(win), det, scale, SPEC_MODES[mode],
                                _lib.ptr(out), _lib.ptr(ws), ws_bytes, _lib.stream_handle()), "wc_spectrogram")
    return freqs, times, out.view((S, F) + tuple(x.shape[1:])).movedim(0, -1)


CONN_BITS = {"plv": 1, "pli": 2, "wpli": 4, "aec_orth": 8}  # WC_CONN_*, the order of wc_phase_conn's out
CONN_MEASURES = ("plv", "pli", "wpli", "aec", "aec_orth")


AEC_GROUP = 48      # _aec_corrcoef: columns per group, two groups a wc_corrcoef call (its N <= 96 kernels)


def _aec_corrcoef(amp):
    """corrcoef of the envelopes amp [M][B][N] -> [B][N][N], of which only the entries i < j are
    defined.  N <= 96: one corrcoef call.  Beyond, wc_corrcoef would change kernels (wc_fc_large.hip
    takes the mean as one sum over time, wc_corr.hip from time-block sums) and an entry would differ
    in its last bit from the same two columns' entry in a narrower call; so the columns go in groups
    of AEC_GROUP and every pair of groups a <= b through a call of its own, always the N <= 96
    kernels, where an entry depends on its two columns, M and B only."""
    M, B, N = amp.shape
    if N <= 2 * AEC_GROUP:
        return corrcoef(amp, B, N)
    fc = torch.empty((B, N, N), dtype=torch.float64, device=amp.device)
    groups = [(g, min(g + AEC_GROUP, N)) for g in range(0, N, AEC_GROUP)]
    for ka, (a0, a1) in enumerate(groups):
        if a1 - a0 > 1:
            fc[:, a0:a1, a0:a1] = corrcoef(amp[:, :, a0:a1].contiguous(), B, a1 - a0)
        for b0, b1 in groups[ka + 1:]:
            both = torch.cat((amp[:, :, a0:a1], amp[:, :, b0:b1]), dim=2)
            fc[:, a0:a1, b0:b1] = corrcoef(both, B, both.shape[2])[:, :a1 - a0, a1 - a0:]
    return fc


def phase_connectivity_from(phasor, amp=None, measures=CONN_MEASURES, ws_bytes=None):
    """Connectivity matrices from tensors the caller already holds: phasor [T][C][2] or
    [T][B][N][2] fp64 (hilbert_phase's unit phasors) and, for "wpli", "aec" and "aec_orth", the
    envelopes amp [T][C] or [T][B][N] fp64 (hilbert_envelope) -> a dict from measure name to a
    [C][C] or [B][N][N] device tensor; pairs are formed within a simulation b only.

    "plv", "pli", "wpli" and "aec_orth" come from wc_phase_conn (N <= 1024), "aec" from corrcoef of
    the envelopes (N > 96: of every pair of 48-column groups, _aec_corrcoef): its entries i < j,
    mirrored, with the defined diagonal, 1 (wc_corrcoef needs two columns: a single column gives
    that diagonal alone).  Every matrix is exactly symmetric;
    the diagonals are 1 (plv, aec) and 0.  A zero denominator gives NaN (wpli and aec_orth of two
    identical columns, a constant envelope).  ws_bytes: workspace size (default and least: the
    minimum); the result does not depend on it."""
    names = _args.names("phase_connectivity_from", measures, CONN_MEASURES)
    phasor, single, B, N = _args.stack("phase_connectivity_from", "phasor must be a [T][C][2] or [T][B][N][2] fp64 "
                                       "device tensor", phasor, ndim=4, batch=1, last=2)
    need_amp = any(m in ("wpli", "aec", "aec_orth") for m in names)
    if need_amp:
        _args.tensor("phase_connectivity_from", "wpli, aec and aec_orth need amp, an fp64 tensor of the phasors' "
                     "[T][C] or [T][B][N] on their device", amp, torch.float64, shapes=(tuple(phasor.shape[:-1]),),
                     device=phasor.device)
    M = phasor.shape[0]
    shape = (N, N) if single else (B, N, N)
    amp = amp.contiguous() if need_amp else None
    res = {}
    bits = sum(CONN_BITS[m] for m in names if m in CONN_BITS)
    if bits:
        L = _lib.lib()
        need = L.wc_phase_conn_workspace_size(B, N, M, bits)
        nbytes = max(need, ws_bytes or 0) or 16      # need == 0: the call says why
        ws = _args.workspace(nbytes, phasor.device)
        got = [m for m in CONN_BITS if CONN_BITS[m] & bits]  # ascending bit order
        out = torch.empty((len(got), B, N, N), dtype=torch.float64, device=phasor.device)
        _lib.check(L.wc_phase_conn(B, N, M, _lib.ptr(phasor), _lib.ptr(amp if bits & 12 else None), bits,
                                   _lib.ptr(out), _lib.ptr(ws), nbytes, _lib.stream_handle()), "wc_phase_conn")
        for k, m in enumerate(got):
            res[m] = out[k].view(shape)
    if "aec" in names:
        if N > 1:
            # wc_corrcoef keeps np.corrcoef's division order in either triangle (c / sd_i / sd_j against
            # c / sd_j / sd_i: a last-bit difference) and its computed diagonal: the entries i < j are kept
            # and mirrored, the diagonal is set
            fc = _aec_corrcoef(amp.view(M, B, N))
            upper = torch.ones((N, N), dtype=torch.bool, device=fc.device).triu(1)
            aec = torch.where(upper, fc, fc.transpose(1, 2))
            aec.diagonal(dim1=1, dim2=2).fill_(1.0)
        else:
            aec = torch.ones((B, 1, 1), dtype=torch.float64, device=phasor.device)
        res["aec"] = aec.view(shape)
    return {m: res[m] for m in names}


def phase_connectivity(x, measures=CONN_MEASURES):
    """Phase and envelope connectivity between the columns of a real, already band-limited device
    tensor x [T][C] or [T][B][N] fp64 -> a dict from measure name to a [C][C] or [B][N][N] tensor:
    "plv" phase-locking value, "pli" phase-lag index, "wpli" weighted phase-lag index, "aec"
    amplitude-envelope correlation, "aec_orth" its pairwise orthogonalised form (Hipp et al. 2012,
    no logarithm), all from z = scipy.signal.hilbert(x, axis=0): the phasors z / |z| through
    hilbert_phase, the envelopes |z| (only where a measure needs them) through hilbert_envelope,
    each with its own dispatch.  2 <= T <= 524288, N <= 1024; see phase_connectivity_from."""
    names = _args.names("phase_connectivity", measures, CONN_MEASURES)
    _args.tensor("phase_connectivity", "x must be a [T][C] or [T][B][N] fp64 device tensor", x, torch.float64, (2, 3))
    T = x.shape[0]
    x2 = x.reshape(T, -1).contiguous()
    ph = hilbert_phase(x2).view(tuple(x.shape) + (2,))
    amp = None
    if any(m in ("wpli", "aec", "aec_orth") for m in names):
        amp = hilbert_envelope(x2).view(x.shape)
    return phase_connectivity_from(ph, amp, names)


def sim_bold(E_t, bold_downsamp=1000, neq=NEQ, bold_dt=0.04):
    """simBOLD (wc:140-158) of E [T][C] (time-major, any C) -> [M][C] fp64."""
    T = E_t.shape[0]
    C = int(np.prod(E_t.shape[1:]))
    bs = BoldStream(C, T, neq, bold_downsamp, bold_dt, E_t.device)
    bs.feed(E_t.reshape(T, C).contiguous())
    return bs.finish()


def corrcoef(x, B, N):
    """np.corrcoef(x[:, b, :].T) for every b of a time-major [M][B][N] fp64 device series
    (wc_corrcoef: split over time blocks, for long series and small batches) -> [B][N][N]."""
    L = _lib.lib()
    x = x.contiguous()
    M = x.shape[0]
    fc = torch.empty((B, N, N), dtype=torch.float64, device=x.device)
    ws_bytes = (L.wc_corrcoef_workspace_size(B, N, M) // 8 + 1) * 8   # the minimum, rounded up past a multiple of 8
    _lib.check(L.wc_corrcoef(B, N, M, _lib.ptr(x), _lib.ptr(fc), _lib.ptr(_args.workspace(ws_bytes, x.device)),
                             ws_bytes, _lib.stream_handle()), "wc_corrcoef")
    return fc

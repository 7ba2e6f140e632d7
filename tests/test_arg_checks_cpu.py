"""One table of refused calls per entry point that checks its arguments through csrc/wc_args.h, driven
through the C ABI with fake pointers (no GPU: every row is refused before any device work).

The expected return codes were recorded from a build of the commit before the entry points moved onto
wc_args.h (this table run against that library through WCSDE_LIB_OVERRIDE): the shared helpers must
refuse exactly what the hand-written checks refused, with the same code.  Every row is a call that
library refuses; "these two may abut" is only ever shown by a later refusal (ws_bytes = 0 giving
WC_EWORKSPACE), so entries without a workspace have no such rows.  The seeded entries
(wc_graph_louvain_sign, wc_graph_rewire, wc_graph_null_model, wc_surrogate_fc, wc_surrogate_test) were
recorded the same way from the commit before wc_check_seeded and wc_plan_slots.

Per entry: each shape bound; each required pointer NULL; each pointer misaligned by half its alignment;
each (output, input) and (output, output) pair that the entry checks, overlapping by one element; and
for a workspace: one byte short, NULL, misaligned, and over each buffer the entry checks it against.
A workspace of slots has no size function and is refused with WC_EINVAL: it is listed as the last
output, of min(ws_bytes / slot, runs) slots, with "ws_bytes one byte under one slot" among the shapes.

FIRST: calls to the seeded entries and to wc_graph_louvain and wc_graph_agreement that are wrong in two
ways, with the code and the whole message of the refusal that comes first: the order of the checks and
the wording of the clauses that the shared helpers take from their callers.
"""
import ctypes
from collections import namedtuple

import pytest

EINVAL, EUNSUPPORTED, EWORKSPACE = -1, -2, -3
NEED = "need"                                     # ws_bytes: what the entry's size function returns
INF, NAN = float("inf"), float("nan")

Span = namedtuple("Span", "role bytes align elem required")   # align 0: the entry never looks at it
Entry = namedtuple("Entry", "fn params spans shapes pairs ws")


def P(k):
    """Fake device pointers 2^44 bytes apart: no base array reaches its neighbour."""
    return (k + 1) << 44


def entry(fn, params, spans, shapes, pairs=None, ws=None):
    """pairs None: every output against every input and every earlier output."""
    if pairs is None:
        ins = [n for n, s in spans.items() if s.role == "in"]
        outs = [n for n, s in spans.items() if s.role == "out"]
        pairs = [(o, i) for o in outs for i in ins] + [(o, e) for k, o in enumerate(outs) for e in outs[:k]]
    return Entry(fn, params, spans, shapes, pairs, ws)


def graph(fn, args, outs, extra_shapes=(), extra_spans=None, extra_pairs=()):
    """The wc_graph_* family: w [B][N][N], optional outputs (at least one), all 8-byte aligned."""
    B, N = 2, 90
    params = dict(B=B, N=N, **args)
    spans = dict(w=Span("in", B * N * N * 8, 8, 8, True), **(extra_spans or {}))
    spans.update({o: Span("out", B * per * elem, 8, elem, False) for o, (per, elem) in outs.items()})
    for k, name in enumerate(spans):
        params[name] = P(k)
    shapes = [(dict(B=0), EINVAL), (dict(N=1), EINVAL), (dict(N=97), EUNSUPPORTED),
              ({o: None for o in outs}, EINVAL), *extra_shapes]
    return entry(fn, params, spans, shapes, pairs=[(o, "w") for o in outs] + list(extra_pairs))


def welch_family(fn, size_fn, out, out_bytes, mode=None, extra_shapes=()):
    """wc_welch_psd, wc_csd, wc_spectrogram: x [T][C], window [n]; only (out, x) is checked for overlap."""
    C, T, n, nov = 6, 3000, 256, 128
    params = dict(C=C, T=T, x=P(0), nperseg=n, noverlap=nov, window=P(1), detrend=1, scale=1.0)
    if mode is not None:
        params["mode"] = mode
    params.update({out: P(2), "workspace": P(3), "ws_bytes": NEED})
    spans = dict(x=Span("in", T * C * 8, 8, 8, True), window=Span("in", n * 8, 8, 8, True),
                 **{out: Span("out", out_bytes(C, T, n, nov), 8, 8, True)}, workspace=Span("ws", 0, 16, 16, True))
    shapes = [(dict(C=0), EINVAL), (dict(nperseg=1, noverlap=0), EINVAL), (dict(noverlap=-1), EINVAL),
              (dict(noverlap=n), EINVAL), (dict(noverlap=n - 1, ws_bytes=0), EWORKSPACE),
              (dict(T=n - 1), EINVAL), (dict(T=n, ws_bytes=0), EWORKSPACE),
              (dict(detrend=2), EINVAL), (dict(detrend=-1), EINVAL),
              (dict(scale=0.0), EINVAL), (dict(scale=INF), EINVAL), (dict(scale=NAN), EINVAL),
              (dict(nperseg=2, noverlap=1, T=(1 << 31) + 1), EINVAL),                  # 2^31 - 1 hops: 2^31 segments
              (dict(T=10000, nperseg=4097), EUNSUPPORTED), (dict(T=10000, nperseg=4096, ws_bytes=0), EWORKSPACE),
              *extra_shapes]
    size = (size_fn, ("nperseg",)) if fn == "wc_spectrogram" else (size_fn, ("C", "T", "nperseg", "noverlap"))
    return entry(fn, params, spans, shapes, pairs=[(out, "x")], ws=("workspace", "ws_bytes", *size, ()))


def kmeans_shapes(with_ws):
    ws0 = dict(ws_bytes=0) if with_ws else None
    rows = [(dict(R=0), EINVAL), (dict(R=(1 << 40) + 1), EUNSUPPORTED), (dict(N=1), EINVAL),
            (dict(N=1025), EUNSUPPORTED), (dict(K=0), EINVAL), (dict(K=33), EUNSUPPORTED),
            (dict(metric=2), EINVAL), (dict(metric=-1), EINVAL)]
    if with_ws:
        rows += [(dict(N=1024, **ws0), EWORKSPACE), (dict(N=2, **ws0), EWORKSPACE), (dict(K=32, **ws0), EWORKSPACE),
                 (dict(K=1, **ws0), EWORKSPACE), (dict(metric=1, **ws0), EWORKSPACE)]
    return rows


def seeded_shapes(min_n):
    """The seeded family (B matrices, R seeds, a run each): B, R, N, and B R just past INT32_MAX."""
    return [(dict(B=0), EINVAL), (dict(R=0), EINVAL), (dict(N=min_n - 1), EINVAL), (dict(N=97), EUNSUPPORTED),
            (dict(B=1 << 16, R=1 << 15), EINVAL)]


# at N = 90: 4005 iterations a swap, 46 attempts each; 11657 swaps reach 2^31 attempts; N = 4: a slot of 48 bytes
NULL_MODEL_SWAPS = [(dict(bin_swaps=-1), EINVAL), (dict(bin_swaps=11657), EINVAL), (dict(ws_bytes=32039), EINVAL),
                    (dict(N=4, ws_bytes=47), EINVAL)]
SURROGATE_SHAPES = [(dict(B=0), EINVAL), (dict(N=1), EINVAL), (dict(N=97), EUNSUPPORTED), (dict(S=1), EINVAL),
                    (dict(B=1 << 16, S=1 << 15), EINVAL)]

ENTRIES = [
    entry("wc_graph_louvain",
          dict(B=2, R=3, N=90, obj=P(0), norm=P(1), ci0=P(2), seeds=P(3), ci=P(4), q=P(5), info=P(6)),
          dict(obj=Span("in", 2 * 90 * 90 * 8, 8, 8, True), norm=Span("in", 2 * 8, 8, 8, True),
               ci0=Span("in", 2 * 90 * 4, 4, 4, False), seeds=Span("in", 3 * 8, 8, 8, True),
               ci=Span("out", 2 * 3 * 90 * 4, 4, 4, True), q=Span("out", 2 * 3 * 8, 8, 8, True),
               info=Span("out", 2 * 3 * 2 * 4, 4, 4, False)),
          [(dict(B=0), EINVAL), (dict(R=0), EINVAL), (dict(N=1), EINVAL), (dict(N=97), EUNSUPPORTED),
           (dict(B=1 << 16, R=1 << 15), EINVAL)]),
    entry("wc_graph_agreement", dict(B=2, R=3, N=90, ci=P(0), D=P(1)),
          dict(ci=Span("in", 2 * 3 * 90 * 4, 4, 4, True), D=Span("out", 2 * 90 * 90 * 8, 8, 8, True)),
          [(dict(B=0), EINVAL), (dict(R=0), EINVAL), (dict(N=1), EINVAL), (dict(N=97), EUNSUPPORTED)]),
    entry("wc_graph_louvain_sign",                                   # 6 runs, a slot of 16 N^2 bytes each
          dict(B=2, R=3, N=90, w=P(0), gamma=1.0, qtype=0, seeds=P(1), ci=P(2), q=P(3), info=P(4), workspace=P(5),
               ws_bytes=6 * 129600),
          dict(w=Span("in", 2 * 90 * 90 * 8, 8, 8, True), seeds=Span("in", 3 * 8, 8, 8, True),
               ci=Span("out", 2 * 3 * 90 * 4, 4, 4, True), q=Span("out", 2 * 3 * 8, 8, 8, True),
               info=Span("out", 2 * 3 * 2 * 4, 4, 4, False), workspace=Span("out", 6 * 129600, 8, 8, True)),
          [*seeded_shapes(2), (dict(qtype=5), EINVAL), (dict(qtype=-1), EINVAL), (dict(gamma=INF), EINVAL),
           (dict(gamma=NAN), EINVAL), (dict(ws_bytes=129599), EINVAL), (dict(N=2, ws_bytes=63), EINVAL)]),
    entry("wc_graph_rewire",                                         # 6 runs, a slot of 4 N (N - 1) bytes each
          dict(B=2, R=3, N=90, w=P(0), bin_swaps=5, seeds=P(1), wr=P(2), info=P(3), workspace=P(4), ws_bytes=6 * 32040),
          dict(w=Span("in", 2 * 90 * 90 * 8, 8, 8, True), seeds=Span("in", 3 * 8, 8, 8, True),
               wr=Span("out", 6 * 90 * 90 * 8, 8, 8, True), info=Span("out", 6 * 3 * 4, 4, 4, False),
               workspace=Span("out", 6 * 32040, 8, 8, True)),
          [*seeded_shapes(4), *NULL_MODEL_SWAPS]),
    entry("wc_graph_null_model",
          dict(B=2, R=3, N=90, w=P(0), bin_swaps=5, period=10, neg_mode=1, seeds=P(1), w0=P(2), r=P(3), info=P(4),
               workspace=P(5), ws_bytes=6 * 32040),
          dict(w=Span("in", 2 * 90 * 90 * 8, 8, 8, True), seeds=Span("in", 3 * 8, 8, 8, True),
               w0=Span("out", 6 * 90 * 90 * 8, 8, 8, True), r=Span("out", 6 * 2 * 8, 8, 8, False),
               info=Span("out", 6 * 3 * 4, 4, 4, False), workspace=Span("out", 6 * 32040, 8, 8, True)),
          [*seeded_shapes(4), *NULL_MODEL_SWAPS, (dict(period=-1), EINVAL), (dict(period=65), EUNSUPPORTED),
           (dict(neg_mode=2), EINVAL), (dict(neg_mode=-1), EINVAL)]),
    entry("wc_surrogate_fc",                                         # 150 bins of 180 columns, P = 4005 pairs
          dict(B=2, N=90, L=298, S=3, spec=P(0), seeds=P(1), sfc=P(2)),
          dict(spec=Span("in", 150 * 180 * 16, 16, 16, True), seeds=Span("in", 3 * 8, 8, 8, True),
               sfc=Span("out", 2 * 3 * 4005 * 8, 8, 8, True)),
          [*SURROGATE_SHAPES, (dict(L=2), EINVAL), (dict(L=299), EINVAL), (dict(L=4098), EUNSUPPORTED)]),
    entry("wc_surrogate_test",
          dict(B=2, N=90, S=3, fc=P(0), sfc=P(1), alpha=0.05, p_adj=P(2), fc_adj=P(3), mu=P(4), sd=P(5), p=P(6)),
          dict(fc=Span("in", 2 * 90 * 90 * 8, 8, 8, True), sfc=Span("in", 2 * 3 * 4005 * 8, 8, 8, True),
               p_adj=Span("out", 2 * 90 * 90 * 8, 8, 8, True), fc_adj=Span("out", 2 * 90 * 90 * 8, 8, 8, True),
               mu=Span("out", 2 * 4005 * 8, 8, 8, False), sd=Span("out", 2 * 4005 * 8, 8, 8, False),
               p=Span("out", 2 * 4005 * 8, 8, 8, False)),
          [*SURROGATE_SHAPES, (dict(alpha=0.0), EINVAL), (dict(alpha=1.0), EINVAL), (dict(alpha=NAN), EINVAL)]),
    graph("wc_graph_paths", dict(w=0, lengths=0, include_infinite=1),
          dict(dist=(90 * 90, 8), hops=(90 * 90, 4), stats=(4, 8), ecc=(90, 8))),
    graph("wc_graph_local_efficiency", dict(), dict(eloc=(90, 8)),
          extra_shapes=[(dict(B=(1 << 31) // 96 + 1, N=96), EINVAL)]),
    graph("wc_graph_clustering", dict(),
          dict(clustering=(90, 8), transitivity=(1, 8), strengths=(90, 8), degrees=(90, 4))),
    graph("wc_graph_betweenness", dict(w=0, lengths=0), dict(bc=(90, 8))),
    graph("wc_graph_modules", dict(K=5, w=0, ci=0, degree=0, zflag=0, gamma=1.0), dict(part=(90, 8), z=(90, 8), q=(1, 8)),
          extra_shapes=[(dict(K=0), EINVAL), (dict(K=91), EINVAL), (dict(degree=2), EINVAL), (dict(degree=-1), EINVAL),
                        (dict(zflag=4), EINVAL), (dict(zflag=-1), EINVAL)],
          extra_spans=dict(ci=Span("in", 2 * 90 * 4, 4, 4, True)), extra_pairs=[(o, "ci") for o in ("part", "z", "q")]),
    entry("wc_leida_eigvec", dict(R=6, N=90, phasor=P(0), vec=P(1), share=P(2)),
          dict(phasor=Span("in", 6 * 90 * 16, 16, 16, True), vec=Span("out", 6 * 90 * 8, 8, 8, True),
               share=Span("out", 6 * 8, 8, 8, True)),
          [(dict(R=0), EINVAL), (dict(R=(1 << 40) + 1), EUNSUPPORTED), (dict(N=1), EINVAL), (dict(N=1025), EUNSUPPORTED)]),
    entry("wc_kmeans_assign", dict(R=6, N=90, K=4, x=P(0), cent=P(1), metric=0, labels=P(2), dist=P(3)),
          dict(x=Span("in", 6 * 90 * 8, 8, 8, True), cent=Span("in", 4 * 90 * 8, 8, 8, True),
               labels=Span("out", 6 * 4, 4, 4, True), dist=Span("out", 6 * 8, 8, 8, True)),
          kmeans_shapes(False)),
    entry("wc_kmeans_update",
          dict(R=6, N=90, K=4, x=P(0), labels=P(1), cent_prev=P(2), metric=0, cent=P(3), count=P(4), workspace=P(5),
               ws_bytes=NEED),
          dict(x=Span("in", 6 * 90 * 8, 8, 8, True), labels=Span("in", 6 * 4, 4, 4, True),
               cent_prev=Span("in", 4 * 90 * 8, 8, 8, True), cent=Span("out", 4 * 90 * 8, 8, 8, True),
               count=Span("out", 4 * 8, 8, 8, True), workspace=Span("ws", 0, 8, 8, True)),
          kmeans_shapes(True),
          ws=("workspace", "ws_bytes", "wc_kmeans_workspace_size", ("R", "N", "K", "metric"),
              ("x", "labels", "cent_prev", "cent", "count"))),
    entry("wc_state_stats", dict(B=2, M=50, K=4, labels=P(0), occupancy=P(1), dwell=P(2), trans=P(3)),
          dict(labels=Span("in", 50 * 2 * 4, 4, 4, True), occupancy=Span("out", 2 * 4 * 8, 8, 8, True),
               dwell=Span("out", 2 * 4 * 8, 8, 8, True), trans=Span("out", 2 * 4 * 4 * 8, 8, 8, True)),
          [(dict(B=0), EINVAL), (dict(M=0), EINVAL), (dict(K=0), EINVAL), (dict(K=33), EUNSUPPORTED)]),
    entry("wc_fcd",                                                  # 27 windows of 30 samples, P = 4005 pairs
          dict(B=2, N=90, M=298, x=P(0), win=30, step=10, fcd=P(1), winfc=P(2), workspace=P(3), ws_bytes=NEED),
          dict(x=Span("in", 298 * 2 * 90 * 8, 8, 8, True), fcd=Span("out", 2 * 27 * 27 * 8, 8, 8, True),
               winfc=Span("out", 2 * 27 * 4005 * 8, 8, 8, False), workspace=Span("ws", 0, 8, 8, True)),
          [(dict(B=0), EINVAL), (dict(N=2), EINVAL), (dict(N=3, ws_bytes=0), EWORKSPACE), (dict(N=97), EUNSUPPORTED),
           (dict(N=96, ws_bytes=0), EWORKSPACE), (dict(win=1), EINVAL), (dict(win=2, ws_bytes=0), EWORKSPACE),
           (dict(win=299), EINVAL), (dict(win=298, ws_bytes=0), EWORKSPACE), (dict(step=0), EINVAL),
           (dict(step=1, ws_bytes=0), EWORKSPACE), (dict(M=4098, win=2, step=1), EUNSUPPORTED),
           (dict(M=4097, win=2, step=1, ws_bytes=0), EWORKSPACE)],
          ws=("workspace", "ws_bytes", "wc_fcd_workspace_size", ("B", "N", "M", "win", "step"), ("x", "fcd", "winfc"))),
    entry("wc_fcd_phase", dict(B=2, N=90, M=298, phasor=P(0), fcd=P(1)),
          dict(phasor=Span("in", 298 * 2 * 90 * 16, 8, 16, True), fcd=Span("out", 2 * 298 * 298 * 8, 8, 8, True)),
          [(dict(B=0), EINVAL), (dict(N=1), EINVAL), (dict(N=97), EUNSUPPORTED), (dict(M=0), EINVAL),
           (dict(M=4097), EUNSUPPORTED)]),
    entry("wc_phase_conn",
          dict(B=2, N=90, M=298, phasor=P(0), amp=P(1), measures=15, out=P(2), workspace=P(3), ws_bytes=NEED),
          dict(phasor=Span("in", 298 * 2 * 90 * 16, 8, 16, True), amp=Span("in", 298 * 2 * 90 * 8, 8, 8, True),
               out=Span("out", 4 * 2 * 90 * 90 * 8, 8, 8, True), workspace=Span("ws", 0, 16, 16, True)),
          [(dict(B=0), EINVAL), (dict(N=0), EINVAL), (dict(M=1), EINVAL), (dict(M=2, ws_bytes=0), EWORKSPACE),
           (dict(measures=0), EINVAL), (dict(measures=16), EINVAL), (dict(N=1025), EUNSUPPORTED),
           (dict(N=1024, ws_bytes=0), EWORKSPACE), (dict(M=524289), EUNSUPPORTED),
           (dict(M=524288, ws_bytes=0), EWORKSPACE), (dict(B=1 << 22, N=1024, M=2), EINVAL),
           (dict(amp=None, measures=3, ws_bytes=0), EWORKSPACE)],           # PLV and PLI take no envelopes
          ws=("workspace", "ws_bytes", "wc_phase_conn_workspace_size", ("B", "N", "M", "measures"), ())),
    welch_family("wc_welch_psd", "wc_welch_psd_workspace_size", "psd", lambda C, T, n, nov: (n // 2 + 1) * C * 8),
    welch_family("wc_csd", "wc_csd_workspace_size", "out", lambda C, T, n, nov: (n // 2 + 1) * C * C * 16, mode=0,
                 extra_shapes=[(dict(C=(1 << 24) + 1), EINVAL), (dict(mode=-1), EINVAL), (dict(mode=4), EINVAL),
                               (dict(C=7, mode=2), EINVAL), (dict(C=1025), EUNSUPPORTED),
                               (dict(C=1024, ws_bytes=0), EWORKSPACE)]),
    welch_family("wc_spectrogram", "wc_spectrogram_workspace_size", "out",
                 lambda C, T, n, nov: ((T - n) // (n - nov) + 1) * (n // 2 + 1) * C * 8, mode=0,
                 extra_shapes=[(dict(C=(1 << 24) + 1), EINVAL), (dict(mode=-1), EINVAL), (dict(mode=4), EINVAL),
                               (dict(C=1 << 24, T=1 << 36, nperseg=4096, noverlap=0), EINVAL)]),   # x of 2^63 bytes
    entry("wc_hma", dict(B=2, N=90, fc=P(0), hin=P(1), hse=P(2), hin_node=P(3), hse_node=P(4), clus_num=P(5), sv=P(6)),
          dict({n: Span("out", 0, 0, 8, True) for n in ("fc", "hin", "hse", "hin_node", "hse_node")}),
          [(dict(B=0), EINVAL), (dict(N=2), EINVAL), (dict(N=97), EUNSUPPORTED)], pairs=[]),
    entry("wc_hma_modes",
          dict(B=2, N=90, lam=P(0), vt=P(1), hin=P(2), hse=P(3), hin_node=P(4), hse_node=P(5), clus_num=P(6), sv=P(7)),
          dict({n: Span("out", 0, 0, 8, True) for n in ("lam", "vt", "hin", "hse", "hin_node", "hse_node")}),
          [(dict(B=0), EINVAL), (dict(N=2), EINVAL), (dict(N=20000), EUNSUPPORTED)], pairs=[]),
    entry("wc_hilbert_phase_long", dict(C=7, M=298, x=P(0), phasor=P(1), workspace=P(2), ws_bytes=NEED),
          dict(x=Span("in", 0, 0, 8, True), phasor=Span("out", 0, 16, 16, True), workspace=Span("ws", 0, 16, 16, True)),
          [(dict(C=0), EINVAL), (dict(M=1), EINVAL), (dict(M=2, ws_bytes=0), EWORKSPACE), (dict(M=524289), EUNSUPPORTED),
           (dict(M=524288, ws_bytes=0), EWORKSPACE)],
          pairs=[], ws=("workspace", "ws_bytes", "wc_hilbert_long_workspace_size", ("C", "M"), ())),
    entry("wc_hilbert_envelope",                                     # method 2: the long transform's checks
          dict(C=7, M=298, x=P(0), env=P(1), method=2, workspace=P(2), ws_bytes=NEED),
          dict(x=Span("in", 0, 8, 8, True), env=Span("out", 0, 8, 8, True), workspace=Span("ws", 0, 16, 16, True)),
          [(dict(M=524289), EUNSUPPORTED), (dict(M=524288, ws_bytes=0), EWORKSPACE)],
          pairs=[], ws=("workspace", "ws_bytes", "wc_hilbert_envelope_workspace_size", ("C", "M", "method"), ())),
]


def need(L, e, kw):
    _, _, size_fn, size_args, _ = e.ws
    return getattr(L, size_fn)(*(kw[a] for a in size_args))


def call(L, e, over):
    kw = dict(e.params, **over)
    if kw.get("ws_bytes") == NEED:
        kw["ws_bytes"] = need(L, e, kw)
    args = [ctypes.c_void_p(v) if (k in e.spans or k in ("clus_num", "sv")) and v is not None else v
            for k, v in kw.items()]
    return getattr(L, e.fn)(*args, None)


def one_element_over(e, o, i):
    """Where o overlaps i by one of o's elements: o's tail over i's head or o's head over i's tail,
    whichever leaves o aligned."""
    so, si = e.spans[o], e.spans[i]
    tail, head = e.params[i] - so.bytes + so.elem, e.params[i] + si.bytes - so.elem
    return tail if tail % so.align == 0 else head


def rows(L, e):
    """(what, overrides, code, the argument the message must name or None)"""
    out = [(f"shape {o}", o, code, None) for o, code in e.shapes]
    for name, s in e.spans.items():
        if s.required and s.role != "ws":
            out.append((f"{name} NULL", {name: None}, EINVAL, None))
        if s.align:
            out.append((f"{name} misaligned", {name: e.params[name] + s.align // 2}, EINVAL, name))
    out += [(f"{o} over {i}", {o: one_element_over(e, o, i)}, EINVAL, o) for o, i in e.pairs]
    if e.ws:
        ws, nbytes, _, _, against = e.ws
        full = need(L, e, e.params)
        assert full > 0
        out += [("workspace one byte short", {nbytes: full - 1}, EWORKSPACE, None),
                ("workspace NULL", {ws: None}, EWORKSPACE, None),
                ("workspace NULL, no bytes", {ws: None, nbytes: 0}, EWORKSPACE, None)]
        out += [(f"workspace over {b}", {ws: e.params[b] + e.spans[b].bytes - 8}, EINVAL, "workspace") for b in against]
    return out


@pytest.mark.parametrize("e", ENTRIES, ids=lambda e: e.fn)
def test_refused_calls_keep_their_codes(e):
    from nremmodfc_amd import _lib
    L = _lib.lib()
    table = rows(L, e)
    # a row that passed every check would launch on fake pointers where there is a GPU: none may
    assert all(code in (EINVAL, EUNSUPPORTED, EWORKSPACE) for _, _, code, _ in table)
    for what, over, code, names in table:
        assert call(L, e, over) == code, (e.fn, what)
        msg = L.wc_last_error()
        assert msg.startswith(e.fn.encode() + b": "), (e.fn, what, msg)
        if names:
            assert names.encode() in msg, (e.fn, what, msg)


BIG = dict(B=1 << 16, R=1 << 15)
N97 = "N = 97 > 96 (one matrix per workgroup, in LDS)"
# (entry point, overrides that are wrong in two ways or more, code, the message of the check that fires first)
FIRST = [
    ("wc_graph_louvain", dict(B=0, R=0), EINVAL, "B < 1"),
    ("wc_graph_louvain", dict(R=0, N=97), EINVAL, "R < 1"),
    ("wc_graph_louvain", dict(N=1, **BIG), EINVAL, "N < 2"),
    ("wc_graph_louvain", dict(N=97, **BIG), EUNSUPPORTED, N97),
    ("wc_graph_louvain", dict(obj=None, **BIG), EINVAL, "2^31 workgroups or more (B times R)"),
    ("wc_graph_louvain", dict(obj=None, seeds=P(3) + 4), EINVAL, "obj, norm, seeds, ci or q is NULL"),
    ("wc_graph_agreement", dict(B=0, R=0), EINVAL, "B < 1"),
    ("wc_graph_agreement", dict(R=0, N=97), EINVAL, "R < 1"),
    ("wc_graph_agreement", dict(N=1, ci=None), EINVAL, "N < 2"),
    ("wc_graph_agreement", dict(N=97, ci=None), EUNSUPPORTED, N97),
    ("wc_graph_agreement", dict(ci=None, **BIG), EINVAL, "ci or D is NULL"),          # no bound on B R: a grid of B
    ("wc_graph_louvain_sign", dict(B=0, R=0), EINVAL, "B < 1"),
    ("wc_graph_louvain_sign", dict(R=0, N=97), EINVAL, "R < 1"),
    ("wc_graph_louvain_sign", dict(N=1, **BIG), EINVAL, "N < 2"),
    ("wc_graph_louvain_sign", dict(N=97, **BIG), EUNSUPPORTED,
     "N = 97 > 96 (the node-to-module degrees of one matrix per workgroup, in LDS)"),
    ("wc_graph_louvain_sign", dict(qtype=5, **BIG), EINVAL, "2^31 problems or more (B times R)"),
    ("wc_graph_louvain_sign", dict(qtype=5, gamma=NAN), EINVAL, "qtype = 5, must be 0 .. 4 (sta, pos, smp, gja, neg)"),
    ("wc_graph_louvain_sign", dict(gamma=INF, w=None), EINVAL, "gamma is not finite"),
    ("wc_graph_louvain_sign", dict(workspace=None, ws_bytes=0), EINVAL, "w, seeds, ci, q or workspace is NULL"),
    ("wc_graph_louvain_sign", dict(ws_bytes=129599, seeds=P(1) + 4), EINVAL,
     "ws_bytes = 129599 is less than one slot of 16 N^2 = 129600 bytes"),
    ("wc_graph_louvain_sign", dict(seeds=P(1) + 4, workspace=P(4)), EINVAL, "seeds must be 8-byte aligned"),
    ("wc_graph_louvain_sign", dict(ws_bytes=129600, workspace=P(4) - 129600 + 8), EINVAL, "workspace must not alias info"),
    ("wc_graph_rewire", dict(B=0, R=0), EINVAL, "B < 1"),
    ("wc_graph_rewire", dict(R=0, N=3), EINVAL, "R < 1"),
    ("wc_graph_rewire", dict(N=3, **BIG), EINVAL, "N = 3 < 4 (a rewiring takes four distinct nodes)"),
    ("wc_graph_rewire", dict(N=97, **BIG), EUNSUPPORTED, N97),
    ("wc_graph_rewire", dict(bin_swaps=-1, **BIG), EINVAL, "2^31 problems or more (B times R)"),
    ("wc_graph_rewire", dict(bin_swaps=-1, w=None), EINVAL, "bin_swaps = -1 < 0"),
    ("wc_graph_rewire", dict(bin_swaps=11657, w=None), EINVAL,
     "bin_swaps = 11657: 46686285 iterations of 46 attempts reach 2^31"),
    ("wc_graph_rewire", dict(wr=None, ws_bytes=0), EINVAL, "w, seeds, wr or workspace is NULL"),
    ("wc_graph_rewire", dict(ws_bytes=32039, w=P(0) + 4), EINVAL,
     "ws_bytes = 32039 is less than one slot of 4 N (N - 1) = 32040 bytes"),
    ("wc_graph_rewire", dict(ws_bytes=32040, workspace=P(2) - 32040 + 8), EINVAL, "workspace must not alias wr"),
    ("wc_graph_null_model", dict(N=3, **BIG), EINVAL, "N = 3 < 4 (a rewiring takes four distinct nodes)"),
    ("wc_graph_null_model", dict(N=97, **BIG), EUNSUPPORTED, N97),
    ("wc_graph_null_model", dict(bin_swaps=-1, period=65), EINVAL, "bin_swaps = -1 < 0"),
    ("wc_graph_null_model", dict(period=-1, neg_mode=2), EINVAL, "period = -1 < 0"),
    ("wc_graph_null_model", dict(period=65, neg_mode=2), EUNSUPPORTED, "period = 65 > 64 (the picks of one period, in LDS)"),
    ("wc_graph_null_model", dict(neg_mode=2, w0=None), EINVAL, "neg_mode = 2, must be 0 (the reference's) or 1 (BCT)"),
    ("wc_graph_null_model", dict(w0=None, ws_bytes=0), EINVAL, "w, seeds, w0 or workspace is NULL"),
    ("wc_graph_null_model", dict(ws_bytes=32039, r=P(3) + 4), EINVAL,
     "ws_bytes = 32039 is less than one slot of 4 N (N - 1) = 32040 bytes"),
    ("wc_surrogate_fc", dict(B=0, N=1), EINVAL, "B < 1"),
    ("wc_surrogate_fc", dict(N=1, S=1), EINVAL, "N < 2"),
    ("wc_surrogate_fc", dict(N=97, S=1), EUNSUPPORTED,
     "N = 97 > 96 (the products of one matrix per workgroup, in registers)"),
    ("wc_surrogate_fc", dict(S=1, L=2), EINVAL, "S = 1, needs at least 2 surrogates"),
    ("wc_surrogate_fc", dict(B=1 << 16, S=1 << 15, L=2), EINVAL, "2^31 surrogates or more (B times S)"),
    ("wc_surrogate_fc", dict(L=2, spec=None), EINVAL, "L = 2 < 4"),
    ("wc_surrogate_fc", dict(L=299, spec=None), EINVAL,
     "L = 299 is odd (the reference's stacked phases need an even length)"),
    ("wc_surrogate_fc", dict(L=4098, spec=None), EUNSUPPORTED, "L = 4098 > 4096 (wc_spectrogram's longest segment)"),
    ("wc_surrogate_fc", dict(sfc=None, seeds=P(1) + 4), EINVAL, "spec, seeds or sfc is NULL"),
    ("wc_surrogate_test", dict(S=1, alpha=0.0), EINVAL, "S = 1, needs at least 2 surrogates"),
    ("wc_surrogate_test", dict(B=1 << 16, S=1 << 15, alpha=0.0), EINVAL, "2^31 surrogates or more (B times S)"),
    ("wc_surrogate_test", dict(alpha=1.0, fc=None), EINVAL, "alpha = 1, must lie in (0, 1)"),
    ("wc_surrogate_test", dict(fc=None, mu=P(4) + 4), EINVAL, "fc, sfc, p_adj or fc_adj is NULL"),
]


@pytest.mark.parametrize("fn, over, code, message", FIRST, ids=[f"{r[0]}-{k}" for k, r in enumerate(FIRST)])
def test_first_refusal_and_its_message(fn, over, code, message):
    from nremmodfc_amd import _lib
    L = _lib.lib()
    e = next(e for e in ENTRIES if e.fn == fn)
    assert call(L, e, over) == code
    assert L.wc_last_error().decode() == f"{fn}: {message}"

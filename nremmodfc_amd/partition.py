"""Partition search on signed matrices and consensus partitions on the device (wc_louvain_sign.hip):
the reference's modularity_louvain_und_sign and consensus_und for a batch.  With sigchain.fc_metrics,
graph_consensus_matrix and graph_module_measures a stack of raw functional-connectivity matrices goes
from matrix to one consensus partition per simulation to participation and z-score on the device.

Device tensors in and out; partition_np holds the numpy facades that graph_utils re-exports.
"""
import math

import torch

from . import _args, _lib, sigchain

LOUVAIN_SIGN_QTYPES = ("sta", "pos", "smp", "gja", "neg")   # wc_graph_louvain_sign's qtype codes 0 .. 4
LOUVAIN_SIGN_SLOTS = 2048   # default workspace: a slot for each problem, at most this many (295 MB at N = 96)


def louvain_sign_slot_bytes(N):
    """One workgroup's slot of wc_graph_louvain_sign's workspace: the pooled W0 and W1, 2 N^2 fp64."""
    return 16 * N * N


def graph_louvain_sign(w, seeds=0, gamma=1.0, qtype="sta", want_info=False, ws_bytes=None):
    """Louvain community search on matrices with weights of both signs, on the device
    (wc_graph_louvain_sign; the reference's modularity_louvain_und_sign, Rubinov & Sporns 2011):
    w [B][N][N] or [N][N] fp64 device tensor, 2 <= N <= 96 -> (ci int32, q fp64), ci [B][R][N] with labels
    0 .. K-1 (the reference's minus 1) and q [B][R] the signed modularity of the last level.  seeds is
    an int or a sequence of R ints; an int gives no R axis, as an [N][N] input gives no batch axis
    (sigchain.graph_louvain's rules).  Every (matrix, seed) pair is an independent run in one launch.

    qtype weighs the positive and the negative part, dQ = d0 dQ0 - d1 dQ1: "sta" (1/s0, 1/(s0+s1)),
    "pos" (1/s0, 0), "smp" (1/s0, 1/s1), "gja" (1/(s0+s1), 1/(s0+s1)), "neg" (0, 1/s1), s0 and s1 the
    sums of the positive and of the negative weights.  On a non-negative matrix the four positive types
    agree; "neg" moves nothing there.  An all-zero matrix gives N singletons and q = 0.

    The algorithm is the reference's, decision for decision; the visiting order is the engine's, as in
    sigchain.graph_louvain.  A matrix with a NaN or inf has ci = -1 and q = NaN; so has a run whose
    level does not settle within 1000 sweeps or that would need a 301st level, where the reference
    raises.  want_info=True adds info int32 [B][R][2]: levels and node sweeps in all.

    ws_bytes: the pooled matrices of a run lie in global memory, in one slot of 16 N^2 bytes per
    workgroup; the launch has min(B R, ws_bytes / slot) workgroups, which stride over the runs.  None
    takes a slot per run, at most 2048.  The result does not depend on it, bit for bit."""
    name = "graph_louvain_sign"
    if not isinstance(qtype, str) or qtype not in LOUVAIN_SIGN_QTYPES:
        raise ValueError(f"{name}: modularity type unknown: qtype {qtype!r}, must be one of {list(LOUVAIN_SIGN_QTYPES)}")
    _args.real(name, f"gamma = {gamma!r}, must be a finite number", gamma, math.isfinite)
    seed_arr, scalar = _args.seeds(name, seeds)
    w, single, B, N = sigchain._graph_stack(name, w)
    R, slot = len(seed_arr), louvain_sign_slot_bytes(N)
    ws_bytes = _args.slot_ws_bytes(name, f"ws_bytes = {ws_bytes!r}, needs at least one slot of 16 N^2 = {slot} bytes",
                                   ws_bytes, slot, B * R * slot, LOUVAIN_SIGN_SLOTS * slot)
    dev = w.device
    ws, seeds_dev = _args.workspace(ws_bytes, dev), _args.upload_seeds(seed_arr, dev)
    out = torch.empty((B, R, N), dtype=torch.int32, device=dev)
    q = torch.empty((B, R), dtype=torch.float64, device=dev)
    info = torch.empty((B, R, 2), dtype=torch.int32, device=dev) if want_info else None
    _lib.check(_lib.lib().wc_graph_louvain_sign(B, R, N, _lib.ptr(w), float(gamma), LOUVAIN_SIGN_QTYPES.index(qtype),
                                                _lib.ptr(seeds_dev), _lib.ptr(out), _lib.ptr(q), _lib.ptr(info),
                                                _lib.ptr(ws), ws_bytes, _lib.stream_handle()),
               "wc_graph_louvain_sign")
    return _args.unrun(scalar, single, (out, q) + ((info,) if want_info else ()))


def _first_occurrence(ci):
    """ci [b][N] labels -> the same partitions labelled 0, 1, ... in the order of first occurrence."""
    n = ci.shape[1]
    same = ci[:, :, None] == ci[:, None, :]
    first = same.to(torch.int8).argmax(dim=2)                      # where node i's label first occurs
    is_first = first == torch.arange(n, device=ci.device)[None, :]
    rank = is_first.cumsum(dim=1) - 1                               # the label a first occurrence opens
    return rank.gather(1, first).to(torch.int32)


def graph_consensus(D, tau, reps=1000, seeds=None, max_iter=100):
    """Consensus partitions on the device (the reference's consensus_und, after Lancichinetti &
    Fortunato 2012): D [B][N][N] or [N][N] fp64 device tensor of agreement probabilities
    (sigchain.graph_consensus_matrix gives one) -> (ci int32 [B][N] or [N], iterations int32 [B] or a
    scalar tensor).  Per iteration dt = D (D >= tau) with a zero diagonal is clustered reps times by
    graph_louvain_sign ("sta", gamma 1) in one launch over the matrices still open, and one
    graph_agreement counts the results; a matrix whose reps partitions coincide (every entry of its
    agreement is 0 or reps) has converged, keeps that partition and leaves the batch, the others go
    on with D = agreement / reps.  One flag readback per iteration.

    The seed of rep r in iteration k is seeds[r] + k reps mod 2^64, seeds 0 .. reps-1 by default.
    ci is labelled 0, 1, ... by first occurrence (the reference's unique_partitions order, minus 1).
    ci is -1 for a matrix where a run was refused (a non-finite entry, graph_louvain_sign's guards) or
    that has not converged after max_iter iterations; iterations holds the count made.  The reference
    has neither a cap nor a refusal: it loops until convergence and raises from the search.  Its
    branch for a dt without zeros cannot be taken, the diagonal being zero, and is left out."""
    name = "graph_consensus"
    reps = _args.integer(name, f"reps = {reps!r}, must be a positive int", reps, 1)
    max_iter = _args.integer(name, f"max_iter = {max_iter!r}, must be a positive int", max_iter, 1)
    _args.real(name, f"tau = {tau!r}, must be a finite number", tau, math.isfinite)
    base = _args.seed_list(name, f"seeds must be a sequence of length reps = {reps}, or None", seeds, reps)
    D, single, B, N = sigchain._graph_stack(name, D)
    dev = D.device
    ci = torch.full((B, N), -1, dtype=torch.int32, device=dev)
    iters = torch.full((B,), max_iter, dtype=torch.int32, device=dev)
    open_idx = torch.arange(B, device=dev)
    cur = D.reshape(B, N, N)
    eye = torch.eye(N, dtype=torch.bool, device=dev)
    for k in range(max_iter):
        dt = (cur * (cur >= float(tau))).masked_fill(eye, 0.0)        # a NaN stays one, as in the reference
        run_seeds = [(int(s) + k * reps) % (1 << 64) for s in base]
        part, _ = graph_louvain_sign(dt, seeds=run_seeds)
        agr = sigchain.graph_agreement(part)
        refused = agr[:, 0, 0].isnan()
        done = ((agr == 0) | (agr == reps)).flatten(1).all(dim=1)
        flags = torch.stack([done, refused]).cpu()
        done_h, left_h = flags[0], ~(flags[0] | flags[1])
        closed = ~left_h.to(dev)
        iters[open_idx[closed]] = k + 1
        if bool(done_h.any()):
            sel = done_h.to(dev)
            ci[open_idx[sel]] = _first_occurrence(part[sel, 0])
        if not bool(left_h.any()):
            break
        keep = left_h.to(dev)
        open_idx, cur = open_idx[keep], agr[keep] / reps
    return _args.unbatch(single, (ci, iters))

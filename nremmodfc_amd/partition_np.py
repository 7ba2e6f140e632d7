"""numpy facades of partition.graph_louvain_sign and partition.graph_consensus with the reference's
signatures (graph_utils.py:697-855, :1124-1207); graph_utils imports them by name, so
graph_utils.modularity_louvain_und_sign and graph_utils.consensus_und are drop-ins.  torch and the
device modules are imported on first use."""
import os

import numpy as np

CONSENSUS_MAX_ITER = 100   # consensus_und: the reference has no cap


def _device(fn, a, **kw):
    import torch

    from . import partition
    out = getattr(partition, fn)(torch.from_numpy(a).cuda(), **kw)
    return tuple(t.cpu().numpy() for t in out)


def _matrices(name, W):
    from .graph_utils import _matrices
    return _matrices(name, W, False)


def modularity_louvain_und_sign(W, gamma=1, qtype='sta', seed=None):
    """(ci, Q): Louvain community structure of a matrix with positive and negative weights and the
    signed modularity reached (graph_utils.py:697-855); labels from 1.  qtype 'sta', 'pos', 'smp',
    'gja' or 'neg' (Rubinov & Sporns 2011); an unknown one raises ValueError where the reference raises
    KeyError.  seed None draws one from os.urandom.  W is an N x N matrix or a [B, N, N] stack (ci
    [B, N], Q [B]; one launch).  The visiting order is the engine's: see community_louvain."""
    a = _matrices("modularity_louvain_und_sign", W)
    if seed is None:
        seed = int.from_bytes(os.urandom(8), "little")
    part, q = _device("graph_louvain_sign", a, seeds=int(seed), gamma=float(gamma), qtype=qtype)
    part = part.astype(np.int64) + 1
    return (part, float(q)) if a.ndim == 2 else (part, q)


def consensus_und(D, tau, reps=1000):
    """The consensus partition of the agreement matrix D (graph_utils.py:1124-1207): D thresholded at
    tau is clustered reps times with modularity_louvain_und_sign until all reps partitions coincide;
    labels from 1, in the order of first occurrence.  As in the reference every call draws fresh seeds
    (one base from os.urandom; partition.graph_consensus takes seeds).  D is an N x N matrix or a
    [B, N, N] stack (ci [B, N]).  The reference loops without end where the partitions never coincide;
    this raises RuntimeError after 100 iterations, and ValueError for a non-finite D."""
    a = _matrices("consensus_und", D)
    base = int.from_bytes(os.urandom(8), "little")
    seeds = [(base + r) % (1 << 64) for r in range(int(reps))]
    ci, iters = _device("graph_consensus", a, tau=float(tau), reps=int(reps), seeds=seeds, max_iter=CONSENSUS_MAX_ITER)
    if (ci < 0).any():
        if not np.isfinite(a).all():
            raise ValueError("consensus_und: D holds NaN or inf")
        raise RuntimeError(f"consensus_und: no consensus after {CONSENSUS_MAX_ITER} iterations "
                           f"(iterations made: {np.atleast_1d(iters).tolist()})")
    return ci.astype(np.int64) + 1

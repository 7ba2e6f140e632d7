"""The three graph_utils helpers the SC optimiser uses (graph_utils.py:92-164), and
the weighted, undirected core of the reference's graph measures on the device.

get_uptri, matrix_recon and thresholding: same call surface and results as the
reference's, host numpy on N x N matrices, O(N^2) bookkeeping once per optimiser
iteration.  distance_wei, efficiency_wei, clustering_coef_wu, transitivity_wu,
strengths_und and degrees_und (with cuberoot, invert and the host charpath) run
on the device through sigchain.graph_measures, for one matrix or a [B, N, N]
stack; betweenness_wei and betweenness_bin through sigchain.graph_betweenness,
participation_coef and module_degree_zscore through
sigchain.graph_module_measures (which also gives the modularity Q of a given
partition); community_louvain, agreement and get_agreement_matrix through
sigchain.graph_louvain, graph_agreement and graph_consensus_matrix;
modularity_louvain_und_sign and consensus_und through partition (partition_np);
probabilistic_thresholding, the surrogate test that decides which FC entries are
links at all, through surrogate.fc_surrogate_test (surrogate_np);
randmio_und_signed, null_model_und_sign and participation_coef_norm through
nullmodel (nullmodel_np); rich_club_wu, rich_club_wd, rich_club_bu, rich_club_bd,
assortativity_wei, assortativity_bin and score_wu through hubs (hubs_np).  torch and
the library are imported on first use, so importing this module stays light.

Outside: of the partition search the 'negative_sym' and 'negative_asym'
objectives (unreachable in the reference, which refuses negative weights
first), the spectral search of modularity_und (its kci form is
graph_module_measures' Q), and N > 96; probabilistic_thresholding2, the
rank-remapped variant of the surrogate test.  The rest of the 2,600-line
toolbox (the other null models) is analysis outside the sweep path.
"""
import numpy as np

from .hubs_np import (assortativity_bin, assortativity_wei, rich_club_bd, rich_club_bu, rich_club_wd,  # noqa: F401
                      rich_club_wu, score_wu)  # (wc_hubs.hip)
from .nullmodel_np import null_model_und_sign, participation_coef_norm, randmio_und_signed  # noqa: F401  (wc_nullmodel.hip)
from .partition_np import consensus_und, modularity_louvain_und_sign  # noqa: F401  (wc_louvain_sign.hip)
from .surrogate_np import probabilistic_thresholding  # noqa: F401  (wc_surrogate.hip)


def get_uptri(x):
    """Strict upper triangle, row-major (graph_utils.py:92-105)."""
    x = np.asarray(x)
    return x[np.triu_indices(x.shape[0], 1)].astype(np.float64)


def matrix_recon(x):
    """Symmetric matrix with zero diagonal from its strict upper triangle (graph_utils.py:107-119)."""
    x = np.asarray(x, dtype=np.float64)
    n = int((1 + np.sqrt(1 + 8 * len(x))) // 2)
    m = np.zeros((n, n))
    m[np.triu_indices(n, 1)] = x
    return m + m.T


def thresholding(x, threshold=0.20, zero_diag=True, direct="undirected"):
    """Keep the strongest `threshold` fraction of links (graph_utils.py:135-164).

    Like the reference, zero_diag fills the caller's diagonal with 0 in place, and
    the kept set is np.argsort(...)[::-1][:k] (ties resolved as numpy resolves them).
    """
    n = x.shape[0]
    if zero_diag:
        np.fill_diagonal(x, 0)
    if direct == "directed":
        xv = x.reshape((1, n * n))
        k = int((n * n - n) * threshold)
        keep = np.argsort(xv)[0, ::-1][:k]
        out = np.zeros(n * n)
        out[keep] = xv[0, keep]
        return out.reshape((n, n))
    if direct == "undirected":
        xv = get_uptri(x)
        k = int(((n * n - n) // 2) * threshold)
        keep = np.argsort(xv)[::-1][:k]
        out = np.zeros_like(xv)
        out[keep] = xv[keep]
        return matrix_recon(out)
    raise ValueError("Invalid type of matrix -> direct options: undirected or directed")


# ---- weighted graph measures on the device (sigchain.graph_measures) ----
# The reference's call surface and return shapes for one N x N matrix; as an extension a [B, N, N]
# stack gives stacked results from one batched launch.  torch and the library load on first use.

GRAPH_MAX_N = 96  # sigchain.GRAPH_MAX_N: one matrix per workgroup, in LDS


def cuberoot(x):
    """sign(x) |x|^(1/3) (graph_utils.py:38-43)."""
    x = np.asarray(x, dtype=np.float64)
    r = np.abs(x) ** (1 / 3)
    return np.where(x < 0, -r, r)


def invert(W, copy=True):
    """1/W where W != 0: weights to lengths (graph_utils.py:68-90); in place with copy=False."""
    out = W.copy() if copy else W
    nz = out != 0
    out[nz] = 1.0 / out[nz]
    return out


def _matrices(name, W, nonnegative):
    """W as a contiguous fp64 [N][N] or [B][N][N] array, refused here where the device would refuse it."""
    a = np.ascontiguousarray(W, dtype=np.float64)
    if a.ndim not in (2, 3) or a.shape[-1] != a.shape[-2] or a.shape[0] == 0:
        raise ValueError(f"{name}: needs an N x N matrix or a [B, N, N] stack, got shape {a.shape}")
    N = a.shape[-1]
    if N < 2 or N > GRAPH_MAX_N:
        raise ValueError(f"{name}: N = {N}, the device kernels take 2 <= N <= {GRAPH_MAX_N}")
    if nonnegative and not (a >= 0).all():
        raise ValueError(f"{name}: negative or NaN entries (the shortest paths are undefined)")
    return a


def _on_device(fn, *arrays, **kw):
    """sigchain's `fn` on device copies of the numpy arrays among its arguments (anything else goes as it
    is), its tensors back as numpy arrays.  torch and sigchain are imported here, on first use."""
    import torch

    from . import sigchain

    def up(v):
        return torch.from_numpy(v).cuda() if isinstance(v, np.ndarray) else v

    def down(v):
        if isinstance(v, dict):
            return {k: down(x) for k, x in v.items()}
        return tuple(down(x) for x in v) if isinstance(v, tuple) else v.cpu().numpy()

    return down(getattr(sigchain, fn)(*map(up, arrays), **{k: up(v) for k, v in kw.items()}))


def _device(a, names, **kw):
    got = _on_device("graph_measures", a, names, **kw)
    return [got[m] for m in names]


def distance_wei(G):
    """(D, B): shortest weighted paths over the connection lengths G and their numbers of edges
    (graph_utils.py:1462-1529); inf and 0 for an unreachable pair."""
    D, B = _device(_matrices("distance_wei", G, True), ("dist", "hops"), lengths=True)
    return D, B.astype(np.float64)


def charpath(D, include_diagonal=False, include_infinite=True):
    """(lambda, efficiency, ecc, radius, diameter) of a distance matrix (graph_utils.py:1533-1591), on
    the host: O(N^2).  A row of which the two flags leave nothing has ecc NaN and is passed over by
    radius and diameter (the reference's masked maximum leaves numpy's fill value there)."""
    D = np.asarray(D, dtype=np.float64)
    if D.ndim == 3:
        lam, eff, ecc, rad, dia = zip(*(charpath(d, include_diagonal, include_infinite) for d in D))
        return np.array(lam), np.array(eff), np.array(ecc), np.array(rad), np.array(dia)
    keep = ~np.isnan(D)
    if not include_diagonal:
        keep &= ~np.eye(D.shape[0], dtype=bool)
    if not include_infinite:
        keep &= ~np.isinf(D)
    with np.errstate(divide="ignore", invalid="ignore"):
        v = D[keep]
        lam = v.mean() if v.size else np.nan
        eff = (1 / v).mean() if v.size else np.nan
    ecc = np.array([row[k].max() if k.any() else np.nan for row, k in zip(D, keep)])
    some = ecc[~np.isnan(ecc)]
    return lam, eff, ecc, (some.min() if some.size else np.nan), (some.max() if some.size else np.nan)


def efficiency_wei(Gw, local=False):
    """Global efficiency (a float) or, with local=True, the local efficiency of every node
    (graph_utils.py:597-690)."""
    a = _matrices("efficiency_wei", Gw, True)
    E, = _device(a, ("local_efficiency" if local else "efficiency",))
    return E if local or a.ndim == 3 else float(E)


def clustering_coef_wu(W):
    """Weighted clustering coefficient of every node (graph_utils.py:1305-1323)."""
    return _device(_matrices("clustering_coef_wu", W, False), ("clustering",))[0]


def transitivity_wu(W):
    """Weighted transitivity (graph_utils.py:1673-1689)."""
    a = _matrices("transitivity_wu", W, False)
    T, = _device(a, ("transitivity",))
    return T if a.ndim == 3 else float(T)


def strengths_und(CIJ):
    """Node strengths: column sums (graph_utils.py:1766-1778)."""
    return _device(_matrices("strengths_und", CIJ, False), ("strengths",))[0]


def degrees_und(CIJ):
    """Node degrees: non-zeros of every column (graph_utils.py:1721-1737)."""
    return _device(_matrices("degrees_und", CIJ, False), ("degrees",))[0].astype(np.float64)


# ---- node measures on the device (sigchain.graph_betweenness, sigchain.graph_module_measures) ----

def betweenness_wei(G):
    """Node betweenness centrality over the connection lengths G (graph_utils.py:1983-2052): ordered
    pairs, so an undirected graph has twice the textbook value."""
    return _on_device("graph_betweenness", _matrices("betweenness_wei", G, True), lengths=True)


def betweenness_bin(G):
    """Node betweenness centrality of a binary graph (graph_utils.py:1929-1980): the same kernel on
    the lengths (G != 0)."""
    return _on_device("graph_betweenness", (_matrices("betweenness_bin", G, False) != 0).astype(np.float64),
                      lengths=True)


def _labels(name, ci, a):
    """ci [N] or, with a stack, [B, N] -> (int32 labels 0 .. K-1 through np.unique, as the reference
    relabels them, K)."""
    ci = np.asarray(ci)
    N = a.shape[-1]
    if ci.ndim not in (1, 2) or ci.shape[-1] != N or (ci.ndim == 2 and (a.ndim != 3 or ci.shape[0] != a.shape[0])):
        raise ValueError(f"{name}: ci needs one label per node, [N] or [B, N] with a stack, got shape {ci.shape} "
                         f"for matrices of shape {a.shape}")
    rows = [np.unique(row, return_inverse=True)[1].reshape(-1) for row in ci.reshape(-1, N)]
    lab = np.ascontiguousarray(np.array(rows, dtype=np.int32).reshape(ci.shape))
    return lab, int(lab.max()) + 1


def _modules(a, lab, K, name, **kw):
    return _on_device("graph_module_measures", a, lab, (name,), n_modules=K, **kw)[name]


def participation_coef(W, ci, degree="undirected"):
    """Participation coefficient of every node for the partition ci (graph_utils.py:271-307); degree
    'undirected', 'out' (rows) or 'in' (columns)."""
    a = _matrices("participation_coef", W, False)
    if degree not in ("undirected", "in", "out"):
        raise ValueError(f"participation_coef: degree {degree!r}, must be 'undirected', 'in' or 'out'")
    lab, K = _labels("participation_coef", ci, a)
    return _modules(a, lab, K, "participation", degree=degree)


def module_degree_zscore(W, ci, flag=0):
    """Within-module degree z-score of every node for the partition ci (graph_utils.py:2103-2140);
    flag 0 undirected, 1 in, 2 out, 3 in and out, as the reference evaluates them: W, W, W^T,
    W + W^T."""
    a = _matrices("module_degree_zscore", W, False)
    if isinstance(flag, bool) or flag not in (0, 1, 2, 3):
        raise ValueError(f"module_degree_zscore: flag {flag!r}, must be 0, 1, 2 or 3")
    lab, K = _labels("module_degree_zscore", ci, a)
    return _modules(a, lab, K, "zscore", zflag=int(flag))


# ---- partition search on the device (sigchain.graph_louvain, graph_agreement, graph_consensus_matrix) ----

def _louvain_args(name, W, ci, B):
    """(W checked, starting labels or None, the objective as sigchain.graph_louvain takes it), refused
    here where the reference refuses."""
    a = _matrices(name, W, False)
    if a.min() < -1e-10:                                         # graph_utils.py:999
        raise ValueError(f"{name}: adjmat must not contain negative weights")
    lab = None if ci is None else _labels(name, ci, a)[0]
    if isinstance(B, str):
        if B in ("negative_sym", "negative_asym"):
            raise ValueError(f"{name}: B = {B!r} is not built: the reference refuses negative weights before it "
                             "reaches that objective")
        if B not in ("modularity", "potts"):
            raise ValueError(f"{name}: unknown objective function type {B!r}, must be 'modularity', 'potts' or a matrix")
        if B == "potts" and not ((a == 0) | (a == 1)).all():
            raise ValueError(f"{name}: Potts hamiltonian requires binary input matrix")
        return a, lab, B
    obj = np.ascontiguousarray(B, dtype=np.float64)
    if obj.shape != a.shape and obj.shape != a.shape[-2:]:
        raise ValueError(f"{name}: objective function matrix does not match size of adjacency matrix")
    return a, lab, obj


def community_louvain(W, gamma=1, ci=None, B="modularity", seed=None):
    """(ci, q): Louvain community structure of W and the objective reached (graph_utils.py:958-1122);
    labels from 1.  B 'modularity', 'potts' or an objective matrix (symmetrised with a warning where
    it is not symmetric); ci the starting partition; seed None draws one from os.urandom.  W is an
    N x N matrix or a [B, N, N] stack (ci [B, N], q [B]; one launch).

    The algorithm is the reference's; the order in which a sweep visits the nodes is the engine's
    (Philox words keyed by the seed and the sweep's number, sigchain.graph_louvain), so a given seed
    does NOT reproduce the partition numpy's generator gives for that seed, only the reference's
    algorithm under the engine's order.  The same seed always gives the same result.
    Not built: B 'negative_sym' and 'negative_asym' (unreachable in the reference, which raises on
    negative weights first), modularity_und's spectral search, N > 96.  Matrices with weights of both
    signs go to modularity_louvain_und_sign."""
    import os
    a, lab, obj = _louvain_args("community_louvain", W, ci, B)
    if seed is None:
        seed = int.from_bytes(os.urandom(8), "little")
    part, q = _on_device("graph_louvain", a, seeds=int(seed), gamma=float(gamma), ci=lab, objective=obj)
    part = part.astype(np.int64) + 1
    return (part, float(q)) if a.ndim == 2 else (part, q)


def agreement(ci, buffsz=1000):
    """Agreement matrix D of the partitions ci [N, M], one per column, the reference's orientation
    (graph_utils.py:890-932): D[i, j] partitions put i and j together; 0 on the diagonal.  A
    [B, N, M] stack gives [B, N, N].  buffsz is accepted and ignored."""
    c = np.asarray(ci)
    if c.ndim not in (2, 3) or c.shape[-1] == 0:
        raise ValueError(f"agreement: ci needs [vertex x partition], or a [B, N, M] stack, got shape {c.shape}")
    if c.shape[-2] < 2 or c.shape[-2] > GRAPH_MAX_N:
        raise ValueError(f"agreement: N = {c.shape[-2]}, the device kernels take 2 <= N <= {GRAPH_MAX_N}")
    lab = np.unique(c, return_inverse=True)[1].reshape(c.shape).astype(np.int32)   # any labels: equality is kept
    lab = np.ascontiguousarray(np.swapaxes(lab, -1, -2))
    return _on_device("graph_agreement", lab)


def get_agreement_matrix(W, reps=100, tau=0.5, gamma=1, ci=None, B="modularity", seeds=None):
    """Thresholded agreement of reps Louvain runs (graph_utils.py:935-956): seeds 0 .. reps-1, the
    agreement divided by reps, entries below tau set to 0, diagonal 0.  The reference cannot run with
    seeds given (it reads seed_vector before assigning it); this accepts a sequence of length reps.
    W is an N x N matrix or a [B, N, N] stack.  The visiting order is the engine's: see
    community_louvain."""
    a, lab, obj = _louvain_args("get_agreement_matrix", W, ci, B)
    if seeds is not None and (np.ndim(seeds) != 1 or len(seeds) != reps):
        raise ValueError("get_agreement_matrix: seeds must be an array of length equal to reps, or None")
    return _on_device("graph_consensus_matrix", a, reps=int(reps), tau=float(tau), gamma=float(gamma), ci=lab,
                      objective=obj, seeds=None if seeds is None else [int(v) for v in seeds])

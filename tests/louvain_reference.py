"""Host reference of the Louvain tests (test_louvain_cpu.py pins it to the golden outputs of the
reference's own community_louvain and agreement run under the engine's visiting order,
test_louvain_gpu.py checks the device against it): a numpy restatement of wc_graph_louvain and
wc_graph_agreement written from their definitions in include/wcsde.h, the visiting order, and the
objective matrices.

The visiting order.  Sweeps are numbered t = 0, 1, 2, ... over all levels of one run; sweep t over n
current nodes visits them in the stable argsort of n 32-bit keys, key i = word i % 4 of the
Philox4x32-10 block with key (WC_PHILOX_KEY0, WC_PHILOX_KEY1) and counter
(t & 0xffffffff, ((t >> 32) << 16) | i // 4, seed lo32, seed hi32).  Philox is written out here in
plain integers (Salmon et al., SC'11; the Random123 constants).

No symmetry is assumed anywhere."""
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "golden_louvain.npz")
TOL = 1e-10              # graph_utils.py:1066, :1081
SWEEP_GUARD = 1000       # :1071
MIN_MARGIN = 1e-9        # every committed and every tested run decides by at least this much
ZERO_BAND = 1e-12        # a tested quantity this close to 0 is left out of the margin, see louvain()
CASES = ("sc", "fc_dense", "fc_thr", "rand90", "dir24", "pendant12")
GAMMAS = (0.7, 1.3)

_M32 = 0xFFFFFFFF
PHILOX_KEY = (0x243F6A88, 0x85A308D3)   # WC_PHILOX_KEY0, WC_PHILOX_KEY1 of include/wcsde.h


def philox4x32_10(ctr, key=PHILOX_KEY):
    """One Philox4x32-10 block: four 32-bit counter words and two key words -> four words."""
    c0, c1, c2, c3 = (int(c) & _M32 for c in ctr)
    k0, k1 = key
    for _ in range(10):
        p0, p1 = 0xD2511F53 * c0, 0xCD9E8D57 * c2
        c0, c1, c2, c3 = (p1 >> 32) ^ c1 ^ k0, p1 & _M32, (p0 >> 32) ^ c3 ^ k1, p0 & _M32
        k0, k1 = (k0 + 0x9E3779B9) & _M32, (k1 + 0xBB67AE85) & _M32
    return c0, c1, c2, c3


def sweep_keys(seed, t, n):
    seed, t = int(seed), int(t)
    blocks = [philox4x32_10((t & _M32, ((t >> 32) << 16) | quad, seed & _M32, seed >> 32))
              for quad in range((n + 3) // 4)]
    return np.array([w for blk in blocks for w in blk][:n], dtype=np.uint32)


def sweep_order(seed, t, n):
    """The nodes of sweep t over n current nodes, in visiting order; ties go to the lower index."""
    return np.argsort(sweep_keys(seed, t, n), kind="stable")


def objective(W, gamma=1.0, kind="modularity"):
    """(obj, s): the reference's B after graph_utils.py:1032-1052 and its s = sum W."""
    W = np.asarray(W, dtype=np.float64)
    s = W.sum()
    with np.errstate(divide="ignore", invalid="ignore"):
        if isinstance(kind, str) and kind == "modularity":
            obj = W - gamma * np.outer(W.sum(axis=1), W.sum(axis=0)) / s
        elif isinstance(kind, str) and kind == "potts":
            obj = W - gamma * np.logical_not(W)
        else:
            obj = np.array(kind, dtype=np.float64)
            if not np.allclose(obj, obj.T):
                obj = (obj + obj.T) / 2
    return obj, s


def relabel(lab):
    return np.unique(np.asarray(lab), return_inverse=True)[1].reshape(-1)


def louvain(obj, s, seed, ci0=None):
    """(ci, q, info, margin) of one run.  ci: labels 0 .. K-1; info: (levels, sweeps in all); margin:
    the smallest, over every decision of the run, of |max dQ - 1e-10|, the gap between the best and
    the second-best distinct dQ where a node moves, and |q - q0 - 1e-10| at each level test: how far
    the run is from taking another turn under rounding.  An exact tie at the largest dQ between two
    modules that hold nodes is a margin of 0 (sums taken in another order may break it the other way),
    unless obj is integer-valued, where every sum is exact.  A tested quantity within 1e-12 of 0 is left
    out: every run ends on them (max dQ is the exact 0 of dQ[ma] wherever a node has nothing to gain,
    and q - q0 of the last level is 0 to rounding), they lie 1e-10 from the threshold, a million times
    the rounding of sums of <= 96 terms of size <= 1, and could never reach a margin of 1e-9; anything
    else near the threshold counts.  A non-finite obj or s gives ci = -1, q = NaN,
    info = (0, 0); a level that has not settled after 1000 sweeps gives ci = -1, q = NaN."""
    B = np.array(obj, dtype=np.float64)
    N = n = B.shape[0]
    if not (np.isfinite(B).all() and np.isfinite(s)):
        return np.full(N, -1), np.nan, (0, 0), np.inf
    whole = bool((B == np.rint(B)).all())                  # integer-valued: every sum is exact in any order
    Mb = np.arange(N) if ci0 is None else relabel(ci0)
    ci = Mb.copy()
    Hnm = np.zeros((n, n))
    for m in range(n):
        Hnm[:, m] = B[:, Mb == m].sum(axis=1)
    with np.errstate(divide="ignore", invalid="ignore"):
        q = B[Mb[:, None] == Mb[None, :]].sum() / s
    q0 = -np.inf
    t = levels = 0
    first = True
    margin = np.inf
    while True:
        with np.errstate(invalid="ignore"):
            gain = q - q0
        if np.isfinite(gain) and abs(gain) > ZERO_BAND:
            margin = min(margin, abs(gain - TOL))
        if not gain > TOL:
            break
        it, moved = 0, True
        while moved:
            it += 1
            if it > SWEEP_GUARD:
                return np.full(N, -1), np.nan, (levels, t), margin
            moved = False
            order = sweep_order(seed, t, n)
            t += 1
            for u in order:
                ma = Mb[u]
                dQ = Hnm[u, :] - Hnm[u, ma] + B[u, u]
                dQ[ma] = 0
                best = dQ.max()
                if abs(best) > ZERO_BAND:
                    margin = min(margin, abs(best - TOL))
                if best > TOL:
                    mb = int(np.argmax(dQ))
                    rest = dQ[dQ < best]
                    if rest.size:
                        margin = min(margin, best - rest.max())
                    tied = np.flatnonzero(dQ == best)[1:]
                    if not whole and np.isin(tied, Mb).any():
                        margin = 0.0
                    Hnm[:, mb] += B[:, u]
                    Hnm[:, ma] -= B[:, u]
                    Mb[u] = mb
                    moved = True
        Mb = relabel(Mb)
        ci = Mb.copy() if first else Mb[ci]
        first = False
        K = int(Mb.max()) + 1
        b1 = np.zeros((K, K))
        for i in range(K):
            for j in range(i, K):
                b1[i, j] = b1[j, i] = B[np.ix_(Mb == i, Mb == j)].sum()
        B, Hnm, Mb, n = b1, b1.copy(), np.arange(K), K
        q0 = q
        with np.errstate(divide="ignore", invalid="ignore"):
            q = np.trace(B) / s
        levels += 1
    return ci, float(q), (levels, t), margin


def agreement(ci):
    """D [N][N] of the partitions ci [R][N]: how many put i and j together, 0 on the diagonal; NaN
    throughout where a label is negative."""
    ci = np.asarray(ci)
    if (ci < 0).any():
        return np.full((ci.shape[1], ci.shape[1]), np.nan)
    D = (ci[:, :, None] == ci[:, None, :]).sum(axis=0).astype(np.float64)
    np.fill_diagonal(D, 0.0)
    return D


def consensus(ci, tau):
    """get_agreement_matrix's thresholding of the partitions ci [R][N]."""
    D = agreement(ci) / ci.shape[0]
    D[D < tau] = 0.0
    return D


def local_gain(obj, ci):
    """The largest dQ that moving one node to another module, or to a module of its own, would bring:
    at most 1e-10 at a partition Louvain has settled on."""
    obj, ci = np.asarray(obj, dtype=np.float64), relabel(ci)
    K = int(ci.max()) + 1
    Hnm = np.stack([obj[:, ci == m].sum(axis=1) for m in range(K)] + [np.zeros(len(obj))], axis=1)
    best = -np.inf
    for u in range(len(obj)):
        dQ = Hnm[u] - (Hnm[u, ci[u]] - obj[u, u])      # joining m: Hnm[u, m], leaving: Hnm[u, ma] - obj[u, u]
        dQ[ci[u]] = 0.0
        best = max(best, dQ.max())
    return best


def load_golden():
    """tests/golden/golden_louvain.npz as {key: array}, read only."""
    out = {}
    with np.load(GOLDEN) as z:
        for key in z.files:
            a = z[key]
            a.setflags(write=False)
            out[key] = a
    return out

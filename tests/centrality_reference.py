"""Host reference of the centrality tests (test_centrality_cpu.py pins it to the golden outputs of the
reference's own functions, test_centrality_gpu.py checks the device against it): numpy restatements
of wc_graph_betweenness and wc_graph_modules, written from their definitions, and the partitions.

Betweenness is Brandes' algorithm on the connection lengths L (a zero is no edge, the diagonal is
ignored, ordered pairs are counted).  From every source u, Dijkstra in rounds: all unsettled nodes
at the minimum distance are settled together; an edge v -> w out of a settled v into an unsettled w
is tried with the single sum D[v] + L[v][w]: strictly shorter replaces w's predecessors and its
number of shortest paths by v's, equal adds v and v's number.  Then the dependencies, the rounds
backwards and a round's nodes in descending order: dep[v] += (1 + dep[w]) NP[v] / NP[w] for every
predecessor v of w, and bc[w] += dep[w] for every w but the source.

No symmetry is assumed anywhere."""
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "golden_centrality.npz")
PARTITIONS = ("mod4", "hemi", "singletons", "lonely")
# sum of the reference's betweenness_wei over the nodes, per path case (integers: unique shortest paths)
BC_SUMS = {"sc": 23374, "fc_dense": 720, "fc_thr": 10472, "rand90": 6924, "dir24": 500, "pendant12": 74}
BINARY_CASES = ("fc_thr", "dir24")


def betweenness(L):
    """Node betweenness centrality of the connection lengths L [N][N]."""
    L = np.array(L, dtype=np.float64)
    n = L.shape[0]
    np.fill_diagonal(L, 0.0)
    edge = L != 0
    bc = np.zeros(n)
    for u in range(n):
        D = np.full(n, np.inf)
        D[u] = 0.0
        NP = np.zeros(n)
        NP[u] = 1.0
        settled = np.zeros(n, dtype=bool)
        pred = np.zeros((n, n), dtype=bool)
        rounds = []
        while not settled.all():
            m = D[~settled].min()
            if not m < np.inf:
                break                                            # the rest is out of reach
            V = np.flatnonzero(~settled & (D == m))
            settled[V] = True
            rounds.append(V)
            for v in V:
                w = edge[v] & ~settled
                cand = D[v] + L[v]
                shorter, equal = w & (cand < D), w & (cand == D)
                D[shorter] = cand[shorter]
                NP[shorter] = NP[v]
                pred[shorter] = False
                pred[shorter, v] = True
                NP[equal] += NP[v]
                pred[equal, v] = True
        dep = np.zeros(n)
        order = list(np.flatnonzero(~settled)) + [w for V in rounds[:0:-1] for w in V[::-1]]
        for w in order:
            bc[w] += dep[w]
            for v in np.flatnonzero(pred[w]):
                dep[v] += (1 + dep[w]) * NP[v] / NP[w]
    return bc


def relabel(ci):
    """Labels 0 .. K-1 in the order of the sorted distinct values of ci, and K."""
    u, inv = np.unique(np.asarray(ci), return_inverse=True)
    return inv.reshape(-1).astype(np.int32), len(u)


def participation(W, ci, degree="undirected"):
    """P_i = 1 - sum_m (sum_{j in m} W_ij)^2 / (sum_j W_ij)^2, 0 where the strength is 0; degree 'in'
    takes the transpose."""
    W = np.asarray(W, dtype=np.float64)
    if degree == "in":
        W = W.T
    lab, K = relabel(ci)
    ko = W.sum(axis=1)
    kc2 = np.zeros(len(W))
    for m in range(K):
        kc2 += W[:, lab == m].sum(axis=1) ** 2
    with np.errstate(divide="ignore", invalid="ignore"):
        P = 1.0 - kc2 / ko ** 2
    P[ko == 0] = 0.0
    return P


def zscore(W, ci, flag=0):
    """(k_i - mean) / std of the within-module degrees of a node's own module, population std, 0 where
    that is NaN; flag 0, 1: W, 2: W^T, 3: W + W^T."""
    W = np.asarray(W, dtype=np.float64)
    A = {0: W, 1: W, 2: W.T, 3: W + W.T}[flag]
    lab, K = relabel(ci)
    Z = np.zeros(len(W))
    for m in range(K):
        idx = np.flatnonzero(lab == m)
        k = A[np.ix_(idx, idx)].sum(axis=1)
        with np.errstate(divide="ignore", invalid="ignore"):
            Z[idx] = (k - k.mean()) / np.sqrt(((k - k.mean()) ** 2).mean())
    Z[np.isnan(Z)] = 0.0
    return Z


def modularity(W, ci, gamma=1.0):
    """Q = (1/s) sum_ij (W_ij - gamma k_i^out k_j^in / s) delta(ci_i, ci_j), s = sum W."""
    W = np.asarray(W, dtype=np.float64)
    lab, _ = relabel(ci)
    s = W.sum()
    with np.errstate(divide="ignore", invalid="ignore"):
        Bm = W - gamma * np.outer(W.sum(axis=1), W.sum(axis=0)) / s
        return Bm[lab[:, None] == lab[None, :]].sum() / s


def deviation_abs(got, want):
    """Largest |got - want| / max(1, |want|): an absolute deviation next to 0, where z and P are
    differences that cancel, a relative one for large values.  NaN and inf must sit in the same places
    (else the deviation is inf)."""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    if got.shape != want.shape:
        return np.inf
    special = ~np.isfinite(want)
    same = (got[special] == want[special]) | (np.isnan(got[special]) & np.isnan(want[special]))
    if not same.all() or not np.isfinite(got[~special]).all():
        return np.inf
    g, w = got[~special], want[~special]
    return float(np.max(np.abs(g - w) / np.maximum(1.0, np.abs(w)))) if w.size else 0.0


def partition(name, n):
    """The test partitions of n nodes, labels 0 .. K-1: four interleaved modules, two hemispheres, all
    singletons, and three modules beside one that has node 0 alone."""
    k = np.arange(n)
    ci = {"mod4": k % 4, "hemi": (k >= (n + 1) // 2).astype(int), "singletons": k,
          "lonely": np.where(k == 0, 0, 1 + k % 3)}[name]
    return relabel(ci)[0]


def load_golden():
    """tests/golden/golden_centrality.npz as {case: {name: array}}, read only."""
    cases = {}
    with np.load(GOLDEN) as z:
        for key in z.files:
            case, name = key.split("/")
            a = z[key]
            a.setflags(write=False)
            cases.setdefault(case, {})[name] = a
    return cases

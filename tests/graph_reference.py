"""Host reference of the graph tests (test_graph_cpu.py pins it to the golden outputs of the
reference's own functions, test_graph_gpu.py checks the device against it): numpy restatements of the
weighted measures of wc_graph_paths, wc_graph_local_efficiency and wc_graph_clustering, and the test
graphs.

Shortest paths are a vectorised Floyd-Warshall (the reference runs Dijkstra per source): D starts as 0
on the diagonal, L where L != 0 and +inf elsewhere; for k = 0 .. N-1 every D[i][j] above
D[i][k] + D[k][j] takes that sum and the hop count h[i][k] + h[k][j].  scipy.sparse.csgraph gives a
second opinion on D.  Hop counts equal Dijkstra's where the shortest path is unique:
second_best_gap measures by how much.

No symmetry is assumed anywhere: the expressions are those of the reference, as written."""
import os

import numpy as np
from scipy.sparse import csgraph

DATA = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "nremmodfc_amd", "data")
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "golden_graph.npz")
# the golden cases with shortest paths (signed5 has clustering and transitivity only)
PATH_CASES = ("sc", "fc_dense", "fc_thr", "rand90", "dir24", "pendant12")
ALL_CASES = PATH_CASES + ("signed5",)


def cuberoot(x):
    return np.sign(x) * np.abs(x) ** (1 / 3)


def lengths_of(w):
    """1/w where w != 0, 0 elsewhere."""
    w = np.asarray(w, dtype=np.float64)
    out = np.zeros_like(w)
    nz = w != 0
    out[nz] = 1.0 / w[nz]
    return out


def floyd_warshall(L):
    """(D, hops) of the connection lengths L [N][N]."""
    n = L.shape[0]
    off = ~np.eye(n, dtype=bool)
    edge = (L != 0) & off
    D = np.where(edge, L, np.inf)
    D[~off] = 0.0
    H = edge.astype(np.int64)
    for k in range(n):
        cand = D[:, k, None] + D[None, k, :]
        better = cand < D
        H = np.where(better, H[:, k, None] + H[None, k, :], H)
        D = np.where(better, cand, D)
    return D, H


def scipy_distances(L):
    """The same D from SciPy's Dijkstra (a zero of the dense matrix is no edge)."""
    return csgraph.shortest_path(np.asarray(L, dtype=np.float64), method="D", directed=True)


def charpath(D, include_infinite=True):
    """(lambda, efficiency, ecc, radius, diameter) over the off-diagonal entries of D.  A row of which
    include_infinite=False leaves nothing has ecc NaN and is passed over by radius and diameter (the
    reference's masked maximum puts numpy's fill value there, 1e20, and in the diameter)."""
    n = D.shape[0]
    keep = ~np.eye(n, dtype=bool)
    if not include_infinite:
        keep &= ~np.isinf(D)
    with np.errstate(divide="ignore", invalid="ignore"):
        v = D[keep]
        lam = v.mean() if v.size else np.nan
        eff = (1 / v).mean() if v.size else np.nan
        ecc = np.array([D[i][keep[i]].max() if keep[i].any() else np.nan for i in range(n)])
    some = ~np.isnan(ecc)
    return lam, eff, ecc, (ecc[some].min() if some.any() else np.nan), (ecc[some].max() if some.any() else np.nan)


def local_efficiency(w):
    w = np.asarray(w, dtype=np.float64)
    n = w.shape[0]
    L = lengths_of(w)
    E = np.zeros(n)
    for u in range(n):
        V = np.flatnonzero((w[u] != 0) | (w[:, u] != 0))
        D, _ = floyd_warshall(L[np.ix_(V, V)])
        with np.errstate(divide="ignore"):
            e = 1 / D
        np.fill_diagonal(e, 0.0)
        se = cuberoot(e) + cuberoot(e.T)
        sw = cuberoot(w[u, V]) + cuberoot(w[V, u])
        numer = (sw[:, None] * sw[None, :] * se).sum() / 2
        if numer != 0:
            sa = (w[u, V] != 0).astype(int) + (w[V, u] != 0).astype(int)
            E[u] = numer / (sa.sum() ** 2 - (sa * sa).sum())
    return E


def cyc3(w):
    """sum_j (ws ws)_ij ws_ji, ws = cuberoot(w)."""
    ws = cuberoot(np.asarray(w, dtype=np.float64))
    return np.einsum("ij,ji->i", ws @ ws, ws)


def clustering(w):
    w = np.asarray(w)
    c3 = cyc3(w)
    K = (w != 0).sum(axis=1).astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(c3 == 0, 0.0, c3 / (K * (K - 1)))


def transitivity(w):
    w = np.asarray(w)
    K = (w != 0).sum(axis=1)
    with np.errstate(divide="ignore", invalid="ignore"):
        return cyc3(w).sum() / np.float64((K * (K - 1)).sum())


def strengths(w):
    return np.asarray(w, dtype=np.float64).sum(axis=0)


def degrees(w):
    return (np.asarray(w) != 0).sum(axis=0)


def measures(w, paths=True):
    """Every measure of one matrix, under the names of sigchain.graph_measures."""
    out = {"clustering": clustering(w), "transitivity": transitivity(w), "strengths": strengths(w),
           "degrees": degrees(w)}
    if paths:
        D, H = floyd_warshall(lengths_of(w))
        lam, eff, ecc, radius, diameter = charpath(D)
        out.update(dist=D, hops=H, charpath=lam, efficiency=eff, ecc=ecc, radius=radius, diameter=diameter,
                   local_efficiency=local_efficiency(w))
    return out


def second_best_gap(L, D):
    """Smallest relative gap, over the reachable pairs i != j, between the best and the second-best
    last edge: min over (i, j) of (second - best) / best of D[i][m] + L[m][j] over the edges m -> j.
    Above rounding, every shortest path is unique (by induction on its last edge) and Floyd-Warshall's
    hop counts are Dijkstra's."""
    n = L.shape[0]
    gap = np.inf
    for j in range(n):
        m = np.flatnonzero((L[:, j] != 0) & (np.arange(n) != j))
        if m.size < 2:
            continue
        cand = np.sort(D[:, m] + L[m, j][None, :], axis=1)      # [i][edge]
        ok = np.isfinite(cand[:, 1]) & (np.arange(n) != j)
        if ok.any():
            gap = min(gap, ((cand[ok, 1] - cand[ok, 0]) / cand[ok, 0]).min())
    return gap


def deviation(got, want):
    """Largest relative deviation |got - want| / |want| over the finite non-zero entries of want; where
    want is 0, infinite or NaN, got must be the same (else the deviation is inf)."""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    if got.shape != want.shape:
        return np.inf
    special = ~np.isfinite(want) | (want == 0)
    same = (got[special] == want[special]) | (np.isnan(got[special]) & np.isnan(want[special]))
    if not same.all():
        return np.inf
    g, w = got[~special], want[~special]
    return float(np.max(np.abs(g - w) / np.abs(w))) if w.size else 0.0


# ---- the test graphs ----

def get_uptri(x):
    return x[np.triu_indices(x.shape[0], 1)]


def threshold_und(x, fraction):
    """The strongest `fraction` of the links of a symmetric matrix (graph_utils.thresholding)."""
    from nremmodfc_amd import graph_utils
    return graph_utils.thresholding(np.array(x, dtype=np.float64), fraction)


def random_graph(n, density, seed, directed=False):
    """Uniform weights in (0.05, 1) on a random support, zero diagonal."""
    rng = np.random.default_rng(seed)
    w = rng.uniform(0.05, 1.0, (n, n)) * (rng.uniform(size=(n, n)) < density)
    np.fill_diagonal(w, 0.0)
    if directed:
        return w
    w = np.triu(w, 1)
    return w + w.T


def pendant_graph():
    """12 nodes: node 11 isolated, node 10 tied to node 0 alone, the other ten a random graph."""
    w = np.zeros((12, 12))
    w[:10, :10] = random_graph(10, 0.6, 3)
    w[0, 10] = w[10, 0] = 0.7
    return w


def signed_graph():
    """5 nodes, symmetric, weights of both signs."""
    rng = np.random.default_rng(5)
    w = np.triu(rng.uniform(-1.0, 1.0, (5, 5)), 1)
    w[0, 4] = 0.0
    return w + w.T


def load_golden():
    """tests/golden/golden_graph.npz as {case: {name: array}}, the packed matrices put together again
    (make_graph_golden.py: a symmetric w from its upper triangle, its distances from their upper
    triangle and the difference of the two triangles' bit patterns)."""
    cases = {}
    with np.load(GOLDEN) as z:
        for key in z.files:
            case, name = key.split("/")
            cases.setdefault(case, {})[name] = z[key]
    for c in cases.values():
        if "w_triu" in c:
            t = c.pop("w_triu")
            n = int((np.sqrt(8 * t.size + 1) - 1) // 2)
            w = np.zeros((n, n))
            w[np.triu_indices(n)] = t
            c["w"] = w + np.triu(w, 1).T
        if "dist_triu" in c:
            n = c["w"].shape[0]
            iu = np.triu_indices(n, 1)
            up, skew = c.pop("dist_triu"), c.pop("dist_skew")
            D = np.zeros((n, n))
            D[iu] = up
            D.T[iu] = (up.view(np.int64) + skew).view(np.float64)
            c["dist"] = D
        if "hops" in c:
            c["hops"] = c["hops"].astype(np.int64)
        for a in c.values():
            a.setflags(write=False)
    return cases


def golden_inputs():
    """The seven matrices of tests/golden/golden_graph.npz, by case name."""
    sc = np.load(os.path.join(DATA, "SC_opti_25julio.npy")).astype(np.float64)
    fc = np.load(os.path.join(DATA, "mean_mat_W_8dic24.npy")).astype(np.float64)
    fc = np.maximum(fc, 0.0)
    np.fill_diagonal(fc, 0.0)
    return {"sc": sc, "fc_dense": fc, "fc_thr": threshold_und(fc, 0.2), "rand90": random_graph(90, 0.3, 1),
            "dir24": random_graph(24, 0.4, 2, directed=True), "pendant12": pendant_graph(),
            "signed5": signed_graph()}

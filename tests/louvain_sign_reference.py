"""Host reference of the signed Louvain and consensus tests (test_louvain_sign_cpu.py pins it to the
golden outputs of the reference's own modularity_louvain_und_sign and consensus_und run under the
engine's visiting order, test_louvain_sign_gpu.py checks the device against it): a numpy restatement of
wc_graph_louvain_sign written from its definition in include/wcsde.h, and of partition.graph_consensus.
The visiting order is louvain_reference.sweep_order.  No symmetry is assumed in the search."""
import os

import numpy as np

from tests import louvain_reference as lr

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "golden_louvain_sign.npz")
TOL = lr.TOL                      # graph_utils.py:772, :807
SWEEP_GUARD = lr.SWEEP_GUARD      # :788
LEVEL_GUARD = 300                 # :773
MIN_MARGIN = lr.MIN_MARGIN
ZERO_BAND = lr.ZERO_BAND
QTYPES = ("sta", "pos", "smp", "gja", "neg")
CASES = ("signed5", "corr24", "fc_centred", "corr96", "fc_thr")
GAMMAS = lr.GAMMAS
# consensus cases: D = the agreement of the case's eight committed "sta" partitions / 8, then (tau, reps)
CONSENSUS = (("signed5", 0.2, 8), ("corr24", 0.4, 8), ("fc_centred", 0.5, 16), ("corr96", 0.3, 8), ("fc_thr", 0.6, 16))
DYADIC = 2.0 ** 20


def dyadic(W):
    """Every entry an integer multiple of 2^-20 and the sum of the magnitudes below 2^20 (2^40 in units of
    2^-20, far below 2^53): every sum of entries the search takes is then exact in any order, so the
    inputs of dQ are the same bits on the device as in numpy."""
    W = np.asarray(W, dtype=np.float64)
    scaled = W * DYADIC
    return bool(np.isfinite(W).all() and (scaled == np.rint(scaled)).all() and np.abs(scaled).sum() < 2.0 ** 40)


def scales(s0, s1, qtype):
    """(s0, s1, d0, d1) after :743-766."""
    with np.errstate(divide="ignore"):
        inv0, inv1, inv01 = np.float64(1.0) / s0, np.float64(1.0) / s1, np.float64(1.0) / (s0 + s1)
    d0, d1 = {"sta": (inv0, inv01), "pos": (inv0, 0.0), "smp": (inv0, inv1), "gja": (inv01, inv01),
              "neg": (0.0, inv1)}[qtype]
    if not s0:
        s0, d0 = 1.0, 0.0
    if not s1:
        s1, d1 = 1.0, 0.0
    return s0, s1, d0, d1


def louvain_sign(W, seed, gamma=1.0, qtype="sta", trace=None):
    """(ci, q, info, margin) of one run.  ci: labels 0 .. K-1; info: (levels, sweeps in all); margin
    as louvain_reference.louvain defines it: the smallest, over every decision of the run, of
    |max dQ - 1e-10|, the gap between the best and the second-best distinct dQ where a node moves, and
    |q - q before - 1e-10| at each level test, quantities within 1e-12 of 0 left out.  An exact tie at
    the largest dQ between two modules that hold nodes is a margin of 0, unless W is dyadic (dyadic()),
    where every sum is exact and every tie breaks as it does in the reference.  A non-finite W gives
    ci = -1, q = NaN, info = (0, 0); a level not settled after 1000 sweeps, or a 301st level, gives
    ci = -1, q = NaN.  trace, a list, receives the number of sweeps of each level (a level of one sweep
    moved nothing)."""
    if qtype not in QTYPES:
        raise KeyError("modularity type unknown")
    W = np.array(W, dtype=np.float64)
    N = n = W.shape[0]
    if not np.isfinite(W).all():
        return np.full(N, -1), np.nan, (0, 0), np.inf
    exact = dyadic(W)
    W0, W1 = W * (W > 0), -W * (W < 0)
    s0, s1, d0, d1 = scales(np.sum(W0), np.sum(W1), qtype)
    ci = np.arange(N)
    q, qprev = 0.0, -1.0
    t = levels = 0
    margin = np.inf
    while True:
        gain = q - qprev
        if abs(gain) > ZERO_BAND:
            margin = min(margin, abs(gain - TOL))
        if not gain > TOL:
            break
        if levels >= LEVEL_GUARD:
            return np.full(N, -1), np.nan, (levels, t), margin
        kn0, kn1 = W0.sum(axis=0), W1.sum(axis=0)
        km0, km1, knm0, knm1 = kn0.copy(), kn1.copy(), W0.copy(), W1.copy()
        m = np.arange(n)
        it, moved = 0, True
        while moved:
            it += 1
            if it > SWEEP_GUARD:
                return np.full(N, -1), np.nan, (levels, t), margin
            moved = False
            order = lr.sweep_order(seed, t, n)
            t += 1
            for u in order:
                ma = m[u]
                dQ0 = (knm0[u, :] + W0[u, u] - knm0[u, ma]) - gamma * kn0[u] * (km0 + kn0[u] - km0[ma]) / s0
                dQ1 = (knm1[u, :] + W1[u, u] - knm1[u, ma]) - gamma * kn1[u] * (km1 + kn1[u] - km1[ma]) / s1
                dQ = d0 * dQ0 - d1 * dQ1
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
                    if not exact and np.isin(tied, m).any():
                        margin = 0.0
                    knm0[:, mb] += W0[:, u]
                    knm0[:, ma] -= W0[:, u]
                    knm1[:, mb] += W1[:, u]
                    knm1[:, ma] -= W1[:, u]
                    km0[mb] += kn0[u]
                    km0[ma] -= kn0[u]
                    km1[mb] += kn1[u]
                    km1[ma] -= kn1[u]
                    m[u] = mb
                    moved = True
        if trace is not None:
            trace.append(it)
        m = lr.relabel(m)
        ci = m[ci]
        n = int(m.max()) + 1
        wn0, wn1 = np.zeros((n, n)), np.zeros((n, n))
        for i in range(n):
            for j in range(i, n):
                sel = np.ix_(m == i, m == j)
                wn0[i, j] = wn0[j, i] = W0[sel].sum()
                wn1[i, j] = wn1[j, i] = W1[sel].sum()
        W0, W1 = wn0, wn1
        qprev = q
        q = float(d0 * (np.trace(W0) - np.sum(np.dot(W0, W0)) / s0) - d1 * (np.trace(W1) - np.sum(np.dot(W1, W1)) / s1))
        levels += 1
    return ci, q, (levels, t), margin


def first_occurrence(ci):
    """Labels renumbered 0, 1, ... in the order in which they first occur (the reference's
    unique_partitions, 0-based)."""
    ci = np.asarray(ci)
    _, first, inverse = np.unique(ci, return_index=True, return_inverse=True)
    return np.argsort(np.argsort(first))[inverse.reshape(-1)]


def consensus(D, tau, reps, seeds=None, max_iter=100):
    """(ci, iterations, margin) of partition.graph_consensus on one matrix: consensus_und (:1124-1207)
    with the seed of rep r in iteration k being seeds[r] + k reps mod 2^64; ci first-occurrence labels
    from 0, or -1 where max_iter iterations did not converge or a run was refused; margin the smallest
    of the runs'."""
    D = np.array(D, dtype=np.float64)
    n = len(D)
    seeds = list(range(reps)) if seeds is None else [int(s) for s in seeds]
    margin = np.inf
    for k in range(max_iter):
        dt = D * (D >= tau)
        np.fill_diagonal(dt, 0)
        cis = np.zeros((reps, n), dtype=np.int64)
        for r in range(reps):
            ci, _, _, mg = louvain_sign(dt, (seeds[r] + k * reps) % (1 << 64))
            margin = min(margin, mg)
            if ci[0] < 0:
                return np.full(n, -1), k + 1, margin
            cis[r] = first_occurrence(ci)
        if (cis == cis[0]).all():
            return cis[0], k + 1, margin
        D = lr.agreement(cis) / reps
    return np.full(n, -1), max_iter, margin


def modularity_sign(W, ci, qtype="sta"):
    """The signed modularity of a partition as the search reports it (:848-850; Rubinov & Sporns 2011
    with the reference's weights d0, d1): gamma scales the moves, not the q returned."""
    W = np.asarray(W, dtype=np.float64)
    W0, W1 = W * (W > 0), -W * (W < 0)
    s0, s1, d0, d1 = scales(W0.sum(), W1.sum(), qtype)
    same = np.asarray(ci)[:, None] == np.asarray(ci)[None, :]
    q0 = (W0 - np.outer(W0.sum(axis=0), W0.sum(axis=0)) / s0)[same].sum()
    q1 = (W1 - np.outer(W1.sum(axis=0), W1.sum(axis=0)) / s1)[same].sum()
    return d0 * q0 - d1 * q1


def split(W):
    """(W0, W1): the positive weights and minus the negative ones (:738-739); a pair is passed on."""
    if isinstance(W, tuple):
        return W
    W = np.asarray(W, dtype=np.float64)
    return W * (W > 0), -W * (W < 0)


def pooled(W, ci):
    """(W0, W1) summed over the pairs of modules of ci: the graph on which every module is a node."""
    ci = lr.relabel(ci)
    K = int(ci.max()) + 1
    return tuple(np.array([[X[np.ix_(ci == i, ci == j)].sum() for j in range(K)] for i in range(K)]) for X in split(W))


def local_gain(W, ci, gamma=1.0, qtype="sta"):
    """The largest dQ, by the search's own expression (:797-803), that moving one node to another
    module of ci, or to a module of its own, would bring: at most 1e-10 where the search stopped at
    this level.  W is a matrix, or the pair (W0, W1) of a pooled graph."""
    W0, W1 = split(W)
    ci = lr.relabel(ci)
    K = int(ci.max()) + 1
    s0, s1, d0, d1 = scales(W0.sum(), W1.sum(), qtype)
    halves = []
    for X, s in ((W0, s0), (W1, s1)):
        kn = X.sum(axis=0)
        km = np.array([kn[ci == m].sum() for m in range(K)] + [0.0])
        knm = np.stack([X[:, ci == m].sum(axis=1) for m in range(K)] + [np.zeros(len(X))], axis=1)
        halves.append((X, s, kn, km, knm))
    best = -np.inf
    for u in range(len(W0)):
        ma = ci[u]
        dq = [(knm[u, :] + X[u, u] - knm[u, ma]) - gamma * kn[u] * (km + kn[u] - km[ma]) / s
              for X, s, kn, km, knm in halves]
        dQ = d0 * dq[0] - d1 * dq[1]
        dQ[ma] = 0.0
        best = max(best, dQ.max())
    return best


# ---- the test matrices ----

def grouped_corr(groups, size, seed, noise=1.0, length=200):
    """The correlation matrix of `groups` noisy groups of `size` series, zero diagonal."""
    rng = np.random.default_rng(seed)
    common = rng.standard_normal((groups, length))
    x = np.repeat(common, size, axis=0) + noise * rng.standard_normal((groups * size, length))
    c = np.corrcoef(x)
    np.fill_diagonal(c, 0.0)
    return c


def signed_graph(n, seed):
    """A symmetric n x n matrix with weights of both signs and group structure: the correlation matrix
    of n noisy series in groups of eight, zero diagonal."""
    rng = np.random.default_rng(seed)
    common = rng.standard_normal(((n + 7) // 8, 64))
    x = common[np.arange(n) // 8] + 1.5 * rng.standard_normal((n, 64))
    c = np.corrcoef(x)
    np.fill_diagonal(c, 0.0)
    return c


def centred_fc():
    """The shipped mean FC with the diagonal zeroed, the mean of its upper triangle subtracted, and
    the diagonal zeroed again: weights of both signs."""
    from tests import graph_reference as gr
    fc = np.load(os.path.join(gr.DATA, "mean_mat_W_8dic24.npy")).astype(np.float64)
    np.fill_diagonal(fc, 0.0)
    fc = fc - gr.get_uptri(fc).mean()
    np.fill_diagonal(fc, 0.0)
    return fc


def inputs():
    """The five matrices of tests/golden/golden_louvain_sign.npz, by case name."""
    from tests import graph_reference as gr
    base = gr.golden_inputs()
    return {"signed5": base["signed5"], "corr24": grouped_corr(3, 8, 24), "fc_centred": centred_fc(),
            "corr96": grouped_corr(6, 16, 96), "fc_thr": base["fc_thr"]}


def load_golden():
    """tests/golden/golden_louvain_sign.npz as {key: array}, read only."""
    out = {}
    with np.load(GOLDEN) as z:
        for key in z.files:
            a = z[key]
            a.setflags(write=False)
            out[key] = a
    return out

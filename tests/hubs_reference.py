"""Host reference of the hub tests (test_hubs_cpu.py pins it to the golden outputs of the reference's own
rich_club_wu, rich_club_wd, rich_club_bu, rich_club_bd, assortativity_wei, assortativity_bin and
score_wu, test_hubs_gpu.py checks the device against it): a numpy restatement of wc_graph_rich_club,
wc_graph_assortativity and wc_graph_score written from their definitions in include/wcsde.h, of
hubs.rich_club_norm composed with nullmodel_reference, and the test matrices."""
import os

import numpy as np

from tests import nullmodel_reference as nr

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "golden_hubs.npz")
# golden cases of the rich club: values (at least half of the rw levels finite) and NaN patterns only
# (fully connected: every rw level NaN)
RICH_VALUE_CASES = ("fc_thr", "pendant12", "sparse17", "sc", "rand90")
RICH_NAN_CASES = ("fc_dense", "corr24", "fc_centred", "corr96")
RICH_SIGNED_CASES = ("signed5",)               # negative weights in the order; no condition
RICH_DIRECTED_CASES = ("dir24",)
ASSORT_CASES = ("fc_thr", "pendant12", "sparse17", "rand90", "dir24", "corr24", "ring12")
SCORE_CASES = ("fc_thr", "pendant12", "sparse17")
SCORE_FRACTIONS = (0.1, 0.25, 0.4, 0.5)     # of the largest strength


def is_bad(W):
    return not np.isfinite(W).all()


def degrees(W, directed=False):
    """Non-zeros of every column, with directed plus those of every row."""
    nz = np.asarray(W) != 0
    return nz.sum(axis=0) + (nz.sum(axis=1) if directed else 0)


def rich_club(W, directed=False, K=None):
    """{rw, rb, nk, ek, maxdeg} of wc_graph_rich_club for one matrix; K levels (default N, 2 N directed)."""
    W = np.asarray(W, dtype=np.float64)
    n = len(W)
    K = (2 * n if directed else n) if K is None else K
    if is_bad(W):
        nan = np.full(K, np.nan)
        return {"rw": nan, "rb": nan.copy(), "nk": np.full(K, -1), "ek": nan.copy(), "maxdeg": -1}
    deg = degrees(W, directed)
    order = np.sort(W.ravel())[::-1]
    rw, rb, ek = np.full(K, np.nan), np.zeros(K), np.zeros(K)
    nk = np.zeros(K, dtype=np.int64)
    with np.errstate(divide="ignore", invalid="ignore"):
        for k in range(K):
            keep = deg >= k + 1
            if not keep.all():
                sub = W[np.ix_(keep, keep)]
                rw[k] = np.float64(sub.sum()) / np.float64(order[:np.count_nonzero(sub)].sum())
            keep = deg > k + 1
            nk[k] = keep.sum()
            ek[k] = W[np.ix_(keep, keep)].sum()
            rb[k] = np.float64(ek[k]) / (np.float64(nk[k]) * (np.float64(nk[k]) - 1.0))
    return {"rw": rw, "rb": rb, "nk": nk, "ek": ek, "maxdeg": int(deg.max())}


def assortativity_terms(W, flag, weighted):
    """(term1, term2, term3) of wc_graph_assortativity."""
    W = np.asarray(W, dtype=np.float64)
    M = W if weighted else (W != 0).astype(np.float64)
    vin, vout = M.sum(axis=0), M.sum(axis=1)
    i, j = np.nonzero(np.triu(W, 1) > 0) if flag == 0 else np.nonzero(W > 0)
    a = (vout if flag in (1, 3) else vin)[i]
    b = (vout if flag in (2, 3) or (flag == 4 and weighted) else vin)[j]
    E = len(i)
    with np.errstate(divide="ignore", invalid="ignore"):
        term1 = np.float64(np.sum(a * b)) / E
        term2 = np.square(np.float64(np.sum(0.5 * (a + b))) / E)
        term3 = np.float64(np.sum(0.5 * (a * a + b * b))) / E
    return term1, term2, term3


def assortativity(W, flag=0):
    """(r_wei, r_bin) of wc_graph_assortativity for one matrix."""
    if flag not in (0, 1, 2, 3, 4):
        raise ValueError("flag out of range")
    if is_bad(np.asarray(W, dtype=np.float64)):
        return np.nan, np.nan
    out = []
    for weighted in (True, False):
        t1, t2, t3 = assortativity_terms(W, flag, weighted)
        with np.errstate(divide="ignore", invalid="ignore"):
            out.append(float((t1 - t2) / (t3 - t2)))
    return tuple(out)


def column_sums(M):
    """Every column added up in row order 0 .. N-1."""
    s = np.zeros(M.shape[1])
    for row in M:
        s = s + row
    return s


def score(W, s, trace=None):
    """(member, sn, rounds) of wc_graph_score for one matrix and level.  trace, a dict, receives
    "gap": the smallest |str - s| / s over the strengths met during the peel."""
    W = np.asarray(W, dtype=np.float64)
    n = len(W)
    if is_bad(W):
        return np.full(n, -1), -1, -1
    M = W.copy()
    member = np.ones(n, dtype=np.int64)
    rounds, gap = 0, np.inf
    while True:
        st = column_sums(M)
        if s > 0:
            gap = min(gap, float(np.min(np.abs(st - s)) / s))
        peel = (st > 0) & (st < s)
        if not peel.any():
            break
        M[peel, :] = 0.0
        M[:, peel] = 0.0
        member[peel] = 0
        rounds += 1
    if trace is not None:
        trace["gap"] = gap
    return member, int((st > 0).sum()), rounds


def core_matrix(W, member):
    keep = np.asarray(member) == 1
    return np.where(keep[:, None] & keep[None, :], W, 0.0)


def rich_club_norm(W, kind="weighted", reps=8, seeds=None, bin_swaps=5, period=10, negative="bct"):
    """{phi, null_mean, null_std, norm, p} of hubs.rich_club_norm for one matrix, and "gap": per level
    the smallest |null - phi| / max(1, |phi|) over the null models whose value is not exactly phi (a
    comparison null >= phi closer than rounding is not the same everywhere)."""
    W = np.asarray(W, dtype=np.float64)
    n = len(W)
    key = "rw" if kind == "weighted" else "rb"
    bad = is_bad(W)
    if kind == "binary":
        W = (W != 0).astype(np.float64)
    nan = np.full(n, np.nan)
    seeds = range(reps) if seeds is None else seeds
    nulls = np.zeros((reps, n))
    for r, seed in enumerate(seeds):
        if bad:
            break
        if kind == "weighted":
            w0, _, info = nr.null_model(W, int(seed), bin_swaps, period, negative)
        else:
            w0, info = nr.rewire(W, int(seed), bin_swaps)
        bad = bad or info[2] != 0
        if not bad:
            nulls[r] = rich_club(w0)[key]
    if bad:
        return {"phi": nan, "null_mean": nan, "null_std": nan, "norm": nan, "p": nan, "gap": nan}
    phi = rich_club(W)[key]
    with np.errstate(divide="ignore", invalid="ignore"):
        mean, std = nulls.mean(axis=0), nulls.std(axis=0)
        norm = phi / mean
        p = (1.0 + (nulls >= phi[None, :]).sum(axis=0)) / (1.0 + reps)
        d = np.abs(nulls - phi[None, :]) / np.maximum(1.0, np.abs(phi))[None, :]
    d[(nulls == phi[None, :]) | np.isnan(d)] = np.inf
    void = np.isnan(phi) | np.isnan(nulls).any(axis=0)
    out = {"phi": phi, "null_mean": mean, "null_std": std, "norm": norm, "p": p, "gap": d.min(axis=0)}
    for k in ("null_mean", "null_std", "norm", "p", "gap"):
        out[k] = np.where(void, np.nan, out[k])
    return out


# ---- the test matrices ----

def sparse_graph(n, seed=0):
    """Symmetric, non-negative, about a third of the pairs connected, weights in (0, 1], diagonal 0."""
    rng = np.random.default_rng(1000 * n + seed)
    W = np.triu((1.0 - rng.random((n, n))) * (rng.random((n, n)) < 0.35), 1)
    return W + W.T


def signed_graph(n, seed=0):
    """Symmetric, every pair connected, weights in (-1, 1), diagonal 0."""
    rng = np.random.default_rng(2000 * n + seed)
    W = np.triu(rng.uniform(-1.0, 1.0, (n, n)), 1)
    return W + W.T


def directed_graph(n, seed=0):
    """Not symmetric, non-negative, about a third of the ordered pairs connected, diagonal 0."""
    rng = np.random.default_rng(3000 * n + seed)
    W = (1.0 - rng.random((n, n))) * (rng.random((n, n)) < 0.35)
    np.fill_diagonal(W, 0.0)
    return W


def ring(n, width=2):
    """A regular graph: every node tied to its `width` neighbours on either side, weights 1."""
    W = np.zeros((n, n))
    for d in range(1, width + 1):
        W += np.eye(n, k=d) + np.eye(n, k=-d) + np.eye(n, k=n - d) + np.eye(n, k=d - n)
    return (W > 0).astype(np.float64)


def golden_inputs():
    """The matrices of tests/golden/golden_hubs.npz by case name: graph_reference.golden_inputs(),
    nullmodel_reference.inputs(), sparse17 and ring12."""
    from tests import graph_reference as gr
    out = dict(nr.inputs())
    out.update(gr.golden_inputs())
    out["sparse17"] = nr.sparse_nonneg(nr.signed(17))
    out["ring12"] = ring(12)
    return out


def score_levels(W):
    """The s-core levels of a golden case: SCORE_FRACTIONS of the largest strength."""
    top = column_sums(np.asarray(W, dtype=np.float64)).max()
    return [float(f * top) for f in SCORE_FRACTIONS]


def load_golden():
    """tests/golden/golden_hubs.npz as {key: array}, read only."""
    out = {}
    with np.load(GOLDEN) as z:
        for key in z.files:
            a = z[key]
            a.setflags(write=False)
            out[key] = a
    return out

"""Host reference of the null-model tests (test_nullmodel_cpu.py pins it to the golden outputs of the
reference's own randmio_und_signed, null_model_und_sign and participation_coef_norm run under the
engine's draws, test_nullmodel_gpu.py checks the device against it): a numpy restatement of
wc_graph_rewire and wc_graph_null_model written from their definition in include/wcsde.h, and of
nullmodel.participation_norm.  Philox is louvain_reference.philox4x32_10; the rewiring draws, of which
a run takes hundreds of thousands, come from the same function written over numpy arrays."""
import os

import numpy as np

from tests import louvain_reference as lr

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "golden_nullmodel.npz")
QUAD_REWIRE = 0x8000
QUAD_SHUFFLE = 0x4000
MAX_PERIOD = 64
NEGATIVE = ("reference", "bct")
# golden cases: name -> seeds, the reference's mode, bin_swaps 5, period 10
GOLDEN_CASES = (("signed5", 2), ("corr24", 2), ("fc_thr", 2), ("fc_centred", 1))
GOLDEN_REPS = 8          # participation_coef_norm of fc_thr
_M32 = np.uint64(0xFFFFFFFF)


def philox_many(steps, quad, seed):
    """philox4x32_10 of the counters (step, quad, seed) for an array of steps -> uint64 [len][4]."""
    steps = np.asarray(steps, dtype=np.uint64)
    seed = int(seed)
    c0 = steps & _M32
    c1 = ((steps >> np.uint64(32)) << np.uint64(16)) | np.uint64(quad)
    c2 = np.full_like(steps, seed & 0xFFFFFFFF)
    c3 = np.full_like(steps, seed >> 32)
    k0, k1 = lr.PHILOX_KEY
    for _ in range(10):
        p0, p1 = np.uint64(0xD2511F53) * c0, np.uint64(0xCD9E8D57) * c2
        c0, c1, c2, c3 = (p1 >> np.uint64(32)) ^ c1 ^ np.uint64(k0), p1 & _M32, (p0 >> np.uint64(32)) ^ c3 ^ np.uint64(k1), p0 & _M32
        k0, k1 = (k0 + 0x9E3779B9) & 0xFFFFFFFF, (k1 + 0xBB67AE85) & 0xFFFFFFFF
    return np.stack([c0, c1, c2, c3], axis=1)


class Draws:
    """The rewiring draws of one run: draw d -> (a, b, c, d) = (x[k] n) >> 32 of the block
    (d, QUAD_REWIRE, seed)."""
    CHUNK = 4096

    def __init__(self, seed, n):
        self.seed, self.n, self.lo, self.rows = seed, n, 0, []

    def __call__(self, d):
        if not self.lo <= d < self.lo + len(self.rows):
            self.lo = d
            x = philox_many(np.arange(d, d + self.CHUNK, dtype=np.uint64), QUAD_REWIRE, self.seed)
            self.rows = ((x * np.uint64(self.n)) >> np.uint64(32)).tolist()
        return self.rows[d - self.lo]


def attempts(n):
    return int(np.round(n / 2)) + 1


def status_of(W):
    """3 for a NaN or an infinity anywhere, else 2 for w[i][j] != w[j][i] somewhere, else 0."""
    W = np.asarray(W, dtype=np.float64)
    if not np.isfinite(W).all():
        return 3
    return 0 if (W == W.T).all() else 2


def rewire_chain(M, itr, seed):
    """The rewiring of M [n][n] (diagonal 0) in place -> (eff, draws)."""
    n = len(M)
    sg = np.sign(M).astype(np.int8).tolist()
    draw, A = Draws(seed, n), attempts(n)
    d = eff = 0
    for _ in range(itr):
        att = 0
        while att < A:
            a, b, c, e = draw(d)
            d += 1
            if a == b or a == c or a == e or b == c or b == e or c == e:
                continue
            if sg[a][b] == sg[c][e] and sg[a][e] == sg[c][b] and sg[a][b] != sg[a][e]:
                ab, cd, ad, cb = M[a, b], M[c, e], M[a, e], M[c, b]
                M[a, e] = M[e, a] = ab
                M[a, b] = M[b, a] = ad
                M[c, b] = M[b, c] = cd
                M[c, e] = M[e, c] = cb
                for (i, j), v in (((a, e), ab), ((a, b), ad), ((c, b), cd), ((c, e), cb)):
                    sg[i][j] = sg[j][i] = int(np.sign(v))
                eff += 1
                break
            att += 1
    return eff, d


def rewire(W, seed, bin_swaps=5):
    """(wr, info) of wc_graph_rewire for one matrix and seed; info = (eff, draws, status)."""
    W = np.array(W, dtype=np.float64)
    n = len(W)
    st = status_of(W)
    if st:
        return np.full((n, n), np.nan), (0, 0, st)
    np.fill_diagonal(W, 0.0)
    eff, d = rewire_chain(W, bin_swaps * (n * (n - 1) // 2), seed)
    return W, (eff, d & 0xFFFFFFFF, 0)


def shuffle_head(m, k, p, npass, seed):
    """R[0 .. k): the first k values of the Fisher-Yates shuffle of 0 .. m-1 of period p, pass npass."""
    arr = np.arange(m)
    seed = int(seed)
    for q in range(k):
        word = lr.philox4x32_10((p & 0xFFFFFFFF, ((p >> 32) << 16) | (QUAD_SHUFFLE + 0x100 * npass + (q >> 2)),
                                 seed & 0xFFFFFFFF, seed >> 32))[q & 3]
        j = q + ((word * (m - q)) >> 32)
        arr[q], arr[j] = arr[j], arr[q]
    return arr[:k].copy()


def corr(x, y):
    with np.errstate(divide="ignore", invalid="ignore"):
        return float(np.corrcoef(x, y)[0, 1])


def null_model(W, seed, bin_swaps=5, period=10, negative="bct", trace=None):
    """(w0, r, info) of wc_graph_null_model for one matrix and seed: r = (rpos, rneg), info = (eff,
    draws, status).  trace, a dict, receives "ties": the number of sorts in which two live keys were
    exactly equal, and "gap": the smallest relative gap between neighbouring live keys."""
    if negative not in NEGATIVE or not 0 <= period <= MAX_PERIOD:
        raise ValueError("negative or period out of range")
    W = np.array(W, dtype=np.float64)
    n = len(W)
    st = status_of(W)
    nan = np.full((n, n), np.nan)
    if st:
        return nan, (np.nan, np.nan), (0, 0, st)
    np.fill_diagonal(W, 0.0)
    eff = draws = 0
    Wr = W
    if np.count_nonzero(W > 0) < n * (n - 1):
        Wr = W.copy()
        eff, draws = rewire_chain(Wr, bin_swaps * (n * (n - 1) // 2), seed)
    W0 = np.zeros((n, n))
    ties, gap = 0, np.inf
    for npass, sign in enumerate((1, -1)):
        Acur = W > 0 if sign > 0 else W < 0
        Ar = Wr > 0 if sign > 0 else Wr < 0
        src = -W if (npass and negative == "bct") else W
        S = np.sum(src * Acur, axis=0)
        Wv = np.sort(src[np.triu(Acur)])
        Lij = np.flatnonzero(np.triu(Ar))
        P = np.outer(S, S)
        out = -1.0 if npass else 1.0

        def order(live):
            nonlocal ties, gap
            keys = P.flat[live] + 0.0
            o = np.argsort(keys, kind="stable")
            if len(o) > 1:
                ks = keys[o]
                dk = np.diff(ks)
                ties += bool((dk == 0).any())
                with np.errstate(divide="ignore", invalid="ignore"):
                    rel = dk / np.maximum(np.abs(ks[1:]), np.abs(ks[:-1]))
                if np.isfinite(rel).any():
                    gap = min(gap, float(np.nanmin(rel[np.isfinite(rel)])))
            return o

        if period == 0:
            W0.flat[Lij[order(Lij)]] = out * Wv
            continue
        p, m = 0, len(Wv)
        while m > 0:
            k = min(m, period)
            Oind = order(Lij)
            R = shuffle_head(m, k, p, npass, seed)
            for r in R:
                o = Oind[r]
                i, j = divmod(int(Lij[o]), n)
                v = Wv[r]
                if S[i] == 0 or S[j] == 0:
                    return nan, (np.nan, np.nan), (eff, draws & 0xFFFFFFFF, 1)
                W0[i, j] = out * v
                fi, fj = 1 - v / S[i], 1 - v / S[j]
                P[i, :] *= fi
                P[:, i] *= fi
                P[j, :] *= fj
                P[:, j] *= fj
                S[i] -= v
                S[j] -= v
            Lij = np.delete(Lij, Oind[R])
            Wv = np.delete(Wv, R)
            m -= period
            p += 1
    W0 = W0 + W0.T
    r = (corr(np.sum(W * (W > 0), axis=0), np.sum(W0 * (W0 > 0), axis=0)),
         corr(np.sum(-W * (W < 0), axis=0), np.sum(-W0 * (W0 < 0), axis=0)))
    if trace is not None:
        trace["ties"], trace["gap"] = ties, gap
    return W0, r, (eff, draws & 0xFFFFFFFF, 0)


def participation_norm(W, ci, reps=100, seeds=None, bin_swaps=5, period=10, negative="bct"):
    """(mean, std) of nullmodel.participation_norm for one matrix; NaN where a run is refused."""
    W = np.asarray(W, dtype=np.float64)
    n = len(W)
    seeds = range(reps) if seeds is None else seeds
    lab = lr.relabel(ci)
    H = (lab[:, None] == np.arange(lab.max() + 1)[None, :]).astype(np.float64)
    Ko = W.sum(axis=1)
    Km = W @ H
    P = np.zeros((reps, n))
    for k, seed in enumerate(seeds):
        W0, _, info = null_model(W, int(seed), bin_swaps, period, negative)
        if info[2]:
            return np.full(n, np.nan), np.full(n, np.nan)
        with np.errstate(divide="ignore", invalid="ignore"):
            p = 1 - np.sqrt(0.5 * (((Km - W0 @ H) / Ko[:, None]) ** 2).sum(axis=1))
        p[Ko == 0] = 0
        p[p < 0] = 0
        P[k] = p
    return P.mean(axis=0), P.std(axis=0)


# ---- the test matrices ----

def sparse_nonneg(W):
    """A non-negative copy of W: the entries below the median of its strict upper triangle zeroed,
    the rest as magnitudes."""
    W = np.abs(np.asarray(W, dtype=np.float64))
    W = W * (W >= np.median(W[np.triu_indices(len(W), 1)]))
    np.fill_diagonal(W, 0.0)
    return W


def uptri(a):
    a = np.asarray(a)
    iu = np.triu_indices(a.shape[-1], 1)
    return a[..., iu[0], iu[1]]


def from_uptri(v):
    """The symmetric matrix with a zero diagonal of a strict upper triangle, row-major."""
    v = np.asarray(v, dtype=np.float64)
    n = int((1 + np.sqrt(1 + 8 * len(v))) // 2)
    m = np.zeros((n, n))
    m[np.triu_indices(n, 1)] = v
    return m + m.T


def symmetric(W):
    """W with its strict upper triangle mirrored and a zero diagonal: np.corrcoef's matrices differ
    from their transposes in the last bit, which the null model refuses (status 2)."""
    return from_uptri(uptri(W))


def inputs():
    """louvain_sign_reference.inputs(), every matrix made exactly symmetric (symmetric())."""
    from tests import louvain_sign_reference as ls
    return {name: symmetric(W) for name, W in ls.inputs().items()}


def signed(n):
    """louvain_sign_reference.signed_graph(n, n), exactly symmetric."""
    from tests import louvain_sign_reference as ls
    return symmetric(ls.signed_graph(n, n))


def load_golden():
    """tests/golden/golden_nullmodel.npz as {key: array}, read only."""
    out = {}
    with np.load(GOLDEN) as z:
        for key in z.files:
            a = z[key]
            a.setflags(write=False)
            out[key] = a
    return out

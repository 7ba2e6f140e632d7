"""LEiDA restated in numpy, independently of the kernels' algebra (include/wcsde.h holds the contract):
the leading eigenvector of every phase-coherence matrix by np.linalg.eigh of the full N x N matrix plus
Cabral's sign rule, k-means as a plain Lloyd loop, the state statistics as explicit Python loops over runs
and pairs, the symmetrised KL divergence term by term.  closed_form() restates the kernel's 2 x 2 form, for
the CPU test that holds it against eigh and for the constant of test_leida_gpu.py's bound.
"""
import math

import numpy as np

EPS = float(np.finfo(np.float64).eps)


def make_phasors(R, N, seed):
    """Unit phasors [R][N][2]: the even rows' phases uniform on the circle, the odd rows' concentrated
    (sigma = 0.8 rad) about a uniform mean, so that cc > ss and cc < ss and both sign branches occur."""
    rng = np.random.default_rng(seed)
    th = rng.uniform(-np.pi, np.pi, size=(R, N))
    conc = rng.uniform(-np.pi, np.pi, size=(R, 1)) + 0.8 * rng.standard_normal((R, N))
    th[1::2] = conc[1::2]
    return np.stack((np.cos(th), np.sin(th)), axis=-1)


def sign_rule(v):
    """Cabral's rule: most entries negative; a draw is decided by the sum."""
    p = int((v > 0).sum())
    if 2 * p > v.size or (2 * p == v.size and v.sum() > 0):
        return -v
    return v


def eigvec(ph):
    """ph [R][N][2] -> (vec [R][N], share [R], gap [R]) by eigh of dPC = c c^T + s s^T; gap is
    (lambda1 - lambda2) / lambda1.  A row with a NaN or an infinity: NaN; lambda1 = lambda2 exactly: the
    vector NaN, share 0.5 (NaN for an all-zero row)."""
    ph = np.asarray(ph, dtype=np.float64)
    R, N = ph.shape[:2]
    vec, share, gap = np.full((R, N), np.nan), np.full(R, np.nan), np.full(R, np.nan)
    for r in range(R):
        c, s = ph[r, :, 0], ph[r, :, 1]
        if not np.isfinite(ph[r]).all():
            continue
        lam, V = np.linalg.eigh(np.outer(c, c) + np.outer(s, s))
        l1, l2 = lam[-1], lam[-2]
        if l1 == l2:
            share[r] = 0.5 if l1 > 0 else np.nan
            gap[r] = 0.0
            continue
        share[r] = l1 / (l1 + l2)
        gap[r] = (l1 - l2) / l1
        vec[r] = sign_rule(V[:, -1])
    return vec, share, gap


def closed_form(ph):
    """The 2 x 2 Gram form of include/wcsde.h in numpy -> (vec, share); no NaN rules (finite rows only)."""
    ph = np.asarray(ph, dtype=np.float64)
    vec, share = np.empty(ph.shape[:2]), np.empty(ph.shape[0])
    for r in range(ph.shape[0]):
        c, s = ph[r, :, 0], ph[r, :, 1]
        cc, ss, cs = c @ c, s @ s, c @ s
        h = (cc - ss) / 2
        rr = math.hypot(h, cs)
        w = (h + rr, cs) if h >= 0 else (cs, rr - h)
        u = w[0] * c + w[1] * s
        vec[r] = sign_rule(u / np.sqrt(u @ u))
        share[r] = ((cc + ss) / 2 + rr) / (cc + ss)
    return vec, share


def vec_error(got, want):
    """Per row, the largest |got - want| up to sign (min over +-)."""
    got, want = np.asarray(got), np.asarray(want)
    return np.minimum(np.abs(got - want).max(axis=1), np.abs(got + want).max(axis=1))


def distances(x, cent, metric):
    """[R][K] distances; NaN where the row or the centroid cannot be used."""
    x, cent = np.asarray(x, dtype=np.float64), np.asarray(cent, dtype=np.float64)
    D = np.full((x.shape[0], cent.shape[0]), np.nan)
    for r, row in enumerate(x):
        if not np.isfinite(row).all() or (metric == "cosine" and not (row * row).sum() > 0):
            continue
        for k, c in enumerate(cent):
            if not np.isfinite(c).all() or (metric == "cosine" and not (c * c).sum() > 0):
                continue
            if metric == "sqeuclidean":
                D[r, k] = ((row - c) ** 2).sum()
            else:
                D[r, k] = 1.0 - (row * c).sum() / (np.sqrt((row * row).sum()) * np.sqrt((c * c).sum()))
    return D


def assign(x, cent, metric):
    """-> (labels int32 [R], dist [R], D [R][K]): the smallest distance, a tie to the lowest k; -1 / NaN
    where nothing can be chosen."""
    D = distances(x, cent, metric)
    labels, dist = np.full(D.shape[0], -1, dtype=np.int32), np.full(D.shape[0], np.nan)
    for r in range(D.shape[0]):
        for k in range(D.shape[1]):
            if not np.isnan(D[r, k]) and (labels[r] < 0 or D[r, k] < dist[r]):
                labels[r], dist[r] = k, D[r, k]
    return labels, dist, D


def update(x, labels, cent, metric):
    """-> (centroids [K][N], count [K] int64): the mean of the member rows (cosine: divided by their
    norms); an empty cluster keeps its centroid."""
    x, cent = np.asarray(x, dtype=np.float64), np.array(cent, dtype=np.float64)
    count = np.zeros(cent.shape[0], dtype=np.int64)
    for k in range(cent.shape[0]):
        rows = x[np.asarray(labels) == k]
        count[k] = rows.shape[0]
        if count[k]:
            if metric == "cosine":
                rows = rows / np.sqrt((rows * rows).sum(axis=1, keepdims=True))
            cent[k] = rows.mean(axis=0)
    return cent, count


def lloyd(x, init, metric, max_iter=100):
    """-> (centroids, labels, inertia, n_iter): assign; stop if the labels repeat or after max_iter
    updates; else update and assign again."""
    cent, prev, n_iter = np.array(init, dtype=np.float64), None, 0
    while True:
        labels, dist, _ = assign(x, cent, metric)
        if (prev is not None and (labels == prev).all()) or n_iter >= max_iter:
            break
        cent, _ = update(x, labels, cent, metric)
        prev, n_iter = labels, n_iter + 1
    return cent, labels, float(np.nansum(dist)), n_iter


def state_stats(labels, K):
    """labels [M][B] -> (occupancy [B][K], dwell [B][K], trans [B][K][K]); anything but 0 .. K-1 is no state."""
    labels = np.asarray(labels)
    M, B = labels.shape
    occ, dwell, trans = np.full((B, K), np.nan), np.full((B, K), np.nan), np.full((B, K, K), np.nan)
    for b in range(B):
        seq = [int(v) if 0 <= v < K else -1 for v in labels[:, b]]
        n_valid = sum(1 for v in seq if v >= 0)
        runs = [[] for _ in range(K)]                    # the lengths of the maximal runs of each state
        t = 0
        while t < M:
            u = t
            while u + 1 < M and seq[u + 1] == seq[t]:
                u += 1
            if seq[t] >= 0:
                runs[seq[t]].append(u - t + 1)
            t = u + 1
        pairs = [[0] * K for _ in range(K)]
        for t in range(M - 1):
            if seq[t] >= 0 and seq[t + 1] >= 0:
                pairs[seq[t]][seq[t + 1]] += 1
        for k in range(K):
            if n_valid:
                occ[b, k] = sum(1 for v in seq if v == k) / n_valid
            if runs[k]:
                dwell[b, k] = sum(runs[k]) / len(runs[k])
            if sum(pairs[k]):
                trans[b, k] = [pairs[k][j] / sum(pairs[k]) for j in range(K)]
    return occ, dwell, trans


def state_kl(p, q):
    """0.5 (KL(p||q) + KL(q||p)) of one row p against q; 0 log 0 = 0, a zero on one side only: +inf."""
    def kl(a, b):
        tot = 0.0
        for ai, bi in zip(a, b):
            if math.isnan(ai) or math.isnan(bi):
                return math.nan
            if ai > 0:
                tot += math.inf if bi == 0 else ai * (math.log(ai) - math.log(bi))
        return tot
    p, q = [float(v) for v in p], [float(v) for v in q]
    return 0.5 * (kl(p, q) + kl(q, p))


def same(got, want):
    """Exactly equal, NaN in the same places."""
    got, want = np.asarray(got), np.asarray(want)
    return got.shape == want.shape and bool(((got == want) | (np.isnan(got) & np.isnan(want))).all())

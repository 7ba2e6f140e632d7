"""numpy restatement of the dynamic-FC definitions of include/wcsde.h (wc_fcd, wc_fcd_phase) and of
sigchain.fcd_ks, for test_fcd_cpu.py and test_fcd_gpu.py.  Nothing in the reference computes FCD, so
this file, not a golden, is the pin: np.corrcoef per window, an explicit two-pass Pearson between the
stacked patterns (so that the NaN rules are in the open), explicit cosine matrices for the phase form.
"""
import numpy as np


def n_windows(M, W, S):
    return (M - W) // S + 1


def window_patterns(x, W, S):
    """x [M][N] -> [nw][P]: the strict upper triangle, row-major, of np.corrcoef of every window."""
    M, N = x.shape
    iu = np.triu_indices(N, 1)                                   # row-major: utils.flat_FC's order
    out = np.empty((n_windows(M, W, S), len(iu[0])))
    with np.errstate(invalid="ignore", divide="ignore"):
        for k in range(out.shape[0]):
            out[k] = np.corrcoef(x[k * S:k * S + W].T)[iu]       # a constant column: NaN, as numpy
    return out


def pearson_rows(v):
    """[n][P] -> [n][n] Pearson correlation between the rows, two passes; a row with a NaN or without
    variance gives NaN in its row and column, the diagonal included; the diagonal is 1 elsewhere."""
    d = v - v.mean(axis=1, keepdims=True)
    norm = np.sqrt((d * d).sum(axis=1))
    with np.errstate(invalid="ignore", divide="ignore"):
        r = np.clip((d @ d.T) / norm[:, None] / norm[None, :], -1.0, 1.0)
    r = np.triu(r, 1)
    r = r + r.T
    np.fill_diagonal(r, np.where((norm > 0) & np.isfinite(norm), 1.0, np.nan))
    bad = ~((norm > 0) & np.isfinite(norm))
    r[bad, :] = np.nan
    r[:, bad] = np.nan
    return r


def fcd(x, W, S):
    """x [M][N] -> (fcd [nw][nw], patterns [nw][P])."""
    v = window_patterns(x, W, S)
    return pearson_rows(v), v


def fcd_batch(x, W, S):
    """x [M][B][N] -> (fcd [B][nw][nw], patterns [B][nw][P])."""
    both = [fcd(x[:, b], W, S) for b in range(x.shape[1])]
    return np.stack([f for f, _ in both]), np.stack([v for _, v in both])


def fcd_phase(phasor):
    """phasor [M][N][2] -> [M][M]: cosine similarity between the strict upper triangles of the explicit
    matrices d_t[i][j] = cos(theta_i - theta_j) = c_i c_j + s_i s_j."""
    c, s = phasor[..., 0], phasor[..., 1]
    d = c[:, :, None] * c[:, None, :] + s[:, :, None] * s[:, None, :]        # [M][N][N]
    iu = np.triu_indices(phasor.shape[1], 1)
    v = d[:, iu[0], iu[1]]
    norm = np.sqrt((v * v).sum(axis=1))
    with np.errstate(invalid="ignore", divide="ignore"):
        r = np.clip((v @ v.T) / norm[:, None] / norm[None, :], -1.0, 1.0)
    r = np.triu(r, 1)
    r = r + r.T
    ok = (norm > 0) & np.isfinite(norm)
    np.fill_diagonal(r, np.where(ok, 1.0, np.nan))
    r[~ok, :] = np.nan
    r[:, ~ok] = np.nan
    return r


def ks_statistic(a, b):
    """Two-sample Kolmogorov-Smirnov statistic: the largest distance between the empirical distribution
    functions of the 1-D samples a and b (scipy.stats.ks_2samp(a, b).statistic)."""
    a, b = np.sort(np.asarray(a, dtype=np.float64)), np.sort(np.asarray(b, dtype=np.float64))
    pooled = np.concatenate((a, b))
    cdf_a = np.searchsorted(a, pooled, side="right").astype(np.float64) / a.size
    cdf_b = np.searchsorted(b, pooled, side="right").astype(np.float64) / b.size
    return np.abs(cdf_a - cdf_b).max()


def fcd_ks(f, emp, lag=1):
    """KS statistic between the entries f[k][l], l - k >= lag, of one FCD matrix and the sample emp; NaN if
    one of those entries is NaN."""
    a = f[np.triu_indices(f.shape[0], lag)]
    return np.nan if np.isnan(a).any() else ks_statistic(a, emp)


def deviation(got, want):
    """Largest |got - want| over the entries where want is finite; inf if the shapes differ, or if NaN or
    infinite entries are not in the same places with the same values."""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    if got.shape != want.shape:
        return np.inf
    fin = np.isfinite(want)
    if not np.array_equal(np.isnan(got), np.isnan(want)) or not np.array_equal(got[~fin & ~np.isnan(want)],
                                                                               want[~fin & ~np.isnan(want)]):
        return np.inf
    return float(np.abs(got[fin] - want[fin]).max()) if fin.any() else 0.0


def make_input(M, B, N, seed, W=None, S=1):
    """Seeded series [M][B][N]: three shared slow components mixed with per-column weights, independent
    noise, per-column offsets of several standard deviations (BOLD's non-zero means: a one-pass
    covariance would lose digits on them).  With W given, asserts that no window of any simulation has a
    constant column and that every pattern's variance is well away from 0."""
    rng = np.random.default_rng(seed)
    t = np.arange(M)[:, None, None]
    freq = rng.uniform(0.02, 0.12, size=(3, 1, B, 1))
    phase = rng.uniform(0, 2 * np.pi, size=(3, 1, B, 1))
    slow = np.sin(2 * np.pi * freq * t[None] + phase)                        # [3][M][B][1]
    weights = rng.uniform(-1.0, 1.0, size=(3, 1, B, N))
    x = (slow * weights).sum(axis=0) + 0.7 * rng.standard_normal((M, B, N))
    x = x + rng.uniform(3.0, 8.0, size=(1, B, N)) * rng.choice([-1.0, 1.0], size=(1, B, N))
    if W is not None:
        for b in range(B):
            for k in range(n_windows(M, W, S)):
                assert x[k * S:k * S + W, b].std(axis=0).min() > 1e-3
            v = window_patterns(x[:, b], W, S)
            assert np.isfinite(v).all() and v.std(axis=1).min() > 1e-3
    return x

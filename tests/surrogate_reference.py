"""numpy restatement of wc_surrogate_fc and wc_surrogate_test from the definitions in include/wcsde.h,
the Philox phases included, and the inputs of tests/golden/golden_surrogate.npz.

surrogate_fc follows the header's frequency-domain rows; surrogate_fc_time restates the reference's own
loop (fft, the stacked phases, ifft, .real, corrcoef), against which the Parseval identity is tested.
surrogate_test is the per-pair normal fit, p = 1 - Phi(z) and the Benjamini-Hochberg adjustment.
"""
import os

import numpy as np
from scipy import special

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "golden_surrogate.npz")
ALPHA = 0.05
MIN_GAP = 1e-9     # every committed case: |p_adj - alpha| of every pair at least this, so the kept set is determinate
# name: (L, N, S, groups): the shipped shape, the largest N and P, an L that is no power of two with an N
# that is no multiple of 16, a tiny one, and an L = 2 mod 4 (h odd)
CASES = {"tiny": (16, 5, 8, 2), "odd_h": (30, 11, 12, 3), "mid": (100, 24, 20, 3), "wide": (128, 96, 10, 6),
         "shipped": (298, 90, 50, 5)}

PHILOX_KEY = (0x243F6A88, 0x85A308D3)   # WC_PHILOX_KEY0, WC_PHILOX_KEY1 of include/wcsde.h
_M32 = np.uint64(0xFFFFFFFF)


def philox_blocks(c0, c1, c2, c3, key=PHILOX_KEY):
    """Philox4x32-10 on arrays of counter words (louvain_reference.philox4x32_10, vectorised) -> [..., 4]."""
    c0, c1, c2, c3 = (np.asarray(c, dtype=np.uint64) & _M32 for c in np.broadcast_arrays(c0, c1, c2, c3))
    k0, k1 = np.uint64(key[0]), np.uint64(key[1])
    for _ in range(10):
        p0, p1 = np.uint64(0xD2511F53) * c0, np.uint64(0xCD9E8D57) * c2
        c0, c1, c2, c3 = (p1 >> np.uint64(32)) ^ c1 ^ k0, p1 & _M32, (p0 >> np.uint64(32)) ^ c3 ^ k1, p0 & _M32
        k0, k1 = (k0 + np.uint64(0x9E3779B9)) & _M32, (k1 + np.uint64(0xBB67AE85)) & _M32
    return np.stack([c0, c1, c2, c3], axis=-1)


def phase_words(seed, h, N):
    """w [h][N] uint64 (32-bit values): word n & 3 of the block with counter (k, n >> 2, seed lo, seed hi)."""
    seed = int(seed)
    k = np.arange(h, dtype=np.uint64)[:, None]
    quad = np.arange((N + 3) // 4, dtype=np.uint64)[None, :]
    blk = philox_blocks(k & _M32, ((k >> np.uint64(32)) << np.uint64(16)) | quad, seed & 0xFFFFFFFF, seed >> 32)
    return blk.reshape(h, -1)[:, :N]


def phases(seed, h, N):
    """rv [h][N] = 2 pi w 2^-32, the engine's stand-in for np.random.uniform(0, 2 pi, (h, N))."""
    return 2.0 * np.pi * (phase_words(seed, h, N).astype(np.float64) * 2.0 ** -32)


def uptri(m):
    return m[np.triu_indices(m.shape[0], 1)]


def surrogate_fc(y, seeds):
    """sfc [S][P] of y [L][N], L even: the normalised Gram matrix of the rows sqrt(2) Re X(k),
    sqrt(2) Im X(k) (k = 1 .. h - 1) and X(h)."""
    y = np.asarray(y, dtype=np.float64)
    L, N = y.shape
    h = L // 2
    Y = np.fft.fft(y - y.mean(axis=0), axis=0)
    out = np.empty((len(seeds), N * (N - 1) // 2))
    k = np.arange(1, h)
    for s, seed in enumerate(seeds):
        rv = phases(seed, h, N)
        X = Y[k] * (0.5 * (np.exp(1j * rv[k]) + np.exp(-1j * rv[k - 1])))
        A = np.concatenate([np.sqrt(2.0) * X.real, np.sqrt(2.0) * X.imag, (Y[h].real * np.cos(rv[h - 1]))[None, :]])
        G = A.T @ A
        with np.errstate(divide="ignore", invalid="ignore"):
            isd = 1.0 / np.sqrt(np.diag(G))
            out[s] = np.clip(uptri(G * isd[:, None] * isd[None, :]), -1.0, 1.0)
    return out


def surrogate_fc_time(y, seeds):
    """The same by the reference's route: fft, the phases stacked over their own reverse, ifft, .real, corrcoef."""
    y = np.asarray(y, dtype=np.float64)
    L, N = y.shape
    yf = np.fft.fft(y - y.mean(axis=0), axis=0)
    out = np.empty((len(seeds), N * (N - 1) // 2))
    for s, seed in enumerate(seeds):
        rv = phases(seed, L // 2, N)
        sur = np.fft.ifft(yf * np.exp(1j * np.vstack((rv, rv[::-1]))), axis=0).real
        out[s] = uptri(np.corrcoef(sur.T))
    return out


def upper_tail(z):
    """1 - Phi(z), as the reference's 1 - stats.norm.cdf (which is special.ndtr)."""
    return 1.0 - special.ndtr(z)


def benjamini_hochberg(p):
    """Sorted ascending, p_(r) (P / r), the running minimum from the top, at most 1, back in place."""
    p = np.asarray(p, dtype=np.float64)
    P = len(p)
    order = np.argsort(p, kind="stable")
    adj = p[order] * (P / np.arange(1, P + 1))
    adj = np.minimum(np.minimum.accumulate(adj[::-1])[::-1], 1.0)
    out = np.empty(P)
    out[order] = adj
    return out


def recon(v, N):
    m = np.zeros((N, N))
    m[np.triu_indices(N, 1)] = v
    return m + m.T


def surrogate_test(fc, sfc, alpha=ALPHA):
    """fc [N][N], sfc [S][P] -> dict of mu, sd, p [P] and p_adj, fc_adj [N][N]; NaN matrices where a p is not finite."""
    fc, sfc = np.asarray(fc, dtype=np.float64), np.asarray(sfc, dtype=np.float64)
    N = fc.shape[0]
    mu = sfc.sum(axis=0) / sfc.shape[0]
    sd = np.sqrt(((sfc - mu) ** 2).sum(axis=0) / sfc.shape[0])
    with np.errstate(divide="ignore", invalid="ignore"):
        p = np.where(sd > 0.0, upper_tail((uptri(fc) - mu) / sd), np.nan)
    if not np.isfinite(p).all():
        nan = np.full((N, N), np.nan)
        return {"mu": mu, "sd": sd, "p": p, "p_adj": nan, "fc_adj": nan.copy()}
    adj = benjamini_hochberg(p)
    return {"mu": mu, "sd": sd, "p": p, "p_adj": recon(adj, N), "fc_adj": recon(uptri(fc) * (adj < alpha), N)}


def thresholded(y, seeds, alpha=ALPHA):
    """The whole restatement for one series y [L][N]; adds sfc [S][P] and fc [N][N]."""
    y = np.asarray(y, dtype=np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        fc = np.corrcoef(y.T)
    sfc = surrogate_fc(y, seeds)
    return dict(surrogate_test(fc, sfc, alpha), sfc=sfc, fc=fc)


def margins(res, alpha=ALPHA):
    """(smallest |p_adj - alpha| over the pairs, smallest sd) of a result of surrogate_test."""
    return float(np.abs(uptri(res["p_adj"]) - alpha).min()), float(res["sd"].min())


def case_input(name):
    """The series of a committed case: noisy columns in a few groups with a non-zero mean, so that a fair share
    of the pairs is kept and a fair share dropped; float32 values (the file stores them as such) -> y [L][N] fp64."""
    L, N, S, g = CASES[name]
    rng = np.random.default_rng(L + N)
    common = rng.standard_normal((L, g))
    y = common[:, np.arange(N) % g] + rng.standard_normal((L, N)) + 3.0
    return y.astype(np.float32).astype(np.float64)


def case_seeds(name):
    return np.arange(1, CASES[name][2] + 1, dtype=np.uint64)    # the reference's np.random.seed(i + 1)


def load_golden():
    """name -> dict of y, seeds, fc_adj and p_adj [N][N], mu, sd [P], sfc3 [3][P] of the reference's own run."""
    with np.load(GOLDEN) as z:
        out = {}
        for name, (L, N, S, g) in CASES.items():
            out[name] = {"y": z[f"{name}/y"].astype(np.float64), "seeds": z[f"{name}/seeds"],
                         "fc_adj": recon(z[f"{name}/fc_adj_triu"], N), "p_adj": recon(z[f"{name}/p_adj_triu"], N),
                         "mu": z[f"{name}/mu"], "sd": z[f"{name}/sd"], "sfc3": z[f"{name}/sfc3"]}
        return out

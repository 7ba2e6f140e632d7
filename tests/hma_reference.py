"""High-precision reference of the HMA tests (test_hma.py pins the host facade to it, test_hma_gpu.py
the device): seeded input families with structure, and hma_mp, the reference's definitions
(HMA.py:30-203, as restated in nremmodfc_amd/HMA.py) in mpmath arithmetic with mpmath.eigsy in place of
the SVD.

F = (clip(FC) + clip(FC)^T) / 2 is symmetric, so its singular values are |lambda| in descending order
and its singular vectors the eigenvectors up to sign; every output is sign-invariant.  The ordering
and the sign splits are only defined away from ties, so a case is admitted to the golden file
(tests/golden/make_hma_golden.py) only if, on the reference alone, consecutive |lambda| differ by at
least MIN_GAP of the largest and the smallest |u| over the modes used for splitting (u_1 .. u_{N-2})
is at least MIN_U.

Input families, generated unclipped (hma clips):
  zero_diag  uniform (-1, 1), symmetric, zero diagonal: about N / 2 negative eigenvalues after the clip
  signed_fc  np.corrcoef of T = 40 white series: about half the entries negative before the clip
  asym       uniform (-0.5, 1), not symmetric: about N / 2 negative eigenvalues

The golden file holds, per case, the reference's outputs rounded to fp64, the absolute deviation of
the host facade (numpy fp64) from them per output, and a few entries and the sum of the input (a drift
of the generators fails loudly); inputs themselves are not stored.  Tests never call mpmath."""
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "golden_hma_hp.npz")
FAMILIES = ("zero_diag", "signed_fc", "asym")
SIZES = (3, 4, 5, 16, 17, 33, 64, 65, 90, 95, 96)
PER_SIZE = 2
MIN_GAP = 1e-6
MIN_U = 1e-7
FLOAT_OUTPUTS = ("hin", "hse", "hin_node", "hse_node", "sv")
# (family, N, i) -> seed where the default, 100 N + i, does not meet the admission condition: at
# N <= 5 the clip often isolates a node or leaves a path graph (an eigenvector with an exact zero);
# asym/95/0 had |u| = 5.7e-8
SEEDS = {
    ("zero_diag", 3, 0): 346, ("zero_diag", 3, 1): 317, ("zero_diag", 4, 0): 412, ("zero_diag", 4, 1): 419,
    ("zero_diag", 5, 1): 515, ("signed_fc", 3, 0): 324, ("signed_fc", 3, 1): 311, ("signed_fc", 4, 0): 410,
    ("signed_fc", 5, 0): 514, ("signed_fc", 5, 1): 515, ("asym", 95, 0): 9510,
}


def seed_of(family, N, i):
    return SEEDS.get((family, N, i), 100 * N + i)


def make_input(family, N, i):
    """Matrix i of a family at size N, unclipped."""
    rng = np.random.default_rng([FAMILIES.index(family), seed_of(family, N, i)])
    if family == "zero_diag":
        a = rng.uniform(-1.0, 1.0, (N, N))
        a = np.triu(a, 1)
        return a + a.T
    if family == "signed_fc":
        return np.corrcoef(rng.standard_normal((40, N)).T)
    if family == "asym":
        return rng.uniform(-0.5, 1.0, (N, N))
    raise ValueError(family)


def cases():
    """Every (family, N, i) of the golden file, in its order."""
    return [(f, N, i) for f in FAMILIES for N in SIZES for i in range(PER_SIZE)]


def key(family, N, i):
    return f"{family}/{N}/{i}"


def clipped(F):
    """FC[FC < 0] = 0 (HMA.py:55)."""
    return np.where(F < 0, 0.0, F)


def pins(F):
    """What the golden file keeps of an input: its sum and four entries."""
    N = F.shape[0]
    return np.array([F.sum(), F[0, 1], F[1, 0], F[N - 1, N // 2], F[N // 2, N - 1]])


def host_facade(F):
    """The host facade's outputs (numpy fp64 SVD) on a copy of F, as a dict with the device's keys."""
    from nremmodfc_amd import HMA
    f = F.copy()
    cn, cs, _ = HMA.Functional_HP(f)
    hin, hse = HMA.Balance(f, cn, cs)
    hin_n, hse_n = HMA.nodal_measures(f, cn, cs)
    sv = np.linalg.svd((f + f.T) / 2, compute_uv=False)
    return {"hin": np.float64(hin), "hse": np.float64(hse), "hin_node": hin_n, "hse_node": hse_n, "sv": sv,
            "clus_num": np.asarray(cn, dtype=np.int32), "clipped": f}


def hma_mp(F, dps=40):
    """The reference's HMA of F in mpmath arithmetic at dps digits -> (outputs rounded to fp64,
    smallest relative gap between consecutive |lambda|, smallest |u| over the splitting modes)."""
    import mpmath as mp
    N = F.shape[0]
    Fc = clipped(np.asarray(F, dtype=np.float64))
    with mp.workdps(dps):
        A = mp.matrix(N, N)
        for r in range(N):
            for c in range(N):
                A[r, c] = (mp.mpf(float(Fc[r, c])) + mp.mpf(float(Fc[c, r]))) / 2
        E, Q = mp.eigsy(A)
        order = sorted(range(N), key=lambda j: -abs(E[j]))
        s = [abs(E[j]) for j in order]
        U = [[Q[k, j] for k in range(N)] for j in order]  # U[m][k]: component k of mode m
        gap = min(s[m] - s[m + 1] for m in range(N - 1)) / s[0]
        min_u = min(abs(U[m][k]) for m in range(1, N - 1) for k in range(N))
        labels = [0] * N
        clus_num, hf = [], []
        for m in range(N - 1):
            sizes = {}
            for lab in labels:
                sizes[lab] = sizes.get(lab, 0) + 1
            C = len(sizes)
            # p[N-2] is never set by the reference (stays 0)
            p = sum(abs(n - mp.mpf(N) / C) for n in sizes.values()) / N if m < N - 2 else mp.mpf(0)
            hf.append(s[m] ** 2 * C * (1 - p))
            clus_num.append(C)
            if m == N - 2:
                break
            pairs = [(labels[k], U[m + 1][k] >= 0) for k in range(N)]
            ids = {pr: n for n, pr in enumerate(sorted(set(pairs)))}
            labels = [ids[pr] for pr in pairs]
        out = {
            "hin": np.float64(hf[0] / N ** 2),
            "hse": np.float64(mp.fsum(hf[1:]) / N ** 2),
            "hin_node": np.array([float(hf[0] / N * U[0][k] ** 2) for k in range(N)]),
            "hse_node": np.array([float(mp.fsum(hf[m] / N * U[m][k] ** 2 for m in range(1, N - 1)))
                                  for k in range(N)]),
            "sv": np.array([float(x) for x in s]),
            "clus_num": np.array(clus_num, dtype=np.int32),
        }
        return out, float(gap), float(min_u)


def pack(per_case):
    """The golden file's two arrays from {(family, N, i): {name: value}}: per case, in cases() order,
    "floats" holds hin, hse, hin_node [N], hse_node [N], sv [N], the five deviations (FLOAT_OUTPUTS'
    order), the five pins, gap and min_u; "clus_num" holds the N - 1 module counts."""
    fl, cn = [], []
    for c in cases():
        r = per_case[c]
        fl += [np.ravel(r[n]) for n in FLOAT_OUTPUTS] + [np.array([r[f"dev_{n}"] for n in FLOAT_OUTPUTS]),
                                                         np.ravel(r["pins"]), np.array([r["gap"], r["min_u"]])]
        cn.append(np.asarray(r["clus_num"], dtype=np.int32))
    return {"floats": np.concatenate(fl).astype(np.float64), "clus_num": np.concatenate(cn)}


def load_golden():
    """{(family, N, i): {output: reference, "dev_" + output: the host facade's deviation, "pins", "gap",
    "min_u"}} (see pack)."""
    g = np.load(GOLDEN)
    fl, cn = g["floats"], g["clus_num"]
    out, a, b = {}, 0, 0
    for c in cases():
        N = c[1]
        r = {}
        for n, size in (("hin", 1), ("hse", 1), ("hin_node", N), ("hse_node", N), ("sv", N)):
            r[n] = fl[a] if size == 1 else fl[a:a + size]
            a += size
        for n in FLOAT_OUTPUTS:
            r[f"dev_{n}"] = float(fl[a])
            a += 1
        r["pins"] = fl[a:a + 5]
        r["gap"], r["min_u"] = float(fl[a + 5]), float(fl[a + 6])
        a += 7
        r["clus_num"] = cn[b:b + N - 1]
        b += N - 1
        out[c] = r
    assert a == fl.size and b == cn.size
    return out


def bound(ref, name, N, factor):
    """The larger of factor x the host facade's recorded deviation for this case and output and
    N 2^-52 times the output's largest magnitude."""
    return max(factor * ref[f"dev_{name}"], N * 2.0 ** -52 * float(np.abs(ref[name]).max()))


def checked_input(family, N, i, ref):
    """make_input, with the generator's drift checked against the golden file's pins."""
    F = make_input(family, N, i)
    np.testing.assert_array_equal(pins(F), ref["pins"], err_msg=f"{key(family, N, i)}: the input generator drifted")
    return F

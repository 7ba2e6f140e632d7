"""LEiDA on the device (wc_leida_eigvec, wc_kmeans_assign, wc_kmeans_update, wc_state_stats through
sigchain.leida, leida_from_phasors, kmeans_assign, kmeans_update, kmeans, state_stats, leida_states and
utils.leida) against tests/leida_reference.py: np.linalg.eigh of the full N x N phase-coherence matrix, a
plain Lloyd loop, explicit loops over runs and pairs.

Bounds, none of them taken from the device's output:
  eigenvectors  up to sign (min over +-), per row |dv|_inf <= K_EIG eps lambda1 / (lambda1 - lambda2): the
                inverse gap is eigenvector perturbation theory.  The numpy restatement of the closed form
                against eigh stays below 3.4 eps lambda1 / (lambda1 - lambda2) over 21,000 random rows at
                N = 2 .. 96; re-measured on the CPU at N = 130: 1.49 (400 rows), at N = 1000: 1.36 (60 rows).
                Both are below 4, so K_EIG = 16 stands: four times the measured constant, for a different
                summation order and N up to 1000.  Rows with a relative gap below 1e-6 are left out of the
                vector comparison (at most 1 % of the rows; with these inputs none), never of share.
  share         |d| <= 8 eps
  sign          on the device's own rows: 2 p < N, or 2 p = N with sum v <= 0.  The kernel decides a draw by
                the sum in its own order; numpy's order differs from it by at most (N - 1) eps sum |v_i|,
                which is what the assertion allows above 0.
  assign        labels equal on every row whose two smallest reference distances differ by more than 1e-9
                relative (at least 99 % of the rows); dist within 64 eps (sum x^2 + sum c^2) for
                sqeuclidean, 64 eps absolute for cosine
  update        means within 8 eps max |x| log2 R of numpy's (cosine: x the rows divided by their norms);
                counts, kept centroids, repeated calls and workspace sizes exact
  kmeans        labels and n_iter equal, centroids within 1e-12
  statistics    exactly equal, NaN in the same places

Sizes: the eigenvector kernel gives a row 16 lanes up to N = 128 (16 rows a workgroup; 1, 4, 6 or 8 nodes a
lane) and a wave beyond (4 rows a workgroup; 4 or 16 nodes a lane): N = 2, 3, 63 | 64 | 65, 96, 130, 1000;
R = 37, and three workgroups and a row: 49 and 13.  The paths those leave out: N = 17 (2 nodes a lane),
128 | 129 (8 nodes a lane of 16, the step to a wave a row), 300 (8 nodes a lane of 64).
Assign: 64 rows a workgroup, 32 nodes at a time, wave g the centroids g, g + 4, ..: R = 150, N = 3, 64 | 65,
130, K = 1, 2, 5, 32.  Update: 256 rows a partial sum, 64 nodes a wave, 4, 8, 16 or 32 accumulators:
R = 255 | 256 | 259, 769 with K = 3, 5, 12, 32 at N = 65, and N = 130.  Statistics: 256 threads stride
over the times: M = 1, 2, 255 | 256 | 257, 1000.
"""
import functools
import math

import numpy as np
import pytest
import torch

from nremmodfc_amd import _lib, utils
from nremmodfc_amd import sigchain as wsg
from tests import leida_reference as ref

pytestmark = pytest.mark.gpu

EPS = ref.EPS
K_EIG = 16
MIN_GAP = 1e-6
ROWS = 49
METRICS = ("sqeuclidean", "cosine")


def frozen(a):
    a = np.asarray(a)
    a.setflags(write=False)
    return a


def cuda(a, dtype=None):
    return torch.from_numpy(np.array(a, dtype=dtype)).cuda()


@functools.lru_cache(maxsize=None)
def phasors(n):
    return frozen(ref.make_phasors(ROWS, n, 1000 + n))


@functools.lru_cache(maxsize=None)
def eig_reference(n):
    """leida_reference.eigvec of phasors(n), computed once, read only."""
    return tuple(frozen(a) for a in ref.eigvec(phasors(n)))


def device_eig(ph):
    v, s = wsg.leida_from_phasors(cuda(ph))
    return v.cpu().numpy(), s.cpu().numpy()


def check_eig(got, want, tag):
    (gv, gs), (v, share, gap) = got, want
    keep = gap >= MIN_GAP
    assert (~keep).sum() <= 0.01 * len(gap), (tag, gap.min())
    ratio = ref.vec_error(gv[keep], v[keep]) * gap[keep] / EPS
    ds = np.abs(gs - share).max() / EPS
    print(f"{tag}: vectors {ratio.max():.2f} eps / gap (bound {K_EIG}), share {ds:.2f} eps (bound 8), "
          f"smallest gap {gap.min():.1e}")
    assert (ratio <= K_EIG).all(), (tag, ratio.max())
    assert ds <= 8, (tag, ds)
    check_sign(gv, tag)


def check_sign(gv, tag):
    n = gv.shape[1]
    fin = np.isfinite(gv).all(axis=1)
    v = gv[fin]
    p = (v > 0).sum(axis=1)
    slack = (n - 1) * EPS * np.abs(v).sum(axis=1)
    assert ((2 * p < n) | ((2 * p == n) & (v.sum(axis=1) <= slack))).all(), tag


# ---- eigenvectors ----

@pytest.mark.parametrize("rows", [ROWS, 37, 13])
@pytest.mark.parametrize("n", [2, 3, 63, 64, 65, 96, 130, 1000])
def test_eigvec_sizes(n, rows):
    ph = phasors(n)[:rows]
    h = (ph[..., 0] ** 2).sum(axis=1) - (ph[..., 1] ** 2).sum(axis=1)
    assert (h > 0).any() and (h < 0).any()                       # both forms of the 2 x 2 eigenvector
    check_eig(device_eig(ph), tuple(a[:rows] for a in eig_reference(n)), f"N = {n}, R = {rows}")


@pytest.mark.parametrize("n", [17, 128, 129, 300])
def test_eigvec_other_paths(n):
    """2 and 8 nodes a lane of 16, the step from 16 lanes a row to a wave (128 | 129), 8 nodes a lane of 64."""
    check_eig(device_eig(phasors(n)), eig_reference(n), f"N = {n}, R = {ROWS}")


def test_eigvec_rows_do_not_depend_on_the_batch():
    ph = phasors(65)
    whole, part = device_eig(ph), device_eig(ph[9:22])
    assert (whole[0][9:22] == part[0]).all() and (whole[1][9:22] == part[1]).all()
    again = device_eig(ph)
    assert (whole[0] == again[0]).all() and (whole[1] == again[1]).all()


def test_eigvec_degenerate_rows():
    two = np.array(phasors(2)[:6])
    two[1] = [[1.0, 0.0], [0.0, 1.0]]                            # phases exactly pi / 2 apart: lambda1 = lambda2
    two[4] = 0.0                                                 # nothing at all
    v, s = device_eig(two)
    clean = device_eig(phasors(2)[:6])
    assert np.isnan(v[1]).all() and s[1] == 0.5
    assert np.isnan(v[4]).all() and np.isnan(s[4])
    keep = [0, 2, 3, 5]
    assert (v[keep] == clean[0][keep]).all() and (s[keep] == clean[1][keep]).all()
    rv, rs, _ = ref.eigvec(two)
    assert ref.same(np.isnan(v), np.isnan(rv)) and ref.same(s[[1, 4]], rs[[1, 4]])


@pytest.mark.parametrize("n", [3, 65, 130])
def test_eigvec_isolates_nan_and_inf(n):
    ph = np.array(phasors(n))
    ph[5, n - 1, 0] = np.nan
    ph[20, 0, 1] = np.inf
    ph[21, 1, 0] = -np.inf
    v, s = device_eig(ph)
    cv, cs = device_eig(phasors(n))
    bad = np.zeros(ROWS, dtype=bool)
    bad[[5, 20, 21]] = True
    assert np.isnan(v[bad]).all() and np.isnan(s[bad]).all()
    assert (v[~bad] == cv[~bad]).all() and (s[~bad] == cs[~bad]).all()


@pytest.mark.parametrize("n", [2, 65])
def test_eigvec_of_phasors_that_are_not_unit(n):
    check_eig(device_eig(3.0 * phasors(n)), eig_reference(n), f"N = {n}, phasors scaled by 3")


# ---- assign ----

@functools.lru_cache(maxsize=None)
def assign_case(n, k, metric):
    rng = np.random.default_rng(7 * n + k)
    x, cent = frozen(rng.standard_normal((150, n))), frozen(rng.standard_normal((k, n)))
    return x, cent, tuple(frozen(a) for a in ref.assign(x, cent, metric))


def device_assign(x, cent, metric):
    lab, dist = wsg.kmeans_assign(cuda(x), cuda(cent), metric)
    assert lab.dtype == torch.int32
    return lab.cpu().numpy(), dist.cpu().numpy()


@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("k", [1, 2, 5, 32])
@pytest.mark.parametrize("n", [3, 64, 65, 130])
def test_assign_sizes(n, k, metric):
    x, cent, (lab, dist, D) = assign_case(n, k, metric)
    glab, gdist = device_assign(x, cent, metric)
    if k > 1:
        two = np.sort(D, axis=1)[:, :2]
        clear = (two[:, 1] - two[:, 0]) > 1e-9 * np.abs(two[:, 1])
    else:
        clear = np.ones(len(x), dtype=bool)
    assert clear.mean() >= 0.99
    assert (glab[clear] == lab[clear]).all()
    if metric == "sqeuclidean":
        scale = (x * x).sum(axis=1) + (cent[lab] ** 2).sum(axis=1)
    else:
        scale = 1.0
    dev = (np.abs(gdist - dist) / scale).max() / EPS
    print(f"assign N = {n}, K = {k}, {metric}: dist {dev:.2f} eps of the scale (bound 64)")
    assert dev <= 64


@pytest.mark.parametrize("metric", METRICS)
def test_assign_rules(metric):
    rng = np.random.default_rng(11)
    x = rng.standard_normal((70, 9))
    cent = rng.standard_normal((6, 9))
    cent[1] = cent[0]                                            # a tie: always the lower index
    cent[4] = cent[3]
    cent[2, 8] = np.nan                                          # never chosen
    cent[5] = 0.0                                                # no direction: never chosen under cosine
    x[3, 0] = np.nan
    x[65, 8] = np.nan
    x[40] = 0.0                                                  # no direction: no label under cosine
    glab, gdist = device_assign(x, cent, metric)
    lab, dist, _ = ref.assign(x, cent, metric)
    assert (glab == lab).all() and ref.same(np.isnan(gdist), np.isnan(dist))
    assert glab[3] == -1 and glab[65] == -1 and np.isnan(gdist[[3, 65]]).all()
    assert not np.isin(glab, [1, 2, 4]).any()
    if metric == "cosine":
        assert glab[40] == -1 and np.isnan(gdist[40]) and not (glab == 5).any()
        assert (glab == 0).any() and (glab == 3).any()
    else:
        assert glab[40] == 5 and gdist[40] == 0.0
    # x itself as the centroids, each row twice: the distance 0 (cosine: a rounding of it) at the lower index
    twice = np.repeat(x[:5], 2, axis=0)
    twice[0:2], twice[6:8] = x[10], x[11]                        # rows 3 and 40 of x are no centroids
    glab, gdist = device_assign(twice, twice, metric)
    assert (glab == [0, 0, 2, 2, 4, 4, 6, 6, 8, 8]).all() and np.abs(gdist).max() <= 64 * EPS
    # nothing to choose from
    none = np.full((3, 9), np.nan)
    if metric == "cosine":
        none[1] = 0.0
    glab, gdist = device_assign(x, none, metric)
    assert (glab == -1).all() and np.isnan(gdist).all()


# ---- update ----

BLOCK = 256


def update_case(R, n, k, seed):
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((R, n))
    states = np.array([s for s in range(-1, k) if s != 1 or k == 1])    # cluster 1 stays empty
    labels = rng.choice(states, size=R).astype(np.int32)
    x[np.flatnonzero(labels == -1)[0], 2] = np.nan               # a row of nobody's: its NaN reaches no centroid
    prev = rng.standard_normal((k, n))
    return x, labels, prev


@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("R,n,k", [(BLOCK - 1, 65, 3), (BLOCK, 65, 5), (BLOCK + 3, 65, 12), (3 * BLOCK + 1, 65, 32),
                                   (BLOCK + 3, 130, 5), (3 * BLOCK + 1, 3, 2)])
def test_update_sizes(R, n, k, metric):
    assert BLOCK == wsg.KMEANS_UPDATE_BLOCK
    x, labels, prev = update_case(R, n, k, R + n + k)
    want, wcount = ref.update(x, labels, prev, metric)
    args = (cuda(x), cuda(labels), cuda(prev), metric)
    cent, count = wsg.kmeans_update(*args)
    assert count.dtype == torch.int64 and (count.cpu().numpy() == wcount).all()
    got = cent.cpu().numpy()
    data = x[labels >= 0]
    if metric == "cosine":
        data = data / np.sqrt((data * data).sum(axis=1, keepdims=True))
    bound = 8 * EPS * np.abs(data).max() * math.log2(R)
    dev = np.abs(got - want).max()
    print(f"update R = {R}, N = {n}, K = {k}, {metric}: {dev:.1e} (bound {bound:.1e})")
    assert np.isfinite(got).all() and dev <= bound
    if k > 1:
        assert wcount[1] == 0 and (got[1] == prev[1]).all()      # bit for bit
    need = _lib.lib().wc_kmeans_workspace_size(R, n, k, wsg.KMEANS_METRICS[metric])
    large, lcount = wsg.kmeans_update(*args, ws_bytes=16 * need)
    again, _ = wsg.kmeans_update(*args)
    assert torch.equal(large, cent) and torch.equal(again, cent) and torch.equal(lcount, count)
    with pytest.raises(_lib.WCSDEError, match="EWORKSPACE"):
        wsg.kmeans_update(*args, ws_bytes=need - 8)


def test_update_does_not_depend_on_the_rows_of_others():
    """A NaN in a member row reaches its own centroid only."""
    x, labels, prev = update_case(BLOCK + 3, 65, 5, 3)
    clean, _ = wsg.kmeans_update(cuda(x), cuda(labels), cuda(prev), "sqeuclidean")
    r = np.flatnonzero(labels == 3)[0]
    x[r, 64] = np.nan
    got, _ = wsg.kmeans_update(cuda(x), cuda(labels), cuda(prev), "sqeuclidean")
    got, clean = got.cpu().numpy(), clean.cpu().numpy()
    assert np.isnan(got[3, 64])
    got[3, 64] = clean[3, 64]
    assert (got == clean).all()


# ---- kmeans ----

@functools.lru_cache(maxsize=None)
def planted():
    """600 unit vectors around three orthogonal directions, noise 0.05, N = 20."""
    rng = np.random.default_rng(21)
    member = rng.integers(0, 3, 600)
    member[:3] = [0, 1, 2]
    x = 0.05 * rng.standard_normal((600, 20))
    x[np.arange(600), member] += 1.0
    x /= np.sqrt((x * x).sum(axis=1, keepdims=True))
    return frozen(x), frozen(member)


@pytest.mark.parametrize("metric", METRICS)
def test_kmeans_equals_the_reference_lloyd_loop(metric):
    x, member = planted()
    init = x[:3]                                                 # one row of each cluster
    cent, labels, inertia, n_iter = wsg.kmeans(cuda(x), cuda(init), metric)
    wcent, wlabels, winertia, wn = ref.lloyd(x, init, metric)
    assert n_iter == wn and 1 <= n_iter < 100
    assert (labels.cpu().numpy() == wlabels).all() and (wlabels == member).all()
    assert np.abs(cent.cpu().numpy() - wcent).max() <= 1e-12
    assert abs(inertia - winertia) <= 1e-12 * 600
    zero, lab0, _, n0 = wsg.kmeans(cuda(x), cuda(init), metric, max_iter=0)
    assert n0 == 0 and torch.equal(zero, cuda(init)) and (lab0.cpu().numpy() == member).all()


@pytest.mark.parametrize("metric", METRICS)
def test_kmeans_with_an_integer_k(metric):
    x, _ = planted()
    xd = cuda(x).view(20, 30, 20)                                # pooled over (time, simulation)
    one = wsg.kmeans(xd, 3, metric, seed=4)
    same = wsg.kmeans(xd, 3, metric, seed=4)
    assert torch.equal(one[0], same[0]) and torch.equal(one[1], same[1]) and one[2:] == same[2:]
    assert one[0].shape == (3, 20) and one[1].shape == (20, 30) and one[1].dtype == torch.int32
    four = wsg.kmeans(xd, 3, metric, n_init=4, seed=4)
    assert four[2] <= one[2]
    with pytest.raises(ValueError, match="fewer than k"):
        wsg.kmeans(torch.full((2, 5), float("nan"), dtype=torch.float64, device="cuda"), 3)


# ---- state statistics ----

def device_stats(labels, k):
    res = wsg.state_stats(cuda(labels, np.int32), k)
    return tuple(res[n].cpu().numpy() for n in ("occupancy", "dwell", "trans"))


@pytest.mark.parametrize("M", [1, 2, 255, 256, 257, 1000])
def test_state_stats_sizes(M):
    rng = np.random.default_rng(M)
    labels = rng.integers(0, 4, (M, 3)).astype(np.int32)
    labels[:, 0] = np.repeat(labels[:(M + 1) // 2, 0], 2)[:M]    # runs longer than 1
    labels[rng.random(M) < 0.2, 1] = -1
    labels[:, 2] = -1
    got, want = device_stats(labels, 4), ref.state_stats(labels, 4)
    for g, w, name in zip(got, want, ("occupancy", "dwell", "trans")):
        assert ref.same(g, w), name
    assert np.isnan(got[0][2]).all() and np.isnan(got[1][2]).all() and np.isnan(got[2][2]).all()


def test_state_stats_hand_case():
    hand = np.array([0, 0, 1, -1, 1, 1, 0], dtype=np.int32)
    nan = math.nan
    occ, dwell, trans = (r[0] for r in device_stats(hand[:, None], 3))
    assert ref.same(occ, [3 / 6, 3 / 6, 0.0]) and ref.same(dwell, [3 / 2, 3 / 2, nan])
    assert ref.same(trans, [[1 / 2, 1 / 2, 0.0], [1 / 2, 1 / 2, 0.0], [nan, nan, nan]])
    single = wsg.state_stats(cuda(hand), 3)                      # 1-D labels: no leading axis
    assert single["occupancy"].shape == (3,) and single["trans"].shape == (3, 3)
    assert ref.same(single["dwell"].cpu().numpy(), dwell)
    # a label that is no state counts as -1 (include/wcsde.h)
    odd = hand.copy()
    odd[3] = 3
    for g, w in zip(device_stats(odd[:, None], 3), (occ, dwell, trans)):
        assert ref.same(g[0], w)
    odd[3] = -9
    assert ref.same(device_stats(odd[:, None], 3)[2][0], trans)


# ---- end to end ----

@functools.lru_cache(maxsize=None)
def series():
    """[300][3][10]: a slow oscillation a node with its own phase drift, a little noise."""
    rng = np.random.default_rng(33)
    t = np.arange(300.0)[:, None, None]
    f = 0.05 + 0.01 * rng.standard_normal((1, 3, 10))
    x = np.sin(2 * np.pi * f * t + rng.uniform(0, 2 * np.pi, (1, 3, 10))) + 0.05 * rng.standard_normal((300, 3, 10))
    return frozen(x)


def test_leida_from_a_series():
    x = cuda(series())
    trim = 10
    vec, share = wsg.leida(x, trim)
    assert vec.shape == (280, 3, 10) and share.shape == (280, 3)
    ph = wsg.hilbert_phase(x.reshape(300, 30))[trim:290].view(280, 3, 10, 2)
    v2, s2 = wsg.leida_from_phasors(ph)
    assert torch.equal(vec, v2) and torch.equal(share, s2)
    want = ref.eigvec(ph.cpu().numpy().reshape(840, 10, 2))
    check_eig((vec.cpu().numpy().reshape(840, 10), share.cpu().numpy().reshape(840)), want, "leida [300][3][10]")
    one, sone = wsg.leida(x[:, 1].contiguous(), trim)            # a single simulation: [M][C]
    assert one.shape == (280, 10) and sone.shape == (280,)
    assert ref.vec_error(one.cpu().numpy(), vec[:, 1].cpu().numpy()).max() <= 1e-9
    assert (sone - share[:, 1]).abs().max() <= 1e-12


def test_utils_leida():
    x = series()
    dt, freqs, trim = 2.0, [0.03, 0.07], 10
    xd = cuda(x)
    (bb, ba), _ = wsg.envelope_filters(dt, freqs[0], freqs[1], None)
    vec, share = wsg.leida(wsg.filtfilt(bb, ba, xd), trim)
    cent, _, _, _ = wsg.kmeans(vec, 3, seed=1)
    states = wsg.leida_states(vec, cent)
    assert states["labels"].shape == (280, 3) and states["trans"].shape == (3, 3, 3)
    res = utils.leida(x, dt, freqs, centroids=cent.cpu().numpy(), trim=trim)
    assert sorted(res) == ["dwell", "labels", "occupancy", "share", "trans", "vec"]
    assert (res["vec"] == vec.cpu().numpy()).all() and (res["share"] == share.cpu().numpy()).all()
    for name in ("labels", "occupancy", "dwell", "trans"):
        assert ref.same(res[name], states[name].cpu().numpy()), name
    assert np.abs(res["occupancy"].sum(axis=1) - 1).max() <= 4 * EPS
    want = ref.state_stats(res["labels"], 3)
    assert ref.same(res["occupancy"], want[0]) and ref.same(res["dwell"], want[1]) and ref.same(res["trans"], want[2])
    kl = wsg.state_kl(states["occupancy"], res["occupancy"][0])
    assert kl.shape == (3,) and float(kl[0]) == 0.0 and bool((kl >= 0).all())
    # float32 in; an integer k clusters first; a single simulation
    f32 = utils.leida(x.astype(np.float32), dt, freqs, k=3, trim=trim, metric="sqeuclidean")
    assert f32["vec"].dtype == np.float64 and f32["centroids"].shape == (3, 10) and f32["n_iter"] >= 1
    assert f32["occupancy"].shape == (3, 3) and f32["inertia"] >= 0
    solo = utils.leida(x[:, 0], dt, None, centroids=cent.cpu().numpy())
    assert solo["vec"].shape == (300, 10) and solo["labels"].shape == (300,) and solo["trans"].shape == (3, 3)

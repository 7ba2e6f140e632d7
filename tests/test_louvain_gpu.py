"""Louvain and agreement on the device (wc_graph_louvain and wc_graph_agreement through
sigchain.graph_louvain, graph_agreement, graph_consensus_matrix and the graph_utils facades) against
tests/louvain_reference.py, the numpy restatement that test_louvain_cpu.py pins to the reference's own
outputs, and against those outputs directly (tests/golden/golden_louvain.npz).

Bounds.  ci: exactly equal.  q: |got - want| <= 1e-12 max(1, |want|)
(centrality_reference.deviation_abs).  Every compared run asserts the restatement's decision margin
>= 1e-9 (louvain_reference.louvain): the device sums in another order than numpy, to 1e-16.
Agreement: exactly equal, the counts are integers.

N: 2 and 3, 16 and 17, 64 and 65 (a lane's second module begins at 65), 90, and 96 dense (the limit).
Committed runs and their margins: test_louvain_cpu.py's header.

Measured on MI355X, largest over the runs of a test (each is printed before it is asserted):
  ci exactly equal everywhere; q: sizes 2.2e-16 (N = 3: one module, q is 0 to rounding; 6.9e-17
  elsewhere), golden runs 6.9e-17, B = 5 batch 1.1e-16, gamma 5.6e-17,
  ci0 2.8e-17, potts and the symmetric custom objective 0, dir24 5.6e-17, composition 5.6e-17;
  wc_graph_modules' Q against q 2.2e-16 at most.  Local optimum (check_optimum, on every device result
  with a symmetric objective outside the agreement and facade tests): module-level gain 0 on all 93 runs,
  node-level gain 0 on the 9 of them known to end at the node level.  dir24 at gamma 1.3: all nine runs end
  in the sweep guard, as the reference and the restatement do; same bits alone, in a batch and again.
  Agreement exact.
"""
import functools
import warnings

import numpy as np
import pytest
import torch

from nremmodfc_amd import graph_utils as gu
from nremmodfc_amd import sigchain as wsg
from tests import centrality_reference as cref
from tests import graph_reference as ref
from tests import louvain_reference as lref
from tests.test_graph_gpu import SIZES, frozen, graph
from tests.test_louvain_cpu import runs

pytestmark = pytest.mark.gpu

BOUND = 1e-12
DENSITIES = (0.1, 0.3, 0.5, 0.8, 1.0)


@functools.lru_cache(maxsize=None)
def inputs():
    return {k: frozen(v) for k, v in ref.golden_inputs().items()}


@functools.lru_cache(maxsize=None)
def golden():
    return lref.load_golden()


@functools.lru_cache(maxsize=None)
def host(n, density, gseed, seed, gamma=1.0, kind="modularity"):
    """louvain_reference.louvain of graph(n, density, gseed), computed once; the margin asserted."""
    w = graph(n, density, gseed)
    w = (np.asarray(w) != 0).astype(np.float64) if kind == "potts" else w
    ci, q, info, margin = lref.louvain(*lref.objective(w, gamma, kind), seed)
    assert margin >= lref.MIN_MARGIN, (n, density, gseed, seed, margin)
    return frozen(ci), q, info


def cuda(a, dtype=None):
    return torch.from_numpy(np.array(a, dtype=dtype)).cuda()


def device(w, seeds=0, **kw):
    if kw.get("ci") is not None:
        kw["ci"] = cuda(kw["ci"])
    return tuple(t.cpu().numpy() for t in wsg.graph_louvain(cuda(w), seeds=seeds, **kw))


def check(got_ci, got_q, want_ci, want_q, tag):
    dev = cref.deviation_abs(got_q, want_q)
    print(f"{tag}: q {dev:.1e}  modules {int(np.max(want_ci)) + 1}")
    np.testing.assert_array_equal(got_ci, want_ci)
    assert dev <= BOUND, (tag, dev)


def check_optimum(obj, ci, levels=None, tag=""):
    """No single move gains more than 1e-10 at a partition the device returned.  Where the run ended
    after the level that follows the node level (levels == 2: the pooled graph did not move) the
    partition is the node level's own and the moves are those of single nodes, into another module or
    an empty one.  Deeper runs merge whole modules afterwards, after which a single node may gain again
    (Louvain promises nothing there; on the host such gains reach 0.7): for every run the same is
    checked on the pooled graph, where every module is a node.  For a symmetric obj only: the pooled
    graph of a directed one is mirrored at every level and is no function of the final partition.
    Returns (module-level gain, node-level gain or None)."""
    obj = np.asarray(obj)
    if not np.allclose(obj, obj.T, rtol=0.0, atol=1e-12):
        return None, None
    K = int(np.max(ci)) + 1
    pooled = np.array([[obj[np.ix_(ci == i, ci == j)].sum() for j in range(K)] for i in range(K)])
    gain = lref.local_gain(pooled, np.arange(K))
    node = lref.local_gain(obj, ci) if levels == 2 else None
    print(f"{tag}: levels {levels}, module-level gain {gain:.2e}, node-level gain {node}")
    assert gain <= lref.TOL + 1e-12, (tag, gain)
    assert node is None or node <= lref.TOL + 1e-12, (tag, node)
    return gain, node


def check_settled(w, ci, q, gamma=1.0, tag="", levels=None):
    """wc_graph_modules' Q of the partition is the q returned, which ties the new kernel to the
    existing one, and check_optimum on the modularity objective of w."""
    check_optimum(lref.objective(w, gamma)[0], ci, levels, tag)
    mod = wsg.graph_module_measures(cuda(w), cuda(ci, np.int32), "modularity", gamma=gamma)["modularity"].cpu().numpy()
    dev = cref.deviation_abs(mod, q)
    print(f"{tag}: modules kernel Q against q {dev:.1e}")
    assert dev <= BOUND


# ---- sizes ----

@pytest.mark.parametrize("n", list(SIZES))
def test_sizes(n):
    w = graph(n, SIZES[n], n)
    ci, q, info = device(w[None], seeds=[0, 1], want_info=True)
    assert ci.shape == (1, 2, n) and ci.dtype == np.int32 and q.shape == (1, 2) and info.shape == (1, 2, 2)
    for k, seed in enumerate((0, 1)):
        want_ci, want_q, want_info = host(n, SIZES[n], n, seed)
        check(ci[0, k], q[0, k], want_ci, want_q, f"N={n} seed {seed}")
        assert tuple(info[0, k]) == want_info
        check_settled(w, ci[0, k], q[0, k], tag=f"N={n} seed {seed}", levels=info[0, k, 0])
    one_ci, one_q = device(w, seeds=1)                           # [N][N] and an int: no batch axis, no R axis
    assert one_ci.shape == (n,) and one_q.shape == ()
    np.testing.assert_array_equal(one_ci, ci[0, 1])
    assert one_q == q[0, 1]


# ---- golden ----

@pytest.mark.parametrize("case", lref.CASES)
def test_golden_runs(case):
    """The reference's own community_louvain under the engine's order, every committed run."""
    w = inputs()[case]
    for gamma, seed, ci0, want_ci, want_q, margin in runs(case):
        assert margin >= lref.MIN_MARGIN
        ci, q = device(w, seeds=seed, gamma=gamma, ci=ci0)
        check(ci + 1, q, want_ci, want_q, f"{case} gamma {gamma} seed {seed}{'' if ci0 is None else ' hemi'}")
    seeds = golden()[f"{case}/seeds"].tolist()
    ci, q = device(w, seeds=seeds)                               # the eight gamma-1 runs in one launch
    np.testing.assert_array_equal(ci + 1, golden()[f"{case}/ci"])
    D = wsg.graph_agreement(cuda(ci)).cpu().numpy()
    np.testing.assert_array_equal(D, golden()[f"{case}/agreement"])
    for k in range(len(seeds)):
        check_settled(w, ci[k], q[k], tag=f"{case} seed {seeds[k]}")


# ---- batch independence ----

def test_batch_of_five_matrices_and_three_seeds():
    ws = np.stack([graph(65, d, 100 + k) for k, d in enumerate(DENSITIES)])
    seeds = [5, 0, 9]
    ci, q, info = device(ws, seeds=seeds, want_info=True)
    assert ci.shape == (5, 3, 65)
    for b in range(5):
        for r, seed in enumerate(seeds):
            one = device(ws[b], seeds=seed, want_info=True)
            np.testing.assert_array_equal(one[0], ci[b, r])
            assert one[1].tobytes() == q[b, r].tobytes()         # bit for bit
            np.testing.assert_array_equal(one[2], info[b, r])
            check_settled(ws[b], ci[b, r], q[b, r], tag=f"B=5 matrix {b} seed {seed}", levels=info[b, r, 0])
    again = device(ws, seeds=seeds, want_info=True)
    for a, b in zip(again, (ci, q, info)):
        assert a.tobytes() == b.tobytes()
    perm = [2, 0, 1]
    moved = device(ws, seeds=[seeds[p] for p in perm], want_info=True)
    for a, b in zip(moved, (ci, q, info)):
        assert a.tobytes() == np.ascontiguousarray(b[:, perm]).tobytes()
    for b, d in enumerate(DENSITIES):
        want_ci, want_q, _ = host(65, d, 100 + b, 0)
        check(ci[b, 1], q[b, 1], want_ci, want_q, f"B=5 matrix {b}")


# ---- by hand ----

def two_cliques():
    w = np.zeros((8, 8))
    w[:4, :4] = w[4:, 4:] = 1.0
    np.fill_diagonal(w, 0.0)
    w[3, 4] = w[4, 3] = 1.0
    return w


def test_two_cliques_give_two_modules_for_every_seed():
    ci, q = device(two_cliques(), seeds=list(range(16)))
    for k in range(16):
        assert len(set(ci[k, :4])) == 1 and len(set(ci[k, 4:])) == 1 and ci[k, 0] != ci[k, 4], (k, ci[k])
    assert cref.deviation_abs(q, np.full(16, cref.modularity(two_cliques(), [0] * 4 + [1] * 4))) <= BOUND


def test_no_edges_at_all():
    """s = 0.  Under "modularity" obj is 0 / 0: the engine's non-finite convention, ci = -1 and q = NaN
    (the reference returns the starting singletons with q = NaN).  Under "potts" obj is finite: what
    the reference gives, the singletons and q = -inf, no level run."""
    empty = np.zeros((5, 5))
    ci, q = device(empty)
    assert (ci == -1).all() and np.isnan(q)
    ci, q, info = device(empty, objective="potts", want_info=True)
    want_ci, want_q, want_info = lref.louvain(*lref.objective(empty, 1.0, "potts"), 0)[:3]
    assert ci.tolist() == want_ci.tolist() == [0, 1, 2, 3, 4] and q == want_q == -np.inf and tuple(info) == want_info


def test_starting_partition_with_arbitrary_labels():
    w = graph(17, 0.5, 17)
    labels = 10 * cref.partition("mod4", 17) - 7                 # -7, 3, 13, 23: np.unique orders them
    want_ci, want_q, _, margin = lref.louvain(*lref.objective(w), 2, labels)
    assert margin >= lref.MIN_MARGIN
    ci, q = device(w, seeds=2, ci=labels)
    check(ci, q, want_ci, want_q, "ci0 arbitrary labels")
    check_settled(w, ci, q, tag="ci0 arbitrary labels")
    stack = np.stack([w, graph(17, 0.5, 19)])
    cis = np.stack([labels, cref.partition("hemi", 17)])
    ci2, q2 = device(stack, seeds=2, ci=cis)                     # [B][N] starting labels
    np.testing.assert_array_equal(ci2[0], ci)
    want = lref.louvain(*lref.objective(stack[1]), 2, cis[1])
    assert want[3] >= lref.MIN_MARGIN
    check(ci2[1], q2[1], want[0], want[1], "ci0 per matrix")
    check_settled(stack[1], ci2[1], q2[1], tag="ci0 per matrix")


@pytest.mark.parametrize("gamma", lref.GAMMAS)
def test_gamma(gamma):
    want_ci, want_q, _ = host(65, 0.3, 65, 0, gamma)
    ci, q = device(graph(65, 0.3, 65), gamma=gamma)
    check(ci, q, want_ci, want_q, f"gamma {gamma}")
    check_settled(graph(65, 0.3, 65), ci, q, gamma, f"gamma {gamma}")


def test_potts_on_a_binary_graph():
    a = (np.asarray(graph(17, 0.5, 17)) != 0).astype(np.float64)
    want_ci, want_q, _ = host(17, 0.5, 17, 0, 1.0, "potts")
    ci, q = device(a, objective="potts")
    check(ci, q, want_ci, want_q, "potts")
    check_optimum(lref.objective(a, 1.0, "potts")[0], ci, tag="potts")
    with pytest.raises(ValueError, match="binary"):
        device(graph(17, 0.5, 17), objective="potts")


def test_custom_objectives():
    w = graph(17, 0.5, 17)
    sym = lref.objective(w, 0.9)[0]
    want = lref.louvain(sym, w.sum(), 1)
    assert want[3] >= lref.MIN_MARGIN
    with warnings.catch_warnings():
        warnings.simplefilter("error")                           # symmetric: no warning
        ci, q = device(w, seeds=1, objective=cuda(sym))
    check(ci, q, want[0], want[1], "custom symmetric")
    check_optimum(sym, ci, tag="custom symmetric")
    rng = np.random.default_rng(3)
    skew = sym + rng.uniform(-0.01, 0.01, sym.shape)
    obj, s = lref.objective(w, 1.0, skew)
    assert np.array_equal(obj, obj.T) and not np.allclose(skew, skew.T)
    want = lref.louvain(obj, s, 1)
    assert want[3] >= lref.MIN_MARGIN
    with pytest.warns(UserWarning, match="not symmetric"):
        ci, q = device(w, seeds=1, objective=cuda(skew))
    check(ci, q, want[0], want[1], "custom, symmetrised")
    check_optimum(obj, ci, tag="custom, symmetrised")


def test_directed():
    w = inputs()["dir24"]
    assert not np.array_equal(w, w.T)
    for gamma, seed, ci0, want_ci, want_q, _ in runs("dir24")[:3]:
        ci, q = device(w, seeds=seed)
        check(ci + 1, q, want_ci, want_q, f"dir24 seed {seed}")


def test_directed_above_gamma_one():
    """dir24 at gamma 1.3 has no expected partition: the reference itself raises there (its 1000-sweep
    guard, under numpy's order and under the engine's), the restatement runs into the same guard, and
    on the way nodes choose between emptied modules whose Hnm holds rounding residues of 1e-17, so the
    device, which sums in another order, may legitimately take other turns.  What holds whatever turns
    it takes: a run either ends in the guard (ci = -1, q = NaN, 1000 sweeps or more) or returns dense
    labels whose Q, by wc_graph_modules, is the q returned; every (matrix, seed) gives the same bits
    alone, in a batch and in a second call."""
    w = np.array(inputs()["dir24"])
    assert np.isnan(lref.louvain(*lref.objective(w, 1.3), 0)[1])
    ws = np.stack([w, w.T, w * w])
    seeds = [0, 1, 5]
    ci, q, info = device(ws, seeds=seeds, gamma=1.3, want_info=True)
    for a, b in zip(device(ws, seeds=seeds, gamma=1.3, want_info=True), (ci, q, info)):
        assert a.tobytes() == b.tobytes()
    unsettled = 0
    for b in range(3):
        for r, seed in enumerate(seeds):
            one = device(ws[b], seeds=seed, gamma=1.3, want_info=True)
            for x, y in zip(one, (ci[b, r], q[b, r], info[b, r])):
                assert x.tobytes() == y.tobytes()                # bit for bit, NaN included
            if ci[b, r, 0] < 0:
                unsettled += 1
                assert (ci[b, r] == -1).all() and np.isnan(q[b, r]) and info[b, r, 1] >= lref.SWEEP_GUARD
            else:
                assert sorted(set(ci[b, r].tolist())) == list(range(ci[b, r].max() + 1))
                check_settled(ws[b], ci[b, r], q[b, r], 1.3, f"directed gamma 1.3, matrix {b} seed {seed}")
    print(f"directed gamma 1.3: {unsettled} of 9 runs end in the sweep guard")


# ---- the local optimum ----

def test_local_optimum():
    """check_optimum on four seeds at three sizes, and that both of its branches are met: runs that end
    at the node level (no single node gains) and deeper ones (no single module gains)."""
    seen = {True: 0, False: 0}
    for n in (17, 65, 96):
        w = graph(n, SIZES[n], n)
        obj, _ = lref.objective(w)
        ci, q, info = device(w, seeds=list(range(4)), want_info=True)
        for k in range(4):
            gain, node = check_optimum(obj, ci[k], info[k, 0], f"N={n} seed {k}")
            assert gain is not None
            seen[node is not None] += 1
    print("runs final at the node level:", seen[True], "deeper:", seen[False])
    assert seen[True] and seen[False]


# ---- non-finite and refused ----

def test_nan_spoils_its_matrix_only_and_a_negative_weight_raises():
    ws = np.stack([graph(17, 0.5, 17), graph(17, 0.5, 19), graph(17, 0.3, 18)])
    clean = device(ws, seeds=[0, 1])
    assert (clean[0] >= 0).all() and np.isfinite(clean[1]).all()
    for value, k in ((np.nan, 1), (np.inf, 2), (np.nan, 0)):
        bad = np.array(ws)
        bad[k, 3, 5] = value
        ci, q = device(bad, seeds=[0, 1])
        assert (ci[k] == -1).all() and np.isnan(q[k]).all()
        others = [j for j in range(3) if j != k]
        assert ci[others].tobytes() == clean[0][others].tobytes() and q[others].tobytes() == clean[1][others].tobytes()
        D = wsg.graph_agreement(cuda(ci)).cpu().numpy()
        assert np.isnan(D[k]).all() and np.isfinite(D[others]).all()
    bad = np.array(ws)
    bad[1, 3, 5] = -0.25
    with pytest.raises(ValueError, match="negative weights"):
        device(bad)
    with pytest.raises(ValueError, match="negative weights"):
        gu.community_louvain(np.array(inputs()["signed5"]), seed=0)


# ---- agreement ----

@pytest.mark.parametrize("n,R", [(17, 1), (65, 7), (96, 100), (17, 100), (96, 1)])
def test_agreement_of_random_partitions(n, R):
    rng = np.random.default_rng(n + R)
    ci = rng.integers(0, 6, (3, R, n)).astype(np.int32)
    D = wsg.graph_agreement(cuda(ci)).cpu().numpy()
    for b in range(3):
        np.testing.assert_array_equal(D[b], lref.agreement(ci[b]))
    np.testing.assert_array_equal(wsg.graph_agreement(cuda(ci[1])).cpu().numpy(), D[1])
    bad = np.array(ci)
    bad[1, R // 2, n - 1] = -1
    Db = wsg.graph_agreement(cuda(bad)).cpu().numpy()
    assert np.isnan(Db[1]).all()
    np.testing.assert_array_equal(Db[[0, 2]], D[[0, 2]])


def test_consensus_matrix():
    w, tau = inputs()["fc_thr"], 0.4
    obj, s = lref.objective(w)
    parts = []
    for seed in range(16):
        ci, _, _, margin = lref.louvain(obj, s, seed)
        assert margin >= lref.MIN_MARGIN
        parts.append(ci)
    parts = np.array(parts)
    assert not (lref.agreement(parts) / 16 == tau).any()         # k / 16 is never 0.4
    got = wsg.graph_consensus_matrix(cuda(w), reps=16, tau=tau).cpu().numpy()
    np.testing.assert_array_equal(got, lref.consensus(parts, tau))
    assert (got == 0).any() and (got >= tau).any() and (np.diag(got) == 0).all()
    np.testing.assert_array_equal(gu.get_agreement_matrix(np.array(w), reps=16, tau=tau), got)
    np.testing.assert_array_equal(gu.get_agreement_matrix(np.array(w), reps=16, tau=tau, seeds=np.arange(16)), got)


# ---- facades and composition ----

def test_facades():
    W = np.array(inputs()["sc"])
    ci, q = gu.community_louvain(W, seed=3)
    np.testing.assert_array_equal(ci, golden()["sc/ci"][3])
    assert isinstance(q, float) and abs(q - golden()["sc/q"][3]) <= BOUND and ci.min() == 1
    assert (W == inputs()["sc"]).all()                           # the caller's matrix is left alone
    stack = np.stack([inputs()[c] for c in ("sc", "fc_thr", "rand90")])
    cs, qs = gu.community_louvain(stack, seed=3)
    for k in range(3):
        one = gu.community_louvain(stack[k], seed=3)
        np.testing.assert_array_equal(cs[k], one[0])
        assert qs[k] == one[1]
    D = gu.agreement(np.array(golden()["sc/ci"]).T)              # [N, M], the reference's orientation
    np.testing.assert_array_equal(D, golden()["sc/agreement"])
    a, b = gu.community_louvain(W), gu.community_louvain(W)      # seed=None: a fresh seed each time, both valid
    assert a[0].min() == 1 and b[0].min() == 1 and 0.45 < min(a[1], b[1])


def test_composes_with_fc_metrics():
    rng = np.random.default_rng(11)
    B, N, M = 3, 17, 64
    bold = torch.from_numpy(rng.standard_normal((M, B * N))).cuda()
    fc, _, _ = wsg.fc_metrics(bold, B, N, kuramoto=False, want_fc=True)
    fc.clamp_(min=0.0)
    fc.diagonal(dim1=1, dim2=2).zero_()
    ci, q = wsg.graph_louvain(fc, seeds=4)
    mod = wsg.graph_module_measures(fc, ci)
    hfc, hci, hq = fc.cpu().numpy(), ci.cpu().numpy(), q.cpu().numpy()
    for k in range(B):
        want_ci, want_q, _, margin = lref.louvain(*lref.objective(hfc[k]), 4)
        assert margin >= lref.MIN_MARGIN
        check(hci[k], hq[k], want_ci, want_q, f"fc {k}")
        check_optimum(lref.objective(hfc[k])[0], hci[k], tag=f"fc {k}")
        for m, want in (("participation", cref.participation(hfc[k], hci[k])), ("zscore", cref.zscore(hfc[k], hci[k])),
                        ("modularity", hq[k])):
            assert cref.deviation_abs(mod[m][k].cpu().numpy(), want) <= BOUND, (k, m)

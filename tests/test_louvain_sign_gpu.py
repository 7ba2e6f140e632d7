"""The signed Louvain search and the consensus loop on the device (wc_graph_louvain_sign through
partition.graph_louvain_sign, graph_consensus and the graph_utils facades) against
tests/louvain_sign_reference.py, the numpy restatement that test_louvain_sign_cpu.py pins to the
reference's own outputs, and against those outputs directly (tests/golden/golden_louvain_sign.npz).

Bounds.  ci: exactly equal.  q: |got - want| <= 1e-12 max(1, |want|) (centrality_reference.deviation_abs).
info (levels, sweeps): equal.  Every compared run asserts the restatement's decision margin >= 1e-9: the
device sums in another order than numpy, to 1e-16; on the dyadic matrices of the consensus cases every
sum is exact and exact ties are part of the comparison.

N: 2, 5, 24, 63, 64, 65 (a lane's second module begins at 65), 90, and 96 (the LDS limit), on
louvain_sign_reference.signed_graph(n, n).  Local optimum (check_optimum): where the last level moved
nothing no single module gains more than 1e-10; where the partition is the node level's, no single
node does.

Measured on MI355X, largest over the runs of the file (each is printed before it is asserted): ci and info
exactly equal on all 156 compared runs, q within 4.4e-16; the signed modularity of the returned partition
within 2.2e-16 of the q returned (51 runs); module-level gain 0 on the 45 runs it applies to, node-level gain
0 on 26.  Consensus: the five committed cases exactly, fc_centred in two iterations, the others in one.
"""
import functools

import numpy as np
import pytest
import torch

from nremmodfc_amd import graph_utils as gu
from nremmodfc_amd import partition
from nremmodfc_amd import sigchain as wsg
from tests import centrality_reference as cref
from tests import louvain_sign_reference as ls
from tests.test_louvain_sign_cpu import consensus_input, golden, inputs, runs

pytestmark = pytest.mark.gpu

BOUND = 1e-12
SIZES = (2, 5, 24, 63, 64, 65, 90, 96)


@functools.lru_cache(maxsize=None)
def graph(n, seed=None):
    w = ls.signed_graph(n, n if seed is None else seed)
    w.setflags(write=False)
    return w


@functools.lru_cache(maxsize=None)
def host(n, gseed, seed, gamma=1.0, qtype="sta"):
    """louvain_sign_reference.louvain_sign of graph(n, gseed), computed once; the margin asserted.
    -> (ci, q, info, sweeps per level)"""
    trace = []
    ci, q, info, margin = ls.louvain_sign(graph(n, gseed), seed, gamma, qtype, trace)
    assert margin >= ls.MIN_MARGIN, (n, gseed, seed, gamma, qtype, margin)
    ci.setflags(write=False)
    return ci, q, info, tuple(trace)


def cuda(a, dtype=None):
    return torch.from_numpy(np.array(a, dtype=dtype)).cuda()


def device(w, seeds=0, **kw):
    return tuple(t.cpu().numpy() for t in partition.graph_louvain_sign(cuda(w), seeds=seeds, **kw))


def check(got_ci, got_q, want_ci, want_q, tag):
    dev = cref.deviation_abs(got_q, want_q)
    print(f"{tag}: q {dev:.1e}  modules {int(np.max(want_ci)) + 1}")
    np.testing.assert_array_equal(got_ci, want_ci)
    assert dev <= BOUND, (tag, dev)


def check_optimum(w, ci, q, trace, gamma=1.0, qtype="sta", tag=""):
    """q is the signed modularity of ci (without gamma, as the reference reports it), and no single move gains more than 1e-10 at the level the search
    stopped at: where the last level moved nothing (one sweep) every module is a node that stays; where
    the partition is the node level's own (one level, or a second that moved nothing) every node stays.
    A last level that moved (it gained less than 1e-10, or lost) promises nothing about its modules.
    Returns which of the two was checked."""
    dev = cref.deviation_abs(ls.modularity_sign(w, ci, qtype), q)
    module = ls.local_gain(ls.pooled(w, ci), np.arange(int(ci.max()) + 1), gamma, qtype) if trace[-1] == 1 else None
    node = ls.local_gain(w, ci, gamma, qtype) if len(trace) == 1 or (len(trace) == 2 and trace[-1] == 1) else None
    print(f"{tag}: modularity of ci against q {dev:.1e}, sweeps per level {trace}, module-level gain {module}, "
          f"node-level gain {node}")
    assert dev <= BOUND
    assert module is None or module <= ls.TOL + BOUND, (tag, module)
    assert node is None or node <= ls.TOL + BOUND, (tag, node)
    return module is not None, node is not None


# ---- sizes ----

@pytest.mark.parametrize("n", SIZES)
def test_sizes(n):
    w = graph(n)
    ci, q, info = device(w[None], seeds=[0, 1], want_info=True)
    assert ci.shape == (1, 2, n) and ci.dtype == np.int32 and q.shape == (1, 2) and info.shape == (1, 2, 2)
    for k, seed in enumerate((0, 1)):
        want_ci, want_q, want_info, trace = host(n, n, seed)
        check(ci[0, k], q[0, k], want_ci, want_q, f"N={n} seed {seed}")
        assert tuple(info[0, k]) == want_info
        check_optimum(w, ci[0, k], q[0, k], trace, tag=f"N={n} seed {seed}")
    one_ci, one_q = device(w, seeds=1)                           # [N][N] and an int: no batch axis, no R axis
    assert one_ci.shape == (n,) and one_q.shape == ()
    np.testing.assert_array_equal(one_ci, ci[0, 1])
    assert one_q == q[0, 1]


@pytest.mark.parametrize("qtype", ls.QTYPES)
@pytest.mark.parametrize("gamma", (1.0,) + ls.GAMMAS)
def test_every_qtype_and_gamma(qtype, gamma):
    seen = [False, False]
    for n in (24, 65):
        want_ci, want_q, want_info, trace = host(n, n, 0, gamma, qtype)
        ci, q, info = device(graph(n), gamma=gamma, qtype=qtype, want_info=True)
        check(ci, q, want_ci, want_q, f"N={n} {qtype} gamma {gamma}")
        assert tuple(info) == want_info
        seen = [a or b for a, b in zip(seen, check_optimum(graph(n), ci, q, trace, gamma, qtype, f"N={n} {qtype} gamma {gamma}"))]
    assert seen[0]                                               # the module-level check was made


# ---- golden ----

@pytest.mark.parametrize("case", ls.CASES)
def test_golden_runs(case):
    """The reference's own modularity_louvain_und_sign under the engine's order, every committed run:
    one launch per qtype and gamma."""
    w = inputs()[case]
    table = runs(case)
    for gamma, qtype in sorted({(r[0], r[1]) for r in table}):
        rows = [r for r in table if (r[0], r[1]) == (gamma, qtype)]
        ci, q, info = device(w, seeds=[r[2] for r in rows], gamma=gamma, qtype=qtype, want_info=True)
        for k, (_, _, seed, want_ci, want_q, margin, sweeps) in enumerate(rows):
            assert margin >= ls.MIN_MARGIN
            check(ci[k] + 1, q[k], want_ci, want_q, f"{case} {qtype} gamma {gamma} seed {seed}")
            assert sweeps is None or info[k, 1] == sweeps


# ---- batch and workspace independence ----

@functools.lru_cache(maxsize=None)
def five_by_three():
    ws = np.stack([graph(65, 100 + k) for k in range(5)])
    ws.setflags(write=False)
    return ws, (5, 0, 9), device(ws, seeds=[5, 0, 9], want_info=True)


def test_batch_of_five_matrices_and_three_seeds():
    ws, seeds, (ci, q, info) = five_by_three()
    assert ci.shape == (5, 3, 65)
    for b in range(5):
        for r, seed in enumerate(seeds):
            one = device(ws[b], seeds=seed, want_info=True)
            np.testing.assert_array_equal(one[0], ci[b, r])
            assert one[1].tobytes() == q[b, r].tobytes()         # bit for bit
            np.testing.assert_array_equal(one[2], info[b, r])
    again = device(ws, seeds=list(seeds), want_info=True)
    for a, b in zip(again, (ci, q, info)):
        assert a.tobytes() == b.tobytes()
    for b in range(5):
        want_ci, want_q, want_info, trace = host(65, 100 + b, 0)
        check(ci[b, 1], q[b, 1], want_ci, want_q, f"B=5 matrix {b}")
        check_optimum(ws[b], ci[b, 1], q[b, 1], trace, tag=f"B=5 matrix {b}")


@pytest.mark.parametrize("slots", (1, 3))
def test_workspace_of_one_and_of_three_slots_for_fifteen_problems(slots):
    """A workgroup strides over the problems and reuses its slot and its LDS: the same bits as with a
    slot per problem."""
    ws, seeds, want = five_by_three()
    got = device(ws, seeds=list(seeds), want_info=True, ws_bytes=slots * partition.louvain_sign_slot_bytes(65))
    for a, b in zip(got, want):
        assert a.tobytes() == b.tobytes()


# ---- conventions ----

def test_nan_spoils_its_matrix_only():
    ws = np.stack([graph(24, 1), graph(24, 2), graph(24, 3)])
    clean = device(ws, seeds=[0, 1], want_info=True)
    assert (clean[0] >= 0).all() and np.isfinite(clean[1]).all()
    slot = partition.louvain_sign_slot_bytes(24)
    for value, k, ws_bytes in ((np.nan, 1, None), (np.inf, 2, None), (-np.inf, 0, slot), (np.nan, 1, 2 * slot)):
        bad = np.array(ws)
        bad[k, 3, 5] = value
        ci, q, info = device(bad, seeds=[0, 1], want_info=True, ws_bytes=ws_bytes)
        assert (ci[k] == -1).all() and np.isnan(q[k]).all() and (info[k] == 0).all()
        others = [j for j in range(3) if j != k]
        for got, want in zip((ci, q, info), clean):
            assert got[others].tobytes() == want[others].tobytes()
        D = wsg.graph_agreement(cuda(ci)).cpu().numpy()
        assert np.isnan(D[k]).all() and np.isfinite(D[others]).all()


def test_all_zero_and_all_negative_matrices():
    ci, q, info = device(np.zeros((2, 5, 5)), seeds=[0, 3], want_info=True)
    assert (ci == np.arange(5)).all() and (q == 0).all() and (info == 1).all()
    w = -np.abs(graph(24))
    for qtype in ls.QTYPES:
        want_ci, want_q, want_info, margin = ls.louvain_sign(w, 0, 1.0, qtype)
        assert margin >= ls.MIN_MARGIN
        ci, q, info = device(w, qtype=qtype, want_info=True)
        check(ci, q, want_ci, want_q, f"all negative, {qtype}")
        assert tuple(info) == want_info
    assert device(w, qtype="pos")[0].tolist() == list(range(24))    # no positive weight: nothing moves


def test_neg_on_a_nonnegative_matrix_pools_every_node():
    """K = N at the first pooling, at the LDS limit."""
    w = np.abs(graph(96))
    ci, q, info = device(w, qtype="neg", want_info=True)
    assert ci.tolist() == list(range(96)) and q == 0 and tuple(info) == (1, 1)
    want = device(w, qtype="sta")
    for qtype in ("pos", "smp", "gja"):                          # the positive types agree there
        got = device(w, qtype=qtype)
        np.testing.assert_array_equal(got[0], want[0])
        assert cref.deviation_abs(got[1], want[1]) <= BOUND


# ---- consensus ----

def consensus(D, tau, **kw):
    return tuple(t.cpu().numpy() for t in partition.graph_consensus(cuda(D), tau, **kw))


def test_consensus_golden_cases():
    """The reference's own consensus_und under the engine's order and graph_consensus's seeding."""
    g = golden()
    for case, tau, reps in ls.CONSENSUS:
        ci, iters = consensus(consensus_input(case), tau, reps=reps)
        print(f"consensus {case}: iterations {iters}, modules {ci.max() + 1}")
        np.testing.assert_array_equal(ci + 1, g[f"cons/{case}/ci"])
        assert iters == g[f"cons/{case}/iters"] and ci.dtype == np.int32 and iters.dtype == np.int32


def test_consensus_batch_in_which_one_matrix_converges_first():
    D = np.stack([consensus_input("fc_centred"), consensus_input("fc_thr"), consensus_input("fc_centred")])
    want = [ls.consensus(D[k], 0.5, 16) for k in range(2)]
    assert min(w[2] for w in want) >= ls.MIN_MARGIN and want[0][1] == 2 and want[1][1] == 1
    ci, iters = consensus(D, 0.5, reps=16)
    assert iters.tolist() == [2, 1, 2]
    for k in range(3):
        np.testing.assert_array_equal(ci[k], want[k % 2][0])
    seeds = [7 * r + 1 for r in range(16)]                       # seeds given: rep r of iteration k runs seeds[r] + 16 k
    mine = ls.consensus(D[0], 0.5, 16, seeds)
    assert mine[2] >= ls.MIN_MARGIN
    got = consensus(D[0], 0.5, reps=16, seeds=seeds)
    np.testing.assert_array_equal(got[0], mine[0])
    assert got[1] == mine[1] and got[0].shape == (90,) and got[1].shape == ()


def test_consensus_of_two_cliques_and_the_iteration_cap():
    D = np.zeros((8, 8))
    D[:4, :4] = D[4:, 4:] = 1.0
    D[3, 4] = D[4, 3] = 0.25
    ci, iters = consensus(D, 0.5, reps=8)
    assert ci.tolist() == [0] * 4 + [1] * 4 and iters == 1
    stack = np.stack([consensus_input("fc_centred"), consensus_input("fc_thr")])
    ci, iters = consensus(stack, 0.5, reps=16, max_iter=1)
    assert (ci[0] == -1).all() and iters.tolist() == [1, 1]
    np.testing.assert_array_equal(ci[1], ls.consensus(stack[1], 0.5, 16)[0])
    bad = np.array(stack)
    bad[0, 2, 3] = bad[0, 3, 2] = np.nan                         # refused: -1 after the first iteration
    ci, iters = consensus(bad, 0.5, reps=16)
    assert (ci[0] == -1).all() and iters.tolist() == [1, 1] and (ci[1] >= 0).all()


# ---- facades and composition ----

def test_facades():
    g = golden()
    W = np.array(inputs()["fc_centred"])
    ci, q = gu.modularity_louvain_und_sign(W, seed=3)
    np.testing.assert_array_equal(ci, g["fc_centred/ci_sta"][3])
    assert isinstance(q, float) and abs(q - g["fc_centred/q_sta"][3]) <= BOUND and ci.min() == 1
    assert (W == inputs()["fc_centred"]).all()                   # the caller's matrix is left alone
    ci, q = gu.modularity_louvain_und_sign(W, gamma=0.7, qtype="sta", seed=int(g["fc_centred/seeds_g0.7"][0]))
    np.testing.assert_array_equal(ci, g["fc_centred/ci_g0.7"][0])
    stack = np.stack([inputs()["fc_centred"], inputs()["fc_thr"]])
    cs, qs = gu.modularity_louvain_und_sign(stack, qtype="smp", seed=1)
    np.testing.assert_array_equal(cs[0], g["fc_centred/ci_smp"][1])
    np.testing.assert_array_equal(cs[1], g["fc_thr/ci_smp"][1])
    a, b = gu.modularity_louvain_und_sign(W), gu.modularity_louvain_und_sign(W)   # seed=None: both valid
    assert a[0].min() == 1 and b[0].min() == 1 and 0.4 < min(a[1], b[1])
    with pytest.raises(ValueError, match="modularity type unknown"):
        gu.modularity_louvain_und_sign(W, qtype="std")
    D = np.zeros((8, 8))
    D[:4, :4] = D[4:, 4:] = 1.0
    assert gu.consensus_und(D, 0.5, reps=8).tolist() == [1] * 4 + [2] * 4
    ciu = gu.consensus_und(consensus_input("corr24"), 0.4, reps=8)   # fresh seeds: the three groups all the same
    np.testing.assert_array_equal(ciu, g["cons/corr24/ci"])


def test_raw_fc_to_consensus_partition_to_module_roles():
    """The chain the kernel closes: a signed FC, thresholded agreement of signed runs, consensus,
    participation and z-score, all on the device."""
    fc = cuda(np.stack([inputs()["fc_centred"], inputs()["corr96"][:90, :90]]))
    part, _ = partition.graph_louvain_sign(fc, seeds=list(range(8)))
    D = wsg.graph_agreement(part) / 8
    ci, iters = partition.graph_consensus(D, 0.5, reps=8)
    assert (ci >= 0).all() and (iters >= 1).all()
    roles = wsg.graph_module_measures(fc.clamp(min=0.0), ci)
    hfc, hci = fc.clamp(min=0.0).cpu().numpy(), ci.cpu().numpy()
    for k in range(2):
        want = ls.consensus(D[k].cpu().numpy(), 0.5, 8)
        if want[2] >= ls.MIN_MARGIN:
            np.testing.assert_array_equal(hci[k], want[0])
        assert cref.deviation_abs(roles["participation"][k].cpu().numpy(), cref.participation(hfc[k], hci[k])) <= BOUND
        assert cref.deviation_abs(roles["zscore"][k].cpu().numpy(), cref.zscore(hfc[k], hci[k])) <= BOUND

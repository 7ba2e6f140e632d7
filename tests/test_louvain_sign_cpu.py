"""The signed Louvain search and the consensus loop without a GPU: the numpy restatement
(tests/louvain_sign_reference.py) against the committed outputs of the reference's own
modularity_louvain_und_sign and consensus_und (tests/golden/golden_louvain_sign.npz,
make_louvain_sign_golden.py), properties of the restatement that the device tests rely on, what
wc_graph_louvain_sign refuses through the C ABI (fake pointers: every row is refused before any device
work), and what the wrappers of nremmodfc_amd.partition and partition_np refuse, message for message.

Committed runs: five matrices (signed5, corr24, fc_centred, corr96, fc_thr) x five qtypes (8 seeds for
sta, 2 for the others) and sta at gamma 0.7 and 1.3; smallest decision margin 5.4e-8 (fc_centred sta),
all >= 1e-9 without a seed replaced.  Five consensus cases on the dyadic agreement matrices of the
committed sta partitions: 1 iteration, fc_centred 2; smallest margin 1.4e-5.
"""
import ctypes
import functools

import numpy as np
import pytest
import torch

from nremmodfc_amd import graph_utils as gu
from nremmodfc_amd import partition, partition_np
from tests import louvain_reference as lr
from tests import louvain_sign_reference as ls
from tests.test_arg_checks_cpu import EINVAL, EUNSUPPORTED, INF, NAN, P, Span, call, entry, rows

BOUND = 1e-12


@functools.lru_cache(maxsize=None)
def inputs():
    out = ls.inputs()
    for a in out.values():
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def golden():
    return ls.load_golden()


def runs(case):
    """(gamma, qtype, seed, ci from 1, q, margin, sweeps or None) of every committed run of a case."""
    g, out = golden(), []
    for qtype in ls.QTYPES:
        for k, seed in enumerate(g[f"{case}/seeds_{qtype}"].tolist()):
            out.append((1.0, qtype, seed, g[f"{case}/ci_{qtype}"][k], g[f"{case}/q_{qtype}"][k],
                        g[f"{case}/margin_{qtype}"][k], int(g[f"{case}/sweeps_{qtype}"][k])))
    for gamma in ls.GAMMAS:
        for k, seed in enumerate(g[f"{case}/seeds_g{gamma}"].tolist()):
            out.append((gamma, "sta", seed, g[f"{case}/ci_g{gamma}"][k], g[f"{case}/q_g{gamma}"][k],
                        g[f"{case}/margin_g{gamma}"][k], None))
    return out


def consensus_input(case):
    """The agreement of the case's eight committed sta partitions / 8: dyadic."""
    return lr.agreement(np.asarray(golden()[f"{case}/ci_sta"], dtype=np.int64)) / 8


# ---- the restatement against the reference's outputs ----

@pytest.mark.parametrize("case", ls.CASES)
def test_restatement_gives_the_committed_runs(case):
    w = inputs()[case]
    table = runs(case)
    assert len(table) == 8 + 4 * 2 + 2 * 2
    for gamma, qtype, seed, want_ci, want_q, want_margin, sweeps in table:
        ci, q, info, margin = ls.louvain_sign(w, seed, gamma, qtype)
        np.testing.assert_array_equal(ci + 1, want_ci)
        assert abs(q - want_q) <= BOUND and margin == want_margin and margin >= ls.MIN_MARGIN
        assert sweeps is None or info[1] == sweeps
        assert ci.min() == 0 and sorted(set(ci.tolist())) == list(range(ci.max() + 1))


@pytest.mark.parametrize("case,tau,reps", ls.CONSENSUS)
def test_restatement_gives_the_committed_consensus(case, tau, reps):
    g = golden()
    assert g[f"cons/{case}/tau"] == tau and g[f"cons/{case}/reps"] == reps and reps & (reps - 1) == 0
    D = consensus_input(case)
    assert ls.dyadic(D)
    ci, iters, margin = ls.consensus(D, tau, reps)
    np.testing.assert_array_equal(ci + 1, g[f"cons/{case}/ci"])
    assert iters == g[f"cons/{case}/iters"] and margin == g[f"cons/{case}/margin"] and margin >= ls.MIN_MARGIN


def test_some_committed_consensus_takes_more_than_one_iteration():
    assert max(int(golden()[f"cons/{c}/iters"]) for c, _, _ in ls.CONSENSUS) > 1


# ---- properties of the restatement ----

def test_positive_qtypes_agree_on_a_nonnegative_matrix_and_neg_moves_nothing():
    w = inputs()["fc_thr"]
    assert w.min() >= 0
    want = ls.louvain_sign(w, 3)
    for qtype in ("pos", "smp", "gja"):
        got = ls.louvain_sign(w, 3, 1.0, qtype)
        np.testing.assert_array_equal(got[0], want[0])
        assert got[1] == want[1] and got[2] == want[2]
    ci, q, info, _ = ls.louvain_sign(w, 3, 1.0, "neg")
    assert ci.tolist() == list(range(90)) and q == 0 and info == (1, 1)


def test_on_a_nonnegative_matrix_it_is_community_louvain():
    """The reference's docstring: equivalent to the unsigned search where all weights are positive."""
    w = inputs()["fc_thr"]
    for seed in (0, 1):
        ci, q, info, _ = lr.louvain(*lr.objective(w), seed)
        got = ls.louvain_sign(w, seed)
        np.testing.assert_array_equal(got[0], ci)
        assert abs(got[1] - q) <= BOUND and got[2][1] == info[1]


def test_all_zero_all_negative_and_non_finite():
    ci, q, info, _ = ls.louvain_sign(np.zeros((5, 5)), 0)
    assert ci.tolist() == [0, 1, 2, 3, 4] and q == 0 and info == (1, 1)
    w = -np.abs(inputs()["corr24"])
    for qtype in ("sta", "smp", "gja", "neg"):                  # the negative part alone drives these
        ci, q, _, _ = ls.louvain_sign(w, 0, 1.0, qtype)
        assert ci.min() == 0 and np.isfinite(q)
    ci, q, info, _ = ls.louvain_sign(w, 0, 1.0, "pos")           # d0 = d1 = 0: nothing moves
    assert ci.tolist() == list(range(24)) and q == 0 and info == (1, 1)
    bad = np.array(inputs()["corr24"])
    bad[2, 3] = np.nan
    ci, q, info, _ = ls.louvain_sign(bad, 0)
    assert (ci == -1).all() and np.isnan(q) and info == (0, 0)
    with pytest.raises(KeyError, match="modularity type unknown"):
        ls.louvain_sign(bad, 0, 1.0, "std")


def test_guards_give_minus_one_and_nan(monkeypatch):
    """The output convention of the two guards, on the restatement with the guards lowered (no run
    known reaches 1000 sweeps of a level or 300 levels)."""
    w = inputs()["corr24"]
    trace = []
    _, _, info, _ = ls.louvain_sign(w, 0, trace=trace)
    assert trace[0] > 1 and info[0] > 1 and sum(trace) == info[1]
    monkeypatch.setattr(ls, "SWEEP_GUARD", trace[0] - 1)
    ci, q, got, _ = ls.louvain_sign(w, 0)
    assert (ci == -1).all() and np.isnan(q) and got == (0, trace[0] - 1)
    monkeypatch.setattr(ls, "SWEEP_GUARD", lr.SWEEP_GUARD)
    monkeypatch.setattr(ls, "LEVEL_GUARD", 1)
    ci, q, got, _ = ls.louvain_sign(w, 0)
    assert (ci == -1).all() and np.isnan(q) and got == (1, trace[0])


def test_local_gain_and_modularity_of_the_committed_partitions():
    """What the device test checks on every partition, shown to hold on the host's: no single move
    gains at the level the search stopped at, and q is the signed modularity of the partition."""
    for case in ("signed5", "corr24", "fc_centred"):
        w = inputs()[case]
        for qtype in ls.QTYPES:
            trace = []
            ci, q, info, _ = ls.louvain_sign(w, 0, 1.0, qtype, trace)
            assert abs(ls.modularity_sign(w, ci, qtype) - q) <= BOUND
            assert abs(ls.modularity_sign(w, ls.louvain_sign(w, 0, 0.7, qtype)[0], qtype) - ls.louvain_sign(w, 0, 0.7, qtype)[1]) <= BOUND
            if trace[-1] == 1:
                assert ls.local_gain(ls.pooled(w, ci), np.arange(ci.max() + 1), 1.0, qtype) <= ls.TOL + BOUND
            if len(trace) == 1 or (len(trace) == 2 and trace[-1] == 1):
                assert ls.local_gain(w, ci, 1.0, qtype) <= ls.TOL + BOUND
    worse = np.array(ls.louvain_sign(inputs()["corr24"], 0)[0])
    worse[0] = (worse[0] + 1) % 3
    assert ls.local_gain(inputs()["corr24"], worse) > 1e-3


def test_dyadic_and_first_occurrence():
    assert ls.dyadic(np.array([[0, 0.375], [0.375, 0]])) and ls.dyadic(consensus_input("corr24"))
    assert not ls.dyadic(inputs()["corr24"]) and not ls.dyadic(np.array([[0, 0.1], [0.1, 0]]))
    assert not ls.dyadic(np.array([[0, np.nan], [0.5, 0]]))
    assert ls.first_occurrence([5, 5, 2, 9, 2, 5]).tolist() == [0, 0, 1, 2, 1, 0]
    got = partition._first_occurrence(torch.tensor([[5, 5, 2, 9, 2, 5], [0, 1, 2, 0, 1, 2]], dtype=torch.int32))
    assert got.dtype == torch.int32 and got.tolist() == [[0, 0, 1, 2, 1, 0], [0, 1, 2, 0, 1, 2]]


def test_consensus_of_two_cliques_and_the_iteration_cap():
    D = np.zeros((8, 8))
    D[:4, :4] = D[4:, 4:] = 1.0
    D[3, 4] = D[4, 3] = 0.25
    ci, iters, _ = ls.consensus(D, 0.5, 8)
    assert ci.tolist() == [0] * 4 + [1] * 4 and iters == 1
    ci, iters, _ = ls.consensus(consensus_input("fc_centred"), 0.5, 16, max_iter=1)
    assert (ci == -1).all() and iters == 1


# ---- wc_graph_louvain_sign through the C ABI ----

SLOT = 16 * 90 * 90
SIGN_ENTRY = entry(
    "wc_graph_louvain_sign",
    dict(B=2, R=3, N=90, w=P(0), gamma=1.0, qtype=0, seeds=P(1), ci=P(2), q=P(3), info=P(4), workspace=P(5),
         ws_bytes=6 * SLOT),
    dict(w=Span("in", 2 * 90 * 90 * 8, 8, 8, True), seeds=Span("in", 3 * 8, 8, 8, True),
         ci=Span("out", 2 * 3 * 90 * 4, 4, 4, True), q=Span("out", 2 * 3 * 8, 8, 8, True),
         info=Span("out", 2 * 3 * 2 * 4, 4, 4, False), workspace=Span("out", 6 * SLOT, 8, 8, True)),
    [(dict(B=0), EINVAL), (dict(R=0), EINVAL), (dict(N=1), EINVAL), (dict(N=97), EUNSUPPORTED),
     (dict(B=1 << 16, R=1 << 15), EINVAL), (dict(qtype=-1), EINVAL), (dict(qtype=5), EINVAL),
     (dict(gamma=NAN), EINVAL), (dict(gamma=INF), EINVAL), (dict(gamma=-INF), EINVAL),
     (dict(ws_bytes=SLOT - 1), EINVAL), (dict(ws_bytes=0), EINVAL), (dict(N=96, ws_bytes=16 * 96 * 96 - 1), EINVAL)])


def test_the_library_refuses_bad_arguments():
    from nremmodfc_amd import _lib
    L = _lib.lib()
    table = rows(L, SIGN_ENTRY)
    assert len(table) == 13 + 5 + 6 + 4 * 2 + 6                 # shapes, NULL, misaligned, out x in, out x out
    assert all(code in (EINVAL, EUNSUPPORTED) for _, _, code, _ in table)
    for what, over, code, names in table:
        assert call(L, SIGN_ENTRY, over) == code, what
        msg = L.wc_last_error()
        assert msg.startswith(b"wc_graph_louvain_sign: "), (what, msg)
        if names:
            assert names.encode() in msg, (what, msg)
    assert L.wcsde_abi_version() == 7
    assert L.wc_graph_louvain_sign.argtypes[4] is ctypes.c_double and len(L.wc_graph_louvain_sign.argtypes) == 13


# ---- the wrappers ----

def refused(kind, message, fn, *args, **kw):
    with pytest.raises(kind) as e:
        fn(*args, **kw)
    assert str(e.value) == message
    return e.value


def test_graph_louvain_sign_refusals():
    w = torch.zeros((2, 5, 5), dtype=torch.float64)
    f = partition.graph_louvain_sign
    e = refused(ValueError, "graph_louvain_sign: modularity type unknown: qtype 'std', must be one of "
                "['sta', 'pos', 'smp', 'gja', 'neg']", f, w, qtype="std")
    assert "modularity type unknown" in str(e)                   # the reference's KeyError text
    refused(ValueError, "graph_louvain_sign: modularity type unknown: qtype 0, must be one of "
            "['sta', 'pos', 'smp', 'gja', 'neg']", f, w, qtype=0)
    refused(ValueError, "graph_louvain_sign: gamma = nan, must be a finite number", f, w, gamma=float("nan"))
    refused(ValueError, "graph_louvain_sign: gamma = '1', must be a finite number", f, w, gamma="1")
    refused(ValueError, "graph_louvain_sign: seeds must be an int or a non-empty sequence of ints in [0, 2^64), got -1",
            f, w, seeds=-1)
    refused(ValueError, "graph_louvain_sign: seeds must be an int or a non-empty sequence of ints in [0, 2^64), got []",
            f, w, seeds=[])
    refused(TypeError, "graph_louvain_sign: w must be a [B][N][N] or [N][N] fp64 device tensor", f, w.float())
    refused(TypeError, "graph_louvain_sign: w must be a [B][N][N] or [N][N] fp64 device tensor", f, w[:, :, :4])
    refused(TypeError, "graph_louvain_sign: w must be a [B][N][N] or [N][N] fp64 device tensor", f, np.zeros((5, 5)))
    refused(ValueError, "graph_louvain_sign: N = 97, B = 1: needs B >= 1 and 2 <= N <= 96 (one matrix per workgroup, in LDS)",
            f, torch.zeros((97, 97), dtype=torch.float64))
    refused(ValueError, "graph_louvain_sign: ws_bytes = 399, needs at least one slot of 16 N^2 = 400 bytes", f, w, ws_bytes=399)
    refused(ValueError, "graph_louvain_sign: ws_bytes = 400.0, needs at least one slot of 16 N^2 = 400 bytes", f, w,
            ws_bytes=400.0)
    assert partition.louvain_sign_slot_bytes(96) == 147456 and partition.LOUVAIN_SIGN_QTYPES == ls.QTYPES


def test_graph_consensus_refusals():
    D = torch.zeros((2, 5, 5), dtype=torch.float64)
    f = partition.graph_consensus
    refused(ValueError, "graph_consensus: reps = 0, must be a positive int", f, D, 0.5, reps=0)
    refused(ValueError, "graph_consensus: reps = 8.0, must be a positive int", f, D, 0.5, reps=8.0)
    refused(ValueError, "graph_consensus: max_iter = 0, must be a positive int", f, D, 0.5, reps=8, max_iter=0)
    refused(ValueError, "graph_consensus: tau = nan, must be a finite number", f, D, float("nan"), reps=8)
    refused(ValueError, "graph_consensus: tau = None, must be a finite number", f, D, None, reps=8)
    refused(ValueError, "graph_consensus: seeds must be a sequence of length reps = 8, or None", f, D, 0.5, reps=8,
            seeds=[1, 2, 3])
    refused(ValueError, "graph_consensus: seeds must be a sequence of length reps = 8, or None", f, D, 0.5, reps=8, seeds=3)
    refused(ValueError, "graph_consensus: seeds must be an int or a non-empty sequence of ints in [0, 2^64), got [-1, 2]",
            f, D, 0.5, reps=2, seeds=[-1, 2])
    refused(TypeError, "graph_consensus: w must be a [B][N][N] or [N][N] fp64 device tensor", f, D.float(), 0.5, reps=8)


def test_facades_are_drop_ins_and_refuse_before_the_device():
    assert gu.consensus_und is partition_np.consensus_und
    assert gu.modularity_louvain_und_sign is partition_np.modularity_louvain_und_sign
    assert gu.consensus_und.__module__ == "nremmodfc_amd.partition_np"       # not counted as graph_utils' own
    import inspect
    assert str(inspect.signature(gu.modularity_louvain_und_sign)) == "(W, gamma=1, qtype='sta', seed=None)"
    assert str(inspect.signature(gu.consensus_und)) == "(D, tau, reps=1000)"
    refused(ValueError, "modularity_louvain_und_sign: needs an N x N matrix or a [B, N, N] stack, got shape (5,)",
            gu.modularity_louvain_und_sign, np.zeros(5))
    refused(ValueError, "consensus_und: N = 97, the device kernels take 2 <= N <= 96", gu.consensus_und,
            np.zeros((97, 97)), 0.5)
    for text in (gu.community_louvain.__doc__,):
        assert "consensus_und," not in text

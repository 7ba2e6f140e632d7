"""Louvain and agreement without a device: tests/louvain_reference.py (the numpy restatement that
test_louvain_gpu.py checks the device against) is pinned to tests/golden/golden_louvain.npz, the
outputs of the reference's own community_louvain and agreement run under the engine's visiting order
(make_louvain_golden.py); the order itself is pinned by a known answer; wc_graph_louvain and
wc_graph_agreement validate every argument before any device work (the pointers are fake); the Python
layers refuse bad arguments before touching the device.

Committed runs and the decision margin of each (louvain_reference.louvain; every one >= 1e-9; also in
the file as c/seeds*, c/margin*).  Seeds 0-7 at gamma 1, seeds 0-1 at gamma 0.7 and 1.3 unless noted, and
one run from the hemispheres with seed 0 (sc: nothing moves and no quantity is tested, margin inf):
  sc         gamma 1: 3.3e-04 4.8e-04 3.7e-04 3.3e-04 2.7e-03 4.8e-04 6.6e-04 2.7e-03
             gamma 0.7: 2.9e-04 1.9e-03   gamma 1.3: 9.5e-04 2.7e-03   hemi: inf
  fc_dense   gamma 1: 3.6e-04 7.2e-03 8.1e-03 9.9e-04 8.5e-03 1.4e-03 1.8e-02 3.6e-04
             gamma 0.7: 1.9e-02 4.2e-03   gamma 1.3, seeds 0 and 2 (seed 1 decides by 1.1e-16 only):
             8.1e-04 8.1e-04   hemi: 4.4e-03
  fc_thr     gamma 1: 1.6e-04 1.3e-04 3.3e-03 3.3e-03 1.1e-03 7.2e-03 1.3e-03 1.6e-04
             gamma 0.7: 4.4e-04 2.0e-03   gamma 1.3: 1.7e-03 4.2e-03   hemi: 4.2e-02
  rand90     gamma 1: 2.9e-03 2.7e-04 2.0e-03 8.3e-04 2.7e-04 6.4e-04 1.6e-03 2.7e-04
             gamma 0.7: 2.7e-05 5.6e-03   gamma 1.3: 5.3e-04 4.9e-04   hemi: 8.1e-02
  dir24      gamma 1: 1.3e-03 7.4e-04 3.2e-05 2.0e-04 1.9e-04 1.2e-03 5.9e-04 1.3e-04
             gamma 0.7: 6.4e-03 6.0e-03   gamma 1.3: no run   hemi: 9.8e-03
  pendant12  gamma 1: 2.4e-02 2.4e-02 2.4e-02 1.1e-02 2.4e-02 1.1e-02 1.1e-02 2.4e-02
             gamma 0.7: 1.8e-02 1.8e-02   gamma 1.3: 1.0e-02 3.6e-02   hemi: 7.0e-02
dir24 at gamma 1.3 is absent: the reference itself raises there (its 1000-sweep guard, under numpy's
order as under the engine's), the restatement ends in the same guard, and no seed reaches the margin
(nodes choose between emptied modules whose Hnm holds rounding residues of 1e-17), see
make_louvain_golden.py; test_louvain_gpu.py::test_directed_above_gamma_one checks what holds there.
"""
import ctypes
import functools
import re

import numpy as np
import pytest

from tests import centrality_reference as cref
from tests import graph_reference as ref
from tests import louvain_reference as lref


@functools.lru_cache(maxsize=None)
def golden():
    return lref.load_golden()


@functools.lru_cache(maxsize=None)
def inputs():
    return ref.golden_inputs()


def runs(case):
    """(gamma, seed, ci0, ci, q, margin) of every committed run of a case."""
    g, n = golden(), inputs()[case].shape[0]
    out = [(1.0, int(s), None, g[f"{case}/ci"][k], g[f"{case}/q"][k], g[f"{case}/margin"][k])
           for k, s in enumerate(g[f"{case}/seeds"])]
    for gamma in lref.GAMMAS:
        out += [(gamma, int(s), None, g[f"{case}/ci_g{gamma}"][k], g[f"{case}/q_g{gamma}"][k],
                 g[f"{case}/margin_g{gamma}"][k]) for k, s in enumerate(g[f"{case}/seeds_g{gamma}"])]
    out.append((1.0, int(g[f"{case}/seed_hemi"][0]), cref.partition("hemi", n), g[f"{case}/ci_hemi"],
                g[f"{case}/q_hemi"][0], g[f"{case}/margin_hemi"][0]))
    return out


def test_known_answer_order():
    """Sweep 1 of seed 3: the block of quad 0 is Philox4x32-10 of counter (1, 0, 3, 0) under the build's
    key, 3e90c569 2501ffba a2f016bf 8d647b78, so nodes 0-3 come in the order 1, 0, 3, 2."""
    assert [hex(k) for k in lref.sweep_keys(3, 1, 4)] == ["0x3e90c569", "0x2501ffba", "0xa2f016bf", "0x8d647b78"]
    assert lref.sweep_order(3, 1, 4).tolist() == [1, 0, 3, 2]
    assert lref.sweep_order(3, 1, 10).tolist() == [1, 0, 7, 3, 2, 6, 8, 9, 5, 4]
    assert lref.sweep_order((1 << 40) + 5, (1 << 33) + 2, 7).tolist() == [6, 3, 0, 1, 2, 4, 5]
    # Random123's known answer for Philox4x32-10: zero counter and key
    assert lref.philox4x32_10((0, 0, 0, 0), (0, 0)) == (0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8)


def test_committed_runs_are_complete():
    g = golden()
    for case in lref.CASES:
        assert g[f"{case}/seeds"].tolist() == list(range(8))
        for gamma in lref.GAMMAS:
            # fc_dense at gamma 1.3: seed 1 decides by 1.1e-16 only and is replaced by seed 2
            want = {("dir24", 1.3): [], ("fc_dense", 1.3): [0, 2]}.get((case, gamma), [0, 1])
            assert g[f"{case}/seeds_g{gamma}"].tolist() == want, (case, gamma)
        assert len({tuple(c) for c in g[f"{case}/ci"].tolist()}) > (1 if case != "pendant12" else 0)


@pytest.mark.parametrize("case", lref.CASES)
def test_restatement_equals_the_reference(case):
    w = inputs()[case]
    for gamma, seed, ci0, ci, q, margin in runs(case):
        obj, s = lref.objective(w, gamma)
        got, gq, info, m = lref.louvain(obj, s, seed, ci0)
        assert m >= lref.MIN_MARGIN and margin >= lref.MIN_MARGIN
        np.testing.assert_array_equal(got + 1, ci)
        assert abs(gq - q) <= 1e-12
        dev = cref.deviation_abs(gq, cref.modularity(w, got, gamma))
        assert dev <= 1e-12, (case, gamma, seed, dev)
        assert info[0] >= 1 and info[1] >= info[0]             # sc from the hemispheres: nothing moves, one level


@pytest.mark.parametrize("case", lref.CASES)
def test_agreement_equals_the_reference(case):
    g = golden()
    D = lref.agreement(g[f"{case}/ci"])
    np.testing.assert_array_equal(D, g[f"{case}/agreement"])
    assert (np.diag(D) == 0).all() and D.max() <= 8
    bad = np.array(g[f"{case}/ci"], dtype=np.int64)
    bad[3, 1] = -1
    assert np.isnan(lref.agreement(bad)).all()


def test_restatement_conventions():
    obj, s = lref.objective(inputs()["pendant12"])
    for spoil in ("obj", "s"):
        o, n = np.array(obj), s
        if spoil == "obj":
            o[2, 5] = np.nan
        else:
            n = np.inf
        ci, q, info, _ = lref.louvain(o, n, 0)
        assert (ci == -1).all() and np.isnan(q) and info == (0, 0)
    empty = np.zeros((5, 5))
    ci, q, _, _ = lref.louvain(*lref.objective(empty), 0)            # modularity: 0 / 0 in obj
    assert (ci == -1).all() and np.isnan(q)
    ci, q, info, _ = lref.louvain(*lref.objective(empty, 1.0, "potts"), 0)   # finite obj, s = 0
    assert ci.tolist() == [0, 1, 2, 3, 4] and q == -np.inf and info == (0, 0)   # the reference: singletons, -inf


# ---- the C ABI ----

def lib():
    from nremmodfc_amd import _lib
    return _lib.lib()


def fake(addr):
    return ctypes.c_void_p(addr)


OBJ, NORM, CI0, SEEDS, CI, Q, INFO, D = (fake(0x10000000 * k) for k in range(1, 9))


def louvain(L, B=1, R=2, N=90, obj=OBJ, norm=NORM, ci0=CI0, seeds=SEEDS, ci=CI, q=Q, info=INFO):
    return L.wc_graph_louvain(B, R, N, obj, norm, ci0, seeds, ci, q, info, None)


def agree(L, B=1, R=2, N=90, ci=CI, D=D):
    return L.wc_graph_agreement(B, R, N, ci, D, None)


@pytest.mark.parametrize("call,name,ptrs", [
    (louvain, b"wc_graph_louvain", ("obj", "norm", "seeds", "ci", "q")),
    (agree, b"wc_graph_agreement", ("ci", "D")),
])
def test_entry_points_validate_without_device_work(call, name, ptrs):
    L = lib()
    err = L.wc_last_error
    assert call(L, B=0) == -1 and b"B < 1" in err() and name in err()
    assert call(L, R=0) == -1 and b"R < 1" in err()
    assert call(L, R=-2) == -1
    assert call(L, N=1) == -1 and b"N < 2" in err()
    assert call(L, N=97) == -2 and b"96" in err()
    assert call(L, N=1000) == -2
    for p in ptrs:
        assert call(L, **{p: None}) == -1 and b"NULL" in err(), p
    assert call(L, ci=fake(CI.value + 2)) == -1 and b"4-byte" in err()
    inside = fake((OBJ if call is louvain else CI).value + 8)    # the last output, one element into the first input
    assert call(L, B=2, **{ptrs[-1]: inside}) == -1 and b"alias" in err()


def test_louvain_validates_its_own_arguments():
    L = lib()
    err = L.wc_last_error
    assert louvain(L, obj=fake(OBJ.value + 4)) == -1 and b"8-byte" in err()
    assert louvain(L, info=fake(CI.value)) == -1 and b"alias" in err()
    assert louvain(L, ci=fake(CI0.value)) == -1 and b"alias ci0" in err()
    assert louvain(L, B=1 << 16, R=1 << 15) == -1 and b"2^31" in err()


def test_header_and_abi_version():
    import os
    hdr = open(os.path.join(os.path.dirname(__file__), "..", "include", "wcsde.h")).read()
    assert re.search(r"#define WCSDE_ABI_VERSION 7\b", hdr)
    for fn in ("wc_graph_louvain", "wc_graph_agreement"):
        assert re.search(rf"\bint {fn}\(", hdr)
    assert lib().wcsde_abi_version() == 7


# ---- the Python layers ----

def test_sigchain_refuses_before_touching_the_device():
    import torch

    from nremmodfc_amd import sigchain
    ok = torch.zeros((2, 5, 5), dtype=torch.float64)
    assert sigchain.GRAPH_LOUVAIN_OBJECTIVES == ("modularity", "potts")
    for name in sigchain.GRAPH_PARTITION_SEARCH:
        assert callable(getattr(sigchain, name))
    for bad in ("negative_sym", "negative_asym", "newman", None, 3):
        with pytest.raises(ValueError, match="objective"):
            sigchain.graph_louvain(ok, objective=bad)
    for bad in ([], -1, 1 << 64, 1.5, [0, -2], "7", True):
        with pytest.raises(ValueError, match="seeds"):
            sigchain.graph_louvain(ok, seeds=bad)
    for t in (ok.float(), ok[0, 0], torch.zeros((2, 5, 4), dtype=torch.float64), ok.numpy(), None):
        with pytest.raises(TypeError, match="graph_louvain"):
            sigchain.graph_louvain(t)
    with pytest.raises(ValueError, match="96"):
        sigchain.graph_louvain(torch.zeros((1, 97, 97), dtype=torch.float64))
    for t in (torch.zeros((3, 5), dtype=torch.int64), torch.zeros(5, dtype=torch.int32), None):
        with pytest.raises(TypeError, match="graph_agreement"):
            sigchain.graph_agreement(t)
    with pytest.raises(ValueError, match="96"):
        sigchain.graph_agreement(torch.zeros((3, 97), dtype=torch.int32))
    for reps in (0, -1, 2.5, True):
        with pytest.raises(ValueError, match="reps"):
            sigchain.graph_consensus_matrix(ok, reps=reps)
    with pytest.raises(ValueError, match="length reps"):
        sigchain.graph_consensus_matrix(ok, reps=4, seeds=[0, 1, 2])


def test_facades_refuse_before_touching_the_device():
    from nremmodfc_amd import graph_utils as gu
    W = inputs()["pendant12"]
    with pytest.raises(ValueError, match="negative weights"):
        gu.community_louvain(inputs()["signed5"], seed=0)
    for B in ("negative_sym", "negative_asym"):
        with pytest.raises(ValueError, match="not built"):
            gu.community_louvain(W, B=B, seed=0)
    with pytest.raises(ValueError, match="unknown objective"):
        gu.community_louvain(W, B="newman", seed=0)
    with pytest.raises(ValueError, match="binary"):
        gu.community_louvain(W, B="potts", seed=0)
    with pytest.raises(ValueError, match="size of adjacency"):
        gu.community_louvain(W, B=np.zeros((5, 5)), seed=0)
    with pytest.raises(ValueError, match="one label per node"):
        gu.community_louvain(W, ci=np.arange(5), seed=0)
    with pytest.raises(ValueError, match="96"):
        gu.community_louvain(np.zeros((97, 97)), seed=0)
    with pytest.raises(ValueError, match="length equal to reps"):
        gu.get_agreement_matrix(W, reps=4, seeds=[0, 1])
    with pytest.raises(ValueError, match="vertex x partition"):
        gu.agreement(np.arange(12))
    with pytest.raises(ValueError, match="96"):
        gu.agreement(np.zeros((97, 3), dtype=int))
    for name in ("community_louvain", "get_agreement_matrix"):
        doc = getattr(gu, name).__doc__
        assert "engine" in doc
    assert "does NOT reproduce" in gu.community_louvain.__doc__ and "seed_vector" in gu.get_agreement_matrix.__doc__

"""Betweenness and the module measures without a GPU: tests/centrality_reference.py (the numpy
restatement that test_centrality_gpu.py compares the device with) equals the golden outputs of the
reference's own functions (tests/golden/golden_centrality.npz, make_centrality_golden.py) and
networkx; wc_graph_betweenness and wc_graph_modules validate every argument before any device work
(the pointers are fake); sigchain.graph_betweenness, sigchain.graph_module_measures and the graph_utils
facades refuse bad names, dtypes, ranks, N > 96 and negative lengths before they touch the device.

Bounds.  Betweenness on the six path cases: exactly equal (their shortest paths are unique, gap >= 1e-9
in golden_graph.npz, so every value is an integer; the sums are centrality_reference.BC_SUMS), and
networkx's betweenness_centrality agrees to 0.  Binary graphs have tied paths, whose fractions add in
another order in betweenness_bin: 1e-12 relative, the project's fp64 bound.  Participation, z-score
and Q: |got - want| <= 1e-12 max(1, |want|) (centrality_reference.deviation_abs), absolute because z
and P are differences that may sit next to 0.

Measured here, restatement against the golden values:
  betweenness 0 (all six)   binary: 4.5e-16 against betweenness_bin, 0 against betweenness_wei
  participation 1.3e-15   z-score 0   Q against networkx 8.3e-16
"""
import ctypes
import functools

import numpy as np
import pytest

from tests import centrality_reference as cref
from tests import graph_reference as ref

BOUND = 1e-12
W, BC, CI, PART, Z, Q = (ctypes.c_void_p(v) for v in (1 << 40, 1 << 36, 1 << 44, 1 << 30, 1 << 32, 1 << 34))
MAT = 90 * 90 * 8


@functools.lru_cache(maxsize=None)
def golden():
    return cref.load_golden()


@functools.lru_cache(maxsize=None)
def inputs():
    got = ref.golden_inputs()
    for a in got.values():
        a.setflags(write=False)
    return got


def lib():
    from nremmodfc_amd import _lib
    return _lib.lib()


# ---- the restatement against the reference's own outputs ----

def test_golden_holds_the_cases():
    g = golden()
    assert set(g) == set(ref.ALL_CASES)
    for c in ref.PATH_CASES:
        bc = g[c]["bc"]
        assert (bc == np.rint(bc)).all() and bc.sum() == cref.BC_SUMS[c]      # unique shortest paths
    assert "bc" not in g["signed5"]
    for c in ref.ALL_CASES:
        for p in cref.PARTITIONS:
            assert g[c][f"part_{p}"].shape == g[c][f"z_{p}"].shape == (inputs()[c].shape[0],)


@pytest.mark.parametrize("case", ref.PATH_CASES)
def test_betweenness_equals_the_golden_exactly(case):
    L = ref.lengths_of(inputs()[case])
    got = cref.betweenness(L)
    np.testing.assert_array_equal(got, golden()[case]["bc"])
    nx = pytest.importorskip("networkx")
    G = nx.from_numpy_array(L, create_using=nx.DiGraph)
    other = nx.betweenness_centrality(G, weight="weight", normalized=False)
    np.testing.assert_array_equal(got, [other[k] for k in range(len(L))])


@pytest.mark.parametrize("case", cref.BINARY_CASES)
def test_binary_betweenness_equals_the_golden(case):
    a = (inputs()[case] != 0).astype(np.float64)
    got = cref.betweenness(a)
    dev = {k: ref.deviation(got, golden()[case][k]) for k in ("bc_bin", "bc_bin_wei")}
    print(case, dev)
    assert max(dev.values()) <= BOUND
    assert (got != np.rint(got)).any()                          # tied paths: fractions


def test_small_graphs_by_hand():
    path = np.zeros((3, 3))
    path[0, 1] = path[1, 0] = path[1, 2] = path[2, 1] = 1.0
    np.testing.assert_array_equal(cref.betweenness(path), [0.0, 2.0, 0.0])
    ring = np.zeros((6, 6))
    for k in range(6):
        ring[k, (k + 1) % 6] = ring[(k + 1) % 6, k] = 1.0
    np.testing.assert_array_equal(cref.betweenness(ring), np.full(6, 4.0))
    np.testing.assert_array_equal(cref.betweenness(np.array([[0.0, 3.0], [3.0, 0.0]])), [0.0, 0.0])
    bc = golden()["pendant12"]["bc"]
    assert bc[11] == 0.0 and bc[10] == 0.0 and bc[0] >= 2 * 9   # every path to the pendant goes through node 0


@pytest.mark.parametrize("case", ref.ALL_CASES)
def test_module_measures_equal_the_golden(case):
    w, g = inputs()[case], golden()[case]
    dev = {"part": 0.0, "z": 0.0}
    for p in cref.PARTITIONS:
        ci = cref.partition(p, w.shape[0])
        dev["part"] = max(dev["part"], cref.deviation_abs(cref.participation(w, ci), g[f"part_{p}"]))
        dev["z"] = max(dev["z"], cref.deviation_abs(cref.zscore(w, ci), g[f"z_{p}"]))
        if case == "dir24":
            for d in ("in", "out"):
                dev["part"] = max(dev["part"], cref.deviation_abs(cref.participation(w, ci, d), g[f"part_{p}_{d}"]))
            for f in (1, 2, 3):
                dev["z"] = max(dev["z"], cref.deviation_abs(cref.zscore(w, ci, f), g[f"z_{p}_{f}"]))
    print(case, dev)
    assert max(dev.values()) <= BOUND
    assert (g["z_singletons"] == 0).all() and g["z_lonely"][0] == 0.0     # single-member modules: 0/0 -> 0


def test_exact_zeros_of_the_module_measures():
    w = np.array(inputs()["pendant12"])
    ci = cref.partition("mod4", 12)
    assert cref.participation(w, ci)[11] == 0.0                 # no neighbours: strength 0
    assert golden()["pendant12"]["part_mod4"][11] == 0.0
    clique = np.ones((8, 8)) - np.eye(8)
    np.testing.assert_array_equal(cref.zscore(clique, cref.partition("hemi", 8)), np.zeros(8))   # equal degrees


@pytest.mark.parametrize("case", ["sc", "dir24"])
def test_modularity_against_networkx(case):
    nx = pytest.importorskip("networkx")
    w = inputs()[case]
    directed = case == "dir24"
    G = nx.from_numpy_array(w, create_using=nx.DiGraph if directed else nx.Graph)
    for p in cref.PARTITIONS:
        ci = cref.partition(p, w.shape[0])
        groups = [set(np.flatnonzero(ci == m).tolist()) for m in range(ci.max() + 1)]
        for gamma in (1.0, 0.7):
            want = nx.algorithms.community.modularity(G, groups, weight="weight", resolution=gamma)
            dev = cref.deviation_abs(cref.modularity(w, ci, gamma), want)
            print(case, p, gamma, want, dev)
            assert dev <= BOUND
    assert abs(cref.modularity(w, np.zeros(w.shape[0], int))) <= BOUND    # one module: Q = 1 - 1


def test_deviation_abs():
    want = np.array([0.0, 1e-20, 5.0, 1e6, np.nan])
    assert cref.deviation_abs(want, want) == 0.0
    assert abs(cref.deviation_abs([1e-13, 1e-20, 5.0, 1e6, np.nan], want) - 1e-13) < 1e-25    # absolute near 0
    assert abs(cref.deviation_abs([0.0, 1e-20, 5.0, 1e6 + 1e-3, np.nan], want) - 1e-9) < 1e-12  # relative above 1
    assert cref.deviation_abs([0.0, 1e-20, 5.0, 1e6, 0.0], want) == np.inf
    assert cref.deviation_abs([np.nan, 1e-20, 5.0, 1e6, np.nan], want) == np.inf
    assert cref.deviation_abs([0.0, 1e-20], want) == np.inf


# ---- the C ABI ----

def between(L, B=1, N=90, w=W, lengths=0, bc=BC):
    return L.wc_graph_betweenness(B, N, w, lengths, bc, None)


def modules(L, B=1, N=90, K=4, w=W, ci=CI, degree=0, zflag=0, gamma=1.0, part=PART, z=Z, q=Q):
    return L.wc_graph_modules(B, N, K, w, ci, degree, zflag, gamma, part, z, q, None)


def at(p, off):
    return ctypes.c_void_p(p.value + off)


@pytest.mark.parametrize("call,name,outs", [
    (between, b"wc_graph_betweenness", ("bc",)),
    (modules, b"wc_graph_modules", ("part", "z", "q")),
])
def test_entry_points_validate_without_device_work(call, name, outs):
    L = lib()
    err = L.wc_last_error
    assert call(L, B=0) == -1 and b"B < 1" in err() and name in err()
    assert call(L, B=-3) == -1
    assert call(L, N=1) == -1 and b"N < 2" in err()
    assert call(L, N=0) == -1 and call(L, N=-90) == -1
    assert call(L, N=97) == -2 and b"96" in err()
    assert call(L, N=1000) == -2
    assert call(L, w=None) == -1 and b"NULL" in err()
    assert call(L, **{o: None for o in outs}) == -1 and b"NULL" in err()
    assert call(L, w=at(W, 4)) == -1 and b"8-byte" in err()
    for o in outs:
        # an output that starts at w, ends one element into it, or starts at its last element
        assert call(L, B=2, **{o: W}) == -1 and b"alias" in err(), o
        assert call(L, B=2, **{o: at(W, 2 * MAT - 8)}) == -1 and b"alias" in err(), o
        assert call(L, B=2, **{o: at(W, -8)}) == -1 and b"alias" in err(), o
        assert call(L, **{o: at(BC, 4)}) == -1 and b"8-byte" in err(), o


def test_modules_validates_its_own_arguments():
    L = lib()
    err = L.wc_last_error
    for K in (0, -1, 91):
        assert modules(L, K=K) == -1 and b"K" in err()
    assert modules(L, ci=None) == -1 and b"ci is NULL" in err()
    assert modules(L, ci=at(CI, 2)) == -1 and b"4-byte" in err()
    for degree in (-1, 2):
        assert modules(L, degree=degree) == -1 and b"degree" in err()
    for zflag in (-1, 4):
        assert modules(L, zflag=zflag) == -1 and b"zflag" in err()
    for o in ("part", "z", "q"):
        assert modules(L, B=2, **{o: CI}) == -1 and b"alias ci" in err(), o
        assert modules(L, B=2, **{o: at(CI, 2 * 90 * 4 - 8)}) == -1 and b"alias ci" in err(), o
    for o in ("part", "z", "q"):                                 # one output alone is enough, before the launch
        others = {x: None for x in ("part", "z", "q") if x != o}
        assert modules(L, K=0, **others) == -1 and b"K" in err()


def test_header_and_abi_version():
    import os
    import re
    hdr = open(os.path.join(os.path.dirname(__file__), "..", "include", "wcsde.h")).read()
    assert re.search(r"#define WCSDE_ABI_VERSION 7\b", hdr)
    for fn in ("wc_graph_betweenness", "wc_graph_modules"):
        assert re.search(rf"\bint {fn}\(", hdr)
    assert lib().wcsde_abi_version() == 7


# ---- the Python layers ----

def test_graph_betweenness_refuses_before_touching_the_device():
    import torch

    from nremmodfc_amd import sigchain
    ok = torch.zeros((2, 5, 5), dtype=torch.float64)
    for t in (ok.float(), ok[0, 0], ok[None], torch.zeros((2, 5, 4), dtype=torch.float64), ok.numpy(), None,
              torch.zeros((5, 5), dtype=torch.complex128)):
        with pytest.raises(TypeError, match="graph_betweenness"):
            sigchain.graph_betweenness(t)
    for n in (97, 1000, 1):
        with pytest.raises(ValueError, match="96"):
            sigchain.graph_betweenness(torch.zeros((1, n, n), dtype=torch.float64))
    assert "betweenness" not in sigchain.GRAPH_MEASURES          # beside graph_measures, not inside it


def test_graph_module_measures_refuses_before_touching_the_device():
    import torch

    from nremmodfc_amd import sigchain
    f = sigchain.graph_module_measures
    assert sigchain.GRAPH_MODULE_MEASURES == ("participation", "zscore", "modularity")
    ok = torch.zeros((2, 5, 5), dtype=torch.float64)
    ci = torch.zeros((2, 5), dtype=torch.int32)
    for bad in ("betweenness", ("zscore", "Q"), ("zscore", None), ()):
        with pytest.raises(ValueError, match="measure"):
            f(None, None, measures=bad)                          # before the tensors are looked at
    with pytest.raises(ValueError, match="degree"):
        f(ok, ci, degree="both")
    for zflag in (-1, 4, 1.0, True, None):
        with pytest.raises(ValueError, match="zflag"):
            f(ok, ci, zflag=zflag)
    for t in (ok.float(), ok[0, 0], ok[None], torch.zeros((2, 5, 4), dtype=torch.float64), ok.numpy(), None):
        with pytest.raises(TypeError, match="w must be"):
            f(t, ci)
    for n in (97, 1):
        with pytest.raises(ValueError, match="96"):
            f(torch.zeros((1, n, n), dtype=torch.float64), torch.zeros(n, dtype=torch.int32))
    for c in (ci.long(), ci.double(), ci[:, :4], ci[:1], ci[None], torch.zeros((), dtype=torch.int32), ci.numpy(),
              None, [0] * 5):
        with pytest.raises(TypeError, match="ci must be"):
            f(ok, c)
    for k in (0, 6, -1):
        with pytest.raises(ValueError, match="n_modules"):
            f(ok, ci, n_modules=k)


def test_facades_refuse_before_touching_the_device():
    from nremmodfc_amd import graph_utils as gu
    w = ref.random_graph(6, 0.8, 0)
    ci = np.arange(6) % 2
    every = (gu.betweenness_wei, gu.betweenness_bin, functools.partial(gu.participation_coef, ci=ci),
             functools.partial(gu.module_degree_zscore, ci=ci))
    for f in every:
        for n in (97, 200):
            with pytest.raises(ValueError, match="96"):
                f(np.zeros((n, n)))
        for shape in ((6,), (2, 2, 6, 6), (6, 5), (2, 6, 5), (0, 6, 6), (1, 1)):
            with pytest.raises(ValueError):
                f(np.zeros(shape))
    neg, nan = w.copy(), w.copy()
    neg[1, 2] = -0.5
    nan[3, 4] = np.nan
    for bad in (neg, nan, np.stack([w, neg])):
        with pytest.raises(ValueError, match="negative or NaN"):
            gu.betweenness_wei(bad)
    for bad_ci in (np.arange(5), np.zeros((2, 6)), np.zeros((1, 1, 6)), 3):
        with pytest.raises(ValueError, match="ci"):
            gu.participation_coef(w, bad_ci)
        with pytest.raises(ValueError, match="ci"):
            gu.module_degree_zscore(w, bad_ci)
    with pytest.raises(ValueError, match="ci"):
        gu.participation_coef(np.stack([w, w]), np.zeros((3, 6)))
    with pytest.raises(ValueError, match="degree"):
        gu.participation_coef(w, ci, degree="both")
    for flag in (4, -1, 0.5, True):
        with pytest.raises(ValueError, match="flag"):
            gu.module_degree_zscore(w, ci, flag=flag)

"""Betweenness and the module measures on the device (wc_graph_betweenness and wc_graph_modules through
sigchain.graph_betweenness, sigchain.graph_module_measures and the graph_utils facades) against
tests/centrality_reference.py, the numpy restatement that test_centrality_cpu.py pins to the
reference's own outputs, and against those outputs directly (tests/golden/golden_centrality.npz).

Bounds.  Betweenness where the shortest paths are unique (every weighted graph here asserts
second_best_gap >= 1e-9): exactly equal, every value is an integer.  Binary graphs carry tied paths,
whose fractions the device adds in another order: 1e-12 relative (graph_reference.deviation; a 0 must
be 0), the project's fp64 bound.  Participation, z-score and Q: |got - want| <= 1e-12 max(1, |want|)
(centrality_reference.deviation_abs), absolute because z and P are differences that may sit next to 0,
where a relative bound measures the cancellation and not the kernel.

N: 2 and 3, 16 and 17, 64 and 65 (a lane's second node begins at 65), 90, and 96 dense (the limit).

Measured on MI355X, largest over the matrices of a test:
  betweenness, weighted graphs (N = 2 .. 96, B = 5, golden cases, composition): 0, exactly equal everywhere
  betweenness, binary graphs: N = 8 0, 17 1.3e-16, 33 2.3e-16, 65 4.0e-16; fc_thr 5.6e-16 against
    betweenness_bin and 7.2e-16 against betweenness_wei, dir24 3.6e-16 against both
  participation 1.1e-15 (sc, hemispheres)   z-score 8.5e-15 (N = 96)   Q 4.1e-15
No measure needs more than the 1e-12 bound.
"""
import functools

import numpy as np
import pytest
import torch

from nremmodfc_amd import graph_utils as gu
from nremmodfc_amd import sigchain as wsg
from tests import centrality_reference as cref
from tests import graph_reference as ref
from tests.test_graph_gpu import MIN_GAP, SIZES, frozen, graph, two_components

pytestmark = pytest.mark.gpu

BOUND = 1e-12
MODULE_SIZES = (2, 17, 65, 96)


@functools.lru_cache(maxsize=None)
def golden():
    return cref.load_golden()


@functools.lru_cache(maxsize=None)
def inputs():
    return {k: frozen(v) for k, v in ref.golden_inputs().items()}


@functools.lru_cache(maxsize=None)
def reference(n, density, seed, directed=False):
    """centrality_reference.betweenness of graph(...), computed once, read only; unique shortest paths asserted."""
    L = ref.lengths_of(graph(n, density, seed, directed))
    if n > 2:
        assert ref.second_best_gap(L, ref.floyd_warshall(L)[0]) >= MIN_GAP
    return frozen(cref.betweenness(L))


@functools.lru_cache(maxsize=None)
def binary(n):
    return frozen((ref.random_graph(n, 0.3 if n > 8 else 0.5, 200 + n) != 0).astype(np.float64))


def device_bc(w, **kw):
    return wsg.graph_betweenness(torch.from_numpy(np.array(w)).cuda(), **kw).cpu().numpy()


def device_modules(w, ci, measures=wsg.GRAPH_MODULE_MEASURES, **kw):
    got = wsg.graph_module_measures(torch.from_numpy(np.array(w)).cuda(),
                                    torch.from_numpy(np.array(ci, dtype=np.int32)).cuda(), measures, **kw)
    return {m: v.cpu().numpy() for m, v in got.items()}


def host_modules(w, ci, degree="undirected", zflag=0, gamma=1.0):
    return {"participation": cref.participation(w, ci, degree), "zscore": cref.zscore(w, ci, zflag),
            "modularity": cref.modularity(w, ci, gamma)}


def check_modules(got, want, tag):
    dev = {m: cref.deviation_abs(got[m], want[m]) for m in got}
    print(f"{tag}: " + "  ".join(f"{m} {v:.1e}" for m, v in dev.items()))
    for m, v in dev.items():
        assert v <= BOUND, (tag, m, v)


# ---- betweenness ----

@pytest.mark.parametrize("n", list(SIZES))
def test_betweenness_sizes(n):
    w, want = graph(n, SIZES[n], n), reference(n, SIZES[n], n)
    got = device_bc(w[None])
    assert got.shape == (1, n) and got.dtype == np.float64
    np.testing.assert_array_equal(got[0], want)
    np.testing.assert_array_equal(device_bc(w), got[0])          # [N][N] in, no batch axis out
    if n == 2:
        assert (got == 0).all()


def test_betweenness_by_hand():
    path = np.zeros((3, 3))
    path[0, 1] = path[1, 0] = path[1, 2] = path[2, 1] = 0.5
    np.testing.assert_array_equal(device_bc(path), [0.0, 2.0, 0.0])
    ring = np.zeros((6, 6))
    for k in range(6):
        ring[k, (k + 1) % 6] = ring[(k + 1) % 6, k] = 1.0
    np.testing.assert_array_equal(device_bc(ring), np.full(6, 4.0))          # two tied paths to the far node


def test_betweenness_batch_of_five_different_matrices():
    """Five matrices of five densities in one call: a per-matrix offset bug shows in the middle ones."""
    dens = (0.1, 0.3, 0.5, 0.8, 1.0)
    ws = np.stack([graph(65, d, 100 + k) for k, d in enumerate(dens)])
    got = device_bc(ws)
    for k, d in enumerate(dens):
        np.testing.assert_array_equal(got[k], reference(65, d, 100 + k))
        np.testing.assert_array_equal(device_bc(ws[k]), got[k])              # the same bits on its own
    np.testing.assert_array_equal(device_bc(ws), got)                        # and in a second call


@pytest.mark.parametrize("case", ref.PATH_CASES)
def test_betweenness_golden_cases(case):
    """The reference's own betweenness_wei: the shipped SC, the dense and the thresholded empirical FC, the
    random symmetric and directed (dir24) graphs, the isolated and pendant nodes."""
    got = device_bc(inputs()[case])
    np.testing.assert_array_equal(got, golden()[case]["bc"])
    assert got.sum() == cref.BC_SUMS[case]


@pytest.mark.parametrize("n", [8, 17, 33, 65])
def test_betweenness_binary_graphs_with_ties(n):
    a = binary(n)
    want = cref.betweenness(a)
    assert (want != np.rint(want)).any()                         # tied paths: fractions
    got = device_bc(a, lengths=True)
    dev = ref.deviation(got, want)
    print(f"binary N={n}: {dev:.1e}")
    assert dev <= BOUND
    np.testing.assert_array_equal(device_bc(a), got)             # 1/1: weights or lengths, the same bits
    np.testing.assert_array_equal(gu.betweenness_bin(np.array(a) * 0.3), got)


@pytest.mark.parametrize("case", cref.BINARY_CASES)
def test_betweenness_binary_golden(case):
    a = (inputs()[case] != 0).astype(np.float64)
    got = device_bc(a, lengths=True)
    dev = {k: ref.deviation(got, golden()[case][k]) for k in ("bc_bin", "bc_bin_wei")}
    print(f"binary {case}: {dev}")
    assert max(dev.values()) <= BOUND


def test_betweenness_with_unreachable_nodes():
    g = golden()["pendant12"]["bc"]
    got = device_bc(inputs()["pendant12"])
    assert got[11] == 0.0 and got[10] == 0.0                     # isolated; pendant: on nobody's way
    assert got[0] == g[0] and got[0] >= 18.0                     # the pendant's neighbour carries its paths
    w = two_components()
    np.testing.assert_array_equal(device_bc(w), cref.betweenness(ref.lengths_of(w)))
    lone = np.zeros((5, 5))                                      # no edge at all
    np.testing.assert_array_equal(device_bc(lone), np.zeros(5))


def test_betweenness_lengths_flag():
    """lengths=True on invert(w) is lengths=False on w, bit for bit."""
    for w in (graph(65, 0.3, 101), inputs()["dir24"], inputs()["pendant12"]):
        np.testing.assert_array_equal(device_bc(w), device_bc(gu.invert(np.array(w)), lengths=True))


def test_betweenness_ignores_the_diagonal():
    w = np.array(graph(17, 0.5, 17))
    want = device_bc(w)
    np.fill_diagonal(w, 0.37)
    np.testing.assert_array_equal(device_bc(w), want)


def test_betweenness_negative_or_nan_spoils_its_matrix_only():
    ws = np.stack([graph(17, 0.5, 17), graph(17, 0.5, 19), graph(17, 0.3, 18)])
    clean = device_bc(ws)
    assert np.isfinite(clean).all()
    for value, k in ((-0.25, 1), (np.nan, 2), (np.nan, 0)):
        bad = np.array(ws)
        bad[k, 3, 5] = value
        got = device_bc(bad)
        assert np.isnan(got[k]).all()
        others = [j for j in range(3) if j != k]
        np.testing.assert_array_equal(got[others], clean[others])


# ---- module measures ----

@pytest.mark.parametrize("n", MODULE_SIZES)
@pytest.mark.parametrize("p", cref.PARTITIONS)
def test_module_sizes(n, p):
    w, ci = graph(n, SIZES.get(n, 0.3), n), cref.partition(p, n)
    got = device_modules(w[None], ci[None])
    assert got["participation"].shape == got["zscore"].shape == (1, n) and got["modularity"].shape == (1,)
    check_modules({m: v[0] for m, v in got.items()}, host_modules(w, ci), f"N={n} {p}")
    single = device_modules(w, ci, n_modules=int(ci.max()) + 1)  # [N][N] and [N] in, no batch axis out
    for m, v in single.items():
        np.testing.assert_array_equal(v, got[m][0])


@pytest.mark.parametrize("case", ref.ALL_CASES)
def test_module_golden_cases(case):
    """The reference's own participation_coef and module_degree_zscore; Q against the restatement."""
    w, g = inputs()[case], golden()[case]
    for p in cref.PARTITIONS:
        ci = cref.partition(p, w.shape[0])
        got = device_modules(w, ci)
        check_modules(got, {"participation": g[f"part_{p}"], "zscore": g[f"z_{p}"],
                            "modularity": cref.modularity(w, ci)}, f"{case} {p}")


@pytest.mark.parametrize("p", cref.PARTITIONS)
def test_module_directed_variants(p):
    w, g = inputs()["dir24"], golden()["dir24"]
    ci = cref.partition(p, 24)
    for degree in ("in", "out"):
        got = device_modules(w, ci, "participation", degree=degree)
        check_modules(got, {"participation": g[f"part_{p}_{degree}"]}, f"dir24 {p} {degree}")
    np.testing.assert_array_equal(device_modules(w, ci, "participation", degree="out")["participation"],
                                  device_modules(w, ci, "participation")["participation"])
    for flag in (0, 1, 2, 3):
        got = device_modules(w, ci, "zscore", zflag=flag)
        check_modules(got, {"zscore": g[f"z_{p}_{flag}" if flag else f"z_{p}"]}, f"dir24 {p} flag {flag}")
    for gamma in (1.0, 0.7):
        got = device_modules(w, ci, "modularity", gamma=gamma)
        check_modules(got, {"modularity": cref.modularity(w, ci, gamma)}, f"dir24 {p} gamma {gamma}")


def test_module_exact_zeros():
    w = inputs()["pendant12"]
    got = device_modules(w, cref.partition("mod4", 12))
    assert got["participation"][11] == 0.0                       # no neighbours: strength 0
    got = device_modules(w, cref.partition("lonely", 12))
    assert got["zscore"][0] == 0.0                               # a single-member module
    got = device_modules(graph(17, 0.5, 17), cref.partition("singletons", 17))
    assert (got["zscore"] == 0.0).all()
    clique = np.ones((8, 8)) - np.eye(8)
    got = device_modules(clique, cref.partition("hemi", 8))
    assert (got["zscore"] == 0.0).all()                          # equal within-module degrees
    assert got["modularity"] == cref.modularity(clique, cref.partition("hemi", 8))


def test_module_batch_with_its_own_partitions_and_outputs_alone():
    ws = np.stack([graph(17, 0.5, 17), graph(17, 0.5, 19), graph(17, 0.3, 18)])
    cis = np.stack([cref.partition(p, 17) for p in ("mod4", "hemi", "lonely")])
    every = device_modules(ws, cis)
    for k in range(3):
        check_modules({m: v[k] for m, v in every.items()}, host_modules(ws[k], cis[k]), f"B=3 matrix {k}")
    for m in wsg.GRAPH_MODULE_MEASURES:
        got = device_modules(ws, cis, (m,))
        assert tuple(got) == (m,)
        np.testing.assert_array_equal(got[m], every[m])
    shared = device_modules(ws, cis[0])                          # one [N] partition for every matrix
    for k in range(3):
        check_modules({m: v[k] for m, v in shared.items()}, host_modules(ws[k], cis[0]), f"shared ci, matrix {k}")


def test_module_label_out_of_range_spoils_its_matrix_only():
    ws = np.stack([graph(17, 0.5, 17), graph(17, 0.5, 19), graph(17, 0.3, 18)])
    cis = np.stack([cref.partition("mod4", 17)] * 3)
    clean = device_modules(ws, cis, n_modules=4)
    for label in (4, -1, 1 << 30):
        bad = np.array(cis)
        bad[1, 7] = label
        got = device_modules(ws, bad, n_modules=4)
        for m in wsg.GRAPH_MODULE_MEASURES:
            assert np.isnan(got[m][1]).all(), m
            np.testing.assert_array_equal(got[m][[0, 2]], clean[m][[0, 2]])
    bad = np.array(cis)
    bad[1, 7] = 4                                                # legal where every label below N is
    got = device_modules(ws, bad)
    assert np.isfinite(got["zscore"]).all() and np.isfinite(got["modularity"]).all()


def test_module_negative_weights_are_summed():
    w, g = inputs()["signed5"], golden()["signed5"]
    ci = cref.partition("hemi", 5)
    got = device_modules(w, ci)
    assert (w < 0).any() and np.isfinite(got["participation"]).all()
    check_modules(got, {"participation": g["part_hemi"], "zscore": g["z_hemi"], "modularity": cref.modularity(w, ci)},
                  "signed5 hemi")


# ---- facades and composition ----

def test_facades_on_the_shipped_sc():
    W, g = np.array(inputs()["sc"]), golden()["sc"]
    np.testing.assert_array_equal(gu.betweenness_wei(gu.invert(W)), g["bc"])
    labels = np.array(["left", "right"])[cref.partition("hemi", 90)]         # any labels: np.unique orders them
    assert cref.deviation_abs(gu.participation_coef(W, labels), g["part_hemi"]) <= BOUND
    assert cref.deviation_abs(gu.module_degree_zscore(W, labels), g["z_hemi"]) <= BOUND
    assert cref.deviation_abs(gu.participation_coef(W, 10 * cref.partition("mod4", 90) + 3), g["part_mod4"]) <= BOUND
    a = (np.array(inputs()["fc_thr"]) != 0).astype(np.float64)
    assert ref.deviation(gu.betweenness_bin(a), golden()["fc_thr"]["bc_bin"]) <= BOUND
    d = np.array(inputs()["dir24"])
    assert cref.deviation_abs(gu.participation_coef(d, np.arange(24) % 4, "in"), golden()["dir24"]["part_mod4_in"]) <= BOUND
    assert cref.deviation_abs(gu.module_degree_zscore(d, np.arange(24) % 4, 3), golden()["dir24"]["z_mod4_3"]) <= BOUND
    assert (W == inputs()["sc"]).all()                           # the caller's matrix is left alone


def test_facade_stacks_equal_the_single_calls():
    stack = np.stack([inputs()[c] for c in ("sc", "fc_thr", "rand90")])
    L = gu.invert(np.array(stack))
    np.testing.assert_array_equal(gu.betweenness_wei(L), np.stack([gu.betweenness_wei(x) for x in L]))
    np.testing.assert_array_equal(gu.betweenness_bin(stack), np.stack([gu.betweenness_bin(x) for x in stack]))
    cis = np.stack([cref.partition(p, 90) for p in ("mod4", "hemi", "lonely")])
    for f in (gu.participation_coef, gu.module_degree_zscore):
        np.testing.assert_array_equal(f(stack, cis), np.stack([f(w, c) for w, c in zip(stack, cis)]))
        np.testing.assert_array_equal(f(stack, cis[0]), np.stack([f(w, cis[0]) for w in stack]))


def test_composes_with_fc_metrics():
    rng = np.random.default_rng(11)
    B, N, M = 3, 17, 64
    bold = torch.from_numpy(rng.standard_normal((M, B * N))).cuda()
    fc, _, _ = wsg.fc_metrics(bold, B, N, kuramoto=False, want_fc=True)
    fc.clamp_(min=0.0)
    fc.diagonal(dim1=1, dim2=2).zero_()
    ci = torch.from_numpy(cref.partition("mod4", N)).cuda()
    bc = wsg.graph_betweenness(fc).cpu().numpy()
    mod = {m: v.cpu().numpy() for m, v in wsg.graph_module_measures(fc, ci, n_modules=4).items()}
    host = fc.cpu().numpy()
    for k in range(B):
        L = ref.lengths_of(host[k])
        assert ref.second_best_gap(L, ref.floyd_warshall(L)[0]) >= MIN_GAP
        np.testing.assert_array_equal(bc[k], cref.betweenness(L))
        check_modules({m: v[k] for m, v in mod.items()}, host_modules(host[k], cref.partition("mod4", N)), f"fc {k}")

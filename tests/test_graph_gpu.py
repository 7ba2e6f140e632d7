"""Graph measures on the device (wc_graph_paths, wc_graph_local_efficiency, wc_graph_clustering through
sigchain.graph_measures and the graph_utils facades) against tests/graph_reference.py, the numpy
Floyd-Warshall restatement that test_graph_cpu.py pins to the reference's own outputs, and against
those outputs directly (tests/golden/golden_graph.npz).

Deviation: graph_reference.deviation, the largest |got - want| / |want| over the finite non-zero entries
of want; where want is 0, infinite or NaN the device must give the same, so an inf out of place or a
local efficiency or clustering that should be exactly 0 fails whatever the bound.  Bounds: hops and
degrees exactly equal (every compared graph asserts unique shortest paths: the second-best last edge at
least 1e-9 longer, relative); everything else 1e-12, the project's fp64 bound.

N: 2 and 3, 16 and 17 (an edge of the 16 x 16 thread grid and of the clustering tiles), 64 and 65 (a
wave), 90, and 96 dense (the limit; the local efficiency runs on 95 neighbours).

Measured on MI355X, largest over the matrices of a test (dist / charpath, efficiency, ecc, radius,
diameter / local_efficiency / clustering / transitivity / strengths; hops and degrees exact everywhere):
  N = 2 .. 96, B = 1:   0 / 3.4e-16 / 4.0e-16 / 7.0e-16 / 6.3e-16 / 0   (dist: the same operations as numpy's)
  B = 5, N = 65:        0 / 4.3e-16 / 5.0e-16 / 5.6e-16 / 4.8e-16 / 0
  golden cases:         3.9e-16 / 6.5e-16 / 4.1e-16 / 7.1e-16 / 6.1e-16 / 0   (the reference's Dijkstra)
No measure needs more than the 1e-12 bound.
"""
import functools

import numpy as np
import pytest
import torch

from nremmodfc_amd import graph_utils as gu
from nremmodfc_amd import sigchain as wsg
from tests import graph_reference as ref

pytestmark = pytest.mark.gpu

BOUND = 1e-12
MIN_GAP = 1e-9
SIZES = {2: 1.0, 3: 1.0, 16: 0.5, 17: 0.5, 64: 0.3, 65: 0.3, 90: 0.4, 96: 1.0}   # N: density
STATS = ("charpath", "efficiency", "radius", "diameter")


def frozen(a):
    a = np.asarray(a)
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def golden():
    return ref.load_golden()


@functools.lru_cache(maxsize=None)
def graph(n, density, seed, directed=False):
    return frozen(ref.random_graph(n, density, seed, directed))


@functools.lru_cache(maxsize=None)
def reference(n, density, seed, directed=False):
    """graph_reference.measures of graph(...), computed once, read only; unique shortest paths asserted."""
    w = graph(n, density, seed, directed)
    want = {m: frozen(v) for m, v in ref.measures(w).items()}
    assert ref.second_best_gap(ref.lengths_of(w), want["dist"]) >= MIN_GAP
    return want


def device(w, measures=wsg.GRAPH_MEASURES, **kw):
    got = wsg.graph_measures(torch.from_numpy(np.array(w)).cuda(), measures, **kw)
    return {m: v.cpu().numpy() for m, v in got.items()}


def check(got, want, tag, paths=True):
    """Asserts the bounds of the module docstring on every measure of one matrix; prints the deviations."""
    np.testing.assert_array_equal(got["degrees"], want["degrees"])
    dev = {m: ref.deviation(got[m], want[m]) for m in ("clustering", "transitivity", "strengths")}
    if paths:
        np.testing.assert_array_equal(got["hops"], want["hops"])
        np.testing.assert_array_equal(np.isinf(got["dist"]), np.isinf(want["dist"]))
        dev.update({m: ref.deviation(got[m], want[m]) for m in ("dist", "ecc", "local_efficiency") + STATS})
    print(f"{tag}: " + "  ".join(f"{m} {v:.1e}" for m, v in dev.items()))
    for m, v in dev.items():
        assert v <= BOUND, (tag, m, v)
    return dev


@pytest.mark.parametrize("n", list(SIZES))
def test_sizes(n):
    w, want = graph(n, SIZES[n], n), reference(n, SIZES[n], n)
    got = device(w[None])
    assert got["dist"].shape == (1, n, n) and got["hops"].dtype == np.int32 and got["degrees"].dtype == np.int32
    assert got["charpath"].shape == (1,) and got["ecc"].shape == (1, n) and got["local_efficiency"].shape == (1, n)
    check({m: v[0] for m, v in got.items()}, want, f"N={n}")
    single = device(w)                                          # [N][N] in, no batch axis out
    for m, v in single.items():
        np.testing.assert_array_equal(v, got[m][0])


def test_batch_of_five_different_matrices():
    """Five matrices of five densities in one call: a per-matrix offset bug shows in the middle ones."""
    dens = (0.1, 0.3, 0.5, 0.8, 1.0)
    ws = np.stack([graph(65, d, 100 + k) for k, d in enumerate(dens)])
    got = device(ws)
    for k, d in enumerate(dens):
        check({m: v[k] for m, v in got.items()}, reference(65, d, 100 + k), f"B=5 N=65 density {d}")
        one = device(ws[k])                                     # and the same bits as on its own
        for m, v in one.items():
            np.testing.assert_array_equal(v, got[m][k])


@pytest.mark.parametrize("only", [STATS, ("hops",), ("ecc",)])
def test_outputs_alone(only):
    ws = np.stack([graph(17, 0.5, 17), graph(17, 0.3, 18)])
    every = device(ws)
    got = device(ws, only)
    assert tuple(got) == tuple(only)
    for m in only:
        np.testing.assert_array_equal(got[m], every[m])
    for k, seed in enumerate((17, 18)):
        want = reference(17, (0.5, 0.3)[k], seed)
        for m in only:
            if m == "hops":
                np.testing.assert_array_equal(got[m][k], want[m])
            else:
                assert ref.deviation(got[m][k], want[m]) <= BOUND


@pytest.mark.parametrize("case", ref.ALL_CASES)
def test_golden_cases(case):
    """The reference's own outputs: the shipped SC, the dense and the thresholded empirical FC, the random
    symmetric and directed graphs, the isolated and pendant nodes, the signed matrix (clustering only)."""
    g = golden()[case]
    paths = case in ref.PATH_CASES
    names = wsg.GRAPH_MEASURES if paths else wsg.GRAPH_CLUSTER_MEASURES
    got = device(g["w"], names)
    want = dict(g)
    if paths:
        want.update(zip(STATS, g["charpath"]))
        assert ref.deviation(got["efficiency"], g["efficiency"]) <= BOUND   # efficiency_wei(local=False)
    check(got, want, case, paths)


def test_isolated_and_pendant_nodes():
    g = golden()["pendant12"]
    got = device(g["w"])
    assert np.isinf(got["dist"][11, :11]).all() and np.isinf(got["dist"][:11, 11]).all()
    assert np.isfinite(got["dist"][:11, :11]).all() and (np.diag(got["dist"]) == 0).all()
    assert (got["hops"][11] == 0).all() and (got["hops"][:, 11] == 0).all()
    assert got["local_efficiency"][10] == 0.0 and got["local_efficiency"][11] == 0.0    # one neighbour, none
    assert got["clustering"][10] == 0.0 and got["clustering"][11] == 0.0
    assert np.isinf(got["charpath"]) and np.isinf(got["diameter"]) and np.isinf(got["ecc"]).all()
    assert 0 < got["efficiency"] < np.inf


def test_negative_entry_spoils_its_matrix_only():
    ws = np.stack([graph(17, 0.5, 17), graph(17, 0.5, 19), graph(17, 0.3, 18)])
    clean = device(ws)
    bad = np.array(ws)
    bad[1, 3, 5] = -0.25
    got = device(bad)
    for m in wsg.GRAPH_PATH_MEASURES + ("local_efficiency",):
        np.testing.assert_array_equal(got[m][0], clean[m][0])
        np.testing.assert_array_equal(got[m][2], clean[m][2])
        if m == "hops":
            assert (got[m][1] == -1).all()
        else:
            assert np.isnan(got[m][1]).all(), m
    for m in wsg.GRAPH_CLUSTER_MEASURES:                         # negative weights are legal there
        np.testing.assert_array_equal(got[m][0], clean[m][0])
        assert ref.deviation(got[m][1], ref.measures(bad[1], paths=False)[m]) <= BOUND
    nan = np.array(ws)
    nan[2, 0, 1] = np.nan
    got = device(nan, ("dist", "hops", "local_efficiency"))
    assert np.isnan(got["dist"][2]).all() and (got["hops"][2] == -1).all() and np.isnan(got["local_efficiency"][2]).all()
    np.testing.assert_array_equal(got["dist"][:2], clean["dist"][:2])


def test_lengths_flag():
    """lengths=True on invert(w) is lengths=False on w, bit for bit."""
    names = wsg.GRAPH_PATH_MEASURES
    for w in (graph(65, 0.3, 101), golden()["dir24"]["w"], golden()["pendant12"]["w"]):
        a, b = device(w, names), device(gu.invert(np.array(w)), names, lengths=True)
        for m in names:
            np.testing.assert_array_equal(a[m], b[m])


@functools.lru_cache(maxsize=None)
def two_components():
    """Seven nodes in two components (4 + 3): infinite distances, and no row of D without a finite one."""
    w = np.zeros((7, 7))
    w[:4, :4] = ref.random_graph(4, 1.0, 7)
    w[4:, 4:] = ref.random_graph(3, 1.0, 8)
    return frozen(w)


@pytest.mark.parametrize("which", ["two_components", "pendant12"])
def test_include_infinite_false(which):
    w = two_components() if which == "two_components" else golden()["pendant12"]["w"]
    D, _ = ref.floyd_warshall(ref.lengths_of(w))
    lam, eff, ecc, radius, diameter = gu.charpath(D, include_infinite=False)
    got = device(w, STATS + ("ecc", "dist"), include_infinite=False)
    assert np.isinf(got["dist"]).any() and np.isfinite([lam, eff, radius, diameter]).all()
    assert ref.deviation([got[m] for m in STATS], [lam, eff, radius, diameter]) <= BOUND
    assert ref.deviation(got["ecc"], ecc) <= BOUND              # NaN where a row has nothing left (node 11)
    assert np.isnan(ecc).sum() == (1 if which == "pendant12" else 0)
    if which == "pendant12":                                     # the reference's own charpath of its own D
        g = golden()["pendant12"]
        assert ref.deviation([got[m] for m in STATS[:3]], g["charpath_finite"][:3]) <= BOUND
        assert ref.deviation(got["ecc"][:11], g["ecc_finite"][:11]) <= BOUND
    with_inf = device(w, STATS)
    assert np.isinf(with_inf["charpath"]) and np.isinf(with_inf["diameter"])
    assert ref.deviation(with_inf["efficiency"], ref.charpath(D)[1]) <= BOUND


def test_facades_on_the_shipped_sc():
    g = golden()["sc"]
    W = np.array(g["w"])
    assert isinstance(gu.efficiency_wei(W), float)
    assert ref.deviation(gu.efficiency_wei(W), g["efficiency"]) <= BOUND
    assert ref.deviation(gu.efficiency_wei(W, local=True), g["local_efficiency"]) <= BOUND
    D, B = gu.distance_wei(gu.invert(W))
    assert ref.deviation(D, g["dist"]) <= BOUND and B.dtype == np.float64
    np.testing.assert_array_equal(B, g["hops"])
    assert ref.deviation(gu.clustering_coef_wu(W), g["clustering"]) <= BOUND
    assert ref.deviation(gu.transitivity_wu(W), g["transitivity"]) <= BOUND
    assert ref.deviation(gu.strengths_und(W), g["strengths"]) <= BOUND
    np.testing.assert_array_equal(gu.degrees_und(W), g["degrees"])
    assert (W == g["w"]).all()                                   # the caller's matrix is left alone


def test_facade_stacks_equal_the_single_calls():
    stack = np.stack([golden()[c]["w"] for c in ("sc", "fc_thr", "rand90")])
    for f in (gu.efficiency_wei, functools.partial(gu.efficiency_wei, local=True), gu.clustering_coef_wu,
              gu.transitivity_wu, gu.strengths_und, gu.degrees_und):
        np.testing.assert_array_equal(f(stack), np.stack([f(w) for w in stack]))
    D, B = gu.distance_wei(gu.invert(stack))
    for k, w in enumerate(stack):
        d, b = gu.distance_wei(gu.invert(w))
        np.testing.assert_array_equal(D[k], d)
        np.testing.assert_array_equal(B[k], b)


@pytest.mark.parametrize("case", ["sc", "rand90"])
def test_symmetric_input_gives_symmetric_results(case):
    """To 1e-12, not exactly: the sums of a path's lengths associate from either end (the reference's own
    D is asymmetric by 7e-15 on the SC)."""
    got = device(golden()[case]["w"], ("dist", "hops"))
    assert ref.deviation(got["dist"].T, got["dist"]) <= BOUND
    np.testing.assert_array_equal(got["hops"].T, got["hops"])


def test_composes_with_fc_metrics_and_hma():
    rng = np.random.default_rng(11)
    B, N, M = 3, 17, 64
    bold = torch.from_numpy(rng.standard_normal((M, B * N))).cuda()
    fc, _, _ = wsg.fc_metrics(bold, B, N, kuramoto=False, want_fc=True)
    wsg.hma(fc)                                                  # clips FC < 0 to 0 in place
    fc.diagonal(dim1=1, dim2=2).zero_()
    got = wsg.graph_measures(fc, ("efficiency", "local_efficiency", "clustering", "hops"))
    host = fc.cpu().numpy()
    for k in range(B):
        want = ref.measures(host[k])
        assert ref.second_best_gap(ref.lengths_of(host[k]), want["dist"]) >= MIN_GAP
        np.testing.assert_array_equal(got["hops"][k].cpu().numpy(), want["hops"])
        for m in ("efficiency", "local_efficiency", "clustering"):
            assert ref.deviation(got[m][k].cpu().numpy(), want[m]) <= BOUND

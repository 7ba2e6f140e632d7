"""The graph measures without a GPU: tests/graph_reference.py (the numpy Floyd-Warshall restatement that
test_graph_gpu.py compares the device with) equals the golden outputs of the reference's own functions
(tests/golden/golden_graph.npz, make_graph_golden.py) -- hops and degrees exactly, inf in the same
places, everything else to 1e-12 relative, the project's fp64 bound -- and SciPy's Dijkstra agrees on
D; wc_graph_paths, wc_graph_local_efficiency and wc_graph_clustering validate every argument before
any device work (the pointers are fake); sigchain.graph_measures and the graph_utils facades refuse bad
names, dtypes, ranks, negative weights and N > 96 before they touch the device.

Measured here, reference restatement against the golden values (largest relative deviation):
  dist 3.9e-16 (sc)  charpath 1.8e-16  efficiency 1.4e-16  ecc 3.6e-16  local_efficiency 3.2e-16
  clustering 5.0e-16 (rand90)  transitivity 5.4e-16 (signed5)  strengths 0
"""
import ctypes
import functools
import subprocess
import sys

import numpy as np
import pytest

from tests import graph_reference as ref

BOUND = 1e-12
W, DIST, HOPS, STATS, ECC = (ctypes.c_void_p(v) for v in (1 << 40, 1 << 36, 1 << 44, 1 << 30, 1 << 32))
MAT = 90 * 90 * 8


@functools.lru_cache(maxsize=None)
def golden():
    return ref.load_golden()


@functools.lru_cache(maxsize=None)
def restated(case):
    return ref.measures(golden()[case]["w"], paths=case in ref.PATH_CASES)


def lib():
    from nremmodfc_amd import _lib
    return _lib.lib()


# ---- the reference restatement against the reference's own outputs ----

def test_golden_holds_the_cases_and_the_inputs_are_reproducible():
    g = golden()
    assert tuple(g) == ref.ALL_CASES
    for name, w in ref.golden_inputs().items():
        np.testing.assert_array_equal(g[name]["w"], w)
    assert [g[c]["w"].shape[0] for c in ref.ALL_CASES] == [90, 90, 90, 90, 24, 12, 5]
    assert not (g["dir24"]["w"] == g["dir24"]["w"].T).all()
    assert (g["signed5"]["w"] < 0).any() and "dist" not in g["signed5"]
    for c in ref.PATH_CASES:
        assert g[c]["gap"] >= 1e-9                      # unique shortest paths: the hop counts are well defined
    assert np.isinf(g["pendant12"]["dist"]).sum() == 22 and not np.isinf(g["sc"]["dist"]).any()


@pytest.mark.parametrize("case", ref.PATH_CASES)
def test_reference_paths_equal_the_golden(case):
    g, got = golden()[case], restated(case)
    np.testing.assert_array_equal(got["hops"], g["hops"])
    np.testing.assert_array_equal(np.isinf(got["dist"]), np.isinf(g["dist"]))
    dev = {"dist": ref.deviation(got["dist"], g["dist"]),
           "charpath": ref.deviation([got["charpath"], got["efficiency"], got["radius"], got["diameter"]],
                                     g["charpath"]),
           "efficiency": ref.deviation(got["efficiency"], g["efficiency"]),
           "ecc": ref.deviation(got["ecc"], g["ecc"]),
           "local_efficiency": ref.deviation(got["local_efficiency"], g["local_efficiency"])}
    print(case, "  ".join(f"{k} {v:.1e}" for k, v in dev.items()))
    assert max(dev.values()) <= BOUND
    assert ref.deviation(ref.second_best_gap(ref.lengths_of(g["w"]), g["dist"]), g["gap"]) <= 1e-6
    # SciPy's Dijkstra as a second opinion on D
    assert ref.deviation(ref.scipy_distances(ref.lengths_of(g["w"])), g["dist"]) <= BOUND
    # include_infinite=False: rows with nothing left are passed over (the reference stores 1e20 there)
    lam, eff, ecc, radius, diameter = ref.charpath(g["dist"], include_infinite=False)
    some = ~np.isnan(ecc)
    assert ref.deviation(ecc[some], g["ecc_finite"][some]) <= BOUND
    assert (g["ecc_finite"][~some] == 1e20).all()
    want = np.array(g["charpath_finite"])
    if not some.all():
        want[3] = g["ecc_finite"][some].max()
    assert ref.deviation([lam, eff, radius, diameter], want) <= BOUND


@pytest.mark.parametrize("case", ref.ALL_CASES)
def test_reference_clustering_equals_the_golden(case):
    g, got = golden()[case], restated(case)
    np.testing.assert_array_equal(got["degrees"], g["degrees"])
    dev = {m: ref.deviation(got[m], g[m]) for m in ("clustering", "transitivity", "strengths")}
    print(case, "  ".join(f"{k} {v:.1e}" for k, v in dev.items()))
    assert max(dev.values()) <= BOUND


def test_pendant_and_isolated_nodes():
    g, got = golden()["pendant12"], restated("pendant12")
    for a in (g, got):
        assert a["local_efficiency"][10] == 0.0 and a["local_efficiency"][11] == 0.0   # one neighbour, none
        assert a["clustering"][10] == 0.0 and a["clustering"][11] == 0.0
        assert np.isinf(a["dist"][11, :11]).all() and np.isinf(a["dist"][:11, 11]).all()
        assert (a["hops"][11] == 0).all() and a["hops"][10, 0] == 1
    assert np.isinf(got["charpath"]) and np.isinf(got["diameter"]) and np.isfinite(got["efficiency"])


def test_deviation_refuses_a_moved_inf_or_zero():
    want = np.array([1.0, np.inf, 0.0, np.nan])
    assert ref.deviation(want, want) == 0.0
    assert ref.deviation([1.0, 1e300, 0.0, np.nan], want) == np.inf
    assert ref.deviation([1.0, np.inf, 1e-300, np.nan], want) == np.inf
    assert ref.deviation([1.0, np.inf, 0.0, 0.0], want) == np.inf
    assert abs(ref.deviation([1.0 + 1e-9, np.inf, 0.0, np.nan], want) - 1e-9) < 1e-15


# ---- the C ABI ----

def paths(L, B=1, N=90, w=W, lengths=0, inc=1, dist=DIST, hops=HOPS, stats=STATS, ecc=ECC):
    return L.wc_graph_paths(B, N, w, lengths, inc, dist, hops, stats, ecc, None)


def local(L, B=1, N=90, w=W, eloc=DIST):
    return L.wc_graph_local_efficiency(B, N, w, eloc, None)


def cluster(L, B=1, N=90, w=W, c=DIST, t=STATS, s=ECC, d=HOPS):
    return L.wc_graph_clustering(B, N, w, c, t, s, d, None)


def at(p, off):
    return ctypes.c_void_p(p.value + off)


@pytest.mark.parametrize("call,name,fp64,int32", [
    (paths, b"wc_graph_paths", ("dist", "stats", "ecc"), ("hops",)),
    (local, b"wc_graph_local_efficiency", ("eloc",), ()),
    (cluster, b"wc_graph_clustering", ("c", "t", "s"), ("d",)),
])
def test_entry_points_validate_without_device_work(call, name, fp64, int32):
    L = lib()
    err = L.wc_last_error
    outs = fp64 + int32
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
        size = 4 if o in int32 else 8
        assert call(L, B=2, **{o: W}) == -1 and b"alias" in err(), o
        assert call(L, B=2, **{o: at(W, 2 * MAT - size)}) == -1 and b"alias" in err(), o
        assert call(L, B=2, **{o: at(W, -size)}) == -1 and b"alias" in err(), o
    for o in outs:                                               # the int32 outputs too
        assert call(L, **{o: at(DIST, 4)}) == -1 and b"8-byte" in err(), o
    assert wcsde_abi(L) == 7


def wcsde_abi(L):
    import os
    import re
    hdr = open(os.path.join(os.path.dirname(__file__), "..", "include", "wcsde.h")).read()
    assert re.search(r"#define WCSDE_ABI_VERSION 7\b", hdr)
    for fn in ("wc_graph_paths", "wc_graph_local_efficiency", "wc_graph_clustering"):
        assert re.search(rf"\bint {fn}\(", hdr)
    return L.wcsde_abi_version()


def test_local_efficiency_grid_limit():
    L = lib()
    assert local(L, B=(1 << 31) // 96 + 1, N=96, w=ctypes.c_void_p(8), eloc=ctypes.c_void_p(1 << 62)) == -1
    assert b"2^31" in L.wc_last_error()


# ---- the Python layers ----

def test_graph_measures_refuses_before_touching_the_device():
    import torch

    from nremmodfc_amd import sigchain
    assert sigchain.GRAPH_MEASURES == ("dist", "hops", "charpath", "efficiency", "ecc", "radius", "diameter",
                                       "local_efficiency", "clustering", "transitivity", "strengths", "degrees")
    for bad in ("betweenness", ("dist", "Hops"), ("dist", None), ()):
        with pytest.raises(ValueError, match="measure"):
            sigchain.graph_measures(None, measures=bad)                 # before the tensor is looked at
    ok = torch.zeros((2, 5, 5), dtype=torch.float64)
    for t in (ok.float(), ok[0, 0], ok[None], torch.zeros((2, 5, 4), dtype=torch.float64), ok.numpy(), None,
              torch.zeros((5, 5), dtype=torch.complex128)):
        with pytest.raises(TypeError, match="graph_measures"):
            sigchain.graph_measures(t)
    for n in (97, 1000, 1):
        with pytest.raises(ValueError, match="96"):
            sigchain.graph_measures(torch.zeros((1, n, n), dtype=torch.float64))
    for m in ("local_efficiency", "clustering", "transitivity", "strengths", "degrees"):
        with pytest.raises(ValueError, match="lengths"):
            sigchain.graph_measures(ok, measures=("dist", m), lengths=True)


def test_facades_refuse_before_touching_the_device():
    from nremmodfc_amd import graph_utils as gu
    w = ref.random_graph(6, 0.8, 0)
    every = (gu.distance_wei, gu.efficiency_wei, gu.clustering_coef_wu, gu.transitivity_wu, gu.strengths_und,
             gu.degrees_und)
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
    for f in (gu.distance_wei, gu.efficiency_wei, functools.partial(gu.efficiency_wei, local=True)):
        for bad in (neg, nan, np.stack([w, neg])):
            with pytest.raises(ValueError, match="negative or NaN"):
                f(bad)


def test_host_helpers_equal_the_golden():
    from nremmodfc_amd import graph_utils as gu
    g = golden()
    x = np.array([-8.0, 0.0, 27.0, -0.001])
    np.testing.assert_array_equal(gu.cuberoot(x), np.sign(x) * np.abs(x) ** (1 / 3))
    w = g["dir24"]["w"]
    L = gu.invert(w)
    np.testing.assert_array_equal(L, ref.lengths_of(w))
    assert L is not w and (w == g["dir24"]["w"]).all()
    w2 = np.array(w)
    assert gu.invert(w2, copy=False) is w2 and (w2 == L).all()
    for case in ref.PATH_CASES:
        c = g[case]
        lam, eff, ecc, radius, diameter = gu.charpath(c["dist"])
        assert ref.deviation([lam, eff, radius, diameter], c["charpath"]) <= BOUND
        assert ref.deviation(ecc, c["ecc"]) <= BOUND
    lam, eff, ecc, radius, diameter = gu.charpath(g["sc"]["dist"], include_infinite=False)
    assert ref.deviation([lam, eff, radius, diameter], g["sc"]["charpath_finite"]) <= BOUND
    lam, eff, ecc, _, _ = gu.charpath(g["sc"]["dist"], include_diagonal=True)
    assert ref.deviation(lam, g["sc"]["dist"].mean()) <= BOUND and np.isinf(eff)
    stack = gu.charpath(np.stack([g["sc"]["dist"], g["rand90"]["dist"]]))
    assert stack[0].shape == (2,) and stack[2].shape == (2, 90)
    assert stack[0][1] == gu.charpath(g["rand90"]["dist"])[0]


def test_importing_graph_utils_stays_light():
    code = ("import sys; from nremmodfc_amd import graph_utils; "
            "assert 'torch' not in sys.modules and 'nremmodfc_amd._lib' not in sys.modules")
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    subprocess.run([sys.executable, "-c", code], check=True, cwd=root)

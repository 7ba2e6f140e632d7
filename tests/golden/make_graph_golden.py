#!/usr/bin/env python3
"""golden_graph.npz: the reference's OWN graph functions on the test graphs (build container only).

The reference's graph_utils.py cannot be imported here (statsmodels at module top level), but the
functions themselves need only numpy.  This generator reads the reference source at generation time,
takes out with `ast` exactly

  cuberoot (:38-43), binarize (:45-65, degrees_und calls it), invert (:68-90),
  efficiency_wei (:597-690), clustering_coef_wu (:1305-1323), distance_wei (:1462-1529),
  charpath (:1533-1591), transitivity_wu (:1673-1689), degrees_und (:1721-1737),
  strengths_und (:1766-1778),

executes those definitions unmodified in a namespace holding numpy, and applies them to the seven
matrices of tests/graph_reference.py:golden_inputs():

  sc         the shipped SC (90 nodes, density 0.40)
  fc_dense   the W empirical FC clipped at 0, zero diagonal (density 0.99)
  fc_thr     the same thresholded to density 0.2 (graph_utils.thresholding)
  rand90     a random symmetric 90-node graph of density 0.3 (default_rng(1))
  dir24      a random directed 24-node graph of density 0.4
  pendant12  one isolated and one pendant node: inf distances, local efficiency of zero and one neighbour
  signed5    weights of both signs: clustering and transitivity only

Only inputs and OUTPUTS are committed; no reference source is copied.  Per case `c` the file holds
c/w, c/clustering, c/transitivity, c/strengths, c/degrees and, but for signed5, c/dist, c/hops,
c/charpath (lambda, efficiency, radius, diameter), c/ecc, c/charpath_finite and c/ecc_finite
(include_infinite=False), c/efficiency, c/local_efficiency and c/gap, the smallest relative gap between
the best and the second-best last edge of a shortest path (graph_reference.second_best_gap): the
generator asserts gap >= 1e-9, on which the exact equality of Floyd-Warshall's and Dijkstra's hop counts
rests.  To stay under 300 KB, a symmetric w is stored as its upper triangle (c/w_triu) and the distances
of a symmetric w as their upper triangle plus the difference of the two triangles' bit patterns
(c/dist_triu, c/dist_skew int8: the reference's D is symmetric to a few ulp only);
graph_reference.load_golden() puts them together again, bit for bit.

  python tests/golden/make_graph_golden.py
"""
import ast
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = "/root/reference"
FUNCS = ("cuberoot", "binarize", "invert", "efficiency_wei", "clustering_coef_wu", "distance_wei", "charpath",
         "transitivity_wu", "degrees_und", "strengths_und")
OUT = os.path.join(HERE, "golden_graph.npz")
MIN_GAP = 1e-9

sys.path.insert(0, ROOT)
from tests import graph_reference as gr  # noqa: E402


def reference_defs():
    """The named top-level functions of the reference's graph_utils.py, executed unchanged."""
    tree = ast.parse(open(os.path.join(REF, "graph_utils.py")).read())
    keep = [n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name in FUNCS]
    assert sorted(n.name for n in keep) == sorted(FUNCS)
    ns = {"np": np}
    exec(compile(ast.Module(body=keep, type_ignores=[]), "graph_utils.py", "exec"), ns)
    return ns


def main():
    g = reference_defs()
    out = {}
    for name, w in gr.golden_inputs().items():
        t0 = time.time()
        sym = bool((w == w.T).all())
        if sym:
            out[f"{name}/w_triu"] = w[np.triu_indices(w.shape[0])]
        else:
            out[f"{name}/w"] = w
        out[f"{name}/clustering"] = g["clustering_coef_wu"](w.copy())
        out[f"{name}/transitivity"] = np.float64(g["transitivity_wu"](w.copy()))
        out[f"{name}/strengths"] = g["strengths_und"](w.copy())
        out[f"{name}/degrees"] = g["degrees_und"](w.copy()).astype(np.int32)
        if name in gr.PATH_CASES:
            L = g["invert"](w, copy=True)
            D, B = g["distance_wei"](L)
            gap = gr.second_best_gap(L, D)
            assert gap >= MIN_GAP, (name, gap)       # unique shortest paths: hop counts are well defined
            assert B.max() < 127 and (B == np.rint(B)).all()
            if sym:
                iu = np.triu_indices(w.shape[0], 1)
                skew = D.T[iu].view(np.int64) - D[iu].view(np.int64)
                assert np.abs(skew).max() < 127, np.abs(skew).max()
                out[f"{name}/dist_triu"], out[f"{name}/dist_skew"] = D[iu], skew.astype(np.int8)
            else:
                out[f"{name}/dist"] = D
            out[f"{name}/hops"] = B.astype(np.int8)
            for tag, inf in (("", True), ("_finite", False)):
                lam, eff, ecc, rad, dia = g["charpath"](D, include_infinite=inf)
                out[f"{name}/charpath{tag}"] = np.array([lam, eff, rad, dia])
                out[f"{name}/ecc{tag}"] = np.asarray(ecc, dtype=np.float64)
            out[f"{name}/efficiency"] = np.float64(g["efficiency_wei"](w.copy()))
            out[f"{name}/local_efficiency"] = g["efficiency_wei"](w.copy(), local=True)
            out[f"{name}/gap"] = np.float64(gap)
            print(f"{name}: N {w.shape[0]} density {np.count_nonzero(w) / (w.size - w.shape[0]):.2f} gap {gap:.1e} "
                  f"max hops {int(B.max())} inf {int(np.isinf(D).sum())} {time.time() - t0:.1f} s")
    np.savez_compressed(OUT, **out)
    size = os.path.getsize(OUT)
    print(OUT, size, "bytes")
    assert size < 300 * 1024
    got = gr.load_golden()
    for name, w in gr.golden_inputs().items():
        assert (got[name]["w"] == w).all()


if __name__ == "__main__":
    main()

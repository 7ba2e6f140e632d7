#!/usr/bin/env python3
"""golden_centrality.npz: the reference's OWN node measures on the test graphs (build container only).

Like make_graph_golden.py: the reference's graph_utils.py cannot be imported, so this generator reads
its source at generation time, takes out with `ast` exactly

  invert (:68-90), participation_coef (:271-307), betweenness_bin (:1929-1980),
  betweenness_wei (:1983-2052), module_degree_zscore (:2103-2140),

executes those definitions unmodified in a namespace holding numpy, and applies them to the seven
matrices of tests/graph_reference.py:golden_inputs().  Only OUTPUTS are committed (the inputs are
reproducible from golden_inputs()); no reference source is copied.  Per case `c` the file holds

  c/bc                 betweenness_wei(invert(w)), the six PATH_CASES; asserted integer, with the sums
                       of centrality_reference.BC_SUMS
  c/bc_bin, c/bc_bin_wei   betweenness_bin(w != 0) and betweenness_wei(w != 0): fc_thr and dir24, the
                       graphs with many tied shortest paths
  c/part_<p>, c/z_<p>  participation_coef(w, ci) and module_degree_zscore(w, ci) for the four partitions
                       p of centrality_reference.PARTITIONS, all seven cases
  dir24/part_<p>_in, dir24/part_<p>_out, dir24/z_<p>_<flag>   the directed variants

  python tests/golden/make_centrality_golden.py
"""
import ast
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = "/root/reference"
FUNCS = ("invert", "participation_coef", "betweenness_bin", "betweenness_wei", "module_degree_zscore")
OUT = os.path.join(HERE, "golden_centrality.npz")

sys.path.insert(0, ROOT)
from tests import centrality_reference as cr  # noqa: E402
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
        n = w.shape[0]
        if name in gr.PATH_CASES:
            bc = g["betweenness_wei"](g["invert"](w, copy=True))
            assert (bc == np.rint(bc)).all() and bc.sum() == cr.BC_SUMS[name], (name, bc.sum())
            out[f"{name}/bc"] = bc
        if name in cr.BINARY_CASES:
            a = (w != 0).astype(np.float64)
            out[f"{name}/bc_bin"] = g["betweenness_bin"](a.copy())
            out[f"{name}/bc_bin_wei"] = g["betweenness_wei"](a.copy())
        with np.errstate(divide="ignore", invalid="ignore"):
            for p in cr.PARTITIONS:
                ci = cr.partition(p, n)
                out[f"{name}/part_{p}"] = g["participation_coef"](w.copy(), ci.copy())
                out[f"{name}/z_{p}"] = g["module_degree_zscore"](w.copy(), ci.copy())
                if name == "dir24":
                    for degree in ("in", "out"):
                        out[f"{name}/part_{p}_{degree}"] = g["participation_coef"](w.copy(), ci.copy(), degree)
                    for flag in (1, 2, 3):
                        out[f"{name}/z_{p}_{flag}"] = g["module_degree_zscore"](w.copy(), ci.copy(), flag)
        print(f"{name}: N {n} {time.time() - t0:.1f} s")
    np.savez_compressed(OUT, **out)
    size = os.path.getsize(OUT)
    print(OUT, size, "bytes")
    assert size < 300 * 1024


if __name__ == "__main__":
    main()

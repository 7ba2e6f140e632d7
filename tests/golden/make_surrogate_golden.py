#!/usr/bin/env python3
"""golden_surrogate.npz: the reference's OWN probabilistic_thresholding on the test series, under the
engine's phases.

The reference's graph_utils.py cannot be imported (statsmodels at module top level, which is not
installed), but the function needs only numpy, scipy.stats and multipletests.  This generator reads the
reference source at generation time, takes out with `ast` exactly

  matrix_recon (:107-119), probabilistic_thresholding (:220-265),

and executes those definitions unmodified in a namespace in which
  * `np` is numpy but for np.random.seed, which notes the surrogate's seed, and np.random.uniform, which
    replays the engine's phases of that seed (tests/surrogate_reference.py:phases, the stream of
    include/wcsde.h) where numpy would draw from its Mersenne Twister; np.corrcoef and stats.norm.fit are
    numpy's and SciPy's, and what they return is noted on the way;
  * `multipletests` is a wrapper around scipy.stats.false_discovery_control(p, method='bh').  The
    Benjamini-Hochberg step is therefore pinned to SciPy's implementation and not to statsmodels'.

Only inputs and OUTPUTS are committed; no reference source is copied.  Per case `c` of
surrogate_reference.CASES the file holds c/y (float32: the inputs are float32 values), c/seeds, the
strict upper triangles c/fc_adj_triu and c/p_adj_triu of FC_adjusted and p_matrix (both are asserted
symmetric with a zero diagonal), and from inside the run c/mu and c/sd, the normal fit of every pair,
and c/sfc3, the first three surrogate FCs (all S would pass the size limit of a committed file).

The generator asserts the condition the tests rest on: |p_adj - alpha| >= 1e-9 and sd > 0 on every pair
of every case, so that the kept set is determinate under rounding.

  python tests/golden/make_surrogate_golden.py <directory of the reference>
"""
import ast
import os
import sys

import numpy as np
from scipy import stats

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
FUNCS = ("matrix_recon", "probabilistic_thresholding")
OUT = os.path.join(HERE, "golden_surrogate.npz")

sys.path.insert(0, ROOT)
from tests import surrogate_reference as sr  # noqa: E402


class Proxy:
    """obj with some attributes replaced."""

    def __init__(self, obj, **over):
        self._obj, self._over = obj, over

    def __getattr__(self, name):
        return self._over[name] if name in self._over else getattr(self._obj, name)


def reference_defs(ref_dir, notes):
    """The reference's two functions, executed unchanged; notes gathers what the run sees inside."""
    tree = ast.parse(open(os.path.join(ref_dir, "graph_utils.py")).read())
    keep = [n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name in FUNCS]
    assert sorted(n.name for n in keep) == sorted(FUNCS)

    def seed(i):
        notes["seed"] = i

    def uniform(low, high, size):
        assert (low, high) == (0, 2 * np.pi)
        return sr.phases(notes["seed"], *size)

    def corrcoef(x):
        r = np.corrcoef(x)
        notes["corr"].append(r)
        return r

    def fit(data):
        r = stats.norm.fit(data)
        notes["fit"].append(r)
        return r

    def multipletests(p, alpha=0.05, method="fdr_bh"):
        assert method == "fdr_bh"
        adj = stats.false_discovery_control(p, method="bh")
        return adj < alpha, adj, None, None

    over = {"random": Proxy(np.random, seed=seed, uniform=uniform), "corrcoef": corrcoef}
    if not hasattr(np, "row_stack"):
        over["row_stack"] = np.vstack
    ns = {"np": Proxy(np, **over), "stats": Proxy(stats, norm=Proxy(stats.norm, fit=fit)), "multipletests": multipletests}
    exec(compile(ast.Module(body=keep, type_ignores=[]), "graph_utils.py", "exec"), ns)
    return ns


def main():
    notes = {}
    g = reference_defs(sys.argv[1], notes)
    out = {}
    for name, (L, N, S, groups) in sr.CASES.items():
        y = sr.case_input(name)
        notes.update(corr=[], fit=[])
        fc_adj, p_mat = g["probabilistic_thresholding"](y.copy(), surr_number=S, alpha=sr.ALPHA)
        assert len(notes["corr"]) == S + 1 and len(notes["fit"]) == N * (N - 1) // 2
        for m in (fc_adj, p_mat):
            assert (m == m.T).all() and (np.diag(m) == 0).all()
        fit = np.array(notes["fit"])
        p_adj = sr.uptri(p_mat)
        gap, sd_min = float(np.abs(p_adj - sr.ALPHA).min()), float(fit[:, 1].min())
        assert gap >= sr.MIN_GAP and sd_min > 0, (name, gap, sd_min)
        out[f"{name}/y"] = y.astype(np.float32)
        assert (out[f"{name}/y"].astype(np.float64) == y).all()
        out[f"{name}/seeds"] = sr.case_seeds(name)
        out[f"{name}/fc_adj_triu"], out[f"{name}/p_adj_triu"] = sr.uptri(fc_adj), p_adj
        out[f"{name}/mu"], out[f"{name}/sd"] = fit[:, 0], fit[:, 1]
        out[f"{name}/sfc3"] = np.array([sr.uptri(c) for c in notes["corr"][1:4]])
        print(f"{name}: L {L} N {N} S {S} kept {int((sr.uptri(fc_adj) != 0).sum())} of {len(p_adj)} pairs, "
              f"min |p_adj - alpha| {gap:.1e}, min sd {sd_min:.3f}, p_adj == 0: {int((p_adj == 0).sum())}")
    np.savez_compressed(OUT, **out)
    size = os.path.getsize(OUT)
    print(OUT, size, "bytes")
    assert size < 1024 * 1024


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""golden_hubs.npz: the reference's OWN rich_club_wu, rich_club_wd, rich_club_bu, rich_club_bd,
assortativity_wei, assortativity_bin and score_wu on the test matrices (build container only).

The method is make_nullmodel_golden.py's: the reference's graph_utils.py cannot be imported, so this
generator reads its source at generation time, takes out with `ast` exactly

  rich_club_bd (:2396-2437), rich_club_bu (:2440-2479), rich_club_wd (:2482-2525), rich_club_wu
  (:2528-2570), score_wu (:2573-2609), assortativity_bin (:1808-1866), assortativity_wei (:1869-1926)
  and their helpers binarize, degrees_dir, degrees_und, strengths_dir, strengths_und,

and executes those definitions unmodified in a namespace holding numpy.  Only OUTPUTS are committed
(the inputs are reproducible from hubs_reference.golden_inputs()); no reference source is copied.

Conditions on the inputs, asserted here:
  rich club   a fully connected matrix has every rw level NaN: RICH_NAN_CASES must have no finite
              level and are kept for their NaN pattern; RICH_VALUE_CASES must have at least half of
              their rw levels finite; RICH_SIGNED_CASES, a small matrix with negative weights, and
              RICH_DIRECTED_CASES (rich_club_wd, rich_club_bd) have no condition;
  s-core      the levels are SCORE_FRACTIONS of the largest strength; a level is kept only if no
              strength met during the peel lies within 1e-9 relative of it, else it is moved up by
              1e-6 of itself until that holds: every comparison str < s then has one answer.  This is
              a condition, not a tolerance;
  assortativity   a value is committed with its |term3 - term2| / term3; where that is below 1e-6 the
              quotient is noise and only a NaN (an exact 0 / 0, the regular graphs) may be committed.
The restatement (hubs_reference) must agree with every committed value: NaN patterns, nk, sn and the
core matrices exactly, fp64 values within 1e-12 of max(1, |want|).  Keys:

  rich/c/rw, rb, nk, ek          klevel None (the matrix's own largest degree)
  rich/pendant12/k12/...         klevel 12, past the largest degree
  assort/c/wei, bin [5], margin [5][2]   flags 0 .. 4
  score/c/s [4], sn [4], alive [4][N] (a node with an entry left in CIJscore), sum [4] (of CIJscore)

  python tests/golden/make_hubs_golden.py /path/to/reference

prints the reference's own time per matrix on this host, one core.
"""
import ast
import os
import sys
import time
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
FUNCS = ("rich_club_bd", "rich_club_bu", "rich_club_wd", "rich_club_wu", "score_wu", "assortativity_bin",
         "assortativity_wei", "binarize", "degrees_dir", "degrees_und", "strengths_dir", "strengths_und")
OUT = os.path.join(HERE, "golden_hubs.npz")
TOL = 1e-12

sys.path.insert(0, ROOT)
from tests import hubs_reference as hr  # noqa: E402
from tests.centrality_reference import deviation_abs  # noqa: E402


def reference_defs(ref_dir):
    """The named top-level functions of the reference's graph_utils.py, executed unchanged."""
    tree = ast.parse(open(os.path.join(ref_dir, "graph_utils.py")).read())
    keep = [n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name in FUNCS]
    assert sorted(n.name for n in keep) == sorted(FUNCS)
    ns = {"np": np}
    exec(compile(ast.Module(body=keep, type_ignores=[]), "graph_utils.py", "exec"), ns)
    return ns


def timed(fn, *args):
    t0 = time.perf_counter()
    out = fn(*args)
    return out, time.perf_counter() - t0


def same(got, want, what):
    d = deviation_abs(np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64))
    assert d <= TOL, (what, d, got, want)
    return d


def main():
    g = reference_defs(sys.argv[1])
    inputs = hr.golden_inputs()
    out = {}
    warnings.simplefilter("ignore", RuntimeWarning)      # the reference divides 0 by 0 where it returns NaN
    worst = 0.0

    for name in hr.RICH_VALUE_CASES + hr.RICH_NAN_CASES + hr.RICH_SIGNED_CASES + hr.RICH_DIRECTED_CASES:
        W = inputs[name]
        directed = name in hr.RICH_DIRECTED_CASES
        rw, tw = timed(g["rich_club_wd" if directed else "rich_club_wu"], W.copy())
        (rb, nk, ek), tb = timed(g["rich_club_bd" if directed else "rich_club_bu"], W.copy())
        finite = int(np.isfinite(rw).sum())
        if name in hr.RICH_NAN_CASES:
            assert finite == 0, (name, finite)
        elif name in hr.RICH_VALUE_CASES:
            assert 2 * finite >= len(rw), (name, finite, len(rw))
        mine = hr.rich_club(W, directed)
        m = mine["maxdeg"]
        assert len(rw) == len(rb) == m, (name, len(rw), m)
        assert (mine["nk"][:m] == nk).all(), name
        d = max(same(mine["rw"][:m], rw, name), same(mine["rb"][:m], rb, name), same(mine["ek"][:m], ek, name))
        worst = max(worst, d)
        out.update({f"rich/{name}/rw": rw, f"rich/{name}/rb": rb, f"rich/{name}/nk": nk.astype(np.int32),
                    f"rich/{name}/ek": ek})
        print(f"rich {name}: N {len(W)} maxdeg {m} finite rw {finite}/{len(rw)}  deviation {d:.1e}  "
              f"reference {1e3 * tw:.1f} ms weighted, {1e3 * tb:.1f} ms binary")

    W = inputs["pendant12"]                               # an explicit klevel past the largest degree
    rw = g["rich_club_wu"](W.copy(), 12)
    rb, nk, ek = g["rich_club_bu"](W.copy(), 12)
    mine = hr.rich_club(W, False, 12)
    assert hr.rich_club(W)["maxdeg"] < 12 and (mine["nk"] == nk).all()
    same(mine["rw"], rw, "k12"), same(mine["rb"], rb, "k12"), same(mine["ek"], ek, "k12")
    out.update({"rich/pendant12/k12/rw": rw, "rich/pendant12/k12/rb": rb, "rich/pendant12/k12/nk": nk.astype(np.int32),
                "rich/pendant12/k12/ek": ek})

    for name in hr.ASSORT_CASES:
        W = inputs[name]
        wei, bin_, margin = np.zeros(5), np.zeros(5), np.zeros((5, 2))
        t = 0.0
        for flag in range(5):
            (wei[flag], bin_[flag]), dt = timed(lambda: (g["assortativity_wei"](W.copy(), flag),
                                                         g["assortativity_bin"](W.copy(), flag)))
            t += dt
            for col, weighted in enumerate((True, False)):
                _, t2, t3 = hr.assortativity_terms(W, flag, weighted)
                margin[flag, col] = abs(t3 - t2) / t3
                got = (wei, bin_)[col][flag]
                assert margin[flag, col] >= 1e-6 or np.isnan(got), (name, flag, col, margin[flag, col], got)
            mine = hr.assortativity(W, flag)
            worst = max(worst, same(mine[0], wei[flag], (name, flag)), same(mine[1], bin_[flag], (name, flag)))
        out.update({f"assort/{name}/wei": wei, f"assort/{name}/bin": bin_, f"assort/{name}/margin": margin})
        print(f"assort {name}: wei {np.round(wei, 4)} bin {np.round(bin_, 4)} least margin {np.nanmin(margin):.1e}  "
              f"reference {1e3 * t / 10:.2f} ms per call")
    assert np.isnan(out["assort/ring12/bin"]).all()       # the regular graph: an exact 0 / 0
    assert out["assort/dir24/wei"][4] == out["assort/dir24/wei"][2]      # flag 4 as written: in/out
    assert out["assort/dir24/bin"][4] != out["assort/dir24/bin"][2]      # in/in there

    for name in hr.SCORE_CASES:
        W = inputs[name]
        levels, sns, alive, sums = [], [], [], []
        for s in hr.score_levels(W):
            while True:
                trace = {}
                member, sn, rounds = hr.score(W, s, trace)
                if trace["gap"] > 1e-9:
                    break
                s *= 1 + 1e-6
            (core, sn_ref), dt = timed(g["score_wu"], W.copy(), s)
            assert core.tobytes() == hr.core_matrix(W, member).tobytes() and int(sn_ref) == sn, (name, s)
            levels.append(s), sns.append(sn), sums.append(core.sum())
            alive.append(((core != 0).any(axis=0) | (core != 0).any(axis=1)).astype(np.uint8))
            print(f"score {name} s {s:.4f}: sn {sn} rounds {rounds} gap {trace['gap']:.1e}  reference {1e3 * dt:.2f} ms")
        out.update({f"score/{name}/s": np.array(levels), f"score/{name}/sn": np.array(sns, dtype=np.int32),
                    f"score/{name}/alive": np.array(alive), f"score/{name}/sum": np.array(sums)})

    print(f"largest deviation of the restatement from the reference: {worst:.1e}")
    np.savez_compressed(OUT, **out)
    size = os.path.getsize(OUT)
    print(OUT, size, "bytes")
    assert size < 300 * 1024


if __name__ == "__main__":
    main()

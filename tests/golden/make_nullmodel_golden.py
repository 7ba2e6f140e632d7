#!/usr/bin/env python3
"""golden_nullmodel.npz: the reference's OWN randmio_und_signed, null_model_und_sign and
participation_coef_norm on the test matrices, run under the engine's draws (build container only).

The method is make_louvain_sign_golden.py's: the reference's graph_utils.py cannot be imported, so this
generator reads its source at generation time, takes out with `ast` exactly

  pick_four_unique_nodes_quickly (:2142-2162), randmio_und_signed (:2165-2217),
  null_model_und_sign (:2219-2338), participation_coef_norm (:2341-2393),

and executes those definitions unmodified in a namespace holding numpy.  During a run
  np.random.seed(s)         starts the engine's streams of seed s (participation_coef_norm calls it);
  np.random.randint(n**4)   returns a + b n + c n^2 + d n^3 of the run's next draw (a, b, c, d), distinct
                            or not (nullmodel_reference.Draws);
  np.random.permutation(m)  returns nullmodel_reference.shuffle_head of the next period, padded with
                            the other values to a full permutation;
  stdout is swallowed; np.argsort is numpy's own, the reference's unstable quicksort.  All are
restored afterwards.  Only OUTPUTS are committed, as strict upper triangles (the inputs are
reproducible from nullmodel_reference.inputs(): louvain_sign_reference.inputs() with the upper
triangle mirrored, np.corrcoef's matrices not being exactly symmetric); no reference source is copied.

A run is kept only if in none of its sorts two live keys are exactly equal (the restatement counts
them); a seed that fails is replaced by the next integer, below 64.  This is a condition, not a
tolerance: without ties every argsort has one answer.  The restatement (nullmodel_reference) must then
agree with the reference on every committed run: w0 and wr as the same bits, eff and draws equal, r,
mean and std within 1e-12.  Per case c of GOLDEN_CASES (the reference's mode, bin_swaps 5, wei_freq 0.1)

  c/seeds, c/w0 [.][N (N - 1) / 2], c/r [.][2], c/eff, c/draws, c/gap (the smallest relative gap of keys)

and  rewire/corr24/seed, wr, eff, draws  (randmio_und_signed, itr 5),
     pnorm/fc_thr/mean, std, ci  (participation_coef_norm, BA_iters 8, the first committed "sta"
     partition of golden_louvain_sign.npz, labels from 1).

  python tests/golden/make_nullmodel_golden.py /path/to/reference

prints the reference's own time per null model on this host, one core.
"""
import ast
import contextlib
import io
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
FUNCS = ("pick_four_unique_nodes_quickly", "randmio_und_signed", "null_model_und_sign", "participation_coef_norm")
OUT = os.path.join(HERE, "golden_nullmodel.npz")
MAX_SEED = 64
PERIOD = 10

sys.path.insert(0, ROOT)
from tests import louvain_sign_reference as ls  # noqa: E402
from tests import nullmodel_reference as nr  # noqa: E402


def reference_defs(ref_dir):
    """The named top-level functions of the reference's graph_utils.py, executed unchanged."""
    tree = ast.parse(open(os.path.join(ref_dir, "graph_utils.py")).read())
    keep = [n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name in FUNCS]
    assert sorted(n.name for n in keep) == sorted(FUNCS)
    ns = {"np": np}
    exec(compile(ast.Module(body=keep, type_ignores=[]), "graph_utils.py", "exec"), ns)
    return ns


class Engine:
    """The engine's streams behind numpy's generator calls, for null models of the matrix W."""

    def __init__(self, W):
        W = np.array(W, dtype=np.float64)
        np.fill_diagonal(W, 0.0)
        self.n = len(W)
        wpos = int(np.count_nonzero(np.triu(W > 0)))
        self.periods_pos = -(-wpos // PERIOD)
        self.seed(0)

    def seed(self, s):
        self.s, self.d, self.calls = int(s), 0, 0
        self.draw = nr.Draws(self.s, self.n)

    def randint(self, high):
        assert high == self.n ** 4
        a, b, c, d = self.draw(self.d)
        self.d += 1
        n = self.n
        return a + b * n + c * n ** 2 + d * n ** 3

    def permutation(self, m):
        npass = int(self.calls >= self.periods_pos)
        p = self.calls - npass * self.periods_pos
        self.calls += 1
        head = nr.shuffle_head(m, min(m, PERIOD), p, npass, self.s)
        rest = np.setdiff1d(np.arange(m), head)
        return np.concatenate([head, rest])


@contextlib.contextmanager
def replaying(engine):
    keep = np.random.seed, np.random.randint, np.random.permutation
    np.random.seed, np.random.randint, np.random.permutation = engine.seed, engine.randint, engine.permutation
    try:
        with contextlib.redirect_stdout(io.StringIO()):
            yield
    finally:
        np.random.seed, np.random.randint, np.random.permutation = keep


def main():
    g = reference_defs(sys.argv[1])
    inputs = nr.inputs()
    out = {}
    for name, count in nr.GOLDEN_CASES:
        W = inputs[name]
        engine = Engine(W)
        seeds, w0s, rs, effs, draws, gaps = [], [], [], [], [], []
        seed = 0
        while len(seeds) < count and seed < MAX_SEED:
            trace = {}
            mine, r_mine, info = nr.null_model(W, seed, 5, PERIOD, "reference", trace)
            if info[2] == 0 and trace["ties"] == 0:
                with replaying(engine):
                    engine.seed(seed)
                    t0 = time.perf_counter()
                    w0, r = g["null_model_und_sign"](W.copy())
                    dt = time.perf_counter() - t0
                assert w0.tobytes() == mine.tobytes(), (name, seed, np.abs(w0 - mine).max())
                assert engine.d == info[1], (name, seed, engine.d, info)
                for got, want in ((r[0], r_mine[0]), (r[1], r_mine[0]), (r[2], r_mine[1]), (r[3], r_mine[1])):
                    assert (np.isnan(got) and np.isnan(want)) or abs(got - want) <= 1e-12, (name, seed, r, r_mine)
                seeds.append(seed), w0s.append(nr.uptri(w0)), rs.append([r[0], r[2]])
                effs.append(info[0]), draws.append(info[1]), gaps.append(trace["gap"])
                print(f"{name} seed {seed}: N {len(W)}  eff {info[0]}  draws {info[1]}  r {r[0]:.4f} {r[2]:.4f}  "
                      f"min gap {trace['gap']:.1e}  signs in/out {(W < 0).sum() // 2}/{(w0 < 0).sum() // 2}  "
                      f"reference {dt:.2f} s")
            else:
                print(f"{name} seed {seed}: status {info[2]}, ties {trace.get('ties')}: PASSED OVER")
            seed += 1
        assert len(seeds) == count, name
        out.update({f"{name}/seeds": np.array(seeds), f"{name}/w0": np.array(w0s), f"{name}/r": np.array(rs),
                    f"{name}/eff": np.array(effs), f"{name}/draws": np.array(draws), f"{name}/gap": np.array(gaps)})

    W = inputs["corr24"]
    engine = Engine(W)
    with replaying(engine):
        engine.seed(3)
        wr, eff = g["randmio_und_signed"](W.copy(), 5)
    mine, info = nr.rewire(W, 3, 5)
    assert wr.tobytes() == mine.tobytes() and eff == info[0] and engine.d == info[1]
    out.update({"rewire/corr24/seed": np.array(3), "rewire/corr24/wr": nr.uptri(wr), "rewire/corr24/eff": np.array(eff),
                "rewire/corr24/draws": np.array(info[1])})
    print(f"rewire corr24: eff {eff} draws {info[1]}")

    W = inputs["fc_thr"]
    ci = np.asarray(ls.load_golden()["fc_thr/ci_sta"][0], dtype=np.int64)
    for seed in range(nr.GOLDEN_REPS):
        trace = {}
        _, _, info = nr.null_model(W, seed, 5, PERIOD, "reference", trace)
        assert info[2] == 0 and trace["ties"] == 0, ("pnorm", seed)
    engine = Engine(W)
    with replaying(engine):
        mean, std = g["participation_coef_norm"](W.copy(), ci.copy(), BA_iters=nr.GOLDEN_REPS)
    m_mine, s_mine = nr.participation_norm(W, ci, nr.GOLDEN_REPS, None, 5, PERIOD, "reference")
    assert np.abs(mean - m_mine).max() <= 1e-12 and np.abs(std - s_mine).max() <= 1e-12
    out.update({"pnorm/fc_thr/mean": mean, "pnorm/fc_thr/std": std, "pnorm/fc_thr/ci": ci.astype(np.int16)})
    print(f"pnorm fc_thr: mean {mean.min():.4f}..{mean.max():.4f}  std max {std.max():.4f}  "
          f"dev {np.abs(mean - m_mine).max():.1e} {np.abs(std - s_mine).max():.1e}")

    np.savez_compressed(OUT, **out)
    size = os.path.getsize(OUT)
    print(OUT, size, "bytes")
    assert size < 300 * 1024


if __name__ == "__main__":
    main()

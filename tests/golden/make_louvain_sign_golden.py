#!/usr/bin/env python3
"""golden_louvain_sign.npz: the reference's OWN modularity_louvain_und_sign and consensus_und on the
test matrices, run under the engine's visiting order (build container only).

The method is make_louvain_golden.py's: the reference's graph_utils.py cannot be imported, so this
generator reads its source at generation time, takes out with `ast` exactly

  modularity_louvain_und_sign (:697-855), dummyvar (:858-887), agreement (:890-932),
  consensus_und (:1124-1207),

and executes those definitions unmodified in a namespace holding numpy.  During each
modularity_louvain_und_sign call np.random.seed is a no-op and np.random.permutation(n) returns
tests/louvain_reference.sweep_order(seed, t, n) for t = 0, 1, 2, ...; both are restored afterwards.
consensus_und calls the search without a seed: in its namespace the search is wrapped so that call c
replays seed base[c % reps] + (c // reps) reps, base = 0 .. reps-1, which is partition.graph_consensus's
seeding.  Only OUTPUTS are committed (the inputs are reproducible from
louvain_sign_reference.inputs(), the agreement matrices from the committed partitions); no reference
source is copied.

The restatement (louvain_sign_reference.louvain_sign, consensus) must agree with the reference on
every committed run: ci exactly, q to 1e-12, the same number of sweeps; iterations for a consensus.
Every committed run decides every step by a margin of at least 1e-9 (the restatement's margin); where
a (case, qtype, seed) falls below, that seed is replaced by the next integer that passes, below 64.
Per case `c` the file holds, for every qtype `t` (8 runs for sta, 2 for the others)

  c/seeds_t, c/ci_t [.][N], c/q_t, c/margin_t, c/sweeps_t                  gamma 1
  c/seeds_g<gamma>, c/ci_g<gamma>, c/q_g<gamma>, c/margin_g<gamma>         sta, gamma 0.7 and 1.3, 2 runs

and per consensus case (CONSENSUS: a case, tau, reps; D is the agreement of the case's eight committed
sta partitions / 8, dyadic, so exact ties are exempt from the margin)

  cons/c/ci [N], cons/c/iters, cons/c/margin, cons/c/tau, cons/c/reps

labels as the reference returns them (from 1).  A consensus case whose margin falls below 1e-9 is
left out and printed; this docstring names any: none.

  python tests/golden/make_louvain_sign_golden.py /path/to/reference
"""
import ast
import os
import sys
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
FUNCS = ("modularity_louvain_und_sign", "dummyvar", "agreement", "consensus_und")
OUT = os.path.join(HERE, "golden_louvain_sign.npz")
MAX_SEED = 64

sys.path.insert(0, ROOT)
from tests import louvain_reference as lr  # noqa: E402
from tests import louvain_sign_reference as ls  # noqa: E402


class BCTParamError(RuntimeError):
    """What the reference raises from its guards (defined outside the functions taken)."""


def reference_defs(ref_dir):
    """The named top-level functions of the reference's graph_utils.py, executed unchanged."""
    tree = ast.parse(open(os.path.join(ref_dir, "graph_utils.py")).read())
    keep = [n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name in FUNCS]
    assert sorted(n.name for n in keep) == sorted(FUNCS)
    ns = {"np": np, "BCTParamError": BCTParamError}
    exec(compile(ast.Module(body=keep, type_ignores=[]), "graph_utils.py", "exec"), ns)
    return ns


def replayed(search, w, seed, gamma=1, qtype="sta"):
    """(ci, q, sweeps) of the reference's search under the engine's order for `seed`."""
    t = [0]

    def permutation(n):
        order = lr.sweep_order(seed, t[0], n)
        t[0] += 1
        return order

    keep = np.random.seed, np.random.permutation
    np.random.seed, np.random.permutation = (lambda *a: None), permutation
    try:
        part, q = search(w.copy(), gamma, qtype, seed)
    finally:
        np.random.seed, np.random.permutation = keep
    return np.asarray(part), float(q), t[0]


def passing_runs(search, w, count, gamma=1, qtype="sta"):
    """The first `count` seeds 0, 1, 2, ... whose run decides everything by MIN_MARGIN, with the
    reference's outputs for them; the restatement must agree with the reference on each."""
    seeds, parts, qs, margins, sweeps = [], [], [], [], []
    seed = 0
    while len(seeds) < count and seed < MAX_SEED:
        mine, q_mine, info, margin = ls.louvain_sign(w, seed, gamma, qtype)
        if margin >= ls.MIN_MARGIN:
            part, q, drawn = replayed(search, w, seed, gamma, qtype)
            assert (part == mine + 1).all() and abs(q - q_mine) <= 1e-12 and drawn == info[1], (seed, q, q_mine)
            seeds.append(seed), parts.append(part), qs.append(q), margins.append(margin), sweeps.append(drawn)
        seed += 1
    assert len(seeds) == count, f"gamma {gamma} {qtype}: no {count} seeds below {MAX_SEED} decide by {ls.MIN_MARGIN:.0e}"
    return (np.array(seeds), np.array(parts, dtype=np.int16), np.array(qs), np.array(margins), np.array(sweeps))


def reference_consensus(g, D, tau, reps):
    """(ci, iterations) of the reference's consensus_und with call c of the search replaying seed
    c % reps + (c // reps) reps."""
    search, calls = g["modularity_louvain_und_sign"], [0]

    def seeded(dt):
        c = calls[0]
        calls[0] += 1
        part, q, _ = replayed(search, dt, c % reps + (c // reps) * reps)
        return part, q

    g["modularity_louvain_und_sign"] = seeded
    try:
        with warnings.catch_warnings():
            warnings.simplefilter("ignore", DeprecationWarning)
            ci = g["consensus_und"](D.copy(), tau, reps)
    finally:
        g["modularity_louvain_und_sign"] = search
    assert calls[0] % reps == 0
    return np.asarray(ci), calls[0] // reps


def main():
    g = reference_defs(sys.argv[1])
    search = g["modularity_louvain_und_sign"]
    inputs = ls.inputs()
    out = {}
    for name in ls.CASES:
        w = inputs[name]
        low = np.inf
        for qtype in ls.QTYPES:
            seeds, ci, q, margin, sweeps = passing_runs(search, w, 8 if qtype == "sta" else 2, 1, qtype)
            out.update({f"{name}/seeds_{qtype}": seeds, f"{name}/ci_{qtype}": ci, f"{name}/q_{qtype}": q,
                        f"{name}/margin_{qtype}": margin, f"{name}/sweeps_{qtype}": sweeps})
            low = min(low, margin.min())
            print(f"{name} {qtype}: N {w.shape[0]}  seeds {seeds.tolist()}  modules {sorted(set(ci.max(axis=1).tolist()))}  "
                  f"min margin {margin.min():.2e}  q {q.min():.4f}..{q.max():.4f}  sweeps {sweeps.tolist()}")
        for gamma in ls.GAMMAS:
            sg, cg, qg, mg, _ = passing_runs(search, w, 2, gamma)
            out.update({f"{name}/seeds_g{gamma}": sg, f"{name}/ci_g{gamma}": cg, f"{name}/q_g{gamma}": qg,
                        f"{name}/margin_g{gamma}": mg})
            low = min(low, mg.min())
        print(f"{name}: min margin {low:.2e}")
    for name, tau, reps in ls.CONSENSUS:
        D = lr.agreement(np.asarray(out[f"{name}/ci_sta"], dtype=np.int64)) / 8
        assert ls.dyadic(D)
        mine, iters_mine, margin = ls.consensus(D, tau, reps)
        if margin < ls.MIN_MARGIN:
            print(f"cons/{name}: margin {margin:.2e}, LEFT OUT")
            continue
        ci, iters = reference_consensus(g, D, tau, reps)
        assert (ci == mine + 1).all() and iters == iters_mine, (name, iters, iters_mine)
        out.update({f"cons/{name}/ci": ci.astype(np.int16), f"cons/{name}/iters": np.array(iters),
                    f"cons/{name}/margin": np.array(margin), f"cons/{name}/tau": np.array(tau),
                    f"cons/{name}/reps": np.array(reps)})
        print(f"cons/{name}: tau {tau} reps {reps}  iterations {iters}  modules {int(ci.max())}  margin {margin:.2e}")
    np.savez_compressed(OUT, **out)
    size = os.path.getsize(OUT)
    print(OUT, size, "bytes")
    assert size < 300 * 1024


if __name__ == "__main__":
    main()

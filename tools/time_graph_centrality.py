#!/usr/bin/env python3
"""wc_graph_betweenness and wc_graph_modules alone between HIP events, at the sizes of docs/CHANGELOG.md:
20,000 matrices of 90 nodes on the shipped SC's support (density 0.40), on the thresholded empirical
FC's (0.2) and on the dense FC's (0.99), every matrix times its own symmetric random factor in
[1, 1.1] so that no two have the same shortest paths.  wc_graph_paths (distances only) on the same
batch gives the scale of an N^3 all-pairs kernel.  Median (min-max) over the repetitions after one
warm-up; the buffers are allocated beforehand.

--host also times, for one matrix of each kind on one host core, the numpy restatement of the tests
(tests/centrality_reference.py) and, where installed, networkx's betweenness_centrality: the host
side of the comparison (the reference's betweenness_wei is three nested Python loops of the same
order).

  python tools/time_graph_centrality.py [--batch 20000] [--host] [--out FILE.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from nremmodfc_amd import _lib, datasets, graph_utils  # noqa: E402
from tools.time_graph import timed  # noqa: E402


def inputs(B, N=90):
    fc = np.maximum(datasets.load_empfc("W").astype(np.float64), 0.0)
    np.fill_diagonal(fc, 0.0)
    base = {"sc": datasets.load_sc().astype(np.float64), "fc_thr": graph_utils.thresholding(fc.copy(), 0.2),
            "fc_dense": fc}
    g = torch.Generator(device="cuda").manual_seed(0)
    f = 1 + 0.1 * torch.rand((B, N, N), dtype=torch.float64, device="cuda", generator=g)
    f = (f + f.transpose(1, 2)) / 2
    return {k: (torch.from_numpy(v).cuda()[None] * f).contiguous() for k, v in base.items()}


def host_times(w):
    from tests import centrality_reference as cref
    from tests import graph_reference as gref
    L = gref.lengths_of(w)
    t0 = time.perf_counter()
    cref.betweenness(L)
    out = {"numpy_restatement_s": time.perf_counter() - t0}
    try:
        import networkx as nx
    except ImportError:
        return out
    G = nx.from_numpy_array(L, create_using=nx.DiGraph)
    t0 = time.perf_counter()
    nx.betweenness_centrality(G, weight="weight", normalized=False)
    out["networkx_s"] = time.perf_counter() - t0
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=20000)
    ap.add_argument("--host", action="store_true")
    ap.add_argument("--out")
    args = ap.parse_args()
    B, N = args.batch, 90
    L, st, p = _lib.lib(), _lib.stream_handle(), _lib.ptr
    f64 = dict(dtype=torch.float64, device="cuda")
    ci = (torch.arange(N, device="cuda", dtype=torch.int32) % 4)[None].repeat(B, 1).contiguous()
    bc, part, z, q = (torch.empty(s, **f64) for s in ((B, N), (B, N), (B, N), (B,)))
    dist = torch.empty((B, N, N), **f64)
    res = {}
    for name, w in inputs(B).items():
        r = {"density": float((w[0] != 0).double().sum() / (N * N - N))}
        r["betweenness"] = timed(lambda: L.wc_graph_betweenness(B, N, p(w), 0, p(bc), st), 5)
        r["modules_all"] = timed(lambda: L.wc_graph_modules(B, N, 4, p(w), p(ci), 0, 0, 1.0, p(part), p(z), p(q), st), 5)
        r["modules_participation_only"] = timed(
            lambda: L.wc_graph_modules(B, N, 4, p(w), p(ci), 0, 0, 1.0, p(part), None, None, st), 5)
        r["paths_dist_only"] = timed(lambda: L.wc_graph_paths(B, N, p(w), 0, 1, p(dist), None, None, None, st), 5)
        if args.host:
            r["host"] = host_times(w[0].cpu().numpy())
        res[name] = r
        print(name, json.dumps(r), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Each graph kernel alone between HIP events, at the sizes of docs/CHANGELOG.md: 20,000 matrices of 90
nodes, dense (the W empirical FC clipped at 0, times a symmetric random factor in [1, 1.1]; density
0.99) and sparse (20,000 copies of the SC, density 0.40).  Median (min-max) over the repetitions after
one warm-up; the buffers are allocated beforehand.

  python tools/time_graph.py [--batch 20000] [--out FILE.json]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from nremmodfc_amd import _lib, datasets  # noqa: E402


def timed(fn, reps):
    _lib.check(fn(), "warm-up")
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        rc = fn()
        b.record()
        torch.cuda.synchronize()
        _lib.check(rc, "timed call")
        ts.append(a.elapsed_time(b))
    return {"ms_median": float(np.median(ts)), "ms_min": min(ts), "ms_max": max(ts), "reps": reps}


def inputs(B, N=90):
    fc = np.maximum(datasets.load_empfc("W").astype(np.float64), 0.0)
    np.fill_diagonal(fc, 0.0)
    g = torch.Generator(device="cuda").manual_seed(0)
    f = 1 + 0.1 * torch.rand((B, N, N), dtype=torch.float64, device="cuda", generator=g)
    dense = (torch.from_numpy(fc).cuda()[None] * (f + f.transpose(1, 2)) / 2).contiguous()
    sc = torch.from_numpy(datasets.load_sc().astype(np.float64)).cuda()[None].repeat(B, 1, 1).contiguous()
    return {"fc_dense": dense, "sc": sc}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=20000)
    ap.add_argument("--out")
    args = ap.parse_args()
    B, N = args.batch, 90
    L, st, p = _lib.lib(), _lib.stream_handle(), _lib.ptr
    f64 = dict(dtype=torch.float64, device="cuda")
    i32 = dict(dtype=torch.int32, device="cuda")
    res = {}
    for name, w in inputs(B).items():
        dist, hops = torch.empty((B, N, N), **f64), torch.empty((B, N, N), **i32)
        stats, ecc = torch.empty((B, 4), **f64), torch.empty((B, N), **f64)
        vec, vec2, tr, deg = torch.empty((B, N), **f64), torch.empty((B, N), **f64), torch.empty(B, **f64), \
            torch.empty((B, N), **i32)
        r = {"density": float((w[0] != 0).double().sum() / (N * N - N))}
        r["paths_all"] = timed(lambda: L.wc_graph_paths(B, N, p(w), 0, 1, p(dist), p(hops), p(stats), p(ecc), st), 5)
        r["paths_stats_only"] = timed(lambda: L.wc_graph_paths(B, N, p(w), 0, 1, None, None, p(stats), None, st), 5)
        r["paths_dist_only"] = timed(lambda: L.wc_graph_paths(B, N, p(w), 0, 1, p(dist), None, None, None, st), 5)
        r["clustering_all"] = timed(lambda: L.wc_graph_clustering(B, N, p(w), p(vec), p(tr), p(vec2), p(deg), st), 7)
        r["strengths_degrees_only"] = timed(
            lambda: L.wc_graph_clustering(B, N, p(w), None, None, p(vec2), p(deg), st), 5)
        r["local_efficiency"] = timed(lambda: L.wc_graph_local_efficiency(B, N, p(w), p(vec), st), 3)
        res[name] = r
        print(name, json.dumps(r), flush=True)
        del dist, hops
    if args.out:
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()

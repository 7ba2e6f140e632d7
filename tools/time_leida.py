#!/usr/bin/env python3
"""The four LEiDA kernels between HIP events at a sweep's shape: 2,000 simulations of 298 BOLD samples x 90
nodes, K = 5 states (wc_leida_eigvec, wc_kmeans_assign and wc_kmeans_update under both metrics,
wc_state_stats, each alone with its buffers allocated beforehand), and a whole sigchain.kmeans from rows
picked at random.  Median (min-max) over the repetitions after one warm-up.

The eigenvector kernel reads 16 bytes and writes 8 per (row, node), and 8 per row for share: its floor is
that traffic at the HBM bandwidth.  Printed beside it: the 8.0 TB/s of the specification, and what a plain
device copy of the same phasors (torch's clone: 16 bytes read, 16 written) achieves in the same process.
The k-means kernels' bytes are x once (and the labels, distances, partial sums), the state statistics' the
labels three times over.

  python tools/time_leida.py [--batch 2000] [--reps 20] [--out FILE.json]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from nremmodfc_amd import _lib, sigchain  # noqa: E402

M, N, K = 298, 90, 5
HBM_PEAK = 8.0e12


def timed(fn, reps, nbytes=None):
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b))
    r = {"ms_median": float(np.median(ts)), "ms_min": min(ts), "ms_max": max(ts), "reps": reps}
    if nbytes is not None:
        r.update(bytes=nbytes, bytes_per_s=nbytes / (r["ms_median"] * 1e-3),
                 fraction_of_hbm_peak=nbytes / (r["ms_median"] * 1e-3) / HBM_PEAK)
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=2000)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out")
    args = ap.parse_args()
    B, reps = args.batch, args.reps
    R = M * B
    L, st, p = _lib.lib(), _lib.stream_handle(), _lib.ptr
    f64 = dict(dtype=torch.float64, device="cuda")
    g = torch.Generator(device="cuda").manual_seed(0)
    # phases that drift about three slow common components: neither uniform nor locked
    th = 2 * np.pi * torch.rand((M, B, N), generator=g, **f64)
    th[:, :, : N // 2] = 0.8 * torch.randn((M, B, N // 2), generator=g, **f64) + th[:, :, :1]
    ph = torch.stack((torch.cos(th), torch.sin(th)), dim=-1).contiguous()
    del th
    res = {"M": M, "B": B, "N": N, "K": K, "hbm_peak_bytes_per_s": HBM_PEAK}

    def show(name, r):
        res[name] = r
        print(name, json.dumps(r), flush=True)

    vec = torch.empty((M, B, N), **f64)
    share = torch.empty((M, B), **f64)
    show("device_copy_of_the_phasors", timed(lambda: ph.clone(), reps, 2 * ph.numel() * 8))
    show("wc_leida_eigvec", timed(lambda: _lib.check(L.wc_leida_eigvec(R, N, p(ph), p(vec), p(share), st),
                                                     "wc_leida_eigvec"), reps, R * N * 24 + R * 8))
    del ph
    x = vec.view(R, N)
    rows = torch.randperm(R, generator=g, device="cuda")[:K]
    cent = x[rows].contiguous()
    labels = torch.empty(R, dtype=torch.int32, device="cuda")
    dist = torch.empty(R, **f64)
    new = torch.empty_like(cent)
    count = torch.empty(K, dtype=torch.int64, device="cuda")
    for metric, code in sigchain.KMEANS_METRICS.items():
        show(f"wc_kmeans_assign_{metric}",
             timed(lambda: _lib.check(L.wc_kmeans_assign(R, N, K, p(x), p(cent), code, p(labels), p(dist), st),
                                      "wc_kmeans_assign"), reps, R * N * 8 + R * 12))
        nbytes = L.wc_kmeans_workspace_size(R, N, K, code)
        ws = torch.empty(nbytes // 8, **f64)
        traffic = R * N * 8 * (2 if metric == "cosine" else 1) + R * 4 + 2 * nbytes
        show(f"wc_kmeans_update_{metric}",
             timed(lambda: _lib.check(L.wc_kmeans_update(R, N, K, p(x), p(labels), p(cent), code, p(new), p(count),
                                                         p(ws), nbytes, st), "wc_kmeans_update"), reps, traffic))
        res[f"wc_kmeans_update_{metric}"]["workspace_bytes"] = nbytes
        del ws
    lab2 = labels.view(M, B)
    occ, dwell, trans = torch.empty((B, K), **f64), torch.empty((B, K), **f64), torch.empty((B, K, K), **f64)
    show("wc_state_stats", timed(lambda: _lib.check(L.wc_state_stats(B, M, K, p(lab2), p(occ), p(dwell), p(trans), st),
                                                    "wc_state_stats"), reps, 3 * R * 4 + B * K * (K + 2) * 8))
    r = timed(lambda: sigchain.kmeans(vec, K, "cosine", max_iter=20, seed=0), 3)
    r["n_iter"] = sigchain.kmeans(vec, K, "cosine", max_iter=20, seed=0)[3]
    show("sigchain_kmeans_cosine_max_iter_20", r)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()

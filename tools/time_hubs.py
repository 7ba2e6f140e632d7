#!/usr/bin/env python3
"""wc_graph_rich_club, wc_graph_assortativity and wc_graph_score alone between HIP events, and
hubs.rich_club_norm end to end; median (min-max) over the repetitions after one warm-up.

  thr       B = 20,000 matrices of 90 nodes: the W empirical FC clipped at 0, every matrix times its own
            symmetric random factor in [1, 1.1] (tools/time_graph.py), thresholded on the device to a
            density of 0.2 and made exactly symmetric: about 800 edges;
  n96       B = 20,000 random symmetric matrices of 96 nodes, a third of the pairs connected: the
            16384-entry sort and 128 KiB of LDS;
  norm      rich_club_norm of 64 thr matrices against 100 null models each, weighted and binary, and the
            share of it that is the curves: wc_graph_rich_club alone on a [6400][90][90] stack.

rich_club is timed with all outputs, and with the binary ones alone (no sort), which gives the sort's
share.  The reference's own time per matrix, one host core, is what tests/golden/make_hubs_golden.py
prints.

  python tools/time_hubs.py [--batch 20000] [--reps 5] [--out FILE.json]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def thr_inputs(B, N=90, density=0.2):
    import torch

    from tools.time_graph import inputs
    dense = inputs(B, N)["fc_dense"]
    iu = torch.triu_indices(N, N, 1, device=dense.device)
    v = dense[:, iu[0], iu[1]]
    keep = int(v.shape[1] * density)
    cut = v.kthvalue(v.shape[1] - keep + 1, dim=1).values
    w = dense * (dense >= cut[:, None, None])
    return ((w + w.transpose(1, 2)) / 2).contiguous()


def n96_inputs(B, N=96):
    import torch
    g = torch.Generator(device="cuda").manual_seed(1)
    w = torch.rand((B, N, N), dtype=torch.float64, device="cuda", generator=g)
    w = torch.triu(w * (torch.rand((B, N, N), device="cuda", generator=g) < 0.35), 1)
    return (w + w.transpose(1, 2)).contiguous()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=20000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out")
    args = ap.parse_args()
    import torch

    from nremmodfc_amd import _lib, hubs
    from tools.time_graph import timed
    if not torch.cuda.is_available():
        raise SystemExit("time_hubs: no GPU")
    L, st, p = _lib.lib(), _lib.stream_handle(), _lib.ptr
    B = args.batch
    res = {"B": B, "cus": torch.cuda.get_device_properties(0).multi_processor_count}

    def launches(w, name):
        B, N = w.shape[0], w.shape[1]
        f = lambda *s: torch.empty(s, dtype=torch.float64, device="cuda")      # noqa: E731
        i = lambda *s: torch.empty(s, dtype=torch.int32, device="cuda")        # noqa: E731
        rw, rb, ek, nk, md = f(B, N), f(B, N), f(B, N), i(B, N), i(B)
        out = {"N": N, "edges": int((w[0] != 0).sum() // 2)}
        out["rich_club"] = timed(lambda: L.wc_graph_rich_club(B, N, p(w), 0, N, p(rw), p(rb), p(nk), p(ek), p(md), st), args.reps)
        out["maxdeg_mean"] = float(md.double().mean())
        out["finite_levels_mean"] = float(torch.isfinite(rw).sum(dim=1).double().mean())
        out["rich_club_binary_only"] = timed(lambda: L.wc_graph_rich_club(B, N, p(w), 0, N, None, p(rb), p(nk), p(ek), p(md), st),
                                             args.reps)
        r1, r2 = f(B), f(B)
        out["assortativity"] = timed(lambda: L.wc_graph_assortativity(B, N, p(w), 0, p(r1), p(r2), st), args.reps)
        S = 4
        lev = (w.sum(dim=1).max(dim=1).values[:, None] * torch.tensor([0.1, 0.25, 0.4, 0.5], dtype=torch.float64, device="cuda")).contiguous()
        mem, sn, rd = i(B, S, N), i(B, S), i(B, S)
        out["score_4_levels"] = timed(lambda: L.wc_graph_score(B, N, S, p(w), p(lev), p(mem), p(sn), p(rd), st), args.reps)
        out["score_rounds_mean"] = float(rd.double().mean())
        out["us_per_matrix_rich_club"] = 1e3 * out["rich_club"]["ms_median"] / B
        print(name, json.dumps(out), flush=True)
        return out

    thr = thr_inputs(B)
    res["thr"] = launches(thr, "thr")
    n96 = n96_inputs(B)
    res["n96"] = launches(n96, "n96")
    del n96

    w = thr[:64].contiguous()
    norm = {"B": 64, "reps": 100}
    for kind in ("weighted", "binary"):
        norm[kind] = timed(lambda: (hubs.rich_club_norm(w, kind, reps=100), 0)[1], max(2, args.reps // 2))
        out = hubs.rich_club_norm(w, kind, reps=100)
        norm[kind]["finite_levels_mean"] = float(torch.isfinite(out["norm"]).sum(dim=1).double().mean())
        norm[kind]["norm_max_mean"] = float(torch.nan_to_num(out["norm"], nan=0.0).max(dim=1).values.mean())
    nulls = thr[:6400].contiguous()                                             # as many matrices as 64 x 100 null models
    n = nulls.shape[0]
    rw, md = torch.empty((n, 90), dtype=torch.float64, device="cuda"), torch.empty((n,), dtype=torch.int32, device="cuda")
    norm["curves_alone"] = dict(timed(lambda: L.wc_graph_rich_club(n, 90, p(nulls), 0, 90, p(rw), None, None, None, p(md), st),
                                      args.reps), matrices=n)
    res["norm"] = norm
    print("norm", json.dumps(norm), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()

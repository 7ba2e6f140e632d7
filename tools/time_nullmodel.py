#!/usr/bin/env python3
"""wc_graph_null_model alone between HIP events at the size one participation_coef_norm sweep step has:
B = 16 matrices of 90 nodes, R = 100 seeds each, 1,600 null models a launch, the defaults (bin_swaps 5,
period 10, the BCT negative half); median (min-max) over the repetitions after one warm-up, and the
time per null model from the median.  Two stacks:

  thr       the W empirical FC clipped at 0, every matrix times its own symmetric random factor in
            [1, 1.1], thresholded to a density of 0.2 (graph_utils.thresholding): 801 positive edges;
  centred   tools/time_louvain_sign.py's signed matrices: the centred FC, about 1,900 positive and 2,100
            negative edges.

The two phases are timed on their own as well: the rewiring as wc_graph_rewire with the same
bin_swaps, the weight assignment as wc_graph_null_model with bin_swaps = 0 (the same number of sorts
and picks, on the pattern of w itself); their shares are those times over their sum.  The reference's
own time per null model, one host core, is what tests/golden/make_nullmodel_golden.py prints.

  python tools/time_nullmodel.py [--batch 16] [--seeds 100] [--reps 5] [--out FILE.json]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def thr_inputs(B, N=90):
    from nremmodfc_amd import datasets, graph_utils
    fc = np.maximum(datasets.load_empfc("W").astype(np.float64), 0.0)
    np.fill_diagonal(fc, 0.0)
    f = 1 + 0.1 * np.random.default_rng(1).random((B, N, N))
    return np.stack([graph_utils.thresholding(m) for m in fc[None] * (f + f.transpose(0, 2, 1)) / 2])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--seeds", type=int, default=100)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out")
    args = ap.parse_args()
    import torch

    from nremmodfc_amd import _lib, nullmodel
    from tools.time_graph import timed
    from tools.time_louvain_sign import signed_inputs
    if not torch.cuda.is_available():
        raise SystemExit("time_nullmodel: no GPU")
    B, R, N = args.batch, args.seeds, 90
    L, st, p = _lib.lib(), _lib.stream_handle(), _lib.ptr
    sd = torch.arange(R, dtype=torch.int64, device="cuda")
    out = torch.empty((B, R, N, N), dtype=torch.float64, device="cuda")
    r = torch.empty((B, R, 2), dtype=torch.float64, device="cuda")
    info = torch.empty((B, R, 3), dtype=torch.int32, device="cuda")
    ws_bytes = B * R * nullmodel.null_model_slot_bytes(N)
    ws = torch.empty(ws_bytes // 8, dtype=torch.float64, device="cuda")
    res = {"B": B, "R": R, "N": N, "nulls": B * R, "bin_swaps": 5, "period": 10, "ws_bytes": ws_bytes,
           "cus": torch.cuda.get_device_properties(0).multi_processor_count}
    for name, stack in (("thr", thr_inputs(B)), ("centred", signed_inputs(B))):
        stack = (stack + stack.transpose(0, 2, 1)) / 2                     # exactly symmetric
        w = torch.from_numpy(np.ascontiguousarray(stack)).cuda()

        def null(swaps):
            return timed(lambda: L.wc_graph_null_model(B, R, N, p(w), swaps, 10, 1, p(sd), p(out), p(r), p(info), p(ws),
                                                       ws_bytes, st), args.reps)

        full = null(5)
        h = info.cpu().numpy().reshape(-1, 3)
        rr = r.cpu().numpy().reshape(-1, 2)
        rewire = timed(lambda: L.wc_graph_rewire(B, R, N, p(w), 5, p(sd), p(out), p(info), p(ws), ws_bytes, st), args.reps)
        assign = null(0)
        both = rewire["ms_median"] + assign["ms_median"]
        res[name] = {"null_model": full, "rewire_alone": rewire, "assignment_alone": assign,
                     "ms_per_null": full["ms_median"] / (B * R),
                     "share_rewiring": rewire["ms_median"] / both, "share_assignment": assign["ms_median"] / both,
                     "edges_pos": int((stack[0] > 0).sum() // 2), "edges_neg": int((stack[0] < 0).sum() // 2),
                     "eff_mean": float(h[:, 0].mean()), "draws_mean": float(h[:, 1].mean()), "refused": int((h[:, 2] != 0).sum()),
                     "rpos_mean": float(np.nanmean(rr[:, 0])), "rneg_mean": float(np.nanmean(rr[:, 1])) if name == "centred" else None}
        print(name, json.dumps(res[name]), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()

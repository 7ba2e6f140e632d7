#!/usr/bin/env python3
"""wc_graph_louvain_sign alone between HIP events, at the size tools/time_louvain.py times the unsigned
kernel at: B = 2,000 matrices of 90 nodes, R = 10 seeds each, 20,000 independent problems a launch;
median (min-max) over the repetitions after one warm-up, and problems per second from the median.  Two
sets of matrices:

  signed    the W empirical FC with the diagonal zeroed and the mean of its upper triangle subtracted
            (weights of both signs), every matrix times its own symmetric random factor in [1, 1.1];
            timed with each of the five qtypes;
  thr       time_louvain.py's own non-negative matrices (the FC clipped at 0, density 0.2), qtype "sta",
            and wc_graph_louvain on the same problems in the same process: the signed kernel finds
            the same partitions there, so the two times compare kernel against kernel.

The runs are summarised (modules, levels, sweeps per problem): the time is the serial node visits.
--slots sets the workspace (a slot of 16 N^2 bytes per workgroup; the default is the wrapper's, 2048).

--host N times the signed problems of the first N matrices ("sta") on 16 host processes (--procs): the
numpy restatement of the tests (tests/louvain_sign_reference.py).  --host-only skips the device.

  python tools/time_louvain_sign.py [--batch 2000] [--seeds 10] [--reps 7] [--slots 2048] [--host 64] [--out FILE.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

QTYPES = ("sta", "pos", "smp", "gja", "neg")


def signed_inputs(B, N=90):
    """[B][N][N] fp64 on the host: the centred W empirical FC times a symmetric factor in [1, 1.1] per matrix."""
    from nremmodfc_amd import datasets
    fc = datasets.load_empfc("W").astype(np.float64)
    np.fill_diagonal(fc, 0.0)
    fc = fc - fc[np.triu_indices(N, 1)].mean()
    np.fill_diagonal(fc, 0.0)
    f = 1 + 0.1 * np.random.default_rng(0).random((B, N, N))
    return fc[None] * (f + f.transpose(0, 2, 1)) / 2


# ---- the host side: worker processes that never touch the device ----

_host = {}


def _host_init():
    from tests import louvain_sign_reference as ls
    _host["ls"] = ls


def _host_run(job):
    w, seed = job
    ci, q, _, _ = _host["ls"].louvain_sign(w, seed)
    return int(np.max(ci)) + 1, q


def host_rate(ws, seeds, procs):
    import multiprocessing as mp
    jobs = [(w, s) for w in ws for s in seeds]
    with mp.get_context("spawn").Pool(procs, _host_init) as pool:
        pool.map(_host_run, jobs[:procs])                  # imports and first calls
        t0 = time.perf_counter()
        out = pool.map(_host_run, jobs, chunksize=max(1, len(jobs) // (4 * procs)))
        dt = time.perf_counter() - t0
    cpus = len(os.sched_getaffinity(0))
    return {"what": "numpy restatement, sta", "procs": procs, "cpus_available": cpus, "problems": len(jobs),
            "seconds": dt, "problems_per_s": len(jobs) / dt,
            "ms_per_problem_per_cpu": 1e3 * dt * min(procs, cpus) / len(jobs),
            "modules_mean": float(np.mean([k for k, _ in out])), "q_mean": float(np.mean([q for _, q in out]))}


# ---- the device ----

def device_rates(signed, thr, seeds, reps, slots):
    import torch

    from nremmodfc_amd import _lib, partition
    from tools.time_graph import timed
    if not torch.cuda.is_available():
        raise SystemExit("time_louvain_sign: no GPU; use --host-only for the host side alone")
    B, N, R = signed.shape[0], signed.shape[1], len(seeds)
    L, st, p = _lib.lib(), _lib.stream_handle(), _lib.ptr
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    sd = torch.from_numpy(np.array(seeds, dtype=np.uint64).view(np.int64)).cuda()
    ci = torch.empty((B, R, N), dtype=torch.int32, device="cuda")
    q = torch.empty((B, R), dtype=torch.float64, device="cuda")
    info = torch.empty((B, R, 2), dtype=torch.int32, device="cuda")
    ws_bytes = min(slots, B * R) * partition.louvain_sign_slot_bytes(N)
    ws = torch.empty(ws_bytes // 8, dtype=torch.float64, device="cuda")
    res = {"B": B, "R": R, "N": N, "problems": B * R, "slots": min(slots, B * R), "ws_bytes": ws_bytes}

    def summary(t):
        h = info.cpu().numpy().reshape(-1, 2)
        t["problems_per_s"] = B * R / (1e-3 * t["ms_median"])
        t["us_per_sweep_per_wave"] = 1e3 * t["ms_median"] * min(B * R, cus) / float(h[:, 1].sum())
        t["runs"] = {"modules_mean": float((ci.max(dim=2).values + 1).double().mean()), "q_mean": float(q.mean()),
                     "levels_mean": float(h[:, 0].mean()), "sweeps_mean": float(h[:, 1].mean()),
                     "sweeps_max": int(h[:, 1].max()), "unsettled": int((ci[:, :, 0] < 0).sum())}
        return t

    def sign(w, qtype):
        return summary(timed(lambda: L.wc_graph_louvain_sign(B, R, N, p(w), 1.0, QTYPES.index(qtype), p(sd), p(ci), p(q),
                                                              p(info), p(ws), ws_bytes, st), reps))

    w = torch.from_numpy(signed).cuda()
    res["signed"] = {qtype: sign(w, qtype) for qtype in QTYPES}
    w = torch.from_numpy(thr).cuda()
    res["thr_sign_sta"] = sign(w, "sta")
    part = ci.clone()
    ko, ki = w.sum(dim=2), w.sum(dim=1)
    s = ko.sum(dim=1).contiguous()
    obj = (w - ko[:, :, None] * ki[:, None, :] / s[:, None, None]).contiguous()
    res["thr_unsigned"] = summary(timed(
        lambda: L.wc_graph_louvain(B, R, N, p(obj), p(s), None, p(sd), p(ci), p(q), p(info), st), reps))
    res["thr_same_partitions"] = float((part == ci).all(dim=2).double().mean())
    res["thr_sign_over_unsigned"] = res["thr_sign_sta"]["ms_median"] / res["thr_unsigned"]["ms_median"]
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=2000)
    ap.add_argument("--seeds", type=int, default=10)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--slots", type=int, default=2048)
    ap.add_argument("--host", type=int, default=0, metavar="MATRICES")
    ap.add_argument("--procs", type=int, default=16)
    ap.add_argument("--host-only", action="store_true")
    ap.add_argument("--out")
    args = ap.parse_args()
    seeds = list(range(args.seeds))
    signed = signed_inputs(max(args.batch, args.host))
    res = {}
    if args.host:                                          # first: its processes start before the device is open
        res["host"] = host_rate(signed[:args.host], seeds, args.procs)
        print("host", json.dumps(res["host"]), flush=True)
    if not args.host_only:
        from tools.time_louvain import inputs
        res["device"] = device_rates(signed[:args.batch], inputs(args.batch), seeds, args.reps, args.slots)
        print("device", json.dumps(res["device"]), flush=True)
        if args.host:
            res["device_over_host"] = res["device"]["signed"]["sta"]["problems_per_s"] / res["host"]["problems_per_s"]
            print("device over host:", round(res["device_over_host"], 1), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""wc_graph_louvain alone between HIP events, at the size of docs/CHANGELOG.md: B = 2,000 FC matrices of
90 nodes on the thresholded empirical FC's support (density 0.2), every matrix times its own symmetric
random factor in [1, 1.1] so that no two runs take the same turns, R = 10 seeds each: 20,000
independent problems a launch.  The objective matrices are built beforehand; median (min-max) over the
repetitions after one warm-up, and problems per second from the median.  Beside it the whole
sigchain.graph_louvain call (objective, refusal check and launch) and wc_graph_agreement on the
partitions found.  The partitions are summarised (modules, levels, sweeps per problem) because the
kernel's time is the serial node visits, sweeps x N per problem.

--host N times the same problems of the first N matrices on 16 host processes (--procs), one GPU's
share of the host: the numpy restatement of the tests (tests/louvain_reference.py) or, with
--reference DIR, the reference's own community_louvain taken out of DIR/graph_utils.py with `ast` and
run unmodified under its own np.random.permutation (as tests/golden/make_louvain_golden.py takes it;
build machine only).  --host-only skips the device.

  python tools/time_louvain.py [--batch 2000] [--seeds 10] [--reps 7] [--host 64] [--reference DIR] [--out FILE.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def inputs(B, N=90):
    """[B][N][N] fp64 on the host: the W empirical FC clipped at 0, thresholded to density 0.2, times
    a symmetric factor in [1, 1.1] per matrix."""
    from nremmodfc_amd import datasets, graph_utils
    fc = np.maximum(datasets.load_empfc("W").astype(np.float64), 0.0)
    np.fill_diagonal(fc, 0.0)
    thr = graph_utils.thresholding(fc.copy(), 0.2)
    f = 1 + 0.1 * np.random.default_rng(0).random((B, N, N))
    return thr[None] * (f + f.transpose(0, 2, 1)) / 2


# ---- the host side: worker processes that never touch the device ----

_host = {}


def _host_init(reference):
    from tests import louvain_reference as lref
    _host["lref"] = lref
    if reference:
        from tests.golden.make_louvain_golden import reference_defs
        _host["ref"] = reference_defs(reference)["community_louvain"]


def _host_run(job):
    w, seed = job
    if "ref" in _host:
        ci, q = _host["ref"](w.copy(), 1, None, "modularity", seed)
        return int(np.max(ci)), float(q)
    ci, q, _, _ = _host["lref"].louvain(*_host["lref"].objective(w), seed)
    return int(np.max(ci)) + 1, q


def host_rate(ws, seeds, procs, reference):
    import multiprocessing as mp
    jobs = [(w, s) for w in ws for s in seeds]
    with mp.get_context("spawn").Pool(procs, _host_init, (reference,)) as pool:
        pool.map(_host_run, jobs[:procs])                  # imports and first calls
        t0 = time.perf_counter()
        out = pool.map(_host_run, jobs, chunksize=max(1, len(jobs) // (4 * procs)))
        dt = time.perf_counter() - t0
    cpus = len(os.sched_getaffinity(0))
    return {"what": "reference community_louvain" if reference else "numpy restatement", "procs": procs,
            "cpus_available": cpus, "problems": len(jobs), "seconds": dt, "problems_per_s": len(jobs) / dt,
            "ms_per_problem_per_cpu": 1e3 * dt * min(procs, cpus) / len(jobs),
            "modules_mean": float(np.mean([k for k, _ in out])), "q_mean": float(np.mean([q for _, q in out]))}


# ---- the device ----

def device_rates(ws, seeds, reps):
    import torch

    from nremmodfc_amd import _lib, sigchain
    from tools.time_graph import timed
    if not torch.cuda.is_available():
        raise SystemExit("time_louvain: no GPU; use --host-only for the host side alone")
    B, N, R = ws.shape[0], ws.shape[1], len(seeds)
    L, st, p = _lib.lib(), _lib.stream_handle(), _lib.ptr
    w = torch.from_numpy(ws).cuda()
    ko, ki = w.sum(dim=2), w.sum(dim=1)
    s = ko.sum(dim=1).contiguous()
    obj = (w - ko[:, :, None] * ki[:, None, :] / s[:, None, None]).contiguous()
    sd = torch.from_numpy(np.array(seeds, dtype=np.uint64).view(np.int64)).cuda()
    ci = torch.empty((B, R, N), dtype=torch.int32, device="cuda")
    q = torch.empty((B, R), dtype=torch.float64, device="cuda")
    info = torch.empty((B, R, 2), dtype=torch.int32, device="cuda")
    D = torch.empty((B, N, N), dtype=torch.float64, device="cuda")
    res = {"B": B, "R": R, "N": N, "problems": B * R, "density": float((w[0] != 0).double().sum() / (N * N - N))}
    res["louvain_kernel"] = timed(
        lambda: L.wc_graph_louvain(B, R, N, p(obj), p(s), None, p(sd), p(ci), p(q), p(info), st), reps)
    res["agreement_kernel"] = timed(lambda: L.wc_graph_agreement(B, R, N, p(ci), p(D), st), reps)

    def whole():
        sigchain.graph_louvain(w, seeds=list(seeds))
        return 0
    res["graph_louvain_call"] = timed(whole, reps)
    for k in ("louvain_kernel", "graph_louvain_call"):
        res[k]["problems_per_s"] = B * R / (1e-3 * res[k]["ms_median"])
    h = info.cpu().numpy().reshape(-1, 2)
    res["runs"] = {"modules_mean": float((ci.max(dim=2).values + 1).double().mean()), "q_mean": float(q.mean()),
                   "levels_mean": float(h[:, 0].mean()), "sweeps_mean": float(h[:, 1].mean()),
                   "sweeps_max": int(h[:, 1].max()), "unsettled": int((ci[:, :, 0] < 0).sum())}
    res["louvain_kernel"]["us_per_sweep_per_wave"] = (   # a wave's time per sweep: waves in flight x time / sweeps
        1e3 * res["louvain_kernel"]["ms_median"] * min(B * R, torch.cuda.get_device_properties(0).multi_processor_count)
        / float(h[:, 1].sum()))
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=2000)
    ap.add_argument("--seeds", type=int, default=10)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--host", type=int, default=0, metavar="MATRICES")
    ap.add_argument("--procs", type=int, default=16)
    ap.add_argument("--reference", metavar="DIR")
    ap.add_argument("--host-only", action="store_true")
    ap.add_argument("--out")
    args = ap.parse_args()
    seeds = list(range(args.seeds))
    ws = inputs(max(args.batch, args.host))
    res = {}
    if args.host:                                          # first: its processes start before the device is open
        res["host"] = host_rate(ws[:args.host], seeds, args.procs, args.reference)
        print("host", json.dumps(res["host"]), flush=True)
    if not args.host_only:
        res["device"] = device_rates(ws[:args.batch], seeds, args.reps)
        print("device", json.dumps(res["device"]), flush=True)
        if args.host:
            res["device_over_host"] = res["device"]["louvain_kernel"]["problems_per_s"] / res["host"]["problems_per_s"]
            print("device over host:", round(res["device_over_host"], 1), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()

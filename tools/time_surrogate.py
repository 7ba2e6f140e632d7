#!/usr/bin/env python3
"""The surrogate test of the FC between HIP events: B = 2,000 simulations of L = 298 samples and N = 90
nodes, S = 50 surrogates each (100,000 correlation matrices a call); median (min-max) over the repetitions
after one warm-up.  Timed apart: the spectrum stage (wc_spectrogram, one segment of L samples),
wc_surrogate_fc, wc_surrogate_test, and the whole of surrogate.fc_surrogate_test (with the copies, the FC
through wc_corrcoef and the Python around them).  The series are the tests' kind: noisy columns in five
groups with a non-zero mean.

--host N times the numpy restatement of the tests (tests/surrogate_reference.py:thresholded) on the first N
series on 16 host processes (--procs), one BLAS thread each.  --host-only skips the device.

  python tools/time_surrogate.py [--batch 2000] [--surr 50] [--reps 7] [--host 64] [--out FILE.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def inputs(B, L=298, N=90, groups=5):
    """[L][B][N] fp64 on the host."""
    rng = np.random.default_rng(0)
    common = rng.standard_normal((L, B, groups))
    return common[:, :, np.arange(N) % groups] + rng.standard_normal((L, B, N)) + 3.0


# ---- the host side: worker processes that never touch the device ----

_host = {}


def _host_init():
    from tests import surrogate_reference as sr
    _host["sr"] = sr


def _host_run(job):
    y, seeds = job
    r = _host["sr"].thresholded(y, seeds)
    return int((_host["sr"].uptri(r["fc_adj"]) != 0).sum())


def host_rate(x, seeds, procs):
    import multiprocessing as mp
    jobs = [(np.ascontiguousarray(x[:, b]), seeds) for b in range(x.shape[1])]
    threads = {k: os.environ.get(k) for k in ("OMP_NUM_THREADS", "OPENBLAS_NUM_THREADS", "MKL_NUM_THREADS")}
    os.environ.update({k: "1" for k in threads})           # a worker is one BLAS thread: it reads this as it starts
    pool = mp.get_context("spawn").Pool(procs, _host_init)
    for k, v in threads.items():
        os.environ.pop(k) if v is None else os.environ.__setitem__(k, v)
    with pool:
        pool.map(_host_run, jobs[:procs])                  # imports and first calls
        t0 = time.perf_counter()
        kept = pool.map(_host_run, jobs, chunksize=1)
        dt = time.perf_counter() - t0
    cpus = len(os.sched_getaffinity(0))
    return {"what": "numpy restatement", "procs": procs, "cpus_available": cpus, "simulations": len(jobs),
            "surrogates": len(seeds), "seconds": dt, "simulations_per_s": len(jobs) / dt,
            "ms_per_simulation_per_cpu": 1e3 * dt * min(procs, cpus) / len(jobs), "kept_mean": float(np.mean(kept))}


# ---- the device ----

def device_rates(x, seeds, reps):
    import torch

    from nremmodfc_amd import _lib, surrogate
    from tools.time_graph import timed
    if not torch.cuda.is_available():
        raise SystemExit("time_surrogate: no GPU; use --host-only for the host side alone")
    Ln, B, N = x.shape
    S, P = len(seeds), N * (N - 1) // 2
    L, st, p = _lib.lib(), _lib.stream_handle(), _lib.ptr
    xd = torch.from_numpy(x).cuda()
    sd = torch.from_numpy(np.array(seeds, dtype=np.uint64).view(np.int64)).cuda()
    ones = torch.ones(Ln, dtype=torch.float64, device="cuda")
    spec = torch.empty((Ln // 2 + 1, B * N), dtype=torch.complex128, device="cuda")
    ws_bytes = L.wc_spectrogram_workspace_size(Ln)
    ws = torch.empty(ws_bytes // 8 + 1, dtype=torch.float64, device="cuda")
    sfc = torch.empty((B, S, P), dtype=torch.float64, device="cuda")
    fc = surrogate._fc(xd)
    p_adj, fc_adj = torch.empty_like(fc), torch.empty_like(fc)
    res = {"B": B, "S": S, "N": N, "L": Ln, "matrices": B * S, "sfc_bytes": sfc.numel() * 8, "spec_bytes": spec.numel() * 16}
    res["spectrum"] = timed(lambda: L.wc_spectrogram(B * N, Ln, p(xd), Ln, 0, p(ones), 1, 1.0, 1, p(spec), p(ws),
                                                     ws_bytes, st), reps)
    t = res["surrogate_fc"] = timed(lambda: L.wc_surrogate_fc(B, N, Ln, S, p(spec), p(sd), p(sfc), st), reps)
    t["matrices_per_s"] = B * S / (1e-3 * t["ms_median"])
    t["gram_tflops"] = 2.0 * N * N * (Ln - 1) * B * S / (1e-3 * t["ms_median"]) / 1e12   # the full N x N products' count
    res["surrogate_test"] = timed(lambda: L.wc_surrogate_test(B, N, S, p(fc), p(sfc), 0.05, p(p_adj), p(fc_adj), None,
                                                              None, None, st), reps)
    res["kept_mean"] = float((fc_adj != 0).sum(dim=(1, 2)).double().mean() / 2)
    res["nan_matrices"] = int(p_adj[:, 0, 0].isnan().sum())
    del sfc, spec

    def whole():
        surrogate.fc_surrogate_test(xd, surr_number=S, seeds=seeds)
        return 0
    res["fc_surrogate_test"] = timed(whole, reps)
    res["kernels_ms"] = sum(res[k]["ms_median"] for k in ("spectrum", "surrogate_fc", "surrogate_test"))
    res["simulations_per_s"] = B / (1e-3 * res["fc_surrogate_test"]["ms_median"])
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=2000)
    ap.add_argument("--surr", type=int, default=50)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--host", type=int, default=0, metavar="SIMULATIONS")
    ap.add_argument("--procs", type=int, default=16)
    ap.add_argument("--host-only", action="store_true")
    ap.add_argument("--out")
    args = ap.parse_args()
    seeds = list(range(1, args.surr + 1))
    x = inputs(max(args.batch, args.host))
    res = {}
    if args.host:                                          # first: its processes start before the device is open
        res["host"] = host_rate(x[:, :args.host], seeds, args.procs)
        print("host", json.dumps(res["host"]), flush=True)
    if not args.host_only:
        res["device"] = device_rates(np.ascontiguousarray(x[:, :args.batch]), seeds, args.reps)
        print("device", json.dumps(res["device"]), flush=True)
        if args.host:
            res["device_over_host"] = res["device"]["simulations_per_s"] / res["host"]["simulations_per_s"]
            print("device over host:", round(res["device_over_host"], 1), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()

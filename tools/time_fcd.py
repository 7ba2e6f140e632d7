#!/usr/bin/env python3
"""Dynamic FC between HIP events at the shipped shape: 20,000 simulations of 298 BOLD samples x 90 nodes,
window 30, steps 1 and 3 (wc_fcd alone, the buffers allocated beforehand, at the facade's default 1 GiB
workspace and at 8 GiB), the phase form (wc_fcd_phase alone, and hilbert_phase before it), the host numpy
restatement (tests/fcd_reference.py) per simulation, and today's composition -- a sigchain.corrcoef launch
per window, the upper triangles gathered, torch.corrcoef per simulation -- at a batch it can hold.
Median (min-max) over the repetitions after one warm-up.  The algorithmic flop count of wc_fcd is
nw P 3 W for the patterns plus nw^2 P for the Gram (multiply-adds counted as two would double it; the
fraction printed is of the 78.6 TFLOP/s fp64 vector peak, with this count as it stands).

  python tools/time_fcd.py [--batch 20000] [--small 64] [--out FILE.json]
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
from nremmodfc_amd import _lib, sigchain  # noqa: E402
from tests import fcd_reference as ref  # noqa: E402

M, N, W = 298, 90, 30
P = N * (N - 1) // 2
PEAK = 78.6e12


def timed(fn, reps):
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
    return {"ms_median": float(np.median(ts)), "ms_min": min(ts), "ms_max": max(ts), "reps": reps}


def series(B):
    """BOLD-like: three slow components shared within a simulation, noise, offsets of several sd."""
    g = torch.Generator(device="cuda").manual_seed(0)
    f64 = dict(dtype=torch.float64, device="cuda")
    t = torch.arange(M, **f64)[:, None, None]
    x = 0.7 * torch.randn((M, B, N), generator=g, **f64)
    for _ in range(3):
        freq = 0.02 + 0.1 * torch.rand((1, B, 1), generator=g, **f64)
        x += torch.sin(2 * np.pi * freq * t) * (2 * torch.rand((1, B, N), generator=g, **f64) - 1)
    return (x + 3 + 5 * torch.rand((1, B, N), generator=g, **f64)).contiguous()


def composition(x, step):
    """What the package could do before wc_fcd: the patterns materialised, a launch per window."""
    B = x.shape[1]
    nw = (M - W) // step + 1
    iu = torch.triu_indices(N, N, 1, device=x.device)
    pats = torch.empty((B, nw, P), dtype=torch.float64, device=x.device)
    for k in range(nw):
        fc = sigchain.corrcoef(x[k * step:k * step + W], B, N)
        pats[:, k] = fc[:, iu[0], iu[1]]
    return torch.stack([torch.corrcoef(pats[b]) for b in range(B)])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=20000)
    ap.add_argument("--small", type=int, default=64)
    ap.add_argument("--out")
    args = ap.parse_args()
    B = args.batch
    L, st, p = _lib.lib(), _lib.stream_handle(), _lib.ptr
    res = {"batch": B, "small_batch": args.small}
    x = series(B)
    for step in (1, 3):
        nw = (M - W) // step + 1
        flop = nw * P * 3 * W + nw * nw * P
        out = torch.empty((B, nw, nw), dtype=torch.float64, device="cuda")
        for gib in (1, 8):
            nbytes = max(L.wc_fcd_workspace_size(B, N, M, W, step), min((nw * P + nw) * 8 * B, gib << 30))
            ws = torch.empty(nbytes // 8, dtype=torch.float64, device="cuda")
            r = timed(lambda: _lib.check(L.wc_fcd(B, N, M, p(x), W, step, p(out), None, p(ws), nbytes, st),
                                         "wc_fcd"), 3)
            r.update(nw=nw, flop_per_sim=flop, ws_bytes=nbytes,
                     fraction_of_fp64_peak=flop * B / (r["ms_median"] * 1e-3) / PEAK)
            res[f"wc_fcd_step{step}_ws{gib}GiB"] = r
            print(f"wc_fcd step {step} ws {gib} GiB", json.dumps(r), flush=True)
            del ws
        # the composition and the kernel at the same small batch
        xs = x[:, :args.small].contiguous()
        r = timed(lambda: composition(xs, step), 2)
        res[f"composition_step{step}_B{args.small}"] = r
        print(f"composition step {step} B {args.small}", json.dumps(r), flush=True)
        r = timed(lambda: sigchain.fcd(xs, W, step), 5)
        res[f"sigchain_fcd_step{step}_B{args.small}"] = r
        print(f"sigchain.fcd step {step} B {args.small}", json.dumps(r), flush=True)
        dev = (composition(xs[:, :2].contiguous(), step) - sigchain.fcd(xs[:, :2].contiguous(), W, step)).abs().max()
        res[f"composition_vs_kernel_step{step}"] = float(dev)
        # the host restatement, one simulation
        h = x[:, 0].cpu().numpy()
        t0 = time.perf_counter()
        for _ in range(3):
            ref.fcd(h, W, step)
        res[f"numpy_step{step}_ms_per_sim"] = (time.perf_counter() - t0) / 3 * 1e3
        print(f"numpy step {step}: {res[f'numpy_step{step}_ms_per_sim']:.1f} ms a simulation", flush=True)
        del out
    # the phase form: hilbert_phase, then wc_fcd_phase alone
    x2 = (x - x.mean(dim=0, keepdim=True)).reshape(M, B * N).contiguous()
    res["hilbert_phase"] = timed(lambda: sigchain.hilbert_phase(x2), 3)
    ph = sigchain.hilbert_phase(x2)
    del x, x2
    out = torch.empty((B, M, M), dtype=torch.float64, device="cuda")
    res["wc_fcd_phase"] = timed(lambda: _lib.check(L.wc_fcd_phase(B, N, M, p(ph), p(out), st), "wc_fcd_phase"), 3)
    print("hilbert_phase", json.dumps(res["hilbert_phase"]), "wc_fcd_phase", json.dumps(res["wc_fcd_phase"]),
          flush=True)
    h = ph.view(M, B, N, 2)[:, 0].cpu().numpy()
    t0 = time.perf_counter()
    for _ in range(3):
        ref.fcd_phase(h)
    res["numpy_phase_ms_per_sim"] = (time.perf_counter() - t0) / 3 * 1e3
    print(f"numpy phase: {res['numpy_phase_ms_per_sim']:.1f} ms a simulation", flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()

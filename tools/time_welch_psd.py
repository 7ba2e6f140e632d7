"""sigchain.welch (wc_welch_psd) at the four shapes of docs/CHANGELOG.md: HIP events, median of 5
after a warm-up, with the bytes the passes move (segment reads nseg * nperseg * C * 8, the block
partials written and read back, the PSD) and the compulsory ones (x once, the PSD once).  Beside
it, for orientation: scipy.signal.welch on the host (one run, wall clock), and at 48,000 x 1,800
the sweep's wc_welch_accumulate (fp64, node-major copy of the same data) per 4000-sample segment.
python tools/time_welch_psd.py"""
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from nremmodfc_amd import sigchain as wsg  # noqa: E402


def med(fn, n=5):
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(n):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b))
    ts.sort()
    return ts[n // 2], ts[0], ts[-1]


def sig(M, C):
    g = torch.Generator(device="cuda").manual_seed(M)
    t = torch.arange(M, device="cuda", dtype=torch.float64)[:, None] * 0.002
    f = 2 + 10 * torch.rand(C, generator=g, device="cuda", dtype=torch.float64)
    return (0.2 + 0.05 * torch.cos(2 * np.pi * f * t) * (1 + 0.3 * torch.sin(0.6 * t))
            + 0.0005 * torch.randn((M, C), generator=g, device="cuda", dtype=torch.float64)).contiguous()


for T, C, n, host in ((300_000, 90, 1000, True), (30_000, 90, 400, True), (298, 5760, 256, True),
                      (48_000, 1800, 4000, False)):
    nov = n // 2
    x = sig(T, C)
    # workspace allocation is inside the wrapper (torch's caching allocator), the window is cached
    t = med(lambda: wsg.welch(x, 500.0, "hann", n, nov))
    nseg = (T - n) // (n - nov) + 1
    sb = 2 * -(-nseg // 32)
    nb, F = -(-nseg // sb), n // 2 + 1
    moved = (nseg * n * C + 2 * nb * F * C + F * C) * 8
    compulsory = (T * C + F * C) * 8
    line = (f"welch T={T} C={C} nperseg={n} noverlap={nov}: {t[0]:.3f} ms ({t[1]:.3f}-{t[2]:.3f})  "
            f"{nseg} segments in {nb} blocks  moved {moved / 1e6:.1f} MB = {moved / t[0] / 1e6:.1f} GB/s  "
            f"compulsory {compulsory / 1e6:.1f} MB = {compulsory / t[0] / 1e6:.1f} GB/s")
    if host:
        from scipy import signal
        xh = x.cpu().numpy()
        t0 = time.perf_counter()
        signal.welch(xh, 500.0, "hann", n, nov, axis=0)
        line += f"  scipy on the host {1e3 * (time.perf_counter() - t0):.1f} ms"
    else:
        B, N = C // 90, 90
        nodemajor = x.t().contiguous()  # [C][T]
        wa = wsg.WelchAccumulator(B, N, x.device)
        a = med(lambda: wa.accumulate(nodemajor, T, T, 1, 0))
        line += (f"  wc_welch_accumulate fp64 {a[0]:.3f} ms per segment ({a[1]:.3f}-{a[2]:.3f}), "
                 f"x {nseg} segments = {a[0] * nseg:.1f} ms; wc_welch_psd per segment {t[0] / nseg:.3f} ms")
        del nodemajor
    print(line, flush=True)
    del x
    torch.cuda.empty_cache()

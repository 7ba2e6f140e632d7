"""sigchain.csd / coherence (wc_csd) at the four shapes of docs/CHANGELOG.md: HIP events, median of 5
after a warm-up, with the bytes the passes move: pass 1 reads the segments (nseg * nperseg * C * 8)
and writes their spectra (nseg * F * C * 16), pass 2 reads two 32-column strips of them per tile
pair and bin (matrix modes) or each spectrum once (pair modes), and the output is written once (the
default workspace holds every segment: one chunk, no running sums re-read).  Beside it, for
orientation only: sigchain.welch (wc_welch_psd) on the same input, the floor of pass 1, and where it
finishes in under a minute a host numpy loop over the segments (one run, wall clock).
python tools/time_csd.py"""
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


def host_loop(x, n, nov, pairs):
    from scipy import signal
    win = signal.get_window("hann", n)[:, None]
    C = x.shape[1]
    P = np.zeros((n // 2 + 1, C // 2) if pairs else (n // 2 + 1, C, C), dtype=np.complex128)
    for s in range((x.shape[0] - n) // (n - nov) + 1):
        seg = x[s * (n - nov):s * (n - nov) + n]
        X = np.fft.rfft((seg - seg.mean(axis=0)) * win, axis=0)
        P += np.conj(X[:, :C // 2]) * X[:, C // 2:] if pairs else np.conj(X)[:, :, None] * X[:, None, :]
    return P


for T, C, n, pairs in ((300_000, 90, 1000, False), (30_000, 90, 400, False), (48_000, 1000, 256, False),
                       (298, 5760, 256, True)):
    nov = n // 2
    x = sig(T, C)
    xa, xb = (x[:, :C // 2].contiguous(), x[:, C // 2:].contiguous()) if pairs else (x, None)
    nseg, F = (T - n) // (n - nov) + 1, n // 2 + 1
    need = wsg._lib.lib().wc_csd_workspace_size(C, T, n, nov)
    block, npairs = 2 * F * C * 16, -(-nseg // 2)
    ws = max(need, min(need + (npairs - 1) * block, wsg.CSD_WS_CAP))      # sigchain's default
    chunks = -(-npairs // (1 + (ws - need) // block))
    widths = [min(32, C - 32 * t) for t in range(-(-C // 32))]
    strips = C if pairs else sum(widths[i] + widths[j] for i in range(len(widths)) for j in range(i, len(widths)))
    cells = F * (C // 2) if pairs else F * C * C
    for name, fn, cell in (("csd", lambda: wsg.csd(xa, xb, 500.0, "hann", n, nov), 16),
                           ("coherence", lambda: wsg.coherence(xa, xb, 500.0, "hann", n, nov), 8)):
        # workspace and output allocation are inside the wrapper (torch's caching allocator), the window is cached
        t = med(fn)
        p1 = (nseg * n * C * 8, nseg * F * C * 16)
        p2 = nseg * F * strips * 16
        out = cells * cell * (3 if (name == "coherence" and not pairs) else 1)  # raw sums, then read and rewritten
        moved = p1[0] + p1[1] + p2 + out
        print(f"{name} {'pairs' if pairs else 'matrix'} T={T} C={C} nperseg={n} noverlap={nov}: {t[0]:.3f} ms "
              f"({t[1]:.3f}-{t[2]:.3f})  {nseg} segments in {chunks} chunk(s)  pass 1 reads {p1[0] / 1e6:.1f} MB writes "
              f"{p1[1] / 1e6:.1f} MB, pass 2 reads {p2 / 1e6:.1f} MB, output {out / 1e6:.1f} MB: moved "
              f"{moved / 1e6:.1f} MB = {moved / t[0] / 1e6:.1f} GB/s", flush=True)
    w = med(lambda: wsg.welch(x, 500.0, "hann", n, nov))
    line = f"  wc_welch_psd on the same input {w[0]:.3f} ms ({w[1]:.3f}-{w[2]:.3f})"
    if nseg * cells < 4e9:
        xh = x.cpu().numpy()
        t0 = time.perf_counter()
        host_loop(xh, n, nov, pairs)
        line += f"  numpy loop on the host {1e3 * (time.perf_counter() - t0):.1f} ms"
    print(line, flush=True)
    del x, xa, xb
    torch.cuda.empty_cache()

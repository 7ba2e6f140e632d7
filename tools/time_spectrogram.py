"""sigchain.spectrogram (wc_spectrogram) at the four shapes of docs/CHANGELOG.md, modes psd and
complex, Hann: HIP events, median of 5 after a warm-up, with the bytes the kernel moves (segment
reads nseg * nperseg * C * 8 and the output, S * F * C cells of 8 or 16 bytes) and the compulsory
ones (x once, the output once).  Beside it, for orientation only: sigchain.welch on the same input
(the same transforms, an output S times smaller).
python tools/time_spectrogram.py"""
import os
import sys

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
    """tools/time_welch_psd.py's signal."""
    g = torch.Generator(device="cuda").manual_seed(M)
    t = torch.arange(M, device="cuda", dtype=torch.float64)[:, None] * 0.002
    f = 2 + 10 * torch.rand(C, generator=g, device="cuda", dtype=torch.float64)
    return (0.2 + 0.05 * torch.cos(2 * np.pi * f * t) * (1 + 0.3 * torch.sin(0.6 * t))
            + 0.0005 * torch.randn((M, C), generator=g, device="cuda", dtype=torch.float64)).contiguous()


def main():
    for T, C, n, nov in ((300_000, 90, 1000, 500), (30_000, 90, 400, 200), (298, 5760, 256, 32),
                         (48_000, 1800, 4000, 2000)):
        x = sig(T, C)
        S, F = (T - n) // (n - nov) + 1, n // 2 + 1
        # output and workspace allocation are inside the wrappers (torch's caching allocator), the window is cached
        w = med(lambda: wsg.welch(x, 500.0, "hann", n, nov))
        for mode, cell in (("psd", 8), ("complex", 16)):
            t = med(lambda: wsg.spectrogram(x, 500.0, "hann", n, nov, mode=mode))
            out = S * F * C * cell
            moved, compulsory = S * n * C * 8 + out, T * C * 8 + out
            print(f"spectrogram {mode} T={T} C={C} nperseg={n} noverlap={nov}: {t[0]:.3f} ms ({t[1]:.3f}-{t[2]:.3f})  "
                  f"{S} segments x {F} bins  output {out / 1e6:.1f} MB  moved {moved / 1e6:.1f} MB = "
                  f"{moved / t[0] / 1e6:.1f} GB/s  compulsory {compulsory / 1e6:.1f} MB = "
                  f"{compulsory / t[0] / 1e6:.1f} GB/s  sigchain.welch {w[0]:.3f} ms ({w[1]:.3f}-{w[2]:.3f})", flush=True)
        del x
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()

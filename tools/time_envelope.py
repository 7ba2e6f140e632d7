"""wc_hilbert_envelope's dispatch table (direct against long at M = 256 .. 4096, C = 90 and 5760) and
the three stages of sigchain.envelope at 300,000 x 90 and 29,800 x 5,760 (docs/CHANGELOG.md): HIP
events, median of 5 after a warm-up.  python tools/time_envelope.py dispatch | stages"""
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
    g = torch.Generator(device="cuda").manual_seed(M)
    t = torch.arange(M, device="cuda", dtype=torch.float64)[:, None] * 0.002
    f = 2 + 10 * torch.rand(C, generator=g, device="cuda", dtype=torch.float64)
    return (torch.cos(2 * np.pi * f * t) * (1 + 0.3 * torch.sin(0.6 * t))
            + 0.01 * torch.randn((M, C), generator=g, device="cuda", dtype=torch.float64)).contiguous()


what = sys.argv[1]
if what == "dispatch":
    for C in (90, 5760):
        for M in (256, 512, 1024, 2048, 4096):
            x = sig(M, C)
            # workspace allocation is inside the wrapper for both methods (torch's caching allocator)
            d = med(lambda: wsg.hilbert_envelope(x, method=1))
            l = med(lambda: wsg.hilbert_envelope(x, method=2))
            print(f"dispatch M={M} C={C}: direct {d[0]:.3f} ms ({d[1]:.3f}-{d[2]:.3f})  "
                  f"long {l[0]:.3f} ms ({l[1]:.3f}-{l[2]:.3f})", flush=True)
else:
    for M, C in ((300_000, 90), (29_800, 5760)):
        x = sig(M, C)
        (bb, ba), (lb, la) = wsg.envelope_filters(0.002, 8.0, 13.0, 2.0)
        v = wsg.filtfilt(bb, ba, x)
        e = wsg.hilbert_envelope(v)
        t1 = med(lambda: wsg.filtfilt(bb, ba, x))
        t2 = med(lambda: wsg.hilbert_envelope(v))
        t3 = med(lambda: wsg.filtfilt(lb, la, e))
        t4 = med(lambda: wsg.envelope(x, fcut=2.0))
        print(f"stages M={M} C={C}: band-pass filtfilt(6) {t1[0]:.2f} ms  |hilbert| {t2[0]:.2f} ms  "
              f"low-pass filtfilt(3) {t3[0]:.2f} ms  envelope() {t4[0]:.2f} ms", flush=True)
        del x, v, e
        torch.cuda.empty_cache()

"""wc_phase_conn and sigchain.phase_connectivity at the three shapes of docs/CHANGELOG.md: HIP events,
median of 5 after a warm-up, with min-max.  wc_phase_conn alone (phase-only: plv and pli; all four
of its measures) on phasors and envelopes computed beforehand, then the whole
sigchain.phase_connectivity (Hilbert phasors, Hilbert envelopes, wc_phase_conn, corrcoef for aec).
Beside them, for orientation only: the two Hilbert calls' own time and, with --host, the numpy loop
of tests/conn_reference.py on the host where it finishes (up to 2e9 pair-samples).
python tools/time_connectivity.py [--host]"""
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from nremmodfc_amd import sigchain as wsg  # noqa: E402

HOST_MAX_PAIR_SAMPLES = 2e9


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


def fmt(t):
    return f"{t[0]:.3f} ms ({t[1]:.3f}-{t[2]:.3f})"


def sig(shape):
    """Amplitude-modulated carriers near 10 Hz at 500 Hz with a shared component and noise."""
    T = shape[0]
    g = torch.Generator(device="cuda").manual_seed(T)
    rest = shape[1:]
    t = torch.arange(T, device="cuda", dtype=torch.float64).view((T,) + (1,) * len(rest)) * 0.002
    f = 9.4 + 1.2 * torch.rand(rest, generator=g, device="cuda", dtype=torch.float64)
    p = 2 * np.pi * torch.rand(rest, generator=g, device="cuda", dtype=torch.float64)
    return ((1 + 0.4 * torch.sin(2 * np.pi * 0.7 * t + p)) * torch.cos(2 * np.pi * f * t + p)
            + 0.4 * torch.cos(2 * np.pi * 10.2 * t) + 0.2
            + 0.2 * torch.randn(shape, generator=g, device="cuda", dtype=torch.float64)).contiguous()


def main():
    host = "--host" in sys.argv
    for shape in ((300_000, 90), (48_000, 1000), (298, 64, 90)):
        x = sig(shape)
        T = shape[0]
        B, N = (1, shape[1]) if len(shape) == 2 else shape[1:]
        x2 = x.view(T, -1)
        ph = wsg.hilbert_phase(x2).view(tuple(shape) + (2,))
        amp = wsg.hilbert_envelope(x2).view(shape)
        pairs = B * N * (N - 1) // 2 * T
        t_hp = med(lambda: wsg.hilbert_phase(x2))
        t_he = med(lambda: wsg.hilbert_envelope(x2))
        # output and workspace allocation are inside the wrappers (torch's caching allocator)
        t_ph = med(lambda: wsg.phase_connectivity_from(ph, None, ("plv", "pli")))
        t_all = med(lambda: wsg.phase_connectivity_from(ph, amp, ("plv", "pli", "wpli", "aec_orth")))
        t_whole = med(lambda: wsg.phase_connectivity(x))
        line = (f"connectivity {' x '.join(map(str, shape))}: {pairs:.2e} pair-samples  wc_phase_conn plv+pli "
                f"{fmt(t_ph)} = {pairs / t_ph[0] / 1e6:.1f} G pair-samples/s  all four {fmt(t_all)}  "
                f"sigchain.phase_connectivity (five measures) {fmt(t_whole)}  hilbert_phase {fmt(t_hp)}  "
                f"hilbert_envelope {fmt(t_he)}")
        if host and pairs <= HOST_MAX_PAIR_SAMPLES:
            from tests import conn_reference as ref
            xh = x.cpu().numpy().reshape(T, B, N)
            t0 = time.perf_counter()
            for b in range(B):
                ref.connectivity(xh[:, b])
            line += f"  numpy loop on the host (with scipy's hilbert) {time.perf_counter() - t0:.1f} s"
        elif host:
            line += "  numpy loop on the host: not run (too long)"
        print(line, flush=True)
        del x, x2, ph, amp
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()

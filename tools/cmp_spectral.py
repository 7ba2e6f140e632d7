"""Bit-compare the spectral kernels (wc_welch_psd, wc_csd, wc_spectrogram, wc_hilbert) of two builds of
libwcsde.so on the same seeded inputs (one process per library: WCSDE_LIB_OVERRIDE selects it).
python tools/cmp_spectral.py save OUT.npz | cmp A.npz B.npz

The cases run every instantiation: one nperseg per Bluestein length L = 64 .. 8192 (a ragged column
group and several workgroups, seven segments -- the last rides alone -- and eight, detrend on and
off; welch, csd and coherence as matrix and as pairs, the spectrogram's four modes) and one M per
Hilbert length L = 2^15 .. 2^20, which covers every (L1, L2) split.  A result above 1 MiB is kept
as its SHA-256 digest."""
import hashlib
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

NPERSEG = [15, 64, 100, 200, 400, 1000, 2048, 4096]       # L = 64, 128, ..., 8192
HILBERT_M = [2048, 20000, 40000, 70000, 140000, 300000]   # L = 2^15 .. 2^20
DIGEST_ABOVE = 1 << 20


def save(out):
    import torch
    from nremmodfc_amd import sigchain as wsg
    from tests.test_welch_psd_gpu import make_signal
    res = {}

    def rec(key, t):
        a = np.ascontiguousarray(t.cpu().numpy())
        if a.nbytes > DIGEST_ABOVE:
            key, a = key + "_sha256", np.frombuffer(hashlib.sha256(a.tobytes()).digest(), dtype=np.uint8)
        res[key] = a

    for n in NPERSEG:
        nov = n // 2
        step = n - nov
        for C in (7, 8, 130):
            xs = torch.tensor(make_signal(n + 7 * step, 2 * C), device="cuda")
            for nseg in (7, 8):
                x2 = xs[:n + (nseg - 1) * step]
                x, y = x2[:, :C].contiguous(), x2[:, C:].contiguous()
                for det in ("constant", False):
                    tag = f"n{n}_C{C}_S{nseg}_{'det' if det else 'raw'}"
                    if C != 8:
                        rec(f"welch_{tag}", wsg.welch(x, 500.0, "hann", n, nov, det)[1])
                        for mode in wsg.SPEC_MODES:
                            rec(f"spec_{mode}_{tag}", wsg.spectrogram(x, 500.0, "hann", n, nov, det, mode=mode)[2])
                    if C != 130:
                        rec(f"csd_{tag}", wsg.csd(x, None, 500.0, "hann", n, nov, det)[1])
                        rec(f"coh_{tag}", wsg.coherence(x, None, 500.0, "hann", n, nov, det)[1])
                        rec(f"csd_pairs_{tag}", wsg.csd(x, y, 500.0, "hann", n, nov, det)[1])
                        rec(f"coh_pairs_{tag}", wsg.coherence(x, y, 500.0, "hann", n, nov, det)[1])
        print(f"nperseg={n}: {len(res)} arrays", flush=True)
    for M in HILBERT_M:
        x = torch.tensor(make_signal(M, 3), device="cuda")
        rec(f"hilbert_phase_M{M}", wsg.hilbert_phase_long(x))
        rec(f"hilbert_env_M{M}", wsg.hilbert_envelope(x, method=2))
        print(f"M={M}: {len(res)} arrays", flush=True)
    torch.cuda.synchronize()
    np.savez(out, **res)


def cmp(a, b):
    x, y = np.load(a), np.load(b)
    bad = sorted(set(x.files) ^ set(y.files))
    for k in bad:
        print(k, "MISSING in one file")
    for k in x.files:
        if k not in y.files:
            continue
        same = x[k].shape == y[k].shape and x[k].tobytes() == y[k].tobytes()
        if not same:
            d = "" if k.endswith("_sha256") or x[k].shape != y[k].shape else f" max|d| {np.nanmax(np.abs(x[k] - y[k])):.3e}"
            print(k, "DIFFER" + d)
            bad.append(k)
    print(f"{len(x.files)} arrays, {len(bad)} differ")
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    save(sys.argv[2]) if sys.argv[1] == "save" else cmp(sys.argv[2], sys.argv[3])

"""Welch PSD per column on the device (wc_welch_psd, sigchain.welch, utils.welch) against
scipy.signal.welch on the same fp64 array.

Bound, per column over every bin:  |sqrt(got) - sqrt(want)| <= 1e-12 * sqrt(max_f want): the
amplitude-domain form of the project's Bluestein bound (test_hilbert_long_gpu.py,
test_envelope_gpu.py: 1e-12 x scale).  dP = 2 |X| |dX|, and the mean over segments keeps it by the
triangle inequality.  Not a per-bin relative bound: single bins of SciPy's own result for this
signal fall to 1e-15 of the column's maximum.  Every case prints its measured maximum of
|sqrt(got) - sqrt(want)| / sqrt(max_f want) over the columns as a `TOL welch-psd-... dev=` line.

Column tiles: the kernel takes as many columns per pass as its workspace holds, so the default call
runs all C in one pass (C = 130 is 3 workgroups of 64 columns at nperseg = 15, 65 of 2 at 1000, 130
of 1 at 4096); the invariance tests add the minimum workspace (130 passes of one column) and one
that holds 37 columns (three full passes and a ragged one of 19).

Measured on MI355X (the deviation above; none of the printed cases above 3.0e-14):
  worst over noverlap and T per nperseg, C = 7:  2: 2.2e-16   3: 7.2e-15   5: 3.0e-14   8: 7.3e-15   15: 6.4e-15
    16: 4.3e-15   64: 4.6e-15   100: 2.6e-15   200: 3.8e-15   400: 8.8e-15   1000: 8.9e-15   1023: 8.7e-15   1024: 1.1e-14   1025: 6.5e-15
    2047: 1.1e-14   2048: 7.5e-15   2049: 1.2e-14   4000: 1.6e-14   4095: 2.3e-14   4096: 2.6e-14
  C = 1 / 90 / 130:  nperseg 15: 9.4e-16 / 6.5e-15 / 4.1e-15   1000: 1.5e-16 / 4.7e-15 / 5.0e-15
    4096: 1.9e-16 / 9.9e-15 / 1.0e-14
  detrend constant / False (density and spectrum alike):  15: 3.1e-15 / 2.1e-16   400: 7.2e-16 / 2.0e-16
    4096: 1.1e-14 / 1.7e-16  -- what deviation there is comes from the segment mean of the offset columns
    (0.2 under 0.05 of signal; at nperseg = 5 the detrended segment is 1e-3 of its mean), which numpy's
    pairwise sum and the kernel's tree round differently
  tukey 1.8e-15   array window 1.5e-15   SciPy's defaults 2.0e-15   clamped nperseg 2.5e-15
  cortex_run.py's calls 4.7e-15 (E_t), 2.3e-15 (EEG)   float32 input 3.8e-16   300,000 x 90: 9.4e-16
  against the sweep kernel's node-mean PSD 3.0e-16
"""
import functools
import warnings

import numpy as np
import pytest
import torch
from scipy import signal

from nremmodfc_amd import _lib, utils
from nremmodfc_amd import sigchain as wsg

pytestmark = pytest.mark.gpu

BOUND = 1e-12
NPERSEG = [2, 3, 5, 8, 15, 16, 64, 100, 200, 400, 1000, 1023, 1024, 1025, 2047, 2048, 2049, 4000, 4095, 4096]


def make_signal(M, C):
    """test_envelope_gpu.py's recipe: amplitude-modulated 2-12 Hz carriers at 500 Hz plus a little
    noise; even columns sit on a 0.2 offset (E-like: the detrend has work to do), odd columns
    rotate through every phase."""
    rng = np.random.default_rng(M)
    t = np.arange(M)[:, None] * 0.002
    f = rng.uniform(2, 12, C)
    p = rng.uniform(0, 2 * np.pi, C)
    g = rng.uniform(0.05, 0.2, C)
    x = (1 + 0.3 * np.sin(2 * np.pi * g * t)) * np.cos(2 * np.pi * f * t + p) + 0.01 * rng.standard_normal((M, C))
    x[:, ::2] = 0.2 + 0.05 * x[:, ::2]
    return np.ascontiguousarray(x)


@functools.lru_cache(maxsize=None)
def sig(M, C):
    """Computed once per shape, read only; shorter series are its leading rows."""
    x = make_signal(M, C)
    x.setflags(write=False)
    return x


def dev(x, cuda):
    return torch.tensor(np.ascontiguousarray(x), device=cuda)  # a copy: the shared cases are read only


def deviation(got, want):
    """max over columns of max_f |sqrt(got) - sqrt(want)| / sqrt(max_f want); [F][...] arrays."""
    got = np.asarray(got).reshape(got.shape[0], -1)
    want = np.asarray(want).reshape(want.shape[0], -1)
    assert got.shape == want.shape
    assert np.isfinite(got).all() and (got >= 0).all()
    return float((np.abs(np.sqrt(got) - np.sqrt(want)).max(axis=0) / np.sqrt(want.max(axis=0))).max())


def check(tag, got, want):
    d = deviation(got, want)
    print(f"TOL welch-psd-{tag} dev={d:.3e}")
    assert d <= BOUND
    return d


def overlaps(n):
    return sorted({n // 2, 0, 3 * n // 4} | ({n - 1} if n <= 16 else set()))


@pytest.mark.parametrize("n", NPERSEG)
def test_segment_lengths_overlaps_and_counts(cuda, n):
    """Every nperseg (the doubling rules at 2 / odd / even, both sides of each L = nextpow2(2 n - 1)
    step, the maximum, cortex_run.py's 1000 and 400) x noverlap (default n // 2, 0, 3 n // 4, and hop 1
    for n <= 16) x T (one segment exactly, one with an ignored tail, two, seven); C = 7."""
    C, worst = 7, 0.0
    for nov in overlaps(n):
        step = n - nov
        x = sig(n + 6 * n, C)  # covers n + 6 step for every overlap
        for T in sorted({n, n + step - 1, n + step, n + 6 * step}):
            fw, want = signal.welch(x[:T], 500.0, "hann", n, nov, axis=0)
            fg, got = wsg.welch(dev(x[:T], cuda), 500.0, "hann", n, nov)
            assert got.is_cuda and got.shape == (n // 2 + 1, C)
            np.testing.assert_array_equal(fg, fw)
            worst = max(worst, check(f"n{n}-nov{nov}-T{T}", got.cpu().numpy(), want))
    print(f"TOL welch-psd-n{n}-worst dev={worst:.3e}")


@pytest.mark.parametrize("n", [15, 1000, 4096])
@pytest.mark.parametrize("C", [1, 90, 130])
def test_column_counts(cuda, n, C):
    """A single column, cortex_run.py's width, and more than one workgroup of columns at every L."""
    T = n + 6 * (n - n // 2)
    x = sig(T, C)
    want = signal.welch(x, 500.0, nperseg=n, axis=0)[1]
    got = wsg.welch(dev(x, cuda), 500.0, nperseg=n)[1]
    check(f"C{C}-n{n}", got.cpu().numpy(), want)


@pytest.mark.parametrize("scaling", ["density", "spectrum"])
@pytest.mark.parametrize("detrend", ["constant", False])
@pytest.mark.parametrize("n", [15, 400, 4096])
def test_detrend_and_scaling(cuda, n, detrend, scaling):
    T = n + 6 * (n - n // 2) + 3
    x = sig(T, 7)
    fw, want = signal.welch(x, 500.0, nperseg=n, detrend=detrend, scaling=scaling, axis=0)
    fg, got = wsg.welch(dev(x, cuda), 500.0, nperseg=n, detrend=detrend, scaling=scaling)
    np.testing.assert_array_equal(fg, fw)
    check(f"n{n}-detrend-{detrend}-{scaling}", got.cpu().numpy(), want)


def test_other_windows(cuda):
    """A parametrised SciPy window, an explicit array window (nperseg from its length), and SciPy's
    defaults (nperseg = 256, noverlap = 128)."""
    n, T = 400, 400 + 6 * 200
    x = sig(T, 7)
    xt = dev(x, cuda)
    fw, want = signal.welch(x, 500.0, ("tukey", 0.25), n, axis=0)
    fg, got = wsg.welch(xt, 500.0, ("tukey", 0.25), n)
    np.testing.assert_array_equal(fg, fw)
    check("n400-tukey", got.cpu().numpy(), want)
    w = np.blackman(n) + 0.1
    fw, want = signal.welch(x, 500.0, w, axis=0)
    fg, got = wsg.welch(xt, 500.0, w)
    np.testing.assert_array_equal(fg, fw)
    check("n400-array-window", got.cpu().numpy(), want)
    check("n400-array-window-nperseg", wsg.welch(xt, 500.0, w, nperseg=n)[1].cpu().numpy(), want)
    fw, want = signal.welch(x, axis=0)
    fg, got = wsg.welch(xt)
    np.testing.assert_array_equal(fg, fw)
    check("defaults", got.cpu().numpy(), want)
    with pytest.raises(ValueError, match="longer"):
        wsg.welch(xt[:300], 500.0, w)
    with pytest.raises(ValueError, match="noverlap"):
        wsg.welch(xt, 500.0, "hann", n, n)
    with pytest.raises(NotImplementedError, match="detrend"):
        wsg.welch(xt, 500.0, detrend="linear")
    with pytest.raises(_lib.WCSDEError, match="4096"):
        wsg.welch(dev(sig(5000, 2), cuda), 500.0, nperseg=4097)


@pytest.mark.parametrize("n", [1000, 4095])
def test_invariance(cuda, n):
    """Bit-equal: a column of the 130-column call and a C = 1 call on that column alone; the minimum
    workspace (one column per pass), one holding 37 columns (ragged last pass) and the default."""
    C = 130
    step = n - n // 2
    T = n + 6 * step
    x = sig(T, C)
    xt = dev(x, cuda)
    full = wsg.welch(xt, 500.0, nperseg=n)[1]
    check(f"invariance-n{n}", full.cpu().numpy(), signal.welch(x, 500.0, nperseg=n, axis=0)[1])
    for c in (0, 64, 129):
        one = wsg.welch(dev(x[:, c:c + 1], cuda), 500.0, nperseg=n)[1]
        np.testing.assert_array_equal(one.cpu().numpy()[:, 0], full.cpu().numpy()[:, c])
    need = _lib.lib().wc_welch_psd_workspace_size(C, T, n, n // 2)
    per_col = 4 * (n // 2 + 1) * 8  # seven segments: four blocks (three pairs and one) of F doubles
    assert need == _lib.lib().wc_welch_psd_workspace_size(1, T, n, n // 2)
    for ws_bytes in (need, need + 36 * per_col):
        got = wsg.welch(xt, 500.0, nperseg=n, ws_bytes=ws_bytes)[1]
        np.testing.assert_array_equal(got.cpu().numpy(), full.cpu().numpy())


def test_against_the_sweep_kernel(cuda):
    """The sweep's fixed Welch (nperseg = 4000, node-summed, node-major ring) on the same data."""
    T, B, N = 8000, 2, 5
    E = dev(sig(T, B * N), cuda).reshape(T, B, N)
    freqs, psd = wsg.welch(E, fs=500.0, nperseg=4000)
    assert psd.shape == (2001, B, N)
    mine = psd.mean(dim=2).cpu().numpy()                   # [F][B]
    peak, theirs = wsg.welch_peak(E, 500.0, want_psd=True)  # [B], [B][F]
    check("sweep-kernel", mine, theirs.cpu().numpy().T)
    for b in range(B):
        assert freqs[np.argmax(mine[:, b])] == peak[b].item()


def test_cortex_run_calls(cuda):
    """cortex_run.py:203-209 as written, utils.welch for signal.welch: [5000][90] at fs = 500."""
    E_t = sig(5000, 90)
    sampling_rate = 1000 / 2  # a float, as cortex_run.py's: nperseg = 1000.0
    freqs, PSDs = utils.welch(E_t, fs=sampling_rate, window='hann', nperseg=sampling_rate * 2,
                              noverlap=sampling_rate * 1, axis=0)
    PSD = np.mean(PSDs, axis=1)
    maxfreq = freqs[np.argmax(PSD)]
    fw, want = signal.welch(E_t, fs=sampling_rate, window='hann', nperseg=sampling_rate * 2,
                            noverlap=sampling_rate * 1, axis=0)
    assert isinstance(PSDs, np.ndarray) and PSDs.shape == (501, 90)
    np.testing.assert_array_equal(freqs, fw)
    check("cortex-run-E_t", PSDs, want)
    assert maxfreq == fw[np.argmax(np.mean(want, axis=1))]

    downsamp = 10  # line 203: fs, window, nperseg, noverlap positionally
    EEG = E_t
    freqs, PSDs = utils.welch(EEG, 1000 // downsamp, 'hann', 4000 // downsamp, 2000 // downsamp, axis=0,
                              scaling='density')
    fw, want = signal.welch(EEG, 1000 // downsamp, 'hann', 4000 // downsamp, 2000 // downsamp, axis=0,
                            scaling='density')
    assert PSDs.shape == (201, 90)
    np.testing.assert_array_equal(freqs, fw)
    check("cortex-run-EEG", PSDs, want)
    assert freqs[np.argmax(np.mean(PSDs, axis=1))] == fw[np.argmax(np.mean(want, axis=1))]


def test_facade_axes_shapes_and_clamp(cuda):
    x = sig(5000, 90)
    f0, p0 = utils.welch(x, 500.0, nperseg=1000, axis=0)
    f1, p1 = utils.welch(np.ascontiguousarray(x.T), 500.0, nperseg=1000)     # axis = -1
    np.testing.assert_array_equal(f0, f1)
    np.testing.assert_array_equal(p1, p0.T)
    f2, p2 = utils.welch(x[:, 3], 500.0, nperseg=1000)                      # one series
    assert p2.shape == (501,)
    np.testing.assert_array_equal(p2, p0[:, 3])
    f3, p3 = utils.welch(x.astype(np.float32), 500.0, nperseg=1000, nfft=1000, axis=0)  # any real dtype
    check("facade-float32-input", p3, signal.welch(x.astype(np.float32).astype(np.float64), 500.0, nperseg=1000,
                                                   axis=0)[1])
    # a named window longer than the series: SciPy's warning and SciPy's clamped result
    short = x[:200, :7]
    with pytest.warns(UserWarning, match="nperseg = 256 is greater than input length"):
        fg, got = utils.welch(short, 500.0, axis=0)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        fw, want = signal.welch(short, 500.0, axis=0)
    np.testing.assert_array_equal(fg, fw)
    check("clamped-nperseg", got, want)
    # [T][B][N] through sigchain.welch
    xt = dev(x[:, :6], cuda)
    fq, p3d = wsg.welch(xt.reshape(5000, 2, 3), 500.0, nperseg=400)
    assert p3d.shape == (201, 2, 3)
    assert torch.equal(p3d.reshape(201, 6), wsg.welch(xt, 500.0, nperseg=400)[1])


def test_workload_shape(cuda):
    """cortex_run.py's E_t, 300,000 x 90 with nperseg = 1000: 599 segments in 16 blocks, the only
    shape at which the segment blocking and the 64-bit sample index have work to do."""
    T, C = 300_000, 90
    x = sig(T, C)
    fw, want = signal.welch(x, 500.0, 'hann', 1000, 500, axis=0)
    fg, got = utils.welch(x, 500.0, 'hann', 1000, 500, axis=0)
    assert got.shape == (501, C)
    np.testing.assert_array_equal(fg, fw)
    check("workload-300000x90-n1000", got, want)
    assert fg[np.argmax(got.mean(axis=1))] == fw[np.argmax(want.mean(axis=1))]

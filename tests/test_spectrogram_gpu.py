"""Spectrograms per column on the device (wc_spectrogram, sigchain.spectrogram, utils.spectrogram)
against scipy.signal.spectrogram(..., axis=0) on the same fp64 array (test_welch_psd_gpu.py's signal).

Bounds: the project's 1e-12 x scale Bluestein bound (test_welch_psd_gpu.py, test_envelope_gpu.py),
per column, the maximum taken over all bins and segments of that column:
  psd                 |sqrt(got) - sqrt(want)| <= 1e-12 sqrt(max want)
  complex, magnitude  |got - want| <= 1e-12 max |want|
  angle               |want_complex| |exp(i got) - exp(i want)| <= 1e-12 max |want_complex|, -pi <= got <= pi
  phase (utils only)  the angle bound on (got, want), and every step along the segments within [-pi, pi]
An angle's error is the value's error over its modulus, so the angle bound is the complex one again;
it does not see SciPy's choice between +pi and -pi, nor a bin without content, nor the multiples of
2 pi by which two unwrappings differ.  Every case prints the measured deviation over its bound's scale
as a `TOL spectrogram-... dev=` line.

Measured on MI355X (the deviations above; none of the printed cases above 4.8e-14, a twentieth of
the bound; per case in docs/CHANGELOG.md):
  worst over noverlap and T per nperseg, C = 7, psd / complex:  2: 1.2e-16 / 7.1e-17   3: 1.4e-14 / 2.0e-14
    5: 3.4e-14 / 4.8e-14   8: 9.5e-15 / 1.3e-14   15: 1.9e-14 / 2.7e-14   16: 1.5e-14 / 2.2e-14   64: 5.5e-15 / 7.7e-15
    100: 5.5e-15 / 7.8e-15   200: 3.8e-15 / 5.4e-15
    400: 8.8e-15 / 1.2e-14   1000: 1.1e-14 / 1.6e-14   1023: 9.4e-15 / 1.3e-14   1024: 1.2e-14 / 1.7e-14
    1025: 1.0e-14 / 1.4e-14   2047: 1.6e-14 / 2.3e-14   2048: 1.4e-14 / 2.0e-14   2049: 1.6e-14 / 2.3e-14
    4000: 2.4e-14 / 3.4e-14   4095: 2.3e-14 / 3.3e-14   4096: 2.6e-14 / 3.7e-14
  C = 1 / 90 / 130, complex:  nperseg 15: 3.5e-15 / 2.0e-14 / 2.0e-14   1000: 2.0e-16 / 1.8e-14 / 1.9e-14
    4096: 1.2e-15 / 4.7e-14 / 4.1e-14
  detrend constant, psd / complex / magnitude / angle (density and spectrum alike):  15: 1.2e-14 / 1.7e-14 /
    1.7e-14 / 8.5e-15   400: 5.5e-15 / 7.7e-15 / 7.7e-15 / 2.3e-15   4096: 2.5e-14 / 3.6e-14 / 3.6e-14 / 7.0e-15;
    detrend False: 2.1e-16 .. 4.5e-16 in every mode -- as in the Welch tests, what deviation there is comes
    from the segment mean of the offset columns, which numpy's pairwise sum and the kernel's tree round
    differently; a single segment is not averaged with its neighbours, hence figures above welch's
  [T][B][N] <= 5.4e-15   SciPy's defaults <= 5.2e-15   array window <= 6.2e-15   clamped nperseg 2.7e-15
  69,999 segments 3.1e-16   mean over segments against sigchain.welch 1.3e-16 / 1.6e-16 / 2.7e-16
  utils.spectrogram <= 7.7e-15 (phase 2.5e-15 .. 3.4e-15, its largest step along the segments exactly pi);
    cortex_run.py's arguments, 6,000 x 90: 1.2e-14 / 1.6e-14 / 1.6e-14 / 8.2e-15, phase 8.2e-15
"""
import warnings

import numpy as np
import pytest
import torch
from scipy import signal

from nremmodfc_amd import _lib, utils
from nremmodfc_amd import sigchain as wsg
from tests.test_welch_psd_gpu import NPERSEG, dev, overlaps, sig
from tests.test_welch_psd_gpu import deviation as welch_deviation

pytestmark = pytest.mark.gpu

BOUND = 1e-12
DEVICE_MODES = ("psd", "complex", "magnitude", "angle")


def canon(a, faxis=0):
    """[F][columns][S] from an array with the frequencies at faxis and the segments last."""
    a = np.moveaxis(np.asarray(a), faxis, 0)
    return a.reshape(a.shape[0], -1, a.shape[-1])


def deviation(mode, got, want, want_complex=None):
    """The mode's deviation over its scale, maximum over the columns; [F][C][S] arrays."""
    assert got.shape == want.shape and np.isfinite(got).all()
    if mode == "psd":
        assert (got >= 0).all()
        err, scale = np.abs(np.sqrt(got) - np.sqrt(want)), np.sqrt(want.max(axis=(0, 2)))
    elif mode in ("complex", "magnitude"):
        err, scale = np.abs(got - want), np.abs(want).max(axis=(0, 2))
    else:
        assert want_complex.shape == got.shape
        mod = np.abs(want_complex)
        err, scale = mod * np.abs(np.exp(1j * got) - np.exp(1j * want)), mod.max(axis=(0, 2))
    return float((err.max(axis=(0, 2)) / scale).max())


def check(tag, mode, got, want, want_complex=None):
    if mode == "angle":
        assert (got >= -np.pi).all() and (got <= np.pi).all()
    d = deviation(mode, got, want, want_complex)
    print(f"TOL spectrogram-{mode}-{tag} dev={d:.3e}")
    assert d <= BOUND
    return d


def reference(x, mode, *args, **kw):
    """(f, t, Sxx, complex Sxx or None) of SciPy along axis 0: [F][C][S]."""
    f, t, s = signal.spectrogram(x, *args, axis=0, mode=mode, **kw)
    c = signal.spectrogram(x, *args, axis=0, mode="complex", **kw)[2] if mode in ("angle", "phase") else None
    return f, t, s, c


def against_scipy(tag, x, cuda, modes, *args, xt=None, **kw):
    """sigchain.spectrogram(x on the device, *args, **kw) against SciPy, every mode of modes."""
    xt = dev(x, cuda) if xt is None else xt
    worst = 0.0
    for mode in modes:
        fw, tw, want, wc = reference(x.reshape(x.shape[0], -1), mode, *args, **kw)
        fg, tg, got = wsg.spectrogram(xt, *args, mode=mode, **kw)
        assert got.is_cuda and got.shape == (len(fw),) + tuple(x.shape[1:]) + (len(tw),)
        assert got.dtype == (torch.complex128 if mode == "complex" else torch.float64)
        np.testing.assert_array_equal(fg, fw)
        np.testing.assert_array_equal(tg, tw)
        worst = max(worst, check(tag, mode, canon(got.cpu().numpy()), want, wc))
    return worst


@pytest.mark.parametrize("n", NPERSEG)
def test_segment_lengths_overlaps_and_counts(cuda, n):
    """Every nperseg of the Welch test (the doubling rules at 2 / odd / even, both sides of each
    L = nextpow2(2 n - 1) step, the maximum) x noverlap (n // 2, 0, 3 n // 4, and hop 1 for n <= 16)
    x T (one segment exactly, one with an ignored tail, two, and seven: an odd last segment rides its
    transform alone); C = 7."""
    C, worst = 7, 0.0
    for nov in overlaps(n):
        step = n - nov
        x = sig(n + 6 * n, C)  # covers n + 6 step for every overlap
        for T in sorted({n, n + step - 1, n + step, n + 6 * step}):
            worst = max(worst, against_scipy(f"n{n}-nov{nov}-T{T}", x[:T], cuda, ("psd", "complex"), 500.0, "hann", n,
                                             nov))
    print(f"TOL spectrogram-n{n}-worst dev={worst:.3e}")


@pytest.mark.parametrize("n", [15, 1000, 4096])
@pytest.mark.parametrize("C", [1, 90, 130])
def test_column_counts(cuda, n, C):
    """A single column, cortex_run.py's width, and more than one workgroup of columns at every L
    (C = 130 is 3 workgroups of 64 columns at nperseg = 15, 65 of 2 at 1000, 130 of 1 at 4096)."""
    T = n + 6 * (n - n // 2)
    against_scipy(f"C{C}-n{n}", sig(T, C), cuda, ("psd", "complex"), 500.0, "hann", n, n // 2)


@pytest.mark.parametrize("scaling", ["density", "spectrum"])
@pytest.mark.parametrize("detrend", ["constant", False])
@pytest.mark.parametrize("n", [15, 400, 4096])
def test_detrend_scaling_and_modes(cuda, n, detrend, scaling):
    T = n + 6 * (n - n // 2) + 3
    against_scipy(f"n{n}-detrend-{detrend}-{scaling}", sig(T, 7), cuda, DEVICE_MODES, 500.0, "hann", n, n // 2,
                  detrend=detrend, scaling=scaling)


def test_time_batch_node_input(cuda):
    """[T][B][N]: Sxx [F][B][N][S], the view of the same buffer as the [T][B * N] call's."""
    x = sig(2000, 6)
    xt = dev(x, cuda)
    against_scipy("TBN", x.reshape(2000, 2, 3), cuda, DEVICE_MODES, 500.0, "hann", 400, 200)
    s3 = wsg.spectrogram(xt.reshape(2000, 2, 3), 500.0, "hann", 400, 200)[2]
    assert s3.shape == (201, 2, 3, 9)
    assert torch.equal(s3.reshape(201, 6, 9), wsg.spectrogram(xt, 500.0, "hann", 400, 200)[2])


def test_windows_and_defaults(cuda):
    """SciPy's defaults (Tukey 0.25, nperseg 256, noverlap 32), an array window (nperseg from its
    length, noverlap an eighth of it), a named window clamped to a short series with SciPy's warning
    (noverlap an eighth of the clamped length), and the refusals."""
    x = sig(2000, 7)
    xt = dev(x, cuda)
    against_scipy("defaults", x, cuda, DEVICE_MODES, xt=xt)
    assert wsg.spectrogram(xt)[2].shape == (129, 7, (2000 - 256) // 224 + 1)
    w = np.blackman(400) + 0.1
    against_scipy("array-window", x, cuda, DEVICE_MODES, 500.0, w, xt=xt)
    against_scipy("array-window-nperseg", x, cuda, ("psd",), 500.0, w, 400, xt=xt)
    assert wsg.spectrogram(xt, 500.0, w)[2].shape == (201, 7, (2000 - 400) // 350 + 1)
    short = x[:200]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        fw, tw, want = signal.spectrogram(short, 500.0, axis=0)
    with pytest.warns(UserWarning, match="nperseg = 256 is greater than input length"):
        fg, tg, got = wsg.spectrogram(dev(short, cuda), 500.0)
    np.testing.assert_array_equal(fg, fw)
    np.testing.assert_array_equal(tg, tw)
    assert got.shape == (101, 7, 1)
    check("clamped-nperseg", "psd", got.cpu().numpy(), want)
    with pytest.raises(ValueError, match="noverlap"):
        wsg.spectrogram(xt, 500.0, "hann", 400, 400)
    with pytest.raises(ValueError, match="noverlap"):
        wsg.spectrogram(xt, 500.0, "hann", 400, 401)
    with pytest.raises(ValueError, match="longer"):
        wsg.spectrogram(xt[:300], 500.0, w)
    with pytest.raises(NotImplementedError, match="detrend"):
        wsg.spectrogram(xt, 500.0, detrend="linear")
    with pytest.raises(NotImplementedError, match="phase"):
        wsg.spectrogram(xt, 500.0, mode="phase")
    with pytest.raises(ValueError, match="unknown value for mode"):
        wsg.spectrogram(xt, 500.0, mode="stft")
    with pytest.raises(_lib.WCSDEError, match="4096"):
        wsg.spectrogram(dev(sig(5000, 2), cuda), 500.0, nperseg=4097)


def test_many_segments(cuda):
    """69,999 segments of two samples: 35,000 segment pairs, more than one launch holds (32,768), so
    the second launch's first segment and the odd last one are in it.  Every segment is compared."""
    x = sig(70_000, 3)
    w = np.array([0.5, 1.0])
    for mode in ("psd", "complex"):
        fw, tw, want, _ = reference(x, mode, 500.0, w, 2, 1)
        fg, tg, got = wsg.spectrogram(dev(x, cuda), 500.0, w, 2, 1, mode=mode)
        assert got.shape == (2, 3, 69_999)
        np.testing.assert_array_equal(tg, tw)
        got = got.cpu().numpy()
        check("69999-segments", mode, got, want)
        for lo, hi in ((0, 65_536), (65_536, 69_999)):  # each launch's share against the bound of its own maximum
            check(f"69999-segments-{lo}-{hi}", mode, got[:, :, lo:hi], want[:, :, lo:hi])


@pytest.mark.parametrize("n", [1000, 4095])
def test_invariance(cuda, n):
    """Bit-equal: a column's slab in the 130-column call and in a C = 1 call on that column alone, and
    two runs of the same call."""
    C = 130
    T = n + 6 * (n - n // 2)
    x = sig(T, C)
    xt = dev(x, cuda)
    for mode in DEVICE_MODES:
        full = wsg.spectrogram(xt, 500.0, "hann", n, n // 2, mode=mode)[2]
        assert torch.equal(full, wsg.spectrogram(xt, 500.0, "hann", n, n // 2, mode=mode)[2])
        for c in (0, 1, 64, 129):
            one = wsg.spectrogram(dev(x[:, c:c + 1], cuda), 500.0, "hann", n, n // 2, mode=mode)[2]
            assert torch.equal(one[:, 0], full[:, c]), (mode, c)


@pytest.mark.parametrize("n", [15, 16, 1000, 4095, 4096])
def test_exact_zeros(cuda, n):
    """An all-zero column gives exactly 0 as psd, magnitude and angle (its neighbours do not); the
    complex spectrum's imaginary part is exactly 0 at bin 0 and, for an even nperseg, at nperseg / 2."""
    T = n + 6 * (n - n // 2)
    x = np.array(sig(T, 5))
    x[:, 2] = 0.0
    xt = dev(x, cuda)
    for detrend in ("constant", False):
        for mode in ("psd", "magnitude", "angle"):
            got = wsg.spectrogram(xt, 500.0, "hann", n, n // 2, detrend=detrend, mode=mode)[2]
            assert (got[:, 2] == 0).all(), (mode, detrend)
            assert (got[:, 1] != 0).any() and (got[:, 3] != 0).any()
        got = wsg.spectrogram(xt, 500.0, "hann", n, n // 2, detrend=detrend, mode="complex")[2]
        assert (got[:, 2] == 0).all()
        assert (got[0].imag == 0).all() and (got[0].real != 0).any()
        if n % 2 == 0:
            assert (got[n // 2].imag == 0).all() and (got[n // 2].real != 0).any()
        assert (got[1].imag != 0).any()


@pytest.mark.parametrize("n", [15, 1000, 4096])
def test_mean_over_segments_is_welch(cuda, n):
    """The parent's wc_welch_psd on the same input: the welch tests' deviation of the mean over the
    segments of the psd mode, within their bound."""
    T = n + 6 * (n - n // 2)
    xt = dev(sig(T, 7), cuda)
    fw, want = wsg.welch(xt, 500.0, "hann", n, n // 2)
    fg, tg, got = wsg.spectrogram(xt, 500.0, "hann", n, n // 2)
    np.testing.assert_array_equal(fg, fw)
    d = welch_deviation(got.mean(dim=-1).cpu().numpy(), want.cpu().numpy())
    print(f"TOL spectrogram-mean-vs-welch-n{n} dev={d:.3e}")
    assert d <= BOUND


def facade(tag, x, *args, faxis, modes=("psd", "complex", "magnitude", "angle", "phase"), **kw):
    """utils.spectrogram against scipy.signal.spectrogram with the same arguments, numpy to numpy."""
    for mode in modes:
        fw, tw, want = signal.spectrogram(x, *args, mode=mode, **kw)
        fg, tg, got = utils.spectrogram(x, *args, mode=mode, **kw)
        assert isinstance(got, np.ndarray) and got.shape == want.shape
        assert got.dtype == want.dtype
        np.testing.assert_array_equal(fg, fw)
        np.testing.assert_array_equal(tg, tw)
        wc = canon(signal.spectrogram(x, *args, mode="complex", **kw)[2], faxis) if mode in ("angle", "phase") else None
        g = canon(got, faxis)
        if mode == "phase":
            # an unwrapped angle: the angle bound is periodic; along the segments no step leaves [-pi, pi]
            d = deviation("phase", g, canon(want, faxis), wc)
            step = np.abs(np.diff(g, axis=-1)).max() if g.shape[-1] > 1 else 0.0
            print(f"TOL spectrogram-phase-{tag} dev={d:.3e} max-step-minus-pi={step - np.pi:.3e}")
            assert d <= BOUND
            assert step <= np.pi
        else:
            check(tag, mode, g, canon(want, faxis), wc)


def test_facade_axes_and_shapes(cuda):
    x = sig(3000, 6)
    facade("axis0", x, 500.0, "hann", 400, 200, faxis=0, axis=0)
    xT = np.ascontiguousarray(x.T)
    facade("axis-1", xT, 500.0, "hann", 400, 200, faxis=1)                    # SciPy's default axis, (C, T)
    np.testing.assert_array_equal(utils.spectrogram(xT, 500.0, "hann", 400, 200)[2],
                                  np.moveaxis(utils.spectrogram(x, 500.0, "hann", 400, 200, axis=0)[2], 0, 1))
    f1, t1, s1 = utils.spectrogram(x[:, 3], 500.0, "hann", 400, 200)          # one series
    assert s1.shape == (201, 14)
    facade("1-D", np.ascontiguousarray(x[:, 3]), 500.0, "hann", 400, 200, faxis=0)
    x3 = np.ascontiguousarray(x.reshape(3000, 2, 3).transpose(1, 0, 2))       # (2, T, 3)
    facade("3-D-axis1", x3, 500.0, "hann", 400, 200, faxis=1, axis=1)
    facade("3-D-axis-2", x3, 500.0, "hann", 400, 200, faxis=1, axis=-2, modes=("psd", "phase"))
    assert utils.spectrogram(x3, 500.0, "hann", 400, 200, axis=1)[2].shape == (2, 201, 3, 14)
    facade("defaults", xT, faxis=1)
    # any real dtype is widened to fp64 (SciPy would stay in float32: the reference is its fp64 result)
    x32 = x.astype(np.float32)
    for mode in ("psd", "complex"):
        fw, tw, want = signal.spectrogram(x32.astype(np.float64), 500.0, "hann", 400, 200, axis=0, mode=mode)
        fg, tg, got = utils.spectrogram(x32, 500.0, "hann", 400, 200, nfft=400, axis=0, mode=mode)
        np.testing.assert_array_equal(tg, tw)
        check("float32-input", mode, got, want)


def test_cortex_run_arguments(cuda):
    """cortex_run.py:203-209's Welch arguments as a spectrogram: an E_t-like [6000][90] at fs = 500,
    Hann, nperseg = 1000 and noverlap = 500.  As integers: welch takes cortex_run.py's floats, but
    SciPy's spectrogram hands nperseg to get_window before any int(), which refuses a float."""
    E_t = sig(6000, 90)
    sampling_rate = 1000 / 2
    nperseg, noverlap = int(sampling_rate * 2), int(sampling_rate * 1)
    facade("cortex-run-E_t", E_t, faxis=0, fs=sampling_rate, window='hann', nperseg=nperseg, noverlap=noverlap,
           axis=0)
    f, t, Sxx = utils.spectrogram(E_t, fs=sampling_rate, window='hann', nperseg=nperseg, noverlap=noverlap, axis=0)
    assert Sxx.shape == (501, 90, 11)
    np.testing.assert_array_equal(t, 1.0 + np.arange(11))  # the segments' centres, every second

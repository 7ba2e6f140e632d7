"""wc_csd validates every argument before any device work, wc_csd_workspace_size returns 0 exactly
for the shapes the call rejects and does not depend on the mode, utils.csd / coherence refuse what
the device does not compute before they touch it (no GPU: the pointers are fake), and the host
reference of test_csd_gpu.py (tests/csd_reference.py) is scipy.signal.csd / coherence in broadcast
form to 1e-14 in the GPU tests' scaled units."""
import ctypes

import numpy as np
import pytest
from scipy import signal

from tests import csd_reference as ref

X, WIN, OUT, WS = (ctypes.c_void_p(v) for v in (1 << 30, 1 << 20, 1 << 32, 1 << 24))
BIG = 1 << 40
MATRIX, COHERENCE, PAIRS, PAIR_COHERENCE = 0, 1, 2, 3


def call(L, C=8, T=298, x=X, nperseg=64, noverlap=32, window=WIN, detrend=1, scale=1.0, mode=MATRIX, out=OUT, ws=WS,
         nbytes=BIG):
    return L.wc_csd(C, T, x, nperseg, noverlap, window, detrend, scale, mode, out, ws, nbytes, None)


def test_csd_validates_without_device_work():
    from nremmodfc_amd import _lib
    L = _lib.lib()
    for mode in (MATRIX, COHERENCE, PAIRS, PAIR_COHERENCE):
        assert call(L, C=0, mode=mode) == -1
        assert call(L, C=-4, mode=mode) == -1
        assert call(L, nperseg=1, noverlap=0, mode=mode) == -1
        assert call(L, nperseg=0, noverlap=0, mode=mode) == -1
        assert call(L, noverlap=-1, mode=mode) == -1
        assert call(L, noverlap=64, mode=mode) == -1                    # noverlap == nperseg
        assert call(L, T=63, mode=mode) == -1                           # T < nperseg
        assert call(L, x=None, mode=mode) == -1
        assert call(L, window=None, mode=mode) == -1
        assert call(L, out=None, mode=mode) == -1
        assert call(L, out=X, mode=mode) == -1                          # out aliasing x
        assert b"alias" in L.wc_last_error()
        assert call(L, out=ctypes.c_void_p((1 << 30) + 8 * 8 * 100), mode=mode) == -1   # out inside x [298][8]
        assert call(L, detrend=2, mode=mode) == -1
        for bad in (0.0, -1.0, float("inf"), float("nan")):
            assert call(L, scale=bad, mode=mode) == -1
        assert call(L, x=ctypes.c_void_p((1 << 30) + 4), mode=mode) == -1     # 8-byte alignment of x, window, out
        assert call(L, window=ctypes.c_void_p((1 << 20) + 4), mode=mode) == -1
        assert call(L, out=ctypes.c_void_p((1 << 32) + 4), mode=mode) == -1
        assert call(L, ws=ctypes.c_void_p((1 << 24) + 8), mode=mode) == -1    # 16-byte alignment of the workspace
        assert call(L, T=10000, nperseg=4097, noverlap=0, mode=mode) == -2
        assert b"4096" in L.wc_last_error()
        assert call(L, ws=None, nbytes=0, mode=mode) == -3
        assert call(L, ws=None, mode=mode) == -3
        assert call(L, nbytes=0, mode=mode) == -3
        assert b"workspace" in L.wc_last_error()
    # the output of the matrix modes ends behind x when it starts in front of it: F C C cells
    before = ctypes.c_void_p((1 << 30) - 33 * 8 * 8 * 8 + 8)
    assert call(L, out=before, mode=COHERENCE, nbytes=0) == -1
    assert b"alias" in L.wc_last_error()
    assert call(L, out=before, mode=PAIR_COHERENCE, nbytes=0) == -3     # [33][4] doubles end before x: on to the workspace
    for mode in (-1, 4, 17):
        assert call(L, mode=mode) == -1
        assert b"mode" in L.wc_last_error()
    for mode in (PAIRS, PAIR_COHERENCE):
        assert call(L, C=7, mode=mode) == -1                            # odd C in a pair mode
        assert b"even" in L.wc_last_error()
        assert call(L, C=5760, nbytes=0, mode=mode) == -3               # wide is fine there
    for mode in (MATRIX, COHERENCE):
        assert call(L, C=7, nbytes=0, mode=mode) == -3
        assert call(L, C=1024, nbytes=0, mode=mode) == -3
        assert call(L, C=1025, mode=mode) == -2
        assert b"1024" in L.wc_last_error()


def test_csd_workspace_size():
    from nremmodfc_amd import _lib
    L = _lib.lib()
    size = L.wc_csd_workspace_size
    for C, T, n, nov in ((0, 298, 64, 32), (-1, 298, 64, 32), (8, 298, 1, 0), (8, 298, 0, 0), (8, 298, 64, -1),
                         (8, 298, 64, 64), (8, 298, 64, 65), (8, 63, 64, 32), (8, 10000, 4097, 0),
                         (8, 100000, 65536, 0)):
        assert size(C, T, n, nov) == 0, (C, T, n, nov)
        assert call(L, C=C, T=T, nperseg=n, noverlap=nov) in (-1, -2)
    for C, T, n, nov in ((8, 298, 2, 1), (90, 300000, 1000, 500), (8, 4096, 4096, 0), (5760, 298, 256, 128)):
        need = size(C, T, n, nov)
        assert need > 0 and need % 16 == 0
        # the minimum does not depend on the mode: one byte less is too little for each, the minimum passes
        # the check (the next refusal is the workspace's alignment)
        for mode in (MATRIX, COHERENCE, PAIRS, PAIR_COHERENCE):
            if C > 1024 and mode in (MATRIX, COHERENCE):
                continue
            assert call(L, C=C, T=T, nperseg=n, noverlap=nov, mode=mode, nbytes=need - 1) == -3
            assert str(need).encode() in L.wc_last_error()
            assert call(L, C=C, T=T, nperseg=n, noverlap=nov, mode=mode, nbytes=need,
                        ws=ctypes.c_void_p((1 << 24) + 8)) == -1
            assert b"16-byte" in L.wc_last_error()
    # tables + running sums [F][C] complex + one segment block (two segments) of spectra for all C columns
    F = 501
    tables = (8192 + 1008 + 2048) * 16
    assert size(90, 300000, 1000, 500) == tables + 3 * F * 90 * 16
    assert size(90, 300000, 1000, 500) == size(90, 1000, 1000, 0)       # and not with the number of segments


@pytest.mark.parametrize("fn,kwargs,word", [
    ("csd", dict(nfft=2048), "nfft"),
    ("csd", dict(nfft=512, nperseg=256), "nfft"),
    ("csd", dict(return_onesided=False), "return_onesided"),
    ("csd", dict(average="median"), "average"),
    ("csd", dict(detrend="linear"), "detrend"),
    ("csd", dict(detrend=lambda v: v), "detrend"),
    ("coherence", dict(nfft=2048), "nfft"),
    ("coherence", dict(detrend="linear"), "detrend"),
])
def test_utils_refuse_before_touching_the_device(fn, kwargs, word):
    from nremmodfc_amd import utils
    x = np.random.default_rng(0).standard_normal((1000, 3))
    with pytest.raises(NotImplementedError, match=word):
        getattr(utils, fn)(x, x[::-1], 500.0, axis=0, **kwargs)


@pytest.mark.parametrize("fn", ["csd", "coherence"])
def test_utils_refuse_complex_and_unequal_shapes(fn):
    from nremmodfc_amd import utils
    x = np.random.default_rng(0).standard_normal((1000, 3))
    with pytest.raises(NotImplementedError, match="complex"):
        getattr(utils, fn)(x * (1 + 1j), x, 500.0, axis=0)
    with pytest.raises(NotImplementedError, match="complex"):
        getattr(utils, fn)(x, x * (1 + 1j), 500.0, axis=0)
    with pytest.raises(NotImplementedError, match="shapes"):
        getattr(utils, fn)(x, x[:900], 500.0, axis=0)                    # SciPy zero-pads the shorter
    with pytest.raises(NotImplementedError, match="shapes"):
        getattr(utils, fn)(x[:, :, None], x[:, None, :], 500.0, axis=0)  # SciPy broadcasts


@pytest.mark.parametrize("fn", ["csd_matrix", "coherence_matrix"])
def test_utils_matrix_refusals(fn):
    from nremmodfc_amd import utils
    x = np.random.default_rng(0).standard_normal((1000, 3))
    with pytest.raises(NotImplementedError, match="detrend"):
        getattr(utils, fn)(x, 500.0, detrend="linear")
    with pytest.raises(NotImplementedError, match="complex"):
        getattr(utils, fn)(x * 1j, 500.0)
    with pytest.raises(ValueError, match="rois"):
        getattr(utils, fn)(x[:, 0], 500.0)


def make_signal(M, C):
    """test_welch_psd_gpu.py's recipe."""
    rng = np.random.default_rng(M)
    t = np.arange(M)[:, None] * 0.002
    f = rng.uniform(2, 12, C)
    p = rng.uniform(0, 2 * np.pi, C)
    g = rng.uniform(0.05, 0.2, C)
    x = (1 + 0.3 * np.sin(2 * np.pi * g * t)) * np.cos(2 * np.pi * f * t + p) + 0.01 * rng.standard_normal((M, C))
    x[:, ::2] = 0.2 + 0.05 * x[:, ::2]
    return np.ascontiguousarray(x)


@pytest.mark.parametrize("T,C,n", [(300, 6, 15), (4500, 5, 1000)])
@pytest.mark.parametrize("kw", [dict(), dict(detrend=False, scaling="spectrum", window=("tukey", 0.25))])
def test_reference_helper_is_scipy(T, C, n, kw):
    """The numpy loop over segments against SciPy's broadcast form (T x C x C on the host: small shapes)."""
    x = make_signal(T, C)
    nov = n // 2
    fw, want = signal.csd(x[:, :, None], x[:, None, :], 500.0, nperseg=n, noverlap=nov, axis=0, **kw)
    fg, got = ref.csd_matrix(x, 500.0, nperseg=n, noverlap=nov, **{"window": "hann", **kw})
    np.testing.assert_array_equal(fg, fw)
    psd = signal.welch(x, 500.0, nperseg=n, noverlap=nov, axis=0, **kw)[1]
    d = ref.csd_deviation(got, want, psd)
    print(f"TOL csd-reference-T{T}-n{n} dev={d:.3e}")
    assert d <= 1e-14
    kc = {k: v for k, v in kw.items() if k != "scaling"}
    cw = signal.coherence(x[:, :, None], x[:, None, :], 500.0, nperseg=n, noverlap=nov, axis=0, **kc)[1]
    d = ref.coherence_deviation(ref.coherence_of(got), cw, psd)
    print(f"TOL coherence-reference-T{T}-n{n} dev={d:.3e}")
    assert d <= 1e-14
    # the columnwise form of the pair modes
    y = make_signal(T + 1, C)[1:]
    fw, want = signal.csd(x, y, 500.0, nperseg=n, noverlap=nov, axis=0, **kw)
    fg, got = ref.csd_pairs(x, y, 500.0, nperseg=n, noverlap=nov, **{"window": "hann", **kw})
    psdy = signal.welch(y, 500.0, nperseg=n, noverlap=nov, axis=0, **kw)[1]
    assert ref.csd_deviation(got, want, psd, psdy) <= 1e-14

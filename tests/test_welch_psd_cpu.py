"""wc_welch_psd validates every argument before any device work, its size function returns 0 exactly
where the call would return anything but WC_OK or WC_EWORKSPACE, and utils.welch refuses what the
device does not compute before it touches the device (no GPU: the pointers are fake)."""
import ctypes

import numpy as np
import pytest

X, WIN, PSD, WS = (ctypes.c_void_p(v) for v in (1 << 30, 1 << 20, 1 << 32, 1 << 24))
BIG = 1 << 40


def call(L, C=7, T=298, x=X, nperseg=64, noverlap=32, window=WIN, detrend=1, scale=1.0, psd=PSD, ws=WS, nbytes=BIG):
    return L.wc_welch_psd(C, T, x, nperseg, noverlap, window, detrend, scale, psd, ws, nbytes, None)


def test_welch_psd_validates_without_device_work():
    from nremmodfc_amd import _lib
    L = _lib.lib()
    assert call(L, C=0) == -1
    assert call(L, C=-3) == -1
    assert call(L, nperseg=1, noverlap=0) == -1
    assert call(L, nperseg=0, noverlap=0) == -1
    assert call(L, noverlap=-1) == -1
    assert call(L, noverlap=64) == -1                     # noverlap == nperseg
    assert call(L, noverlap=65) == -1
    assert call(L, T=63) == -1                            # T < nperseg
    assert call(L, x=None) == -1
    assert call(L, window=None) == -1
    assert call(L, psd=None) == -1
    assert call(L, psd=X) == -1                           # psd aliasing x
    assert b"alias" in L.wc_last_error()
    assert call(L, psd=ctypes.c_void_p((1 << 30) + 8 * 7 * 100)) == -1   # psd inside x [298][7]
    assert call(L, detrend=2) == -1
    assert call(L, detrend=-1) == -1
    for bad in (0.0, -1.0, float("inf"), float("nan")):
        assert call(L, scale=bad) == -1
    assert call(L, x=ctypes.c_void_p((1 << 30) + 4)) == -1               # 8-byte alignment of x, window, psd
    assert call(L, window=ctypes.c_void_p((1 << 20) + 4)) == -1
    assert call(L, psd=ctypes.c_void_p((1 << 32) + 4)) == -1
    assert call(L, ws=ctypes.c_void_p((1 << 24) + 8)) == -1              # 16-byte alignment of the workspace
    assert call(L, T=10000, nperseg=4097, noverlap=0) == -2
    assert b"4096" in L.wc_last_error()
    assert call(L, T=100000, nperseg=65536, noverlap=0) == -2
    assert call(L, ws=None, nbytes=0) == -3
    assert call(L, ws=None) == -3
    assert call(L, nbytes=0) == -3


def test_welch_psd_workspace_size():
    from nremmodfc_amd import _lib
    L = _lib.lib()
    size = L.wc_welch_psd_workspace_size
    for C, T, n, nov in ((0, 298, 64, 32), (-1, 298, 64, 32), (7, 298, 1, 0), (7, 298, 0, 0), (7, 298, 64, -1),
                         (7, 298, 64, 64), (7, 298, 64, 65), (7, 63, 64, 32), (7, 10000, 4097, 0),
                         (7, 100000, 65536, 0)):
        assert size(C, T, n, nov) == 0, (C, T, n, nov)
    for C, T, n, nov in ((7, 298, 2, 1), (90, 300000, 1000, 500), (7, 4096, 4096, 0)):
        need = size(C, T, n, nov)
        assert need > 0 and need % 8 == 0
        assert call(L, C=C, T=T, nperseg=n, noverlap=nov, nbytes=need - 8) == -3
        assert b"workspace" in L.wc_last_error()
    # the minimum is one column's: it does not grow with C
    assert size(1, 300000, 1000, 500) == size(90, 300000, 1000, 500)


@pytest.mark.parametrize("kwargs,word", [
    (dict(nfft=2048), "nfft"),
    (dict(nfft=512, nperseg=256), "nfft"),
    (dict(return_onesided=False), "return_onesided"),
    (dict(average="median"), "average"),
    (dict(detrend="linear"), "detrend"),
    (dict(detrend=lambda v: v), "detrend"),
])
def test_utils_welch_refuses_before_touching_the_device(kwargs, word):
    from nremmodfc_amd import utils
    x = np.random.default_rng(0).standard_normal((1000, 3))
    with pytest.raises(NotImplementedError, match=word):
        utils.welch(x, 500.0, axis=0, **kwargs)


def test_utils_welch_refuses_complex_input():
    from nremmodfc_amd import utils
    x = np.random.default_rng(0).standard_normal((1000, 3)) * (1 + 1j)
    with pytest.raises(NotImplementedError, match="complex"):
        utils.welch(x, 500.0, axis=0)

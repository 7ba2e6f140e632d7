"""wc_spectrogram validates every argument before any device work, for each of its four modes;
wc_spectrogram_workspace_size is the table formula and 0 exactly for the nperseg the call rejects;
utils.spectrogram refuses what the device does not compute before it touches it (no GPU: the
pointers are fake)."""
import ctypes

import numpy as np
import pytest

X, WIN, OUT, WS = (ctypes.c_void_p(v) for v in (1 << 30, 1 << 20, 1 << 32, 1 << 24))
BIG = 1 << 40
PSD, COMPLEX, MAGNITUDE, ANGLE = 0, 1, 2, 3
MODES = (PSD, COMPLEX, MAGNITUDE, ANGLE)


def call(L, C=8, T=298, x=X, nperseg=64, noverlap=32, window=WIN, detrend=1, scale=1.0, mode=PSD, out=OUT, ws=WS,
         nbytes=BIG):
    return L.wc_spectrogram(C, T, x, nperseg, noverlap, window, detrend, scale, mode, out, ws, nbytes, None)


def tables(n):
    """(W_8192 + the chirp padded to 16 entries + the chirp spectrum [L]) complex fp64."""
    L = max(64, 1 << (2 * n - 2).bit_length())  # nextpow2(2 n - 1)
    return (8192 + -(-n // 16) * 16 + L) * 16


def test_spectrogram_validates_without_device_work():
    from nremmodfc_amd import _lib
    L = _lib.lib()
    for mode in MODES:
        assert call(L, C=0, mode=mode) == -1
        assert call(L, C=-4, mode=mode) == -1
        assert call(L, C=(1 << 24) + 1, mode=mode) == -1
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
        assert b"alias" in L.wc_last_error()
        assert call(L, detrend=2, mode=mode) == -1
        assert call(L, detrend=-1, mode=mode) == -1
        for bad in (0.0, -1.0, float("inf"), float("nan")):
            assert call(L, scale=bad, mode=mode) == -1
            assert b"scale" in L.wc_last_error()
        assert call(L, x=ctypes.c_void_p((1 << 30) + 4), mode=mode) == -1     # 8-byte alignment of x, window, out
        assert call(L, window=ctypes.c_void_p((1 << 20) + 4), mode=mode) == -1
        assert call(L, out=ctypes.c_void_p((1 << 32) + 4), mode=mode) == -1
        assert b"8-byte" in L.wc_last_error()
        assert call(L, ws=ctypes.c_void_p((1 << 24) + 8), mode=mode) == -1    # 16-byte alignment of the workspace
        assert b"16-byte" in L.wc_last_error()
        assert call(L, T=10000, nperseg=4097, noverlap=0, mode=mode) == -2
        assert b"4096" in L.wc_last_error()
        assert call(L, ws=None, nbytes=0, mode=mode) == -3
        assert call(L, ws=None, mode=mode) == -3
        assert call(L, nbytes=0, mode=mode) == -3
        assert b"workspace" in L.wc_last_error()
        assert call(L, C=1 << 24, out=ctypes.c_void_p(1 << 50), nbytes=0, mode=mode) == -3   # the widest C
    for mode in (-1, 4, 17):
        assert call(L, mode=mode) == -1
        assert b"mode" in L.wc_last_error()


def test_spectrogram_alias_check_uses_the_modes_output_size():
    """x [298][8] at 2^30; nperseg 64 / noverlap 32: S = 8 segments of F = 33 bins of C = 8 columns =
    2112 cells.  An out that starts 2112 * 8 bytes before x ends where x begins in the real modes
    (on to the workspace check) and reaches 2112 * 8 bytes into it as complex."""
    from nremmodfc_amd import _lib
    L = _lib.lib()
    cells = 8 * 33 * 8
    before = ctypes.c_void_p((1 << 30) - cells * 8)
    for mode in (PSD, MAGNITUDE, ANGLE):
        assert call(L, out=before, mode=mode, nbytes=0) == -3
        assert call(L, out=ctypes.c_void_p((1 << 30) - cells * 8 + 8), mode=mode, nbytes=0) == -1  # one cell into x
        assert b"alias" in L.wc_last_error()
    assert call(L, out=before, mode=COMPLEX, nbytes=0) == -1
    assert b"alias" in L.wc_last_error()
    assert call(L, out=ctypes.c_void_p((1 << 30) - cells * 16), mode=COMPLEX, nbytes=0) == -3
    # behind x: its last byte is at 2^30 + 298 * 8 * 8 - 1
    for mode in MODES:
        assert call(L, out=ctypes.c_void_p((1 << 30) + 298 * 8 * 8), mode=mode, nbytes=0) == -3
        assert call(L, out=ctypes.c_void_p((1 << 30) + 298 * 8 * 8 - 8), mode=mode, nbytes=0) == -1


def test_spectrogram_refuses_an_output_of_2_62_bytes():
    """S F C cells of 8 (complex: 16) bytes: 2^24 columns of 2049 bins are 2^38.0007 bytes a segment in
    the real modes, so just under 2^24 segments reach 2^62, as complex half as many.  Hop 1: x itself,
    (4095 + S) 2^24 8 bytes, stays near 2^51."""
    from nremmodfc_amd import _lib
    L = _lib.lib()
    C, n = 1 << 24, 4096
    seg_bytes = (n // 2 + 1) * C * 8
    for mode in MODES:
        cell = 2 if mode == COMPLEX else 1
        S = -(-(1 << 62) // (seg_bytes * cell))         # the first segment count at or above 2^62 bytes
        kw = dict(C=C, nperseg=n, noverlap=n - 1, x=ctypes.c_void_p(8), out=ctypes.c_void_p(1 << 63), mode=mode)
        assert call(L, T=n + S - 1, **kw) == -1
        assert b"2^62" in L.wc_last_error() and b"output" in L.wc_last_error()
        assert call(L, T=n + S - 2, nbytes=0, **kw) == -3               # one segment fewer: on to the workspace
    assert call(L, C=C, T=1 << 36, nperseg=n, noverlap=0, x=ctypes.c_void_p(8), out=ctypes.c_void_p(1 << 63)) == -1
    assert b"2^62" in L.wc_last_error()                                 # x of 2^63 bytes


def test_spectrogram_workspace_size():
    from nremmodfc_amd import _lib
    L = _lib.lib()
    size = L.wc_spectrogram_workspace_size
    for n in (-5, 0, 1, 4097, 8192, 65536):
        assert size(n) == 0, n
        assert call(L, T=100000, nperseg=n, noverlap=0) in (-1, -2)
    assert size(2) == (8192 + 16 + 64) * 16
    assert size(1000) == (8192 + 1008 + 2048) * 16
    assert size(4096) == (8192 + 4096 + 8192) * 16
    for n in (2, 3, 15, 16, 17, 32, 33, 64, 400, 1000, 1023, 1024, 1025, 2048, 2049, 4000, 4095, 4096):
        need = size(n)
        assert need == tables(n) and need % 16 == 0, n
        for C, T in ((1, n), (90, 300000), (5760, 5000)):                # independent of C and T
            for mode in MODES:
                assert call(L, C=C, T=T, nperseg=n, noverlap=n // 2, mode=mode, nbytes=need - 1) == -3
                assert str(need).encode() in L.wc_last_error()
                # the minimum passes the check: the next refusal is the workspace's alignment
                assert call(L, C=C, T=T, nperseg=n, noverlap=n // 2, mode=mode, nbytes=need,
                            ws=ctypes.c_void_p((1 << 24) + 8)) == -1
                assert b"16-byte" in L.wc_last_error()


@pytest.mark.parametrize("kwargs,word", [
    (dict(nfft=2048), "nfft"),
    (dict(nfft=512, nperseg=256), "nfft"),
    (dict(nfft=2048, window=np.hanning(400)), "nfft"),
    (dict(return_onesided=False), "return_onesided"),
    (dict(detrend="linear"), "detrend"),
    (dict(detrend=lambda v: v), "detrend"),
])
@pytest.mark.parametrize("mode", ["psd", "complex", "magnitude", "angle", "phase"])
def test_utils_spectrogram_refuses_before_touching_the_device(kwargs, word, mode):
    from nremmodfc_amd import utils
    x = np.random.default_rng(0).standard_normal((1000, 3))
    with pytest.raises(NotImplementedError, match=word):
        utils.spectrogram(x, 500.0, axis=0, mode=mode, **kwargs)


def test_utils_spectrogram_refuses_complex_input_and_unknown_modes():
    from scipy import signal

    from nremmodfc_amd import sigchain, utils
    x = np.random.default_rng(0).standard_normal((1000, 3))
    with pytest.raises(NotImplementedError, match="complex"):
        utils.spectrogram(x * (1 + 1j), 500.0, axis=0)
    for mode in ("stft", "PSD", "power", None):
        with pytest.raises(ValueError) as theirs:
            signal.spectrogram(x, 500.0, axis=0, mode=mode)
        with pytest.raises(ValueError) as mine:
            utils.spectrogram(x, 500.0, axis=0, mode=mode)
        assert str(mine.value) == str(theirs.value)
        with pytest.raises(ValueError) as dev:                          # before the tensor is looked at
            sigchain.spectrogram(None, 500.0, mode=mode)
        assert str(dev.value) == str(theirs.value)
    with pytest.raises(NotImplementedError, match="phase"):
        sigchain.spectrogram(None, 500.0, mode="phase")

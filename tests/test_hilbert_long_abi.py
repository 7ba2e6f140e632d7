"""wc_hilbert_phase_long / wc_hilbert_long_workspace_size: sizes and argument validation (no GPU).

Every call here returns before any device work; the arithmetic is checked in
test_hilbert_long_gpu.py."""
import ctypes

import pytest

MAX_M = 524288
VP = ctypes.c_void_p(16)


@pytest.fixture(scope="module")
def L():
    from nremmodfc_amd import _build, _lib
    _build.build()
    return _lib.lib()


def fft_len(M):
    """L = max(2^15, nextpow2(2 M - 1)) (include/wcsde.h)."""
    n = 1 << 15
    while n < 2 * M - 1:
        n *= 2
    return n


def test_workspace_size_zero_when_unsupported(L):
    assert L.wc_hilbert_long_workspace_size(0, 1000) == 0
    assert L.wc_hilbert_long_workspace_size(-3, 1000) == 0
    assert L.wc_hilbert_long_workspace_size(6, 1) == 0
    assert L.wc_hilbert_long_workspace_size(6, 0) == 0
    assert L.wc_hilbert_long_workspace_size(6, MAX_M + 1) == 0
    assert L.wc_hilbert_long_workspace_size(6, MAX_M) > 0


def test_workspace_size_grows_with_m(L):
    sizes = [L.wc_hilbert_long_workspace_size(6, M) for M in (8193, 16384, 16385, 300_000)]
    assert all(s > 0 for s in sizes)
    assert sizes == sorted(sizes)
    assert sizes[2] > sizes[1]  # 2 M - 1 passes 2^15: the FFT length doubles


@pytest.mark.parametrize("M", [2, 8193, 16384, 16385, 29800, 300_000, MAX_M])
def test_workspace_size_holds_tables_and_one_column(L, M):
    n = fft_len(M)
    assert n <= 1 << 20
    # chirp [M] + chirp spectrum [L] + two [L] buffers for one column, complex fp64
    assert L.wc_hilbert_long_workspace_size(1, M) >= (M + n + 2 * n) * 16
    # the minimum is one column's, whatever C
    assert L.wc_hilbert_long_workspace_size(90, M) == L.wc_hilbert_long_workspace_size(1, M)


def test_phase_long_validates_without_device_work(L):
    M = 29800
    need = L.wc_hilbert_long_workspace_size(90, M)
    assert L.wc_hilbert_phase_long(90, M, None, VP, VP, need, None) == -1
    assert L.wc_hilbert_phase_long(90, M, VP, None, VP, need, None) == -1
    assert L.wc_hilbert_phase_long(0, M, VP, VP, VP, need, None) == -1
    assert L.wc_hilbert_phase_long(90, 1, VP, VP, VP, need, None) == -1
    assert L.wc_hilbert_phase_long(90, MAX_M + 1, VP, VP, VP, 1 << 40, None) == -2
    assert b"524288" in L.wc_last_error()
    assert L.wc_hilbert_phase_long(90, M, VP, VP, VP, need - 1, None) == -3
    assert b"workspace" in L.wc_last_error()
    assert L.wc_hilbert_phase_long(90, M, VP, VP, None, need, None) == -3


def test_direct_entry_point_refuses_long_series(L):
    """wc_hilbert_phase holds q[0..M) in a 64 KB LDS launch: M > 8192 names the long entry point."""
    assert L.wc_hilbert_phase(90, 29800, VP, VP, VP, 29800 * 8, None) == -2
    assert b"wc_hilbert_phase_long" in L.wc_last_error()
    assert L.wc_hilbert_phase(90, 8193, VP, VP, VP, 8193 * 8, None) == -2
    # 8192 is still served: validation passes on to the workspace check
    assert L.wc_hilbert_phase(90, 8192, VP, VP, VP, 8192 * 8 - 1, None) == -3

"""wc_phase_conn validates every argument before any device work; wc_phase_conn_workspace_size is the
partial-sum formula and 0 exactly where the call returns neither WC_OK nor WC_EWORKSPACE; the bit order
of measures fixes the layout of out; sigchain.phase_connectivity and utils.connectivity refuse bad
names, dtypes and ranks before they touch the device (no GPU: the pointers are fake); and the host
reference of test_connectivity_gpu.py (tests/conn_reference.py) is pinned to independent forms."""
import ctypes

import numpy as np
import pytest
from scipy import signal

from tests import conn_reference as ref

PH, AMP, OUT, WS = (ctypes.c_void_p(v) for v in (1 << 40, 1 << 36, 1 << 44, 1 << 24))
BIG = 1 << 50
PLV, PLI, WPLI, ORTH = 1, 2, 4, 8
ALL = 15


def call(L, B=1, N=90, M=298, ph=PH, amp=AMP, measures=ALL, out=OUT, ws=WS, nbytes=BIG):
    return L.wc_phase_conn(B, N, M, ph, amp, measures, out, ws, nbytes, None)


def expected_size(B, N, M, measures):
    """Partial sums [B][tile pairs][time blocks][K][32][32] fp64, K = 8 with an amplitude bit and 3
    without, plus the columns' (sum a, sum a^2) [B][time blocks][N] for aec_orth, rounded up to 16."""
    nt, nblk = -(-N // 32), -(-M // 4096)
    part = B * (nt * (nt + 1) // 2) * nblk * (8 if measures & (WPLI | ORTH) else 3) * 1024 * 8
    col = -(-(B * nblk * N * 16) // 16) * 16 if measures & ORTH else 0
    return part + col


def test_phase_conn_validates_without_device_work():
    from nremmodfc_amd import _lib
    L = _lib.lib()
    for measures in range(1, 16):
        kw = dict(measures=measures)
        needs_amp = bool(measures & (WPLI | ORTH))
        assert call(L, B=0, **kw) == -1 and b"B < 1" in L.wc_last_error()
        assert call(L, B=-3, **kw) == -1
        assert call(L, N=0, **kw) == -1 and b"N < 1" in L.wc_last_error()
        assert call(L, N=-90, **kw) == -1
        assert call(L, M=1, **kw) == -1 and b"M < 2" in L.wc_last_error()
        assert call(L, M=0, **kw) == -1
        assert call(L, ph=None, **kw) == -1 and b"NULL" in L.wc_last_error()
        assert call(L, out=None, **kw) == -1 and b"NULL" in L.wc_last_error()
        if needs_amp:
            assert call(L, amp=None, **kw) == -1
            assert b"amp is NULL" in L.wc_last_error()
        else:
            assert call(L, amp=None, nbytes=0, **kw) == -3              # no envelopes needed: on to the workspace
        assert call(L, out=PH, **kw) == -1 and b"alias" in L.wc_last_error()
        assert call(L, out=ctypes.c_void_p((1 << 40) + 16 * 90 * 100), **kw) == -1   # inside the phasors
        assert b"alias" in L.wc_last_error()
        assert call(L, out=AMP, **kw) == -1 and b"alias" in L.wc_last_error()         # amp is looked at if given
        assert call(L, ph=ctypes.c_void_p((1 << 40) + 4), **kw) == -1
        assert b"8-byte" in L.wc_last_error()
        assert call(L, amp=ctypes.c_void_p((1 << 36) + 4), **kw) == -1
        assert b"8-byte" in L.wc_last_error()
        assert call(L, out=ctypes.c_void_p((1 << 44) + 4), **kw) == -1
        assert b"8-byte" in L.wc_last_error()
        assert call(L, ph=ctypes.c_void_p((1 << 40) + 8), nbytes=0, **kw) == -3       # 8-byte phasors are enough
        assert call(L, ws=ctypes.c_void_p((1 << 24) + 8), **kw) == -1
        assert b"16-byte" in L.wc_last_error()
        assert call(L, N=1025, **kw) == -2 and b"1024" in L.wc_last_error()
        assert call(L, M=524289, **kw) == -2 and b"524288" in L.wc_last_error()
        assert call(L, ws=None, nbytes=0, **kw) == -3
        assert call(L, ws=None, **kw) == -3
        assert call(L, nbytes=0, **kw) == -3
        assert b"workspace" in L.wc_last_error()
    for measures in (0, -1, 16, 17, 32, 1 << 20):
        assert call(L, measures=measures) == -1
        assert b"measures" in L.wc_last_error()
    # B times the tile pairs is one grid dimension
    assert call(L, B=1 << 22, N=1024, M=2, ph=ctypes.c_void_p(8), amp=ctypes.c_void_p(1 << 61),
                out=ctypes.c_void_p(1 << 63)) == -1
    assert b"2^31" in L.wc_last_error()


def test_phase_conn_workspace_size():
    from nremmodfc_amd import _lib
    L = _lib.lib()
    size = L.wc_phase_conn_workspace_size
    for B, N, M, measures in ((0, 90, 298, ALL), (-1, 90, 298, ALL), (1, 0, 298, ALL), (1, -5, 298, ALL),
                              (1, 1025, 298, ALL), (1, 90, 1, ALL), (1, 90, 0, ALL), (1, 90, 524289, ALL),
                              (1, 90, 298, 0), (1, 90, 298, 16), (1, 90, 298, -1), (1, 90, 298, 31),
                              (1 << 22, 1024, 298, ALL)):
        assert size(B, N, M, measures) == 0, (B, N, M, measures)
        assert call(L, B=B, N=N, M=M, measures=measures, ph=ctypes.c_void_p(8), amp=ctypes.c_void_p(1 << 61),
                    out=ctypes.c_void_p(1 << 63)) in (-1, -2)
    assert size(1, 90, 300000, PLV | PLI) == 6 * 74 * 3 * 8192
    assert size(1, 90, 300000, ALL) == 6 * 74 * 8 * 8192 + 74 * 90 * 16
    assert size(1, 1000, 48000, ALL) == 528 * 12 * 8 * 8192 + 12 * 1000 * 16
    assert size(64, 90, 298, ALL) == 64 * 6 * 8 * 8192 + 64 * 90 * 16
    for B, N, M in ((1, 1, 2), (1, 2, 2), (1, 3, 3), (1, 32, 4096), (1, 33, 4097), (3, 90, 298), (1, 130, 300),
                    (2, 1024, 8193), (1, 90, 524288), (7, 5, 20000)):
        for measures in range(1, 16):
            need = size(B, N, M, measures)
            assert need == expected_size(B, N, M, measures) and need % 16 == 0 and need > 0, (B, N, M, measures)
            kw = dict(B=B, N=N, M=M, measures=measures)
            assert call(L, nbytes=need - 1, **kw) == -3
            assert str(need).encode() in L.wc_last_error()
            # the minimum passes the check: the next refusal is the workspace's alignment
            assert call(L, nbytes=need, ws=ctypes.c_void_p((1 << 24) + 8), **kw) == -1
            assert b"16-byte" in L.wc_last_error()


def test_phase_conn_measure_bits_fix_the_out_layout():
    """out holds one [B][N][N] matrix per set bit: with the phasors [298][2][90][2] at 2^40, an out whose
    k-th matrix starts where the phasors do aliases them exactly when k matrices or more are asked for."""
    from nremmodfc_amd import _lib
    L = _lib.lib()
    mat = 2 * 90 * 90 * 8
    for measures in range(1, 16):
        n = bin(measures).count("1")
        for k in range(1, 5):
            out = ctypes.c_void_p((1 << 40) - k * mat)                  # matrices 0 .. k - 1 end where the phasors begin
            rc = call(L, B=2, measures=measures, out=out, nbytes=0)
            assert rc == (-3 if n <= k else -1), (measures, k)
            if rc == -1:
                assert b"alias" in L.wc_last_error()
        # one cell of the last matrix inside the envelopes
        out = ctypes.c_void_p((1 << 36) - n * mat + 8)
        assert call(L, B=2, measures=measures, out=out, nbytes=0) == -1
        assert b"alias" in L.wc_last_error()
        assert call(L, B=2, measures=measures, out=ctypes.c_void_p((1 << 36) - n * mat), nbytes=0) == -3
        # the phasors end at 2^40 + 298 * 180 * 16, the envelopes at 2^36 + 298 * 180 * 8
        assert call(L, B=2, measures=measures, out=ctypes.c_void_p((1 << 40) + 298 * 180 * 16), nbytes=0) == -3
        assert call(L, B=2, measures=measures, out=ctypes.c_void_p((1 << 40) + 298 * 180 * 16 - 8), nbytes=0) == -1
        assert call(L, B=2, measures=measures, out=ctypes.c_void_p((1 << 36) + 298 * 180 * 8), nbytes=0) == -3
        assert call(L, B=2, measures=measures, out=ctypes.c_void_p((1 << 36) + 298 * 180 * 8 - 8), nbytes=0) == -1


def test_sigchain_bits_are_the_headers():
    import os
    import re

    from nremmodfc_amd import sigchain
    hdr = open(os.path.join(os.path.dirname(__file__), "..", "include", "wcsde.h")).read()
    for name, macro in (("plv", "PLV"), ("pli", "PLI"), ("wpli", "WPLI"), ("aec_orth", "AEC_ORTH")):
        assert sigchain.CONN_BITS[name] == int(re.search(rf"#define WC_CONN_{macro} (\d+)", hdr).group(1))
    assert list(sigchain.CONN_BITS.values()) == sorted(sigchain.CONN_BITS.values())
    assert re.search(r"#define WCSDE_ABI_VERSION 7\b", hdr)


def test_facades_refuse_before_touching_the_device():
    import torch

    from nremmodfc_amd import sigchain, utils
    x = np.random.default_rng(0).standard_normal((100, 3))
    for bad in ("coh", ("plv", "PLI"), ("plv", None), (), "imcoh"):
        with pytest.raises(ValueError, match="measure"):
            utils.connectivity(x, measures=bad)
        with pytest.raises(ValueError, match="measure"):
            sigchain.phase_connectivity(None, measures=bad)              # before the tensor is looked at
        with pytest.raises(ValueError, match="measure"):
            sigchain.phase_connectivity_from(None, None, measures=bad)
    with pytest.raises(TypeError):
        utils.connectivity(x * (1 + 1j))
    with pytest.raises(TypeError):
        utils.connectivity(np.array([["a", "b"], ["c", "d"]]))
    for shape in ((100,), (10, 2, 3, 4), (0, 3)):
        with pytest.raises(ValueError, match="series"):
            utils.connectivity(np.zeros(shape))
    with pytest.raises(ValueError, match="freqs"):
        utils.connectivity(x, freqs=[8])
    for t in (torch.zeros((100, 3), dtype=torch.float32), torch.zeros(100, dtype=torch.float64),
              torch.zeros((10, 2, 3, 4), dtype=torch.float64), torch.zeros((100, 3), dtype=torch.complex128), x, None):
        with pytest.raises(TypeError, match="phase_connectivity"):
            sigchain.phase_connectivity(t)
    ph = torch.zeros((100, 3, 2), dtype=torch.float64)
    for t in (ph.float(), ph[..., :1], ph[:, 0], torch.zeros((100, 3), dtype=torch.complex128), None):
        with pytest.raises(TypeError, match="phasor"):
            sigchain.phase_connectivity_from(t, None, ("plv",))
    for amp in (None, torch.zeros((100, 3), dtype=torch.float32), torch.zeros((100, 4), dtype=torch.float64),
                torch.zeros((100, 3, 1), dtype=torch.float64)):
        for m in ("wpli", "aec", "aec_orth"):
            with pytest.raises(TypeError, match="amp"):
                sigchain.phase_connectivity_from(ph, amp, (m,))


# ---- the reference itself ----

def test_reference_plv_is_the_complex_gram_form():
    x = ref.make(1000, 9, 1)
    u, _ = ref.analytic(x)
    want = np.abs(u.conj().T @ u) / x.shape[0]
    got = ref.connectivity(x)["plv"]
    assert ref.deviation(got, want) < 1e-14
    assert (np.diag(got) == 1.0).all()


def test_reference_aec_is_corrcoef_of_the_envelopes():
    x = ref.make(1000, 9, 1)
    got = ref.connectivity(x)
    assert ref.deviation(got["aec"], np.corrcoef(np.abs(signal.hilbert(x, axis=0)).T)) < 1e-14
    for m in ref.MEASURES:
        assert (got[m] == got[m].T).all() or m == "aec_orth"            # aec_orth: the two terms add in either order
        np.testing.assert_array_equal(np.diag(got[m]), ref.DIAGONAL[m])
        assert np.abs(ref.off_diagonal(got[m])).max() <= 1.0
    np.testing.assert_array_equal(got["aec_orth"], got["aec_orth"].T)


def test_reference_duplicated_column():
    x = ref.make(4097, 4, 1)
    x[:, 3] = x[:, 1]
    u, _ = ref.analytic(x)
    assert (ref.lag(u, 1)[:, 3] == 0).all()                             # the explicit real form: exactly 0
    got = ref.connectivity(x)
    nan = np.zeros((4, 4), dtype=bool)
    nan[1, 3] = nan[3, 1] = True
    assert got["pli"][1, 3] == 0.0 and got["pli"][3, 1] == 0.0
    for m in ("wpli", "aec_orth"):
        np.testing.assert_array_equal(np.isnan(got[m]), nan)
    assert abs(got["plv"][1, 3] - 1.0) < 1e-14 and abs(got["aec"][1, 3] - 1.0) < 1e-14
    assert ref.near_zero_lags(np.delete(x, 3, axis=1))[0] == 0


def test_reference_column_against_its_hilbert_transform():
    x = ref.make(2001, 2, 1)                                            # odd: no Nyquist bin
    x[:, 0] -= x[:, 0].mean()                                           # nor a mean: z_1 = -i z_0 up to rounding
    x[:, 1] = signal.hilbert(x[:, 0]).imag                              # lags column 0 by a quarter period
    got = ref.connectivity(x)
    assert got["pli"][0, 1] == 1.0
    assert got["wpli"][0, 1] == 1.0
    assert got["plv"][0, 1] > 0.99


def test_generator_meets_the_condition_on_the_tested_shapes():
    """No sample of the reference within 1e-10 of pli's discontinuity at s = 0, at the small shapes
    (test_connectivity_gpu.py asserts the same for every shape it compares)."""
    for T, C in ((3, 3), (64, 7), (257, 7), (1000, 33), (2049, 5)):
        n, least = ref.near_zero_lags(ref.make(T, C, 1))
        assert n == 0 and least > 1e-7, (T, C, least)

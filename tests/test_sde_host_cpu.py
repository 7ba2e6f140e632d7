"""Host-side values of the N <= 96 integrator that must survive a clean-up of its kernels (no GPU).

wc_workspace_size(): callers size their buffers by it, so every value is observable behaviour.
tests/golden/wc_workspace_size.json holds what the library returned before the diagnostic
native-image term was dropped from it (recorded from a build of that commit through the C ABI, the way
tests/test_arg_checks_cpu.py recorded its return codes): N = 1..96, batch sizes on both sides of
every small-batch threshold for 256 CUs (the count the library assumes without a device, and an
MI355X's), both precisions.

wc_diag_integrate(): the numbers of retired diagnostic variants are not reused; each must be refused
with WC_EINVAL before anything is launched.
"""
import ctypes
import json
import os

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
EINVAL = -1
# one retired number per retired variant bit or configuration (docs/CHANGELOG.md)
RETIRED = {0: "fp32 on native fp32 MFMAs", 3: "bf16 x6 coupling", 13: "bf16 x3 coupling", 14: "fp32 with an fp64 a_ie",
           20: "records 4 deep", 28: "normals before the coupling", 29: "normals interleaved 1:6",
           30: "normals interleaved 1:2", 37: "one cell per instruction", 42: "lean a_ie sum", 58: "fp16 x6 coupling"}


@pytest.fixture(autouse=True)
def _default_paths(monkeypatch):
    monkeypatch.delenv("WCSDE_ZMEM", raising=False)
    monkeypatch.delenv("WCSDE_ZPAIR", raising=False)


def test_workspace_sizes_unchanged():
    from nremmodfc_amd import _lib
    L = _lib.lib()
    with open(os.path.join(HERE, "golden", "wc_workspace_size.json")) as f:
        want = json.load(f)
    assert want["B"] == [1, 16, 17, 2500, 4100, 5700, 20000] and want["N"] == [1, 96]
    bad = []
    for prec, key in ((_lib.WC_F32, "f32"), (_lib.WC_F64, "f64")):
        for B, row in zip(want["B"], want[key]):
            assert len(row) == 96
            for N, size in enumerate(row, start=1):
                got = L.wc_workspace_size(B, N, prec)
                if got != size:
                    bad.append((key, B, N, size, got))
    assert not bad, f"{len(bad)} sizes changed, first (precision, B, N, before, now): {bad[:5]}"


@pytest.mark.parametrize("variant", sorted(RETIRED), ids=lambda v: f"{v}-{RETIRED[v].replace(' ', '_')}")
def test_retired_diag_variants_are_refused(variant):
    from nremmodfc_amd import _build, _lib  # (_lib: torch's HIP runtime is loaded first)
    if not os.path.exists(_build.DIAG_LIB):
        pytest.skip("libwcsde_diag.so not built (python -m nremmodfc_amd._build --diag)")
    D = ctypes.CDLL(_build.DIAG_LIB)
    vp, i64 = ctypes.c_void_p, ctypes.c_int64
    D.wc_diag_integrate.restype = ctypes.c_int
    D.wc_diag_integrate.argtypes = [ctypes.c_int, ctypes.POINTER(_lib.WCParamsC), ctypes.c_int, ctypes.c_int,
                                    vp, vp, vp, vp, vp, vp, vp, i64, i64, ctypes.c_double, i64, vp, vp,
                                    ctypes.c_size_t, vp]
    D.wc_workspace_size.restype = ctypes.c_size_t
    D.wc_workspace_size.argtypes = [ctypes.c_int] * 3
    D.wc_last_error.restype = ctypes.c_char_p
    p = _lib.WCParamsC(a_ee=3.5, a_ei=3.75, a_ii=0.0, tauE=0.01, tauI=0.02, P=0.4, rhoE=0.14, rE=0.5, rI=0.5,
                       mu=1.0, sigmaI=3.0, sqdtD=1e-4, dtSim=1e-3)
    B, N = 16, 90
    fake = [(k + 1) << 44 for k in range(9)]  # never dereferenced: the variant is refused on the host
    rc = D.wc_diag_integrate(variant, ctypes.byref(p), B, N, *fake[:7], 0, 10, 2.0, 0, None, fake[8],
                             D.wc_workspace_size(B, N, _lib.WC_F32), None)
    assert rc == EINVAL, (rc, D.wc_last_error())
    assert b"unknown diagnostic variant" in D.wc_last_error()

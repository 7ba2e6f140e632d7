"""Dynamic FC without a GPU: tests/fcd_reference.py (the numpy restatement that test_fcd_gpu.py compares
the device with) equals a naive loop over windows, pairs and samples on a tiny case, its NaN rules hold,
its KS statistic equals scipy.stats.ks_2samp's; wc_fcd_workspace_size, wc_fcd and wc_fcd_phase validate
every argument before any device work (the pointers are fake); sigchain.fcd, sigchain.fcd_ks and
utils.fcd refuse bad arguments before they touch the device.
"""
import ctypes
import math

import numpy as np
import pytest

from tests import fcd_reference as ref

X, FCD, WIN, WS = (ctypes.c_void_p(v) for v in (1 << 40, 1 << 36, 1 << 44, 1 << 46))


def lib():
    from nremmodfc_amd import _lib
    return _lib.lib()


# ---- the restatement ----

def naive_pearson(a, b):
    n = len(a)
    ma, mb = sum(a) / n, sum(b) / n
    sab = sum((p - ma) * (q - mb) for p, q in zip(a, b))
    saa = sum((p - ma) ** 2 for p in a)
    sbb = sum((q - mb) ** 2 for q in b)
    return sab / math.sqrt(saa) / math.sqrt(sbb)


def test_restatement_equals_a_naive_loop():
    M, N, W, S = 11, 4, 4, 2
    x = ref.make_input(M, 1, N, 5, W, S)[:, 0]
    nw = ref.n_windows(M, W, S)
    assert nw == 4                                               # rows 8 .. 10 after the last window: one unused
    pats = []
    for k in range(nw):
        rows = [[float(v) for v in x[k * S + t]] for t in range(W)]
        pats.append([naive_pearson([r[i] for r in rows], [r[j] for r in rows])
                     for i in range(N) for j in range(i + 1, N)])
    want = [[1.0 if k == l else naive_pearson(pats[k], pats[l]) for l in range(nw)] for k in range(nw)]
    got, v = ref.fcd(x, W, S)
    assert v.shape == (nw, 6) and ref.deviation(v, pats) <= 1e-14
    assert ref.deviation(got, want) <= 1e-13
    assert (got == got.T).all() and (np.diag(got) == 1).all()
    both, vb = ref.fcd_batch(x[:, None, :], W, S)
    assert (both[0] == got).all() and (vb[0] == v).all()


def test_restatement_nan_rules():
    x = ref.make_input(40, 1, 5, 6, 10, 10)[:, 0]
    clean, _ = ref.fcd(x, 10, 10)
    x[20:30, 3] = 3.25                                           # constant within window 2 only
    got, v = ref.fcd(x, 10, 10)
    assert np.isnan(v[2]).sum() == 4 and np.isfinite(np.delete(v, 2, axis=0)).all()
    assert np.isnan(got[2]).all() and np.isnan(got[:, 2]).all()
    keep = np.array([0, 1, 3])
    assert (got[np.ix_(keep, keep)] == clean[np.ix_(keep, keep)]).all()
    flat = np.tile(np.arange(5.0), (3, 1))
    flat[1] = 0.5                                                # a pattern without variance
    r = ref.pearson_rows(flat)
    assert np.isnan(r[1]).all() and np.isnan(r[:, 1]).all() and abs(r[0, 2] - 1.0) <= 1e-15 and r[0, 0] == 1.0


def test_phase_restatement_equals_a_naive_loop():
    rng = np.random.default_rng(3)
    th = rng.uniform(-np.pi, np.pi, size=(5, 4))
    ph = np.stack((np.cos(th), np.sin(th)), axis=-1)
    got = ref.fcd_phase(ph)
    for t in range(5):
        for u in range(5):
            a = [math.cos(th[t, i] - th[t, j]) for i in range(4) for j in range(i + 1, 4)]
            b = [math.cos(th[u, i] - th[u, j]) for i in range(4) for j in range(i + 1, 4)]
            want = 1.0 if t == u else sum(p * q for p, q in zip(a, b)) / math.sqrt(sum(p * p for p in a)) \
                / math.sqrt(sum(q * q for q in b))
            assert abs(got[t, u] - want) <= 1e-14
    assert (got == got.T).all()
    two = np.array([[[1.0, 0.0], [0.0, 1.0]], [[1.0, 0.0], [1.0, 0.0]]])    # N = 2, time 0: phases pi / 2 apart
    r = ref.fcd_phase(two)
    assert np.isnan(r[0]).all() and np.isnan(r[:, 0]).all() and r[1, 1] == 1.0


def test_ks_equals_scipy():
    stats = pytest.importorskip("scipy.stats")
    rng = np.random.default_rng(4)
    for na, nb in ((50, 70), (1, 9), (300, 300)):
        a, b = rng.standard_normal(na), 0.3 + rng.standard_normal(nb)
        a[:: 7] = np.round(a[:: 7], 1)                           # ties, within and between the samples
        b[:: 5] = np.round(b[:: 5], 1)
        assert abs(ref.ks_statistic(a, b) - stats.ks_2samp(a, b).statistic) <= 1e-15
    f, _ = ref.fcd(ref.make_input(30, 1, 4, 8, 6, 2)[:, 0], 6, 2)
    emp = rng.uniform(-1, 1, 40)
    for lag in (1, 3):
        sel = [f[k, l] for k in range(f.shape[0]) for l in range(f.shape[0]) if l - k >= lag]
        assert abs(ref.fcd_ks(f, emp, lag) - stats.ks_2samp(sel, emp).statistic) <= 1e-15
    f[1, 4] = np.nan
    assert np.isnan(ref.fcd_ks(f, emp, 1)) and np.isnan(ref.fcd_ks(f, emp, 3)) and not np.isnan(ref.fcd_ks(f, emp, 4))


def test_deviation_refuses_a_moved_nan():
    want = np.array([0.5, np.nan, -1.0])
    assert ref.deviation(want, want) == 0.0
    assert ref.deviation([0.5, 0.0, -1.0], want) == np.inf
    assert ref.deviation([np.nan, np.nan, -1.0], want) == np.inf
    assert ref.deviation([0.5, np.nan], want) == np.inf
    assert abs(ref.deviation([0.5 + 1e-9, np.nan, -1.0], want) - 1e-9) < 1e-15


# ---- the C ABI ----

def call_fcd(L, B=1, N=90, M=298, x=X, win=30, step=1, fcd=FCD, winfc=WIN, ws=WS, ws_bytes=None):
    if ws_bytes is None:
        ws_bytes = L.wc_fcd_workspace_size(B, N, M, win, step) or 1 << 20
    return L.wc_fcd(B, N, M, x, win, step, fcd, winfc, ws, ws_bytes, None)


def call_phase(L, B=1, N=90, M=298, ph=X, fcd=FCD):
    return L.wc_fcd_phase(B, N, M, ph, fcd, None)


def at(p, off):
    return ctypes.c_void_p(p.value + off)


def test_workspace_size():
    L = lib()
    slot = (269 * 4005 + 269) * 8                                # a simulation's centred patterns and norms
    assert L.wc_fcd_workspace_size(1, 90, 298, 30, 1) == slot
    assert L.wc_fcd_workspace_size(3, 90, 298, 30, 1) == 3 * slot
    assert L.wc_fcd_workspace_size(8, 90, 298, 30, 1) == 8 * slot
    assert L.wc_fcd_workspace_size(20000, 90, 298, 30, 1) == 8 * slot       # does not grow with B
    assert L.wc_fcd_workspace_size(20000, 90, 298, 30, 3) == 8 * (90 * 4005 + 90) * 8
    for bad in ((0, 90, 298, 30, 1), (1, 2, 298, 30, 1), (1, 97, 298, 30, 1), (1, 90, 298, 299, 1),
                (1, 90, 298, 1, 1), (1, 90, 298, 30, 0), (1, 90, 5000, 2, 1)):
        assert L.wc_fcd_workspace_size(*bad) == 0, bad


def test_wc_fcd_validates_without_device_work():
    L = lib()
    err = L.wc_last_error
    assert call_fcd(L, B=0) == -1 and b"B < 1" in err() and b"wc_fcd" in err()
    assert call_fcd(L, N=2) == -1 and b"N < 3" in err()
    assert call_fcd(L, N=97) == -2 and b"96" in err()
    assert call_fcd(L, win=299) == -1 and b"win > M" in err()
    assert call_fcd(L, win=1) == -1 and b"win < 2" in err()
    assert call_fcd(L, win=0) == -1 and call_fcd(L, win=-30) == -1
    assert call_fcd(L, step=0) == -1 and b"step < 1" in err()
    assert call_fcd(L, step=-1) == -1
    assert call_fcd(L, M=4097 + 1, win=2) == -2 and b"4096" in err()         # 4097 windows
    assert call_fcd(L, M=4096 + 1, win=2, N=3, ws_bytes=1) == -3            # 4096 windows: the limit itself
    assert call_fcd(L, x=None) == -1 and b"NULL" in err()
    assert call_fcd(L, fcd=None) == -1 and b"NULL" in err()
    for name in ("x", "fcd", "winfc", "ws"):
        assert call_fcd(L, **{name: at(X, 4)}) == -1 and b"8-byte" in err(), name
    assert call_fcd(L, fcd=at(X, 8)) == -1 and b"alias" in err()
    assert call_fcd(L, winfc=at(FCD, 8)) == -1 and b"alias" in err()
    assert call_fcd(L, ws=at(X, 16)) == -1 and b"alias" in err()
    need = L.wc_fcd_workspace_size(1, 90, 298, 30, 1)
    assert call_fcd(L, ws_bytes=need - 8) == -3 and b"workspace" in err()
    assert call_fcd(L, B=20000, ws_bytes=7 * need) == -3
    assert call_fcd(L, ws=None) == -3 and b"workspace" in err()
    assert wcsde_abi(L) == 7


def test_wc_fcd_phase_validates_without_device_work():
    L = lib()
    err = L.wc_last_error
    assert call_phase(L, B=0) == -1 and b"B < 1" in err() and b"wc_fcd_phase" in err()
    assert call_phase(L, N=1) == -1 and b"N < 2" in err()
    assert call_phase(L, N=97) == -2 and b"96" in err()
    assert call_phase(L, M=0) == -1 and call_phase(L, M=-5) == -1
    assert call_phase(L, M=4097) == -2 and b"4096" in err()
    assert call_phase(L, ph=None) == -1 and b"NULL" in err()
    assert call_phase(L, fcd=None) == -1 and b"NULL" in err()
    assert call_phase(L, ph=at(X, 4)) == -1 and b"8-byte" in err()
    assert call_phase(L, fcd=at(FCD, 4)) == -1 and b"8-byte" in err()
    assert call_phase(L, fcd=at(X, 8)) == -1 and b"alias" in err()


def wcsde_abi(L):
    import os
    import re
    hdr = open(os.path.join(os.path.dirname(__file__), "..", "include", "wcsde.h")).read()
    assert re.search(r"#define WCSDE_ABI_VERSION 7\b", hdr)
    assert re.search(r"#define WC_FCD_MAX_WINDOWS 4096\b", hdr) and re.search(r"#define WC_FCD_PHASE_MAX_M 4096\b", hdr)
    for fn in ("size_t wc_fcd_workspace_size", "int wc_fcd", "int wc_fcd_phase"):
        assert re.search(rf"\b{fn}\(", hdr)
    return L.wcsde_abi_version()


# ---- the Python layers ----

def test_sigchain_fcd_refuses_before_touching_the_device():
    import torch

    from nremmodfc_amd import sigchain
    assert sigchain.FCD_MAX_WINDOWS == 4096 and sigchain.FCD_PHASE_MAX_M == 4096 and sigchain.FCD_MAX_N == 96
    ok = torch.zeros((40, 2, 5), dtype=torch.float64)
    with pytest.raises(ValueError, match="method"):
        sigchain.fcd(ok, 10, method="cosine")
    for t in (ok.float(), ok[0, 0], ok[None], ok.numpy(), None, torch.zeros((40, 5), dtype=torch.complex128)):
        with pytest.raises(TypeError, match="fcd"):
            sigchain.fcd(t, 10)
    for n in (97, 1000):
        for method, w in (("corr", 10), ("phase", None)):
            with pytest.raises(ValueError, match="96"):
                sigchain.fcd(torch.zeros((40, 1, n), dtype=torch.float64), w, method=method)
    for kw in (dict(window=None), dict(window=1), dict(window=41), dict(window=10, step=0), dict(window=10, trim=2)):
        with pytest.raises(ValueError, match="corr"):
            sigchain.fcd(ok, **kw)
    with pytest.raises(ValueError, match="N >= 3"):
        sigchain.fcd(torch.zeros((40, 1, 2), dtype=torch.float64), 10)
    with pytest.raises(ValueError, match="4096"):
        sigchain.fcd(torch.zeros((5000, 1, 3), dtype=torch.float64), 2)
    for kw in (dict(window=10), dict(step=1), dict(want_windows=True), dict(ws_bytes=1 << 20)):
        with pytest.raises(ValueError, match="phase"):
            sigchain.fcd(ok, method="phase", **kw)
    for kw in (dict(trim=-1), dict(trim=20)):
        with pytest.raises(ValueError, match="trim"):
            sigchain.fcd(ok, method="phase", **kw)
    with pytest.raises(ValueError, match="4096"):
        sigchain.fcd(torch.zeros((4100, 1, 2), dtype=torch.float64), method="phase", trim=1)


def test_fcd_ks_refuses_bad_arguments_and_runs_on_any_device():
    import torch

    from nremmodfc_amd import sigchain
    f = torch.eye(6, dtype=torch.float64)
    for t in (f.float(), f[0], torch.zeros((2, 6, 5), dtype=torch.float64), f.numpy(), None):
        with pytest.raises(TypeError, match="fcd_ks"):
            sigchain.fcd_ks(t, [0.0, 1.0])
    for lag in (0, -1, 6):
        with pytest.raises(ValueError, match="lag"):
            sigchain.fcd_ks(f, [0.0, 1.0], lag=lag)
    for emp in ([], [[0.0, 1.0]], [0.0, np.nan]):
        with pytest.raises(ValueError, match="emp_values"):
            sigchain.fcd_ks(f, emp)
    # plain torch: the host tensors of this test go the same way as device ones
    rng = np.random.default_rng(9)
    x = ref.make_input(30, 3, 4, 9, 6, 2)
    fs, _ = ref.fcd_batch(x, 6, 2)
    fs[1, 2, 5] = fs[1, 5, 2] = np.nan
    emp = rng.uniform(-1, 1, 33)
    for lag in (1, 3, 4):
        got = sigchain.fcd_ks(torch.from_numpy(fs), emp, lag).numpy()
        want = np.array([ref.fcd_ks(m, emp, lag) for m in fs])
        assert ref.deviation(got, want) <= 1e-15 and np.isnan(got[1]) == (lag <= 3)
        assert ref.deviation(sigchain.fcd_ks(torch.from_numpy(fs[2]), torch.from_numpy(emp), lag).numpy(),
                             want[2]) <= 1e-15


def test_utils_fcd_refuses_before_touching_the_device():
    from nremmodfc_amd import utils
    with pytest.raises(TypeError, match="real"):
        utils.fcd(np.zeros((40, 5), dtype=np.complex128))
    for shape in ((40,), (40, 2, 5, 1), (0, 5)):
        with pytest.raises(ValueError, match="series"):
            utils.fcd(np.zeros(shape))
    with pytest.raises(ValueError, match="method"):
        utils.fcd(np.zeros((40, 5)), method="cosine")
    with pytest.raises(ValueError, match="corr"):
        utils.fcd(np.zeros((40, 5), dtype=np.float32), window=41, device="cpu")
    with pytest.raises(ValueError, match="96"):
        utils.fcd(np.zeros((40, 97)), device="cpu")


def test_sweep_result_gains_fcd_last_with_default_none():
    import dataclasses
    import inspect

    from nremmodfc_amd import pipeline
    fields = dataclasses.fields(pipeline.SweepResult)
    assert fields[-1].name == "fcd" and fields[-1].default is None
    assert inspect.signature(pipeline.run_sweep).parameters["want_fcd"].default is None

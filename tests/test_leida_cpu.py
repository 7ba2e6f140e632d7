"""LEiDA without a GPU: tests/leida_reference.py (the numpy restatement that test_leida_gpu.py compares the
device with) equals a case counted by hand, and the closed 2 x 2 form equals np.linalg.eigh up to sign;
wc_leida_eigvec, wc_kmeans_assign, wc_kmeans_workspace_size, wc_kmeans_update and wc_state_stats validate
every argument before any device work (the pointers are fake); the sigchain and utils layers refuse bad
arguments before they touch the device; sigchain.state_kl, plain torch, equals the restatement on host tensors.
"""
import ctypes
import math
import os
import re

import numpy as np
import pytest

from tests import leida_reference as ref

A, B_, C, D, E, WS = (ctypes.c_void_p(v) for v in (1 << 40, 1 << 42, 1 << 44, 1 << 46, 1 << 48, 1 << 50))
SQ, COS = 0, 1
nan = math.nan


def lib():
    from nremmodfc_amd import _lib
    return _lib.lib()


def at(p, off):
    return ctypes.c_void_p(p.value + off)


# ---- the restatement ----

HAND = [0, 0, 1, -1, 1, 1, 0]          # K = 3: state 2 never occurs
# valid times: 6; state 0 at t = 0, 1, 6 (runs 2, 1), state 1 at t = 2, 4, 5 (runs 1, 2)
HAND_OCC = [3 / 6, 3 / 6, 0 / 6]
HAND_DWELL = [3 / 2, 3 / 2, nan]
# pairs with both ends valid: (0,0) (0,1) | (1,1) (1,0); t = 2 -> 3 and 3 -> 4 touch the -1
HAND_TRANS = [[1 / 2, 1 / 2, 0.0], [1 / 2, 1 / 2, 0.0], [nan, nan, nan]]


def test_restatement_equals_the_hand_count():
    occ, dwell, trans = ref.state_stats(np.array(HAND)[:, None], 3)
    assert ref.same(occ[0], HAND_OCC) and ref.same(dwell[0], HAND_DWELL) and ref.same(trans[0], HAND_TRANS)
    # a label that is no state counts as -1; a simulation without a valid time is NaN throughout
    occ2, dwell2, trans2 = ref.state_stats(np.array([[0, -1], [0, 5], [1, -7], [3, -1], [1, -1], [1, -1], [0, -1]]), 3)
    assert ref.same(occ2[0], HAND_OCC) and ref.same(dwell2[0], HAND_DWELL) and ref.same(trans2[0], HAND_TRANS)
    assert np.isnan(occ2[1]).all() and np.isnan(dwell2[1]).all() and np.isnan(trans2[1]).all()
    one = ref.state_stats(np.array([[1]]), 2)                   # M = 1: no pair at all
    assert ref.same(one[0][0], [0.0, 1.0]) and ref.same(one[1][0], [nan, 1.0]) and np.isnan(one[2]).all()


def test_closed_form_equals_eigh_up_to_sign():
    worst = 0.0
    for n in (2, 3, 7, 64, 90):
        ph = ref.make_phasors(40, n, n)
        v, share, gap = ref.eigvec(ph)
        cv, cshare = ref.closed_form(ph)
        assert gap.min() > 1e-6
        ratio = (ref.vec_error(cv, v) * gap / ref.EPS).max()
        worst = max(worst, ratio)
        assert ratio <= 16 and np.abs(cshare - share).max() <= 8 * ref.EPS, (n, ratio)
        assert np.abs((v * v).sum(axis=1) - 1).max() <= 1e-14
        p = (v > 0).sum(axis=1)
        assert ((2 * p < n) | ((2 * p == n) & (v.sum(axis=1) <= 0))).all()
        assert ((share >= 0.5) & (share <= 1.0)).all()
    print(f"closed form vs eigh: {worst:.2f} eps lambda1 / (lambda1 - lambda2)")
    two = np.array([[[1.0, 0.0], [0.0, 1.0]], [[0.0, 0.0], [0.0, 0.0]], [[1.0, 0.0], [np.nan, 1.0]]])
    v, share, _ = ref.eigvec(two)                               # phases pi / 2 apart; all zero; a NaN
    assert np.isnan(v).all() and share[0] == 0.5 and np.isnan(share[1]) and np.isnan(share[2])


def test_restated_kmeans_rules():
    x = np.array([[1.0, 0.0], [0.0, 2.0], [np.nan, 1.0], [0.0, 0.0]])
    cent = np.array([[1.0, 0.0], [1.0, 0.0], [0.0, 1.0], [np.nan, 0.0], [0.0, 0.0]])
    lab, dist, _ = ref.assign(x, cent, "cosine")
    assert list(lab) == [0, 2, -1, -1] and dist[0] == 0 and dist[1] == 0 and np.isnan(dist[2:]).all()
    lab, dist, _ = ref.assign(x, cent, "sqeuclidean")
    assert list(lab) == [0, 2, -1, 4] and list(dist[[0, 1, 3]]) == [0, 1, 0]
    new, count = ref.update(x[:2], [2, 2], cent[:3], "cosine")
    assert list(count) == [0, 0, 2] and (new[:2] == cent[:2]).all() and list(new[2]) == [0.5, 0.5]
    new, count = ref.update(x[:2], [1, -1], cent[:3], "sqeuclidean")
    assert list(count) == [0, 1, 0] and (new == cent[:3]).all()


# ---- the C ABI ----

def eig(L, R=5, N=90, ph=A, vec=B_, share=C):
    return L.wc_leida_eigvec(R, N, ph, vec, share, None)


def asg(L, R=5, N=90, K=5, x=A, cent=B_, metric=COS, labels=C, dist=D):
    return L.wc_kmeans_assign(R, N, K, x, cent, metric, labels, dist, None)


def upd(L, R=600, N=90, K=5, x=A, labels=B_, prev=C, metric=COS, cent=D, count=E, ws=WS, ws_bytes=None):
    if ws_bytes is None:
        ws_bytes = L.wc_kmeans_workspace_size(R, N, K, metric) or 1 << 20
    return L.wc_kmeans_update(R, N, K, x, labels, prev, metric, cent, count, ws, ws_bytes, None)


def stats(L, B=3, M=298, K=5, labels=A, occ=B_, dwell=C, trans=D):
    return L.wc_state_stats(B, M, K, labels, occ, dwell, trans, None)


def test_wc_leida_eigvec_validates_without_device_work():
    L = lib()
    err = L.wc_last_error
    assert eig(L, R=0) == -1 and b"R < 1" in err() and b"wc_leida_eigvec" in err()
    assert eig(L, R=-3) == -1
    assert eig(L, R=(1 << 40) + 1) == -2 and b"2^40" in err()
    assert eig(L, N=1) == -1 and b"N < 2" in err()
    assert eig(L, N=1025) == -2 and b"1024" in err()
    for name in ("ph", "vec", "share"):
        assert eig(L, **{name: None}) == -1 and b"NULL" in err(), name
    assert eig(L, ph=at(A, 8)) == -1 and b"16-byte" in err()
    assert eig(L, vec=at(B_, 4)) == -1 and b"aligned" in err()
    assert eig(L, share=at(C, 4)) == -1 and b"aligned" in err()
    assert eig(L, vec=at(A, 16)) == -1 and b"alias" in err()
    assert eig(L, share=at(A, 5 * 90 * 16 - 8)) == -1 and b"alias" in err()
    assert eig(L, share=at(B_, 8)) == -1 and b"alias" in err()


def test_wc_kmeans_assign_validates_without_device_work():
    L = lib()
    err = L.wc_last_error
    assert asg(L, R=0) == -1 and b"R < 1" in err() and b"wc_kmeans_assign" in err()
    assert asg(L, R=(1 << 40) + 1) == -2
    assert asg(L, N=1) == -1 and b"N < 2" in err()
    assert asg(L, N=1025) == -2 and b"1024" in err()
    assert asg(L, K=0) == -1 and b"K < 1" in err()
    assert asg(L, K=33) == -2 and b"32" in err()
    assert asg(L, metric=2) == -1 and b"metric" in err()
    assert asg(L, metric=-1) == -1
    for name in ("x", "cent", "labels", "dist"):
        assert asg(L, **{name: None}) == -1 and b"NULL" in err(), name
    for name, off in (("x", 4), ("cent", 4), ("dist", 4), ("labels", 2)):
        assert asg(L, **{name: at(dict(x=A, cent=B_, labels=C, dist=D)[name], off)}) == -1 and b"aligned" in err(), name
    assert asg(L, labels=at(A, 8)) == -1 and b"alias" in err()
    assert asg(L, dist=at(B_, 8)) == -1 and b"alias" in err()
    assert asg(L, dist=at(C, 8)) == -1 and b"alias" in err()


def test_wc_kmeans_update_validates_without_device_work():
    L = lib()
    err = L.wc_last_error
    size = L.wc_kmeans_workspace_size
    # 600 rows: 3 blocks of 256; K N doubles and K int64 a block; the rows' norms under cosine
    assert size(600, 90, 5, SQ) == 3 * (5 * 90 + 5) * 8
    assert size(600, 90, 5, COS) == 3 * (5 * 90 + 5) * 8 + 600 * 8
    assert size(256, 2, 1, SQ) == (2 + 1) * 8 and size(257, 2, 1, SQ) == 2 * (2 + 1) * 8
    for bad in ((0, 90, 5, SQ), (600, 1, 5, SQ), (600, 1025, 5, SQ), (600, 90, 0, SQ), (600, 90, 33, SQ),
                (600, 90, 5, 2), ((1 << 40) + 1, 90, 5, SQ)):
        assert size(*bad) == 0, bad
    assert upd(L, R=0) == -1 and b"R < 1" in err() and b"wc_kmeans_update" in err()
    assert upd(L, N=1) == -1 and upd(L, N=1025) == -2
    assert upd(L, K=0) == -1 and upd(L, K=33) == -2 and b"32" in err()
    assert upd(L, metric=7) == -1 and b"metric" in err()
    for name in ("x", "labels", "prev", "cent", "count"):
        assert upd(L, **{name: None}) == -1 and b"NULL" in err(), name
    ptrs = dict(x=A, labels=B_, prev=C, cent=D, count=E, ws=WS)
    for name in ptrs:
        assert upd(L, **{name: at(ptrs[name], 2 if name == "labels" else 4)}) == -1 and b"aligned" in err(), name
    assert upd(L, cent=at(A, 8)) == -1 and b"alias" in err()
    assert upd(L, cent=at(C, 8)) == -1 and b"alias" in err()              # the previous centroids are read last
    assert upd(L, count=at(B_, 8)) == -1 and b"alias" in err()
    assert upd(L, count=at(D, 8)) == -1 and b"alias" in err()
    assert upd(L, ws=at(A, 16)) == -1 and b"workspace" in err()
    assert upd(L, ws=at(D, 16)) == -1 and b"workspace" in err()
    need = size(600, 90, 5, COS)
    assert upd(L, ws_bytes=need - 8) == -3 and b"workspace" in err()
    assert upd(L, ws_bytes=size(600, 90, 5, SQ)) == -3                     # cosine needs the norms too
    assert upd(L, ws=None) == -3 and b"workspace" in err()


def test_wc_state_stats_validates_without_device_work():
    L = lib()
    err = L.wc_last_error
    assert stats(L, B=0) == -1 and b"B < 1" in err() and b"wc_state_stats" in err()
    assert stats(L, M=0) == -1 and b"M < 1" in err()
    assert stats(L, K=0) == -1 and b"K < 1" in err()
    assert stats(L, K=33) == -2 and b"32" in err()
    for name in ("labels", "occ", "dwell", "trans"):
        assert stats(L, **{name: None}) == -1 and b"NULL" in err(), name
    for name, p, off in (("labels", A, 2), ("occ", B_, 4), ("dwell", C, 4), ("trans", D, 4)):
        assert stats(L, **{name: at(p, off)}) == -1 and b"aligned" in err(), name
    assert stats(L, occ=at(A, 8)) == -1 and b"alias" in err()
    assert stats(L, dwell=at(B_, 8)) == -1 and b"alias" in err()
    assert stats(L, trans=at(C, 8)) == -1 and b"alias" in err()


def test_header_declares_the_entry_points_and_abi_7():
    hdr = open(os.path.join(os.path.dirname(__file__), "..", "include", "wcsde.h")).read()
    assert re.search(r"#define WCSDE_ABI_VERSION 7\b", hdr)
    assert re.search(r"#define WC_KMEANS_UPDATE_BLOCK 256\b", hdr)
    assert re.search(r"WC_KMEANS_SQEUCLIDEAN = 0, WC_KMEANS_COSINE = 1", hdr)
    for fn in ("int wc_leida_eigvec", "int wc_kmeans_assign", "size_t wc_kmeans_workspace_size", "int wc_kmeans_update",
               "int wc_state_stats"):
        assert re.search(rf"\b{fn}\(", hdr), fn
    assert lib().wcsde_abi_version() == 7


# ---- the Python layers ----

def test_sigchain_refuses_before_touching_the_device():
    import torch

    from nremmodfc_amd import sigchain
    assert sigchain.LEIDA_MAX_N == 1024 and sigchain.KMEANS_MAX_K == 32 and sigchain.KMEANS_UPDATE_BLOCK == 256
    f64 = torch.float64
    ok = torch.zeros((40, 2, 5), dtype=f64)
    for t in (ok.float(), ok[0, 0], ok[None], ok.numpy(), None):
        with pytest.raises(TypeError, match="leida"):
            sigchain.leida(t)
    for n in (1, 1025):
        with pytest.raises(ValueError, match="1024"):
            sigchain.leida(torch.zeros((40, 1, n), dtype=f64))
    for trim in (-1, 20):
        with pytest.raises(ValueError, match="trim"):
            sigchain.leida(ok, trim=trim)
    ph = torch.zeros((40, 2, 5, 2), dtype=f64)
    for t in (ph.float(), ph[0, 0], ph[..., :1], ph.numpy(), None):
        with pytest.raises(TypeError, match="leida_from_phasors"):
            sigchain.leida_from_phasors(t)
    for n in (1, 1025):
        with pytest.raises(ValueError, match="1024"):
            sigchain.leida_from_phasors(torch.zeros((4, n, 2), dtype=f64))
    cent = torch.zeros((3, 5), dtype=f64)
    for fn in (sigchain.kmeans_assign, sigchain.kmeans, sigchain.leida_states):
        with pytest.raises(ValueError, match="metric"):
            fn(ok, cent, metric="manhattan")
        for t in (ok.float(), ok[0, 0], ok.numpy(), None):
            with pytest.raises(TypeError, match="x must be"):
                fn(t, cent)
        for c in (cent.float(), cent[0], cent.numpy()):
            with pytest.raises(TypeError, match="centroids"):
                fn(ok, c)
        with pytest.raises(ValueError, match="nodes"):
            fn(ok, torch.zeros((3, 6), dtype=f64))
        for k in (0, 33):
            with pytest.raises(ValueError, match="32"):
                fn(ok, torch.zeros((k, 5), dtype=f64))
        for n in (1, 1025):
            with pytest.raises(ValueError, match="1024"):
                fn(torch.zeros((4, n), dtype=f64), torch.zeros((2, n), dtype=f64))
    for k in (0, 33):
        with pytest.raises(ValueError, match="32"):
            sigchain.kmeans(ok, k)
    with pytest.raises(ValueError, match="n_init"):
        sigchain.kmeans(ok, 3, n_init=0)
    with pytest.raises(ValueError, match="n_init"):
        sigchain.kmeans(ok, cent, n_init=2)
    with pytest.raises(ValueError, match="max_iter"):
        sigchain.kmeans(ok, cent, max_iter=-1)
    with pytest.raises(TypeError, match="kmeans"):
        sigchain.kmeans(ok.float(), 3)
    for lab in (torch.zeros((40, 2), dtype=torch.int64), torch.zeros((40,), dtype=torch.int32), None):
        with pytest.raises(TypeError, match="labels"):
            sigchain.kmeans_update(ok, lab, cent)
    lab = torch.zeros((40, 2), dtype=torch.int32)
    for t in (lab.long(), lab[None], lab.numpy(), None):
        with pytest.raises(TypeError, match="state_stats"):
            sigchain.state_stats(t, 3)
    for k in (0, 33):
        with pytest.raises(ValueError, match="32"):
            sigchain.state_stats(lab, k)


def test_utils_leida_refuses_before_touching_the_device():
    from nremmodfc_amd import utils
    x = np.zeros((40, 5))
    with pytest.raises(TypeError, match="real"):
        utils.leida(x.astype(np.complex128), 2.0, None)
    for shape in ((40,), (40, 2, 5, 1), (0, 5)):
        with pytest.raises(ValueError, match="series"):
            utils.leida(np.zeros(shape), 2.0, None)
    with pytest.raises(ValueError, match="freqs"):
        utils.leida(x, 2.0, [0.04])
    with pytest.raises(ValueError, match="metric"):
        utils.leida(x, 2.0, None, metric="manhattan")
    with pytest.raises(ValueError, match="not both"):
        utils.leida(x, 2.0, None, centroids=np.zeros((2, 5)), k=2)
    for k in (0, 33):
        with pytest.raises(ValueError, match="32"):
            utils.leida(x, 2.0, None, k=k)
    for cent in (np.zeros((2, 6)), np.zeros(5), np.zeros((33, 5)), np.zeros((0, 5))):
        with pytest.raises(ValueError, match="centroids"):
            utils.leida(x, 2.0, None, centroids=cent)
    for bad in (np.zeros((40, 1)), np.zeros((40, 1025))):
        with pytest.raises(ValueError, match="1024"):
            utils.leida(bad, 2.0, None)
    for trim in (-1, 20):
        with pytest.raises(ValueError, match="trim"):
            utils.leida(x.astype(np.float32), 2.0, None, trim=trim)


def test_state_kl_equals_the_restatement_on_host_tensors():
    import torch

    from nremmodfc_amd import sigchain
    rng = np.random.default_rng(5)
    p = rng.uniform(0.05, 1, (6, 4))
    p[1, 2] = 0.0                                                # a zero where q has mass: +inf
    p[2] = np.nan                                                # a simulation without a valid time
    p[3] = [0.5, 0.5, 0.0, 0.0]
    p[:2] /= p[:2].sum(axis=1, keepdims=True)
    p[4:] /= p[4:].sum(axis=1, keepdims=True)
    q = np.array([0.1, 0.2, 0.3, 0.4])
    got = sigchain.state_kl(torch.from_numpy(p), q).numpy()
    want = np.array([ref.state_kl(row, q) for row in p])
    assert got[1] == np.inf and np.isnan(got[2]) and got[3] == np.inf and np.isfinite(got[[0, 4, 5]]).all()
    fin = np.isfinite(want)
    # 8 terms a (log a - log b) of size <= 3 a row, each within a few ulps of the other library's
    assert ref.same(got[~fin], want[~fin]) and np.abs(got[fin] - want[fin]).max() <= 1e-14
    q0 = np.array([0.5, 0.5, 0.0, 0.0])                          # zeros on both sides add nothing
    assert float(sigchain.state_kl(torch.from_numpy(p[3]), torch.from_numpy(q0))) == 0.0 == ref.state_kl(p[3], q0)
    assert float(sigchain.state_kl(torch.from_numpy(p[0]), q0)) == np.inf
    for t in (torch.from_numpy(p).float(), torch.zeros((2, 2, 4), dtype=torch.float64), p, None):
        with pytest.raises(TypeError, match="state_kl"):
            sigchain.state_kl(t, q)
    for bad in (q[:3], q[None], []):
        with pytest.raises(ValueError, match="state_kl"):
            sigchain.state_kl(torch.from_numpy(p), bad)

"""Null models without a GPU: the numpy restatement (nullmodel_reference) against the golden outputs of
the reference's own randmio_und_signed, null_model_und_sign and participation_coef_norm
(tests/golden/make_nullmodel_golden.py) -- w0 and wr as the same bits, eff and draws equal, r, mean
and std within 1e-12 --, the invariants the restatement must keep, and every refusal of
wc_graph_rewire, wc_graph_null_model and the Python layers above them, all raised before any device
work."""
import ctypes
import functools
import inspect

import numpy as np
import pytest

from tests import louvain_reference as lr
from tests import nullmodel_reference as nr
from tests.centrality_reference import deviation_abs

EINVAL, EUNSUPPORTED = -1, -2
NULL_MODEL = nr.null_model          # test_restatement_gives_the_reference_participation patches nr's name


@functools.lru_cache(maxsize=None)
def inputs():
    return nr.inputs()


@functools.lru_cache(maxsize=None)
def golden():
    return nr.load_golden()


@functools.lru_cache(maxsize=None)
def restated(name, seed, negative="reference"):
    """One run of the restatement on a golden case at the defaults, shared among the tests."""
    w0, r, info = NULL_MODEL(inputs()[name], seed, 5, 10, negative)
    w0.setflags(write=False)
    return w0, r, info


def test_philox_over_arrays_is_the_scalar_one():
    steps = [0, 1, 77, (1 << 32) + 5, (1 << 40) + 9]
    for seed in (0, 3, (1 << 63) + 12345):
        many = nr.philox_many(steps, nr.QUAD_REWIRE, seed)
        for row, t in zip(many, steps):
            want = lr.philox4x32_10((t & 0xFFFFFFFF, ((t >> 32) << 16) | nr.QUAD_REWIRE, seed & 0xFFFFFFFF, seed >> 32))
            assert tuple(int(v) for v in row) == want


@pytest.mark.parametrize("name", [c for c, _ in nr.GOLDEN_CASES])
def test_restatement_gives_the_reference_outputs(name):
    g = golden()
    for k, seed in enumerate(g[f"{name}/seeds"]):
        w0, r, info = restated(name, int(seed))
        assert nr.uptri(w0).tobytes() == g[f"{name}/w0"][k].tobytes(), (name, seed)
        assert (w0 == w0.T).all() and not np.diag(w0).any()
        assert info == (int(g[f"{name}/eff"][k]), int(g[f"{name}/draws"][k]), 0)
        dev = deviation_abs(np.array(r), g[f"{name}/r"][k])
        print(f"{name} seed {seed}: r deviation {dev:.1e}")
        assert dev <= 1e-12


def test_restatement_gives_the_reference_rewiring():
    g = golden()
    wr, info = nr.rewire(inputs()["corr24"], int(g["rewire/corr24/seed"]), 5)
    assert nr.uptri(wr).tobytes() == g["rewire/corr24/wr"].tobytes()
    assert info == (int(g["rewire/corr24/eff"]), int(g["rewire/corr24/draws"]), 0)


def test_restatement_gives_the_reference_participation(monkeypatch):
    g = golden()
    # participation_norm through the shared runs: seeds 0 and 1 of fc_thr are golden cases themselves
    monkeypatch.setattr(nr, "null_model", lambda W, seed, bs, period, negative: restated("fc_thr", seed, negative))
    mean, std = nr.participation_norm(inputs()["fc_thr"], g["pnorm/fc_thr/ci"], nr.GOLDEN_REPS, None, 5, 10, "reference")
    dm, ds = deviation_abs(mean, g["pnorm/fc_thr/mean"]), deviation_abs(std, g["pnorm/fc_thr/std"])
    print(f"participation: mean deviation {dm:.1e}, std deviation {ds:.1e}")
    assert dm <= 1e-12 and ds <= 1e-12


def degrees(W):
    return (W > 0).sum(axis=0), (W < 0).sum(axis=0)


@pytest.mark.parametrize("n", [4, 5, 7, 24])
def test_rewiring_keeps_every_degree_per_sign(n):
    W = nr.signed(n)
    wr, (eff, draws, status) = nr.rewire(W, n, 2)
    assert status == 0 and draws >= eff
    for got, want in zip(degrees(wr), degrees(W)):
        assert (got == want).all()
    assert (wr == wr.T).all() and not np.diag(wr).any()
    assert np.sort(nr.uptri(wr)).tobytes() == np.sort(nr.uptri(W)).tobytes()     # the weights only move
    if n >= 24:
        assert eff > 0 and (wr != W).any()


@pytest.mark.parametrize("period", [0, 1, 10, 64])
def test_bct_mode_keeps_degrees_and_the_weights_per_sign(period):
    W = nr.signed(24)
    w0, r, info = nr.null_model(W, 5, 1, period, "bct")
    assert info[2] == 0
    for got, want in zip(degrees(w0), degrees(W)):
        assert (got == want).all()
    assert np.sort(nr.uptri(w0)).tobytes() == np.sort(nr.uptri(W)).tobytes()
    assert np.isfinite(r).all()


def test_reference_mode_loses_the_negative_weights():
    """The documented behaviour of the reference's negative half: it writes -Wv of negative Wv."""
    W = inputs()["corr24"]
    assert (W < 0).sum() == 2 * 65
    w0, r, info = restated("corr24", 0)
    assert (w0 < 0).sum() == 0 and (w0 > 0).sum() == 2 * 276 and np.isnan(r[1])
    assert np.sort(nr.uptri(w0)).tobytes() == np.sort(np.abs(nr.uptri(W))).tobytes()
    bct, rb, _ = nr.null_model(W, 0, 5, 10, "bct")
    assert (bct[bct > 0] == w0[bct > 0]).all() and (bct > 0).sum() == 2 * 211      # the positive half is the same
    assert (bct < 0).sum() == 2 * 65 and np.isfinite(rb[1])


def test_statuses_of_the_restatement():
    W = nr.signed(8)
    bad = W.copy()
    bad[2, 5] += 1e-9
    assert nr.null_model(bad, 0, 1)[2] == (0, 0, 2) and nr.rewire(bad, 0, 1)[1] == (0, 0, 2)
    bad[3, 3] = np.inf
    assert nr.null_model(bad, 0, 1)[2] == (0, 0, 3) and np.isnan(nr.null_model(bad, 0, 1)[0]).all()
    full = np.abs(W) + 0.1
    np.fill_diagonal(full, 0.0)
    assert nr.null_model(full, 0, 5)[2] == (0, 0, 0)        # fully positive: no rewiring (:2268)


# ---- refusals of the entry points, before any device work (fake pointers, as test_arg_checks_cpu.py) ----

def P(k):
    return ctypes.c_void_p((k + 1) << 44)


B, R, N = 2, 3, 90
W_BYTES, OUT_BYTES = B * N * N * 8, B * R * N * N * 8
SLOT = 4 * N * (N - 1)
ATTEMPTS = {90: 46, 5: 3, 7: 5}          # round(N / 2) + 1, half to even: round(2.5) = 2, round(3.5) = 4
REWIRE = dict(B=B, R=R, N=N, w=P(0), bin_swaps=5, seeds=P(1), wr=P(2), info=P(3), workspace=P(4), ws_bytes=6 * SLOT)
NULL = dict(B=B, R=R, N=N, w=P(0), bin_swaps=5, period=10, neg_mode=1, seeds=P(1), w0=P(2), r=P(3), info=P(4),
            workspace=P(5), ws_bytes=6 * SLOT)


def off(p, nbytes):
    return ctypes.c_void_p(p.value + nbytes)


def most_swaps(n):
    """The largest bin_swaps whose iterations times attempts stay below 2^31."""
    return ((1 << 31) - 1) // (n * (n - 1) // 2 * ATTEMPTS[n])


def common(base, out):
    return [
        (dict(B=0), EINVAL, None), (dict(R=0), EINVAL, None), (dict(N=3), EINVAL, None), (dict(N=97), EUNSUPPORTED, None),
        (dict(B=1 << 16, R=1 << 15), EINVAL, None), (dict(bin_swaps=-1), EINVAL, None),
        *[(dict(N=n, bin_swaps=most_swaps(n) + 1), EINVAL, None) for n in ATTEMPTS],
        (dict(w=None), EINVAL, None), (dict(seeds=None), EINVAL, None), (dict(workspace=None), EINVAL, None),
        (dict(ws_bytes=SLOT - 1), EINVAL, None), (dict(ws_bytes=0), EINVAL, None), ({out: None}, EINVAL, None),
        (dict(w=off(base["w"], 4)), EINVAL, "w"), (dict(seeds=off(base["seeds"], 4)), EINVAL, "seeds"),
        ({out: off(base[out], 4)}, EINVAL, out), (dict(info=off(base["info"], 2)), EINVAL, "info"),
        (dict(workspace=off(base["workspace"], 4)), EINVAL, "workspace"),
        ({out: off(base["w"], W_BYTES - 8)}, EINVAL, out), ({out: off(base["seeds"], R * 8 - 8)}, EINVAL, out),
        (dict(info=off(base[out], OUT_BYTES - 4)), EINVAL, "info"),
        (dict(workspace=off(base["w"], W_BYTES - 8)), EINVAL, "workspace"),
        (dict(workspace=off(base[out], -6 * SLOT + 8)), EINVAL, "workspace"),
    ]


REWIRE_ROWS = common(REWIRE, "wr")
NULL_ROWS = common(NULL, "w0") + [
    (dict(period=-1), EINVAL, None), (dict(period=65), EUNSUPPORTED, None), (dict(neg_mode=2), EINVAL, None),
    (dict(neg_mode=-1), EINVAL, None), (dict(r=off(NULL["r"], 4)), EINVAL, "r"),
    (dict(r=off(NULL["w0"], OUT_BYTES - 8)), EINVAL, "r"), (dict(r=off(NULL["seeds"], R * 8 - 8)), EINVAL, "r"),
    (dict(info=off(NULL["r"], B * R * 16 - 4)), EINVAL, "info"),
]


@pytest.mark.parametrize("fn,base,table", [("wc_graph_rewire", REWIRE, REWIRE_ROWS),
                                           ("wc_graph_null_model", NULL, NULL_ROWS)], ids=["rewire", "null_model"])
def test_entry_points_refuse_before_any_device_work(fn, base, table):
    from nremmodfc_amd import _lib
    L = _lib.lib()
    assert L.wcsde_abi_version() == 7
    for over, code, names in table:
        kw = dict(base, **over)
        assert getattr(L, fn)(*kw.values(), None) == code, (fn, over)
        msg = L.wc_last_error()
        assert msg.startswith(fn.encode() + b": "), (fn, over, msg)
        if names:
            assert names.encode() in msg, (fn, over, msg)


def test_the_largest_bin_swaps_passes_the_iteration_check():
    """One below each refused bin_swaps is refused later, for its workspace: the bound is exact."""
    from nremmodfc_amd import _lib
    L = _lib.lib()
    for n in ATTEMPTS:
        kw = dict(NULL, N=n, bin_swaps=most_swaps(n), ws_bytes=0)
        assert L.wc_graph_null_model(*kw.values(), None) == EINVAL
        assert b"ws_bytes" in L.wc_last_error()


def test_slot_bytes():
    from nremmodfc_amd import _lib, nullmodel
    L = _lib.lib()
    for n in (4, 5, 24, 90, 96):
        assert L.wc_graph_null_model_slot_bytes(n) == nullmodel.null_model_slot_bytes(n) == 4 * n * (n - 1)
    assert L.wc_graph_null_model_slot_bytes(3) == 0 and L.wc_graph_null_model_slot_bytes(97) == 0


# ---- refusals of the Python layers ----

def test_batch_api_refuses_before_the_device():
    import torch

    from nremmodfc_amd import nullmodel
    w = torch.zeros((2, 8, 8), dtype=torch.float64)
    cases = [
        (nullmodel.graph_null_model, dict(negative="matlab"), ValueError), (nullmodel.graph_null_model, dict(wei_freq=-0.1), ValueError),
        (nullmodel.graph_null_model, dict(wei_freq=0.01), ValueError), (nullmodel.graph_null_model, dict(wei_freq="x"), ValueError),
        (nullmodel.graph_null_model, dict(bin_swaps=-1), ValueError), (nullmodel.graph_null_model, dict(bin_swaps=1.5), ValueError),
        (nullmodel.graph_null_model, dict(bin_swaps=1 << 30), ValueError), (nullmodel.graph_null_model, dict(seeds=[]), ValueError),
        (nullmodel.graph_null_model, dict(seeds=-1), ValueError), (nullmodel.graph_null_model, dict(ws_bytes=8), ValueError),
        (nullmodel.graph_rewire, dict(bin_swaps=-1), ValueError), (nullmodel.graph_rewire, dict(seeds=1.5), ValueError),
        (nullmodel.graph_rewire, dict(ws_bytes=True), ValueError),
        (nullmodel.participation_norm, dict(ci=np.zeros(8, dtype=np.int64), reps=0), ValueError),
        (nullmodel.participation_norm, dict(ci=np.zeros(8, dtype=np.int64), reps=4, seeds=[1, 2]), ValueError),
        (nullmodel.participation_norm, dict(ci=np.zeros(8, dtype=np.int64), max_bytes=0), ValueError),
        (nullmodel.participation_norm, dict(ci=np.zeros(8, dtype=np.int64), negative="x"), ValueError),
    ]
    for fn, kw, exc in cases:
        with pytest.raises(exc, match=fn.__name__):
            fn(w, **kw)
    for fn in (nullmodel.graph_null_model, nullmodel.graph_rewire):
        with pytest.raises(ValueError, match="four distinct nodes"):
            fn(torch.zeros((3, 3), dtype=torch.float64))
        with pytest.raises(TypeError):
            fn(torch.zeros((8, 8), dtype=torch.float32))
        with pytest.raises(TypeError):
            fn(np.zeros((8, 8)))
    assert nullmodel.period_of("x", 0.1) == 10 and nullmodel.period_of("x", 0) == 0 and nullmodel.period_of("x", 1) == 1
    assert nullmodel.period_of("x", 0.4) == 2 and nullmodel.period_of("x", 1 / 64) == 64      # np.round: 2.5 -> 2


def test_facades_have_the_reference_signatures_and_refuse():
    from nremmodfc_amd import graph_utils as gu
    assert list(inspect.signature(gu.randmio_und_signed).parameters) == ["R", "itr", "seed"]
    sig = inspect.signature(gu.null_model_und_sign)
    assert list(sig.parameters) == ["W", "bin_swaps", "wei_freq", "seed"]
    assert (sig.parameters["bin_swaps"].default, sig.parameters["wei_freq"].default, sig.parameters["seed"].default) == (5, .1, None)
    sig = inspect.signature(gu.participation_coef_norm)
    assert list(sig.parameters) == ["W", "ci", "degree", "BA_iters"]
    assert (sig.parameters["degree"].default, sig.parameters["BA_iters"].default) == ("undirected", 100)
    W = nr.signed(8)
    asym = W.copy()
    asym[1, 2] += 1e-12
    with pytest.raises(TypeError, match="Input must be undirected"):
        gu.null_model_und_sign(asym)
    with pytest.raises(TypeError, match="Input must be undirected"):
        gu.participation_coef_norm(asym, np.arange(8) % 2)
    with pytest.raises(ValueError, match="4 <= N <= 96"):
        gu.null_model_und_sign(W[:3, :3])
    with pytest.raises(ValueError, match="4 <= N <= 96"):
        gu.randmio_und_signed(np.zeros((97, 97)), 1)
    with pytest.raises(ValueError, match="N x N"):
        gu.randmio_und_signed(np.zeros((2, 8, 8)), 1)
    with pytest.raises(ValueError, match="itr"):
        gu.randmio_und_signed(W, -1)
    with pytest.raises(ValueError, match="degree"):
        gu.participation_coef_norm(W, np.arange(8) % 2, degree="both")
    with pytest.raises(ValueError, match="one label per node"):
        gu.participation_coef_norm(W, np.arange(7))

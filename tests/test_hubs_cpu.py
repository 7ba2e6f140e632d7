"""Rich club, assortativity and s-core without a GPU: the numpy restatement (hubs_reference) against
the golden outputs of the reference's own rich_club_wu, rich_club_wd, rich_club_bu, rich_club_bd,
assortativity_wei, assortativity_bin and score_wu (tests/golden/make_hubs_golden.py) -- NaN patterns,
nk, sn and the cores exactly, fp64 values within 1e-12 of max(1, |want|) --, and every refusal of
wc_graph_rich_club, wc_graph_assortativity, wc_graph_score and the Python layers above them, all raised
before any device work."""
import ctypes
import functools
import inspect

import numpy as np
import pytest

from tests import hubs_reference as hr
from tests.centrality_reference import deviation_abs

EINVAL, EUNSUPPORTED = -1, -2
TOL = 1e-12


@functools.lru_cache(maxsize=None)
def inputs():
    return hr.golden_inputs()


@functools.lru_cache(maxsize=None)
def golden():
    return hr.load_golden()


@pytest.mark.parametrize("name", hr.RICH_VALUE_CASES + hr.RICH_NAN_CASES + hr.RICH_SIGNED_CASES + hr.RICH_DIRECTED_CASES)
def test_restatement_gives_the_reference_rich_club(name):
    g = golden()
    mine = hr.rich_club(inputs()[name], name in hr.RICH_DIRECTED_CASES)
    m = mine["maxdeg"]
    assert m == len(g[f"rich/{name}/rw"]) == len(g[f"rich/{name}/nk"])
    assert (mine["nk"][:m] == g[f"rich/{name}/nk"]).all()
    for key in ("rw", "rb", "ek"):
        d = deviation_abs(mine[key][:m], g[f"rich/{name}/{key}"])
        print(f"{name} {key}: deviation {d:.1e}")
        assert d <= TOL
    finite = int(np.isfinite(g[f"rich/{name}/rw"]).sum())
    if name in hr.RICH_NAN_CASES:
        assert finite == 0
    if name in hr.RICH_VALUE_CASES:
        assert 2 * finite >= m
    # past the largest degree nothing is kept: what an explicit klevel there gives
    assert np.isnan(mine["rw"][m:]).all() and np.isnan(mine["rb"][m:]).all() and not mine["nk"][m:].any()


def test_restatement_gives_the_reference_past_the_largest_degree():
    g = golden()
    mine = hr.rich_club(inputs()["pendant12"], False, 12)
    assert mine["maxdeg"] == 8 and (mine["nk"] == g["rich/pendant12/k12/nk"]).all()
    for key in ("rw", "rb", "ek"):
        assert deviation_abs(mine[key], g[f"rich/pendant12/k12/{key}"]) <= TOL
    assert np.isnan(g["rich/pendant12/k12/rw"][8:]).all()


@pytest.mark.parametrize("name", hr.ASSORT_CASES)
def test_restatement_gives_the_reference_assortativity(name):
    g = golden()
    for flag in range(5):
        wei, bin_ = hr.assortativity(inputs()[name], flag)
        d = max(deviation_abs(wei, g[f"assort/{name}/wei"][flag]), deviation_abs(bin_, g[f"assort/{name}/bin"][flag]))
        print(f"{name} flag {flag}: deviation {d:.1e}, margins {g[f'assort/{name}/margin'][flag]}")
        assert d <= TOL
        for col, key in enumerate(("wei", "bin")):     # a value only where the quotient is one
            assert g[f"assort/{name}/margin"][flag, col] >= 1e-6 or np.isnan(g[f"assort/{name}/{key}"][flag])


def test_flag_4_of_the_strengths_is_flag_2_as_the_reference_is_written():
    g = golden()
    assert g["assort/dir24/wei"][4] == g["assort/dir24/wei"][2] != g["assort/dir24/wei"][1]
    assert g["assort/dir24/bin"][4] != g["assort/dir24/bin"][2]
    W = inputs()["dir24"]
    assert hr.assortativity(W, 4)[0] == hr.assortativity(W, 2)[0]
    assert np.isnan(g["assort/ring12/bin"]).all() and np.isnan(hr.assortativity(hr.ring(12), 0)[1])


@pytest.mark.parametrize("name", hr.SCORE_CASES)
def test_restatement_gives_the_reference_score(name):
    g = golden()
    W = inputs()[name]
    for k, s in enumerate(g[f"score/{name}/s"]):
        trace = {}
        member, sn, rounds = hr.score(W, float(s), trace)
        core = hr.core_matrix(W, member)
        assert trace["gap"] > 1e-9                      # no comparison str < s is a matter of rounding
        assert sn == g[f"score/{name}/sn"][k] and core.sum() == g[f"score/{name}/sum"][k]
        alive = (core != 0).any(axis=0) | (core != 0).any(axis=1)
        assert (alive == g[f"score/{name}/alive"][k].astype(bool)).all()
    assert [int(v) for v in g["score/fc_thr/sn"]] == [81, 54, 21, 0]


def test_column_sums_are_numpys():
    """np.sum(axis=0) of a C-ordered matrix adds a column up in row order: the comparisons are the reference's."""
    for n in (5, 90, 96):
        W = hr.sparse_graph(n) * 1e3 + hr.signed_graph(n)
        assert hr.column_sums(W).tobytes() == np.sum(W, axis=0).tobytes()


# ---- refusals of the entry points, before any device work (fake pointers, as test_arg_checks_cpu.py) ----

def P(k):
    return ctypes.c_void_p((k + 1) << 44)


def off(p, nbytes):
    return ctypes.c_void_p(p.value + nbytes)


B, N, K, S = 2, 90, 90, 4
W_BYTES, CURVE, NK = B * N * N * 8, B * K * 8, B * K * 4
RICH = dict(B=B, N=N, w=P(0), directed=0, K=K, rw=P(1), rb=P(2), nk=P(3), ek=P(4), maxdeg=P(5))
ASSORT = dict(B=B, N=N, w=P(0), flag=0, r_wei=P(1), r_bin=P(2))
SCORE = dict(B=B, N=N, S=S, w=P(0), s=P(1), member=P(2), sn=P(3), rounds=P(4))


def shapes(outs):
    return [(dict(B=0), EINVAL, "B < 1"), (dict(B=-1), EINVAL, "B < 1"), (dict(N=1), EINVAL, "N < 2"),
            (dict(N=97), EUNSUPPORTED, "N = 97 > 96"), (dict(w=None), EINVAL, "w is NULL"),
            ({o: None for o in outs}, EINVAL, "every output is NULL"), (dict(w=off(P(0), 4)), EINVAL, "w must be 8-byte")]


RICH_ROWS = shapes(("rw", "rb", "nk", "ek", "maxdeg")) + [
    (dict(K=0), EINVAL, "K = 0"), (dict(K=91), EINVAL, "K = 91, must be in [1, 90]"),
    (dict(directed=1, K=181), EINVAL, "K = 181, must be in [1, 180]"), (dict(N=2, K=3), EINVAL, "K = 3"),
    (dict(rw=off(RICH["rw"], 4)), EINVAL, "rw must be 8-byte"), (dict(rb=off(RICH["rb"], 4)), EINVAL, "rb must be 8-byte"),
    (dict(ek=off(RICH["ek"], 4)), EINVAL, "ek must be 8-byte"), (dict(nk=off(RICH["nk"], 2)), EINVAL, "nk must be 4-byte"),
    (dict(maxdeg=off(RICH["maxdeg"], 2)), EINVAL, "maxdeg must be 4-byte"),
    (dict(rw=off(RICH["w"], W_BYTES - 8)), EINVAL, "rw must not alias w"),
    (dict(maxdeg=off(RICH["w"], -4)), EINVAL, "maxdeg must not alias w"),
    (dict(rb=off(RICH["rw"], CURVE - 8)), EINVAL, "rb must not alias rw"),
    (dict(nk=off(RICH["rb"], -NK + 4)), EINVAL, "nk must not alias rb"),
    (dict(ek=off(RICH["nk"], NK - 8)), EINVAL, "ek must not alias nk"),
    (dict(maxdeg=off(RICH["ek"], CURVE - 4)), EINVAL, "maxdeg must not alias ek"),
    (dict(rw=None, maxdeg=off(RICH["rb"], 0)), EINVAL, "maxdeg must not alias rb"),
]
ASSORT_ROWS = shapes(("r_wei", "r_bin")) + [
    (dict(flag=-1), EINVAL, "flag = -1"), (dict(flag=5), EINVAL, "flag = 5"),
    (dict(r_wei=off(ASSORT["r_wei"], 4)), EINVAL, "r_wei must be 8-byte"),
    (dict(r_bin=off(ASSORT["r_bin"], 4)), EINVAL, "r_bin must be 8-byte"),
    (dict(r_wei=off(ASSORT["w"], W_BYTES - 8)), EINVAL, "r_wei must not alias w"),
    (dict(r_wei=None, r_bin=off(ASSORT["w"], 0)), EINVAL, "r_bin must not alias w"),
    (dict(r_bin=off(ASSORT["r_wei"], 8)), EINVAL, "r_bin must not alias r_wei"),
]
SCORE_ROWS = shapes(("member", "sn", "rounds")) + [
    (dict(S=0), EINVAL, "S < 1"), (dict(B=1 << 16, S=1 << 15), EINVAL, "2^31 cores or more"), (dict(s=None), EINVAL, "s is NULL"),
    (dict(s=off(SCORE["s"], 4)), EINVAL, "s must be 8-byte"), (dict(member=off(SCORE["member"], 2)), EINVAL, "member must be 4-byte"),
    (dict(sn=off(SCORE["sn"], 2)), EINVAL, "sn must be 4-byte"), (dict(rounds=off(SCORE["rounds"], 1)), EINVAL, "rounds must be 4-byte"),
    (dict(member=off(SCORE["w"], W_BYTES - 4)), EINVAL, "member must not alias w"),
    (dict(sn=off(SCORE["s"], B * S * 8 - 4)), EINVAL, "sn must not alias s"),
    (dict(rounds=off(SCORE["s"], -B * S * 4 + 4)), EINVAL, "rounds must not alias s"),
    (dict(sn=off(SCORE["member"], B * S * N * 4 - 4)), EINVAL, "sn must not alias member"),
    (dict(rounds=off(SCORE["sn"], B * S * 4 - 4)), EINVAL, "rounds must not alias sn"),
    (dict(member=None, sn=None, rounds=off(SCORE["w"], 0)), EINVAL, "rounds must not alias w"),
]


@pytest.mark.parametrize("fn,base,table", [("wc_graph_rich_club", RICH, RICH_ROWS), ("wc_graph_assortativity", ASSORT, ASSORT_ROWS),
                                           ("wc_graph_score", SCORE, SCORE_ROWS)], ids=["rich_club", "assortativity", "score"])
def test_entry_points_refuse_before_any_device_work(fn, base, table):
    from nremmodfc_amd import _lib
    L = _lib.lib()
    assert L.wcsde_abi_version() == 7
    for over, code, text in table:
        kw = dict(base, **over)
        assert getattr(L, fn)(*kw.values(), None) == code, (fn, over, L.wc_last_error())
        msg = L.wc_last_error()
        assert msg.startswith(fn.encode() + b": ") and text.encode() in msg, (fn, over, msg)


# ---- refusals of the Python layers ----

def test_batch_api_refuses_before_the_device():
    import torch

    from nremmodfc_amd import hubs
    w = torch.zeros((2, 8, 8), dtype=torch.float64)
    one = torch.zeros((8, 8), dtype=torch.float64)
    cases = [
        (hubs.graph_rich_club, (w,), dict(kinds="mixed")), (hubs.graph_rich_club, (w,), dict(kinds=())),
        (hubs.graph_rich_club, (w,), dict(klevel=0)), (hubs.graph_rich_club, (w,), dict(klevel=9)),
        (hubs.graph_rich_club, (w,), dict(klevel=17, directed=True)), (hubs.graph_rich_club, (w,), dict(klevel=1.5)),
        (hubs.graph_rich_club, (w,), dict(klevel=True)), (hubs.graph_rich_club, (torch.zeros((1, 1), dtype=torch.float64),), {}),
        (hubs.graph_rich_club, (torch.zeros((97, 97), dtype=torch.float64),), {}),
        (hubs.graph_assortativity, (w,), dict(flag=5)), (hubs.graph_assortativity, (w,), dict(flag=-1)),
        (hubs.graph_assortativity, (w,), dict(flag=True)), (hubs.graph_assortativity, (w,), dict(flag=1.0)),
        (hubs.graph_score, (w, []), {}), (hubs.graph_score, (w, "1"), {}), (hubs.graph_score, (w, True), {}),
        (hubs.graph_score, (w, 1j), {}), (hubs.graph_score, (w, np.ones((3, 2))), {}), (hubs.graph_score, (one, np.ones((1, 2))), {}),
        (hubs.graph_score, (w, np.ones((2, 2, 2))), {}), (hubs.graph_score, (w, torch.ones((2, 2), dtype=torch.bool)), {}),
        (hubs.rich_club_norm, (w,), dict(kind="both")), (hubs.rich_club_norm, (w,), dict(reps=0)),
        (hubs.rich_club_norm, (w,), dict(reps=4, seeds=[1, 2])), (hubs.rich_club_norm, (w,), dict(max_bytes=0)),
        (hubs.rich_club_norm, (w,), dict(negative="x")), (hubs.rich_club_norm, (w,), dict(wei_freq=-1)),
        (hubs.rich_club_norm, (w,), dict(bin_swaps=-1)), (hubs.rich_club_norm, (torch.zeros((3, 3), dtype=torch.float64),), {}),
    ]
    for fn, args, kw in cases:
        with pytest.raises(ValueError, match=fn.__name__):
            fn(*args, **kw)
    for fn, extra in ((hubs.graph_rich_club, ()), (hubs.graph_assortativity, ()), (hubs.graph_score, (1.0,)), (hubs.rich_club_norm, ())):
        with pytest.raises(TypeError, match=fn.__name__):
            fn(torch.zeros((8, 8), dtype=torch.float32), *extra)
        with pytest.raises(TypeError, match=fn.__name__):
            fn(np.zeros((8, 8)), *extra)
        with pytest.raises(TypeError, match=fn.__name__):
            fn(torch.zeros((2, 8, 7), dtype=torch.float64), *extra)


def test_facades_have_the_reference_signatures_and_refuse():
    from nremmodfc_amd import graph_utils as gu
    for name in ("rich_club_wu", "rich_club_wd", "rich_club_bu", "rich_club_bd"):
        sig = inspect.signature(getattr(gu, name))
        assert list(sig.parameters) == ["CIJ", "klevel"] and sig.parameters["klevel"].default is None
        with pytest.raises(ValueError, match="2 <= N <= 96"):
            getattr(gu, name)(np.zeros((97, 97)))
        with pytest.raises(ValueError, match="N x N"):
            getattr(gu, name)(np.zeros((4, 5)))
        for klevel in (0, -1, 2.5, True):
            with pytest.raises(ValueError, match="klevel"):
                getattr(gu, name)(np.zeros((8, 8)), klevel)
    for name in ("assortativity_wei", "assortativity_bin"):
        sig = inspect.signature(getattr(gu, name))
        assert list(sig.parameters) == ["CIJ", "flag"] and sig.parameters["flag"].default == 0
        for flag in (5, -1, True, 0.5):
            with pytest.raises(ValueError, match="Flag must be 0-4"):          # the reference's own
                getattr(gu, name)(np.zeros((8, 8)), flag)
        with pytest.raises(ValueError, match="2 <= N <= 96"):
            getattr(gu, name)(np.zeros((1, 1)))
    assert list(inspect.signature(gu.score_wu).parameters) == ["CIJ", "s"]
    with pytest.raises(ValueError, match="must be a number"):
        gu.score_wu(np.zeros((8, 8)), [1.0])
    with pytest.raises(ValueError, match="2 <= N <= 96"):
        gu.score_wu(np.zeros((97, 97)), 1.0)
    assert "rich club" not in gu.__doc__.split("Outside")[1]

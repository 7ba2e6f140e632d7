"""Rich club, assortativity and s-core on the device (wc_hubs.hip, nremmodfc_amd/hubs.py) against the
numpy restatement (hubs_reference) and against the golden outputs of the reference's own code: maxdeg,
nk, member, sn, rounds and every NaN and inf pattern equal, the fp64 values within 1e-12 of
max(1, |want|) (centrality_reference.deviation_abs; the sums are at most 9216 terms of magnitude <= 1).
Every deviation is printed before it is asserted.

Largest deviations measured on an MI355X (68 tests, 5 s): rw 1.1e-15 (N = 90, sparse), rb 2.2e-16, ek 3.1e-15
(N = 65, signed), r_wei 6.3e-14 (N = 91, asymmetric, flag 0), r_bin 0 (the same bits on every case); rich_club_norm
phi 7.8e-16, null_mean 5.6e-16, null_std 2.1e-16, norm 6.7e-16, p 1.1e-16; maxdeg, nk, member, sn, rounds and
every NaN pattern equal on every case."""
import functools

import numpy as np
import pytest
import torch

from tests import hubs_reference as hr
from tests import nullmodel_reference as nr
from tests.centrality_reference import deviation_abs

pytestmark = pytest.mark.gpu

# 90 | 91: the two sides of the 8192-entry sort; 64 | 65: a wave; 96: the limit
SIZES = (2, 3, 4, 5, 16, 17, 63, 64, 65, 90, 91, 96)
KINDS = ("sparse", "signed", "directed")
TOL = 1e-12


@functools.lru_cache(maxsize=None)
def matrix(n, kind):
    W = {"sparse": hr.sparse_graph, "signed": hr.signed_graph, "directed": hr.directed_graph}[kind](n)
    W.setflags(write=False)
    return W


@functools.lru_cache(maxsize=None)
def stack(n):
    W = np.stack([matrix(n, kind) for kind in KINDS])
    W.setflags(write=False)
    return W


@functools.lru_cache(maxsize=None)
def golden():
    return hr.load_golden()


@functools.lru_cache(maxsize=None)
def inputs():
    return hr.golden_inputs()


def dev(a, cuda):
    return torch.from_numpy(np.array(a, dtype=np.float64, order="C")).to(cuda)


def host(out):
    if isinstance(out, dict):
        return {k: v.cpu().numpy() for k, v in out.items()}
    return tuple(v.cpu().numpy() for v in out)


def same_curves(got, want, what, m=None):
    """One matrix's device curves against the restatement's or the golden ones, the first m levels."""
    worst = 0.0
    for key in ("rw", "rb", "ek"):
        if key in want:
            d = deviation_abs(got[key][:m], np.asarray(want[key], dtype=np.float64)[:m])
            print(f"{what} {key}: deviation {d:.1e}")
            assert d <= TOL, (what, key)
            worst = max(worst, d)
    assert (got["nk"][:m] == np.asarray(want["nk"])[:m]).all(), (what, "nk")
    if "maxdeg" in want:
        assert int(got["maxdeg"]) == want["maxdeg"], (what, "maxdeg")
    return worst


@pytest.mark.parametrize("directed", [False, True], ids=["und", "dir"])
@pytest.mark.parametrize("n", SIZES)
def test_rich_club_matches_the_restatement(cuda, n, directed):
    from nremmodfc_amd import hubs
    got = host(hubs.graph_rich_club(dev(stack(n), cuda), directed=directed))
    assert got["rw"].shape == (len(KINDS), 2 * n if directed else n) and got["nk"].dtype == np.int32
    for b, kind in enumerate(KINDS):
        want = hr.rich_club(matrix(n, kind), directed)
        same_curves({k: v[b] for k, v in got.items()}, want, f"N {n} {kind} directed {directed}")


@pytest.mark.parametrize("n", SIZES)
def test_assortativity_matches_the_restatement(cuda, n):
    from nremmodfc_amd import hubs
    for flag in range(5):
        wei, bin_ = host(hubs.graph_assortativity(dev(stack(n), cuda), flag))
        for b, kind in enumerate(KINDS):
            want = hr.assortativity(matrix(n, kind), flag)
            for col, weighted in enumerate((True, False)):     # a value only where the quotient is one (the golden condition)
                _, t2, t3 = hr.assortativity_terms(matrix(n, kind), flag, weighted)
                assert np.isnan(want[col]) or abs(t3 - t2) >= 1e-6 * t3
            dw, db = deviation_abs(wei[b], want[0]), deviation_abs(bin_[b], want[1])
            print(f"N {n} {kind} flag {flag}: r_wei {want[0]:.4f} deviation {dw:.1e}, r_bin {want[1]:.4f} deviation {db:.1e}")
            assert dw <= TOL and db <= TOL
            if not np.isnan(want[1]):
                assert bin_[b] == want[1]              # sums of integers and halves: the same bits


@functools.lru_cache(maxsize=None)
def score_levels(n):
    """[3][4] levels: fractions of each matrix's largest column sum, moved where a strength met during the
    peel lies within 1e-9 of one (the condition of the golden levels)."""
    rows = []
    for kind in KINDS:
        W = matrix(n, kind)
        top = max(float(np.abs(hr.column_sums(W)).max()), 1.0)
        row = []
        for f in hr.SCORE_FRACTIONS:
            s = f * top
            trace = {}
            while hr.score(W, s, trace) and trace["gap"] <= 1e-9:
                s *= 1 + 1e-6
            row.append(s)
        rows.append(row)
    return np.array(rows)


@pytest.mark.parametrize("n", SIZES)
def test_score_matches_the_restatement(cuda, n):
    from nremmodfc_amd import hubs
    lev = score_levels(n)
    member, sn, rounds, core = host(hubs.graph_score(dev(stack(n), cuda), lev, want_matrix=True))
    assert member.shape == (3, 4, n) and member.dtype == sn.dtype == rounds.dtype == np.int32
    for b, kind in enumerate(KINDS):
        for k, s in enumerate(lev[b]):
            wm, wsn, wr = hr.score(matrix(n, kind), float(s))
            assert (member[b, k] == wm).all() and sn[b, k] == wsn and rounds[b, k] == wr, (n, kind, s)
            assert core[b, k].tobytes() == hr.core_matrix(matrix(n, kind), wm).tobytes()
    print(f"N {n}: sn {sn.tolist()} rounds {rounds.tolist()}")
    one = host(hubs.graph_score(dev(stack(n), cuda), float(lev[0, 1])))            # a number: no S axis
    assert one[0].shape == (3, n) and (one[0][0] == member[0, 1]).all() and one[1][0] == sn[0, 1]
    shared = host(hubs.graph_score(dev(matrix(n, "sparse"), cuda), lev[0]))         # [S] for a single matrix
    assert shared[0].shape == (4, n) and (shared[0] == member[0]).all() and (shared[2] == rounds[0]).all()


@pytest.mark.parametrize("name", hr.RICH_VALUE_CASES + hr.RICH_NAN_CASES + hr.RICH_SIGNED_CASES + hr.RICH_DIRECTED_CASES)
def test_golden_rich_club_of_the_reference(cuda, name):
    from nremmodfc_amd import hubs
    g = golden()
    got = host(hubs.graph_rich_club(dev(inputs()[name], cuda), directed=name in hr.RICH_DIRECTED_CASES))
    m = len(g[f"rich/{name}/rw"])
    assert int(got["maxdeg"]) == m                                                 # the reference's default klevel
    same_curves(got, {k: g[f"rich/{name}/{k}"] for k in ("rw", "rb", "nk", "ek")}, f"golden {name}", m)
    if name in hr.RICH_NAN_CASES:
        assert np.isnan(got["rw"]).all()


def test_golden_assortativity_and_score_of_the_reference(cuda):
    from nremmodfc_amd import hubs
    g = golden()
    for name in hr.ASSORT_CASES:
        for flag in range(5):
            wei, bin_ = host(hubs.graph_assortativity(dev(inputs()[name], cuda), flag))
            dw, db = deviation_abs(wei, g[f"assort/{name}/wei"][flag]), deviation_abs(bin_, g[f"assort/{name}/bin"][flag])
            print(f"golden {name} flag {flag}: r_wei deviation {dw:.1e}, r_bin deviation {db:.1e}")
            assert dw <= TOL and db <= TOL
    for name in hr.SCORE_CASES:
        W = inputs()[name]
        member, sn, rounds, core = host(hubs.graph_score(dev(W, cuda), g[f"score/{name}/s"], want_matrix=True))
        assert (sn == g[f"score/{name}/sn"]).all()
        alive = (core != 0).any(axis=1) | (core != 0).any(axis=2)
        assert (alive == g[f"score/{name}/alive"].astype(bool)).all()
        d = deviation_abs(core.sum(axis=(1, 2)), g[f"score/{name}/sum"])
        print(f"golden score {name}: sn {sn.tolist()} rounds {rounds.tolist()} sum deviation {d:.1e}")
        assert d <= TOL


def test_edge_cases(cuda):
    from nremmodfc_amd import hubs
    n = 24
    W = matrix(n, "sparse")
    diag = W.copy()
    np.fill_diagonal(diag, np.linspace(-0.5, 1.0, n))                              # a non-zero diagonal counts
    zero = np.zeros((n, n))
    binary = (W > 0).astype(np.float64)                                            # equal weights: ties in the order
    nan, inf = W.copy(), W.copy()
    nan[3, 3] = np.nan
    inf[2, 7] = np.inf
    batch = [W, nan, diag, inf, zero, binary, W]
    got = host(hubs.graph_rich_club(dev(np.stack(batch), cuda)))
    for b, M in enumerate(batch):
        same_curves({k: v[b] for k, v in got.items()}, hr.rich_club(M), f"edge case {b}")
    assert got["maxdeg"].tolist()[1::2] == [-1, -1, hr.rich_club(binary)["maxdeg"]] and got["maxdeg"][4] == 0
    assert (got["nk"][[1, 3]] == -1).all() and np.isnan(got["rw"][[1, 3]]).all() and np.isnan(got["ek"][[1, 3]]).all()
    assert np.isnan(got["rw"][4]).all() and np.isnan(got["rb"][4]).all() and not got["nk"][4].any()
    for key in got:
        assert got[key][6].tobytes() == got[key][0].tobytes()                      # the clean ones are not affected
    m = int(got["maxdeg"][0])                                                      # an explicit klevel past maxdeg
    assert m < n and np.isnan(got["rw"][0, m:]).all() and np.isnan(got["rb"][0, m:]).all() and not got["nk"][0, m:].any()
    part = host(hubs.graph_rich_club(dev(W, cuda), kinds="binary", klevel=m + 2))
    assert sorted(part) == ["ek", "maxdeg", "nk", "rb"] and part["rb"].shape == (m + 2,)
    assert part["rb"].tobytes() == got["rb"][0, :m + 2].tobytes()
    weighted = host(hubs.graph_rich_club(dev(W, cuda), kinds=("weighted",), klevel=1))
    assert sorted(weighted) == ["maxdeg", "rw"] and weighted["rw"].tobytes() == got["rw"][0, :1].tobytes()

    wei, bin_ = host(hubs.graph_assortativity(dev(np.stack(batch + [hr.ring(n)]), cuda)))
    for b, M in enumerate(batch + [hr.ring(n)]):
        want = hr.assortativity(M)
        assert deviation_abs(wei[b], want[0]) <= TOL and deviation_abs(bin_[b], want[1]) <= TOL, b
    assert np.isnan(wei[[1, 3, 4]]).all() and np.isnan(bin_[[1, 3, 4, 7]]).all() and np.isfinite(bin_[[0, 2, 5, 6]]).all()
    D = matrix(n, "directed")
    flags = [host(hubs.graph_assortativity(dev(D, cuda), flag)) for flag in range(5)]
    assert flags[4][0] == flags[2][0] and flags[4][0] != flags[1][0]               # r_wei flag 4: in/out, as written
    assert flags[4][1] != flags[2][1]                                              # r_bin flag 4: in/in

    member, sn, rounds = host(hubs.graph_score(dev(np.stack(batch), cuda), 1.0))
    for b, M in enumerate(batch):
        wm, wsn, wr = hr.score(M, 1.0)
        assert (member[b] == wm).all() and sn[b] == wsn and rounds[b] == wr, b
    assert (member[[1, 3]] == -1).all() and sn[4] == 0 and (member[4] == 1).all()


def test_a_matrix_gives_the_same_bits_alone_and_in_a_batch(cuda):
    from nremmodfc_amd import hubs
    for n in (17, 91):
        batch = np.stack([matrix(n, "sparse"), matrix(n, "signed"), matrix(n, "directed"), matrix(n, "sparse") * 0.5])
        lev = np.array([0.5, 1.0, 2.0])
        rich = host(hubs.graph_rich_club(dev(batch, cuda), directed=True))
        ass = host(hubs.graph_assortativity(dev(batch, cuda), 1))
        sco = host(hubs.graph_score(dev(batch, cuda), lev))
        for b in range(len(batch)):
            alone = host(hubs.graph_rich_club(dev(batch[b], cuda), directed=True))
            for key in rich:
                assert alone[key].tobytes() == rich[key][b].tobytes(), (n, b, key)
            for a, c in zip(host(hubs.graph_assortativity(dev(batch[b], cuda), 1)), ass):
                assert a.tobytes() == c[b].tobytes()
            for a, c in zip(host(hubs.graph_score(dev(batch[b], cuda), lev)), sco):
                assert a.tobytes() == c[b].tobytes()
        again = host(hubs.graph_rich_club(dev(batch[::-1].copy(), cuda), directed=True))
        for key in rich:
            assert again[key][::-1].tobytes() == rich[key].tobytes()


NORM_CASES = {17: (lambda: hr.sparse_graph(17, 6), 5), 90: (lambda: nr.sparse_nonneg(nr.signed(90)), 1)}


@pytest.mark.parametrize("kind", ["weighted", "binary"])
@pytest.mark.parametrize("n", sorted(NORM_CASES))
def test_rich_club_norm(cuda, n, kind):
    from nremmodfc_amd import hubs
    make, swaps = NORM_CASES[n]
    W = make()
    other = nr.symmetric(np.roll(W, 3, axis=1) * (np.roll(W, 3, axis=1) > 0.3))
    bad = W.copy()
    bad[tuple(np.argwhere(np.triu(W == 0, 1))[0])] = 0.5                           # not symmetric: status 2
    want = hr.rich_club_norm(W, kind, 8, None, swaps)
    finite = np.isfinite(want["norm"])
    assert finite.sum() >= 4 and np.nanmin(want["gap"]) > 1e-9                     # every null >= phi has one answer
    w = dev(np.stack([W, bad, other]), cuda)
    got = host(hubs.rich_club_norm(w, kind, reps=8, bin_swaps=swaps))
    for key in ("phi", "null_mean", "null_std", "norm", "p"):
        d = deviation_abs(got[key][0], want[key])
        print(f"rich_club_norm N {n} {kind} {key}: deviation {d:.1e} ({int(finite.sum())} finite levels)")
        assert d <= TOL
        assert np.isnan(got[key][1]).all()
    assert np.isfinite(got["norm"][2]).any()
    for max_bytes in (1, 3 * 3 * n * n * 8):                                       # one rep at a time; three
        small = host(hubs.rich_club_norm(w, kind, reps=8, bin_swaps=swaps, max_bytes=max_bytes))
        for key in got:
            assert small[key].tobytes() == got[key].tobytes(), (key, max_bytes)
    alone = host(hubs.rich_club_norm(dev(other, cuda), kind, reps=8, bin_swaps=swaps))
    assert alone["norm"].shape == (n,) and alone["norm"].tobytes() == got["norm"][2].tobytes()


def test_facades(cuda):
    from nremmodfc_amd import graph_utils as gu
    g = golden()
    for name in ("fc_thr", "pendant12"):
        W = inputs()[name]
        rw = gu.rich_club_wu(W)
        R, Nk, Ek = gu.rich_club_bu(W)
        assert len(rw) == len(R) == len(g[f"rich/{name}/rw"]) and Nk.dtype == np.float64
        assert deviation_abs(rw, g[f"rich/{name}/rw"]) <= TOL and deviation_abs(R, g[f"rich/{name}/rb"]) <= TOL
        assert (Nk == g[f"rich/{name}/nk"]).all() and deviation_abs(Ek, g[f"rich/{name}/ek"]) <= TOL
    W = inputs()["pendant12"]
    for klevel in (12, 30):                                                        # past the degree, past N
        rw = gu.rich_club_wu(W, klevel)
        R, Nk, Ek = gu.rich_club_bu(W, klevel)
        assert len(rw) == len(R) == klevel and deviation_abs(rw[:12], g["rich/pendant12/k12/rw"]) <= TOL
        assert deviation_abs(R[:12], g["rich/pendant12/k12/rb"]) <= TOL and (Nk[:12] == g["rich/pendant12/k12/nk"]).all()
        assert np.isnan(rw[12:]).all() and np.isnan(R[12:]).all() and not Nk[12:].any() and not Ek[12:].any()
    D = inputs()["dir24"]
    assert deviation_abs(gu.rich_club_wd(D), g["rich/dir24/rw"]) <= TOL
    R, Nk, Ek = gu.rich_club_bd(D)
    assert deviation_abs(R, g["rich/dir24/rb"]) <= TOL and (Nk == g["rich/dir24/nk"]).all()
    both = gu.rich_club_wu(np.stack([inputs()["fc_thr"], inputs()["rand90"]]))      # a stack: each its own length
    assert [len(v) for v in both] == [len(g["rich/fc_thr/rw"]), len(g["rich/rand90/rw"])]
    assert gu.rich_club_wu(np.stack([inputs()["fc_thr"], inputs()["rand90"]]), 7).shape == (2, 7)
    for flag in range(5):
        assert deviation_abs(gu.assortativity_wei(D, flag), g["assort/dir24/wei"][flag]) <= TOL
        assert deviation_abs(gu.assortativity_bin(D, flag), g["assort/dir24/bin"][flag]) <= TOL
    assert isinstance(gu.assortativity_wei(D), float) and np.isnan(gu.assortativity_bin(hr.ring(12)))
    W = inputs()["fc_thr"]
    for k, s in enumerate(g["score/fc_thr/s"]):
        core, sn = gu.score_wu(W, float(s))
        assert sn == g["score/fc_thr/sn"][k] and isinstance(sn, int) and core.shape == W.shape
        assert ((core != 0).any(axis=0) == g["score/fc_thr/alive"][k].astype(bool)).all()
        assert (core[core != 0] == W[core != 0]).all()
    with pytest.raises(ValueError, match="NaN or inf"):
        gu.rich_club_wu(np.where(np.eye(12) > 0, np.nan, inputs()["pendant12"]))
    with pytest.raises(ValueError, match="NaN or inf"):
        gu.score_wu(np.where(np.eye(12) > 0, np.inf, inputs()["pendant12"]), 1.0)


def test_chain_from_thresholded_fc_to_the_normalised_rich_club(cuda):
    """Thresholded FC -> null models -> their rich-club curves, nothing leaving the device."""
    from nremmodfc_amd import hubs
    w = dev(np.stack([inputs()["fc_thr"], inputs()["fc_thr"] * 0.5]), cuda)
    out = hubs.rich_club_norm(w, reps=4)
    assert out["norm"].shape == (2, 90) and out["norm"].is_cuda
    some = torch.isfinite(out["norm"])
    assert int(some[0].sum()) >= 20 and (out["p"][some] > 0).all() and (out["p"][some] <= 1).all()
    assert torch.equal(some[0], some[1])

"""Null models on the device (wc_nullmodel.hip, nremmodfc_amd/nullmodel.py) against the numpy
restatement (nullmodel_reference) and against the golden outputs of the reference's own code: w0 and wr
as the same bits, info equal, r, mean and std within 1e-12 of max(1, |want|)
(centrality_reference.deviation_abs).  Every deviation is printed before it is asserted.

Largest deviations measured on an MI355X (38 tests, 6 s): r 7.8e-16 (N = 96, sparse), participation mean
2.2e-16 and std 5.6e-17; w0, wr and info equal on every case."""
import functools

import numpy as np
import pytest
import torch

from tests import nullmodel_reference as nr
from tests.centrality_reference import deviation_abs

pytestmark = pytest.mark.gpu

SIZES = (4, 5, 7, 24, 63, 64, 65, 90, 96)
TOL = 1e-12


@functools.lru_cache(maxsize=None)
def matrix(n, kind):
    W = nr.signed(n)
    W = nr.sparse_nonneg(W) if kind == "sparse" else W
    W.setflags(write=False)
    return W


@functools.lru_cache(maxsize=None)
def golden():
    return nr.load_golden()


@functools.lru_cache(maxsize=None)
def inputs():
    return nr.inputs()


def dev(a, cuda):
    return torch.from_numpy(np.array(a, order="C")).to(cuda)


def null_model(cuda, W, seeds, **kw):
    from nremmodfc_amd import nullmodel
    return tuple(t.cpu().numpy() for t in nullmodel.graph_null_model(dev(W, cuda), seeds=seeds, want_stats=True, **kw))


def rewire(cuda, W, seeds, bin_swaps):
    from nremmodfc_amd import nullmodel
    return tuple(t.cpu().numpy() for t in nullmodel.graph_rewire(dev(W, cuda), bin_swaps, seeds, want_info=True))


def same_run(got, want, what):
    """One device run (w0, r, info) against the restatement's."""
    w0, r, info = got
    assert tuple(int(v) for v in info) == tuple(want[2]), (what, info, want[2])
    assert w0.tobytes() == want[0].tobytes(), (what, "w0 differs", np.nanmax(np.abs(w0 - want[0])))
    d = deviation_abs(r, np.array(want[1]))
    print(f"{what}: info {tuple(want[2])}  r {np.array(want[1])}  r deviation {d:.1e}")
    assert d <= TOL, what
    return d


@pytest.mark.parametrize("kind", ["signed", "sparse"])
@pytest.mark.parametrize("n", SIZES)
def test_null_model_and_rewiring_match_the_restatement(cuda, n, kind):
    W = matrix(n, kind)
    for negative in (("reference", "bct") if kind == "signed" else ("bct",)):
        got = null_model(cuda, W, n, bin_swaps=1, negative=negative)
        same_run(got, nr.null_model(W, n, 1, 10, negative), f"N {n} {kind} {negative}")
    wr, info = rewire(cuda, W, n + 1, 1)
    want, winfo = nr.rewire(W, n + 1, 1)
    assert tuple(int(v) for v in info) == winfo and wr.tobytes() == want.tobytes()


def test_rewiring_edge_cases(cuda):
    W = matrix(24, "signed")
    wr, info = rewire(cuda, W, 0, 0)                                   # bin_swaps = 0: nothing moves
    assert tuple(info) == (0, 0, 0) and wr.tobytes() == W.tobytes()
    full = np.abs(W) + 0.25
    np.fill_diagonal(full, 0.0)
    got = null_model(cuda, full, 3)                                    # fully positive: the rewiring is skipped (:2268)
    assert tuple(got[2]) == (0, 0, 0)
    same_run(got, nr.null_model(full, 3), "full positive")
    wr, info = rewire(cuda, full, 3, 2)                                # wc_graph_rewire always rewires: no swap is
    want, winfo = nr.rewire(full, 3, 2)                                # possible, every budget is exhausted
    assert winfo[0] == 0 and winfo[1] >= 2 * 276 * 13 and tuple(info) == winfo and wr.tobytes() == full.tobytes()
    got = null_model(cuda, -full, 3, bin_swaps=2)                      # the same through the null model
    want = nr.null_model(-full, 3, 2)
    assert want[2][0] == 0 and want[2][1] == winfo[1]
    same_run(got, want, "all negative")


@pytest.mark.parametrize("negative", ["reference", "bct"])
@pytest.mark.parametrize("wei_freq,period", [(0, 0), (1, 1), (0.1, 10), (1 / 64, 64)])
def test_periods_and_modes(cuda, wei_freq, period, negative):
    for n in (24, 5):                                                  # N = 5: wsize is below every period but 1
        W = matrix(n, "signed") if n > 5 else inputs()["signed5"]
        got = null_model(cuda, W, 7, bin_swaps=1, wei_freq=wei_freq, negative=negative)
        same_run(got, nr.null_model(W, 7, 1, period, negative), f"N {n} period {period} {negative}")
    if negative == "reference":
        assert (got[0] >= 0).all() and np.isnan(got[1][1])             # the reference's negative half, as documented
    else:
        assert ((got[0] < 0).sum(axis=0) == (W < 0).sum(axis=0)).all()


def test_binary_matrix_gives_the_rewired_pattern(cuda):
    A = (matrix(24, "sparse") > 0).astype(np.float64)                  # every key ties: the stable order decides
    got = null_model(cuda, A, 11, bin_swaps=2)
    same_run(got, nr.null_model(A, 11, 2), "binary")
    wr, _ = rewire(cuda, A, 11, 2)
    assert got[0].tobytes() == wr.tobytes() and (wr != A).any()


@pytest.mark.parametrize("name", [c for c, _ in nr.GOLDEN_CASES])
def test_golden_cases_of_the_reference(cuda, name):
    g = golden()
    seeds = [int(s) for s in g[f"{name}/seeds"]]
    w0, r, info = null_model(cuda, inputs()[name], seeds, negative="reference")
    for k, seed in enumerate(seeds):
        assert tuple(info[k]) == (g[f"{name}/eff"][k], g[f"{name}/draws"][k], 0)
        assert nr.uptri(w0[k]).tobytes() == g[f"{name}/w0"][k].tobytes() and (w0[k] == w0[k].T).all()
        d = deviation_abs(r[k], g[f"{name}/r"][k])
        print(f"golden {name} seed {seed}: r deviation {d:.1e}")
        assert d <= TOL


def test_golden_rewiring_of_the_reference(cuda):
    g = golden()
    wr, info = rewire(cuda, inputs()["corr24"], int(g["rewire/corr24/seed"]), 5)
    assert tuple(info) == (g["rewire/corr24/eff"], g["rewire/corr24/draws"], 0)
    assert nr.uptri(wr).tobytes() == g["rewire/corr24/wr"].tobytes() and (wr == wr.T).all()


def test_a_pair_gives_the_same_bits_alone_in_a_batch_and_with_any_workspace(cuda):
    from nremmodfc_amd import nullmodel
    n, seeds = 24, [5, 6, 1 << 40]
    Ws = np.stack([matrix(n, "signed"), matrix(n, "sparse"), -matrix(n, "signed"), matrix(n, "signed") * 0.5,
                   nr.symmetric(np.roll(matrix(n, "signed"), 3, axis=1))])
    slot = nullmodel.null_model_slot_bytes(n)
    runs = [null_model(cuda, Ws, seeds, bin_swaps=1), null_model(cuda, Ws, seeds, bin_swaps=1),
            null_model(cuda, Ws, seeds, bin_swaps=1, ws_bytes=slot), null_model(cuda, Ws, seeds, bin_swaps=1, ws_bytes=3 * slot + 8)]
    for other in runs[1:]:
        for a, b in zip(runs[0], other):
            assert a.tobytes() == b.tobytes()
    assert (runs[0][2][:, :, 2] == 0).all()
    for b in range(len(Ws)):
        for k, seed in enumerate(seeds):
            w0, r, info = null_model(cuda, Ws[b], seed, bin_swaps=1)
            assert w0.tobytes() == runs[0][0][b, k].tobytes() and r.tobytes() == runs[0][1][b, k].tobytes()
            assert (info == runs[0][2][b, k]).all()
    wr = rewire(cuda, Ws, seeds, 1)
    wr1 = rewire(cuda, Ws, seeds, 1)
    assert wr[0].tobytes() == wr1[0].tobytes() and wr[0][2, 1].tobytes() == rewire(cuda, Ws[2], seeds[1], 1)[0].tobytes()


@functools.lru_cache(maxsize=None)
def zero_strength_case():
    """(W, a seed whose run divides by a strength of exactly 0, a seed whose run does not): integer
    weights, so that a node's first weight can use up its whole strength; found with the restatement."""
    rng = np.random.default_rng(8)
    W = np.triu(rng.integers(1, 4, (8, 8)) * (rng.random((8, 8)) < 0.6), 1).astype(np.float64)
    W = W + W.T
    status = [nr.null_model(W, s, 1)[2][2] for s in range(16)]
    return W, status.index(1), status.index(0)


def test_statuses_spoil_only_their_own_runs(cuda):
    good = matrix(8, "signed")
    asym, nan, inf = good.copy(), good.copy(), good.copy()
    asym[1, 2] += 1e-12
    nan[0, 0] = np.nan                                                 # the diagonal counts too
    inf[3, 4] = inf[4, 3] = np.inf
    w0, r, info = null_model(cuda, np.stack([good, asym, nan, good, inf]), [1, 2], bin_swaps=1)
    assert (info[:, :, 2] == np.array([0, 2, 3, 0, 3])[:, None]).all() and (info[[1, 2, 4], :, :2] == 0).all()
    assert np.isnan(w0[[1, 2, 4]]).all() and np.isnan(r[[1, 2, 4]]).all()
    for k, seed in enumerate((1, 2)):
        same_run((w0[0, k], r[0, k], info[0, k]), nr.null_model(good, seed, 1), "good neighbour")
        assert w0[3, k].tobytes() == w0[0, k].tobytes()
    wr, winfo = rewire(cuda, np.stack([asym, good, inf]), [1, 2], 1)
    assert (winfo[:, :, 2] == np.array([2, 0, 3])[:, None]).all() and np.isnan(wr[[0, 2]]).all()
    assert wr[1, 0].tobytes() == nr.rewire(good, 1, 1)[0].tobytes()

    W, bad_seed, good_seed = zero_strength_case()
    seeds = [good_seed, bad_seed, good_seed]
    w0, r, info = null_model(cuda, W, seeds, bin_swaps=1)
    for k, seed in enumerate(seeds):
        same_run((w0[k], r[k], info[k]), nr.null_model(W, seed, 1), f"zero strength, seed {seed}")
    assert info[1, 2] == 1 and np.isnan(w0[1]).all() and np.isnan(r[1]).all() and np.isfinite(w0[[0, 2]]).all()


def test_participation_norm(cuda):
    from nremmodfc_amd import nullmodel
    A, Bm = matrix(24, "sparse").copy(), nr.sparse_nonneg(nr.symmetric(np.roll(matrix(24, "signed"), 5, axis=1)))
    A[:, 7] = A[7, :] = 0.0                                            # a node without neighbours: Ko = 0
    ci = np.stack([np.arange(24) // 8, np.arange(24) % 3 + 4])         # any integers
    mean, std = (t.cpu().numpy() for t in nullmodel.participation_norm(dev(np.stack([A, Bm]), cuda), ci, reps=8))
    for b, W in enumerate((A, Bm)):
        wm, ws = nr.participation_norm(W, ci[b], 8)
        dm, ds = deviation_abs(mean[b], wm), deviation_abs(std[b], ws)
        print(f"participation_norm matrix {b}: mean deviation {dm:.1e}, std deviation {ds:.1e}")
        assert dm <= TOL and ds <= TOL
    assert mean[0, 7] == 0 and std[0, 7] == 0 and (mean >= 0).all() and (mean <= 1).all()
    small = nullmodel.participation_norm(dev(np.stack([A, Bm]), cuda), ci, reps=8, max_bytes=1)   # one rep at a time
    three = nullmodel.participation_norm(dev(np.stack([A, Bm]), cuda), ci, reps=8, max_bytes=3 * 2 * 24 * 24 * 8)
    for got in (small, three):
        assert got[0].cpu().numpy().tobytes() == mean.tobytes() and got[1].cpu().numpy().tobytes() == std.tobytes()
    alone = nullmodel.participation_norm(dev(Bm, cuda), ci[1], reps=8)
    assert alone[0].cpu().numpy().tobytes() == mean[1].tobytes() and alone[0].shape == (24,)

    g = golden()                                                       # the reference's own, N = 90
    W = inputs()["fc_thr"]
    mean, std = (t.cpu().numpy() for t in nullmodel.participation_norm(dev(W, cuda), g["pnorm/fc_thr/ci"].astype(np.int64),
                                                                       reps=nr.GOLDEN_REPS, negative="reference"))
    dm, ds = deviation_abs(mean, g["pnorm/fc_thr/mean"]), deviation_abs(std, g["pnorm/fc_thr/std"])
    print(f"participation_norm golden fc_thr: mean deviation {dm:.1e}, std deviation {ds:.1e}")
    assert dm <= TOL and ds <= TOL
    bad = W.copy()
    bad[2, 3] = np.nan
    mean, std = nullmodel.participation_norm(dev(np.stack([W, bad]), cuda), g["pnorm/fc_thr/ci"].astype(np.int64), reps=2)
    assert torch.isnan(mean[1]).all() and torch.isnan(std[1]).all() and torch.isfinite(mean[0]).all()


def test_facades(cuda):
    from nremmodfc_amd import graph_utils as gu
    g = golden()
    W = inputs()["corr24"]
    w0, r = gu.null_model_und_sign(W, seed=int(g["corr24/seeds"][0]))
    assert nr.uptri(w0).tobytes() == g["corr24/w0"][0].tobytes() and len(r) == 4 and r[0] == r[1] and np.isnan(r[2])
    assert deviation_abs(np.array(r[:1]), g["corr24/r"][0][:1]) <= TOL
    assert (gu.null_model_und_sign(W, seed=4)[0] == gu.null_model_und_sign(W, seed=4)[0]).all()
    withdiag = W.copy()
    np.fill_diagonal(withdiag, 2.0)
    wr, eff = gu.randmio_und_signed(withdiag, 5, seed=int(g["rewire/corr24/seed"]))
    assert eff == g["rewire/corr24/eff"] and nr.uptri(wr).tobytes() == g["rewire/corr24/wr"].tobytes()
    assert (np.diag(wr) == 2.0).all()                                  # the reference leaves the diagonal alone
    asym = W.copy()
    asym[0, 1] += 1e-9
    with pytest.raises(TypeError, match="Input must be undirected"):
        gu.randmio_und_signed(asym, 1, seed=0)
    with pytest.raises(ValueError, match="NaN or inf"):
        gu.null_model_und_sign(np.where(np.eye(24) > 0, np.nan, W), seed=0)
    F = inputs()["fc_thr"]
    mean, std = gu.participation_coef_norm(F, g["pnorm/fc_thr/ci"], BA_iters=nr.GOLDEN_REPS)     # labels from 1
    assert deviation_abs(mean, g["pnorm/fc_thr/mean"]) <= TOL and deviation_abs(std, g["pnorm/fc_thr/std"]) <= TOL
    again, _ = gu.participation_coef_norm(F, g["pnorm/fc_thr/ci"] * 10 - 3, degree="in", BA_iters=nr.GOLDEN_REPS)
    assert again.tobytes() == mean.tobytes()                           # the labels are names only


def test_chain_from_thresholded_fc_to_normalised_participation(cuda):
    """Thresholded FC -> consensus partition -> participation against its own null models, on the device."""
    from nremmodfc_amd import nullmodel, partition, sigchain
    w = dev(np.stack([inputs()["fc_thr"], inputs()["fc_thr"] * 0.5]), cuda)
    D = sigchain.graph_consensus_matrix(w, reps=8, tau=0.0)
    ci, iters = partition.graph_consensus(D, 0.5, reps=8)
    assert (ci >= 0).all()
    mean, std = nullmodel.participation_norm(w, ci, reps=4)
    assert mean.shape == std.shape == (2, 90) and mean.is_cuda
    assert torch.isfinite(mean).all() and (mean >= 0).all() and (mean <= 1).all() and (std >= 0).all()
    assert float(mean.max()) > 0.3 and float(std.max()) > 0

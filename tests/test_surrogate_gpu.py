"""wc_surrogate_fc and wc_surrogate_test on the device against the numpy restatement
(tests/surrogate_reference.py) and the reference's own run (tests/golden/golden_surrogate.npz).

Tolerances: ten times the larger of the restatement's largest deviation from the golden outputs
(test_surrogate_cpu.py) and the device's largest deviation from the restatement, measured on an MI355X
over the five cases:
               restatement vs golden   device vs restatement   tolerance
    sfc        5.0e-16                 5.3e-16                 5e-15
    mu         8.3e-17                 1.1e-16                 1e-15
    sd         1.7e-16                 1.2e-16                 2e-15
    p_adj      1.8e-15                 1.9e-15                 2e-14
    fc_adj     4.4e-16                 8.9e-16                 9e-15
The kept set is compared exactly: every case keeps |p_adj - alpha| >= 1e-9 on every pair."""
import numpy as np
import pytest
import torch

from nremmodfc_amd import graph_utils, surrogate
from tests import surrogate_reference as sr

pytestmark = pytest.mark.gpu

TOL = {"sfc": 5e-15, "mu": 1e-15, "sd": 2e-15, "p_adj": 2e-14, "fc_adj": 9e-15}
_cache = {}


@pytest.fixture(scope="module")
def golden():
    return sr.load_golden()


def restated(golden, name):
    if ("np", name) not in _cache:
        _cache["np", name] = sr.thresholded(golden[name]["y"], golden[name]["seeds"])
    return _cache["np", name]


def device(golden, name):
    """One run of the case alone: fc_adj, p_adj, the statistics and all the surrogate FCs, as numpy."""
    if ("dev", name) not in _cache:
        x = torch.from_numpy(golden[name]["y"]).cuda()
        S = sr.CASES[name][2]
        fc_adj, p_adj, st = surrogate.fc_surrogate_test(x, surr_number=S, alpha=sr.ALPHA, want_stats=True)
        sfc = surrogate.surrogate_fc(x, [int(s) for s in golden[name]["seeds"]])
        _cache["dev", name] = dict({k: v.cpu().numpy() for k, v in st.items()}, fc_adj=fc_adj.cpu().numpy(),
                                   p_adj=p_adj.cpu().numpy(), sfc=sfc.cpu().numpy())
    return _cache["dev", name]


def variants(y):
    """Three different series of one shape: y, y with its columns rolled, y with noise of another seed added."""
    return np.stack([y, np.roll(y, 1, axis=1), y + 0.5 * np.random.default_rng(7).standard_normal(y.shape)], axis=1)


@pytest.mark.parametrize("name", list(sr.CASES))
def test_device_matches_restatement_and_reference(golden, name):
    c, r, d = golden[name], restated(golden, name), device(golden, name)
    L, N, S, _ = sr.CASES[name]
    assert d["sfc"].shape == (S, N * (N - 1) // 2) and d["p_adj"].shape == (N, N) and d["mu"].shape == (N * (N - 1) // 2,)
    dev = {k: float(np.abs(d[k] - r[k]).max()) for k in ("sfc", "mu", "sd", "p", "p_adj", "fc_adj")}
    ref = {"sfc": float(np.abs(d["sfc"][:3] - c["sfc3"]).max()),
           **{k: float(np.abs(d[k] - c[k]).max()) for k in ("mu", "sd", "p_adj", "fc_adj")}}
    print(f"{name}: device vs restatement {dev}; device vs reference {ref}")
    for k in TOL:
        assert dev[k] <= TOL[k] and ref[k] <= TOL[k], (k, dev[k], ref[k])
    assert dev["p"] <= TOL["p_adj"]
    assert ((d["fc_adj"] != 0) == (c["fc_adj"] != 0)).all() and ((d["fc_adj"] != 0) == (r["fc_adj"] != 0)).all()
    assert ((d["p_adj"] < sr.ALPHA) == (c["p_adj"] < sr.ALPHA)).all()
    for m in (d["p_adj"], d["fc_adj"]):
        assert (m == m.T).all() and (np.diag(m) == 0).all()
    assert np.abs(sr.uptri(d["p_adj"]) - sr.ALPHA).min() >= sr.MIN_GAP
    assert (np.abs(d["sfc"]) <= 1).all()


@pytest.mark.parametrize("name", list(sr.CASES))
def test_same_bits_alone_in_a_batch_chunked_and_again(golden, name):
    L, N, S, _ = sr.CASES[name]
    alone = device(golden, name)
    xs = torch.from_numpy(variants(golden[name]["y"])).cuda()                    # [L][3][N]
    runs = [surrogate.fc_surrogate_test(xs, surr_number=S, want_stats=True),
            surrogate.fc_surrogate_test(xs, surr_number=S, want_stats=True, ws_bytes=surrogate.surrogate_slab_bytes(N, S)),
            surrogate.fc_surrogate_test(xs, surr_number=S, want_stats=True)]
    first = runs[0]
    for fc_adj, p_adj, st in runs:
        assert torch.equal(fc_adj, first[0]) and torch.equal(p_adj, first[1])
        for k in st:
            assert torch.equal(st[k], first[2][k])
    assert (first[0][0].cpu().numpy() == alone["fc_adj"]).all() and (first[1][0].cpu().numpy() == alone["p_adj"]).all()
    for k in ("mu", "sd", "p"):
        assert (first[2][k][0].cpu().numpy() == alone[k]).all()
    sfc = surrogate.surrogate_fc(xs, [int(s) for s in golden[name]["seeds"]])
    assert (sfc[0].cpu().numpy() == alone["sfc"]).all()
    assert not torch.equal(first[1][0], first[1][1]) and not torch.equal(first[1][0], first[1][2])
    # the others against the restatement too: a series at position 1 or 2 is computed as at position 0
    for b in (1, 2):
        r = sr.thresholded(xs[:, b].cpu().numpy(), golden[name]["seeds"])
        assert np.abs(first[1][b].cpu().numpy() - r["p_adj"]).max() <= TOL["p_adj"]
        assert np.abs(sfc[b].cpu().numpy() - r["sfc"]).max() <= TOL["sfc"]


def test_a_batch_across_the_fc_groups():
    """130 simulations of 298 samples: wc_corrcoef is called for 127 and for 3 (surrogate._fc_group), or per
    chunk of 50, 50, 30; a simulation has the same bits in all of them and alone."""
    L, B, N, S = 298, 130, 12, 3
    assert surrogate._fc_group(L) == 127 and surrogate._fc_group(4096) == 8 and surrogate._fc_group(64) is None
    rng = np.random.default_rng(5)
    xs = torch.from_numpy(rng.standard_normal((L, B, 3))[:, :, np.arange(N) % 3] + rng.standard_normal((L, B, N))).cuda()
    whole = surrogate.fc_surrogate_test(xs, surr_number=S)
    part = surrogate.fc_surrogate_test(xs, surr_number=S, ws_bytes=50 * surrogate.surrogate_slab_bytes(N, S))
    assert torch.equal(part[0], whole[0]) and torch.equal(part[1], whole[1])
    for b in (0, 126, 127, 129):
        one = surrogate.fc_surrogate_test(xs[:, b].contiguous(), surr_number=S)
        assert torch.equal(one[0], whole[0][b]) and torch.equal(one[1], whole[1][b])
    r = sr.thresholded(xs[:, 127].cpu().numpy(), [1, 2, 3])
    assert np.abs(whole[1][127].cpu().numpy() - r["p_adj"]).max() <= TOL["p_adj"]


def test_a_batch_in_uneven_chunks(golden):
    """Eleven simulations in chunks of 11, 4 + 4 + 3 and 1 each."""
    L, N, S, _ = sr.CASES["odd_h"]
    rng = np.random.default_rng(11)
    y = golden["odd_h"]["y"]
    xs = torch.from_numpy(np.stack([y + 0.3 * rng.standard_normal(y.shape) for _ in range(11)], axis=1)).cuda()
    slab = surrogate.surrogate_slab_bytes(N, S)
    whole = surrogate.fc_surrogate_test(xs, surr_number=S)
    for cap in (4 * slab + 8, slab):
        part = surrogate.fc_surrogate_test(xs, surr_number=S, ws_bytes=cap)
        assert torch.equal(part[0], whole[0]) and torch.equal(part[1], whole[1])
    for b in (0, 7, 8, 10):
        one = surrogate.fc_surrogate_test(xs[:, b].contiguous(), surr_number=S)
        assert torch.equal(one[0], whole[0][b]) and torch.equal(one[1], whole[1][b])
        r = sr.thresholded(xs[:, b].cpu().numpy(), sr.case_seeds("odd_h"))
        assert np.abs(one[1].cpu().numpy() - r["p_adj"]).max() <= TOL["p_adj"]


@pytest.mark.parametrize("name", ["tiny", "mid", "shipped"])
def test_nan_convention_leaves_the_neighbours_alone(golden, name):
    L, N, S, _ = sr.CASES[name]
    ys = variants(golden[name]["y"])
    clean = surrogate.fc_surrogate_test(torch.from_numpy(ys).cuda(), surr_number=S, want_stats=True)
    ys[:, 1, N // 2] = 2.25                                                      # a constant column in the middle matrix
    fc_adj, p_adj, st = surrogate.fc_surrogate_test(torch.from_numpy(ys).cuda(), surr_number=S, want_stats=True)
    assert fc_adj[1].isnan().all() and p_adj[1].isnan().all()
    for b in (0, 2):
        assert torch.equal(fc_adj[b], clean[0][b]) and torch.equal(p_adj[b], clean[1][b])
        assert torch.equal(st["p"][b], clean[2]["p"][b])
    touched = np.zeros((N, N), dtype=bool)
    touched[N // 2, :] = touched[:, N // 2] = True
    pairs = sr.uptri(touched)
    p_mid, p_clean = st["p"][1].cpu().numpy(), clean[2]["p"][1].cpu().numpy()
    assert pairs.sum() == N - 1 and np.isnan(p_mid[pairs]).all()                 # the unadjusted p says which pairs
    assert (p_mid[~pairs] == p_clean[~pairs]).all()
    ys[3, 1, 0] = np.inf                                                         # and a sample that is not finite
    fc_adj, p_adj = surrogate.fc_surrogate_test(torch.from_numpy(ys).cuda(), surr_number=S)
    assert fc_adj[1].isnan().all() and p_adj[1].isnan().all() and torch.equal(p_adj[2], clean[1][2])


def test_alpha_and_seeds_are_honoured(golden):
    c = golden["mid"]
    L, N, S, _ = sr.CASES["mid"]
    x = torch.from_numpy(c["y"]).cuda()
    seeds = [101, 2 ** 63 + 5, 7, 2 ** 40, 12, 13, 14, 15]
    fc_adj, p_adj = surrogate.fc_surrogate_test(x, surr_number=len(seeds), alpha=0.2, seeds=seeds)
    r = sr.thresholded(c["y"], seeds, alpha=0.2)
    gap = np.abs(sr.uptri(r["p_adj"]) - 0.2).min()
    print("alpha 0.2, other seeds: gap", gap, "dp_adj", np.abs(p_adj.cpu().numpy() - r["p_adj"]).max())
    assert np.abs(p_adj.cpu().numpy() - r["p_adj"]).max() <= TOL["p_adj"]
    assert gap >= sr.MIN_GAP                                                     # 6.7e-3 in the restatement
    assert ((fc_adj.cpu().numpy() != 0) == (r["fc_adj"] != 0)).all()
    assert not torch.equal(p_adj, torch.from_numpy(device(golden, "mid")["p_adj"]).cuda())


def test_facade_on_one_matrix_and_on_a_stack(golden):
    c, d = golden["mid"], device(golden, "mid")
    L, N, S, _ = sr.CASES["mid"]
    out = graph_utils.probabilistic_thresholding(c["y"], surr_number=S)
    assert isinstance(out, list) and len(out) == 2 and all(isinstance(m, np.ndarray) and m.shape == (N, N) for m in out)
    assert (out[0] == d["fc_adj"]).all() and (out[1] == d["p_adj"]).all()
    assert (out[0] == c["fc_adj"])[c["fc_adj"] == 0].all() and np.abs(out[0] - c["fc_adj"]).max() <= TOL["fc_adj"]
    stack = np.ascontiguousarray(variants(c["y"]).transpose(1, 0, 2))            # [B, L, N]
    outs = graph_utils.probabilistic_thresholding(stack, surr_number=S, alpha=sr.ALPHA)
    assert outs[0].shape == (3, N, N) and outs[1].shape == (3, N, N)
    assert (outs[0][0] == out[0]).all() and (outs[1][0] == out[1]).all()
    as_float32 = graph_utils.probabilistic_thresholding(c["y"].astype(np.float32), surr_number=S)   # the inputs are float32 values
    assert (as_float32[1] == out[1]).all()

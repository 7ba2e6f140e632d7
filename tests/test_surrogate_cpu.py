"""The surrogate test of the FC without a GPU: the numpy restatement (tests/surrogate_reference.py) of
wc_surrogate_fc and wc_surrogate_test against the reference's own probabilistic_thresholding run under the
engine's phases (tests/golden/golden_surrogate.npz), the conditions the golden cases rest on, the Parseval
identity, the phase stream, the Benjamini-Hochberg step, and what the Python layers and the library refuse.

Tolerances: ten times the largest deviation of the restatement from the golden outputs measured over the
five cases: p_adj 1.8e-15 -> 2e-14, fc_adj 4.4e-16 -> 5e-15 (the reference correlates the centred series,
the restatement the series), sfc 5.0e-16 -> 5e-15, mu 8.3e-17 -> 1e-15, sd 1.7e-16 -> 2e-15."""
import ctypes

import numpy as np
import pytest
import torch
from scipy import stats

from nremmodfc_amd import graph_utils, surrogate
from tests import louvain_reference as lr
from tests import surrogate_reference as sr

TOL = {"p_adj": 2e-14, "fc_adj": 5e-15, "sfc": 5e-15, "mu": 1e-15, "sd": 2e-15}


@pytest.fixture(scope="module")
def golden():
    return sr.load_golden()


@pytest.fixture(scope="module")
def restated(golden):
    return {name: sr.thresholded(c["y"], c["seeds"]) for name, c in golden.items()}


@pytest.mark.parametrize("name", list(sr.CASES))
def test_golden_inputs_are_the_generated_ones(golden, name):
    L, N, S, _ = sr.CASES[name]
    assert golden[name]["y"].shape == (L, N) and (golden[name]["y"] == sr.case_input(name)).all()
    assert (golden[name]["seeds"] == np.arange(1, S + 1)).all()


@pytest.mark.parametrize("name", list(sr.CASES))
def test_golden_cases_are_determinate(golden, name):
    """The condition, on the reference's outputs alone: no pair within 1e-9 of alpha, no pair without spread,
    and a fair share of the pairs on either side."""
    c = golden[name]
    p_adj = sr.uptri(c["p_adj"])
    assert np.abs(p_adj - sr.ALPHA).min() >= sr.MIN_GAP
    assert c["sd"].min() > 0
    kept = int((sr.uptri(c["fc_adj"]) != 0).sum())
    assert kept == int((p_adj < sr.ALPHA).sum()) and 0.05 * len(p_adj) < kept < 0.5 * len(p_adj)


@pytest.mark.parametrize("name", list(sr.CASES))
def test_restatement_matches_reference(golden, restated, name):
    c, r = golden[name], restated[name]
    dev = {"p_adj": np.abs(r["p_adj"] - c["p_adj"]).max(), "fc_adj": np.abs(r["fc_adj"] - c["fc_adj"]).max(),
           "sfc": np.abs(r["sfc"][:3] - c["sfc3"]).max(), "mu": np.abs(r["mu"] - c["mu"]).max(),
           "sd": np.abs(r["sd"] - c["sd"]).max()}
    print(name, dev, "margins", sr.margins(r))
    for k, v in dev.items():
        assert v <= TOL[k], (k, v)
    assert ((r["fc_adj"] != 0) == (c["fc_adj"] != 0)).all()              # the kept set, exactly
    gap, sd_min = sr.margins(r)
    assert gap >= sr.MIN_GAP and sd_min > 0
    for m in (r["p_adj"], r["fc_adj"]):
        assert (m == m.T).all() and (np.diag(m) == 0).all()


@pytest.mark.parametrize("name", list(sr.CASES))
def test_parseval_identity(golden, name):
    """The Gram matrix of the rotated bins against the reference's loop: ifft, .real, corrcoef."""
    c = golden[name]
    seeds = c["seeds"][:4]
    freq, time = sr.surrogate_fc(c["y"], seeds), sr.surrogate_fc_time(c["y"], seeds)
    assert np.abs(freq - time).max() <= TOL["sfc"]
    assert (time[:3] == c["sfc3"]).all()          # the time-domain restatement is the reference's loop, bit for bit


def test_phase_stream_known_answer():
    """Philox4x32-10's published vectors, the vectorised block against louvain_reference's, and which word of
    which block a phase takes."""
    assert tuple(sr.philox_blocks(0, 0, 0, 0, key=(0, 0))) == (0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8)
    assert tuple(sr.philox_blocks(0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344, key=(0xA4093822, 0x299F31D0))) \
        == (0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1)
    seed, h, N = (5 << 32) | 7, 9, 11
    w = sr.phase_words(seed, h, N)
    assert w.shape == (h, N) and w.max() < 1 << 32
    for k in (0, 3, 8):
        for n in (0, 3, 4, 10):
            assert int(w[k, n]) == lr.philox4x32_10((k, n >> 2, 7, 5))[n & 3]
    assert (w[:, :8] == lr.sweep_keys(seed, 2, 8)[None, :])[2].all()     # row k is sweep k's keys: one stream
    rv = sr.phases(seed, h, N)
    assert (rv == 2 * np.pi * (w * 2.0 ** -32)).all() and rv.min() >= 0 and rv.max() < 2 * np.pi
    assert (sr.phases(1, 4, 6) != sr.phases(2, 4, 6)).all()


@pytest.mark.parametrize("p", [
    np.array([0.01, 0.04, 0.04, 0.03, 0.5, 1.0, 1.0, 0.0, 0.0, 0.2]),
    np.array([0.0, 0.0]), np.array([1.0, 1.0, 1.0]), np.array([0.3]),
    np.random.default_rng(3).uniform(size=4560) ** 3,
    np.round(np.random.default_rng(4).uniform(size=500), 2),
], ids=["ties", "zeros", "ones", "single", "P4560", "rounded"])
def test_benjamini_hochberg_matches_scipy(p):
    assert (sr.benjamini_hochberg(p) == stats.false_discovery_control(p, method="bh")).all()


def test_upper_tail_saturates_as_the_reference():
    z = np.array([-40.0, -1.0, 0.0, 0.5, 1.5, 8.0, 8.5, 40.0])
    assert (sr.upper_tail(z) == 1 - stats.norm.cdf(z)).all()
    assert sr.upper_tail(8.5) == 0.0 and sr.upper_tail(8.0) > 0.0


def test_nan_convention_of_the_restatement():
    y = sr.case_input("tiny")
    y[:, 2] = 1.5
    r = sr.thresholded(y, sr.case_seeds("tiny"))
    assert np.isnan(r["p_adj"]).all() and np.isnan(r["fc_adj"]).all()
    same = np.tile(np.linspace(-0.5, 0.5, 10), (4, 1))                   # every surrogate the same: sd = 0
    r = sr.surrogate_test(np.corrcoef(sr.case_input("tiny").T), same)
    assert (r["sd"] == 0).all() and np.isnan(r["p_adj"]).all()


# ---- what the Python layers refuse, on CPU tensors, before the device is touched ----

def _x(L=16, N=5, B=None, dtype=torch.float64):
    return torch.zeros((L, N) if B is None else (L, B, N), dtype=dtype)


@pytest.mark.parametrize("call, exc, text", [
    (lambda: surrogate.fc_surrogate_test(_x(L=15)), ValueError, "L = 15, needs an even number of samples"),
    (lambda: surrogate.fc_surrogate_test(_x(L=2)), ValueError, "L = 2, needs an even number of samples"),
    (lambda: surrogate.fc_surrogate_test(_x(L=4098)), ValueError, "L = 4098 > 4096"),
    (lambda: surrogate.fc_surrogate_test(_x(N=1)), ValueError, "N = 1, B = 1"),
    (lambda: surrogate.fc_surrogate_test(_x(N=97, B=2)), ValueError, "N = 97, B = 2"),
    (lambda: surrogate.fc_surrogate_test(_x(B=0)), ValueError, "B = 0"),
    (lambda: surrogate.fc_surrogate_test(_x(), surr_number=1), ValueError, "surr_number = 1, must be an int of at least 2"),
    (lambda: surrogate.fc_surrogate_test(_x(), surr_number=2.0), ValueError, "surr_number = 2.0"),
    (lambda: surrogate.fc_surrogate_test(_x(), alpha=0.0), ValueError, "alpha = 0.0, must lie in (0, 1)"),
    (lambda: surrogate.fc_surrogate_test(_x(), alpha=1), ValueError, "alpha = 1, must lie in (0, 1)"),
    (lambda: surrogate.fc_surrogate_test(_x(), alpha=float("nan")), ValueError, "alpha = nan"),
    (lambda: surrogate.fc_surrogate_test(_x(), surr_number=3, seeds=[1, 2]), ValueError, "sequence of surr_number = 3 ints"),
    (lambda: surrogate.fc_surrogate_test(_x(), surr_number=2, seeds=[1, -2]), ValueError, "ints in [0, 2^64)"),
    (lambda: surrogate.fc_surrogate_test(_x(dtype=torch.float32)), TypeError, "x must be a [L][N] or time-major [L][B][N] fp64"),
    (lambda: surrogate.fc_surrogate_test(torch.zeros(16, dtype=torch.float64)), TypeError, "x must be a [L][N]"),
    (lambda: surrogate.fc_surrogate_test(torch.zeros((16, 2, 3, 5), dtype=torch.float64)), TypeError, "x must be a [L][N]"),
    (lambda: surrogate.fc_surrogate_test(np.zeros((16, 5))), TypeError, "x must be a [L][N]"),
    (lambda: surrogate.fc_surrogate_test(_x(), surr_number=8, ws_bytes=8 * 8 * 10 - 1), ValueError,
     "ws_bytes = 639, needs at least one simulation's slab of 8 S P = 640 bytes"),
    (lambda: surrogate.fc_surrogate_test(_x(), ws_bytes=1e9), ValueError, "ws_bytes = 1000000000.0"),
    (lambda: surrogate.surrogate_fc(_x(L=15), [1, 2]), ValueError, "surrogate_fc: L = 15"),
    (lambda: surrogate.surrogate_fc(_x(N=97), [1, 2]), ValueError, "surrogate_fc: N = 97"),
    (lambda: surrogate.surrogate_fc(_x(), [1]), ValueError, "surrogate_fc: seeds must be a sequence of at least 2 ints"),
    (lambda: surrogate.surrogate_fc(_x(), 3), ValueError, "surrogate_fc: seeds must be a sequence of at least 2 ints"),
    (lambda: surrogate.surrogate_fc(_x(dtype=torch.int64), [1, 2]), TypeError, "surrogate_fc: x must be"),
    (lambda: graph_utils.probabilistic_thresholding(np.zeros((16, 5)), conn="wpli"), KeyError, "invalid connectivity metric"),
    (lambda: graph_utils.probabilistic_thresholding(np.zeros((15, 5))), ValueError, "probabilistic_thresholding: L = 15"),
    (lambda: graph_utils.probabilistic_thresholding(np.zeros((3, 16, 97))), ValueError, "N = 97, B = 3"),
    (lambda: graph_utils.probabilistic_thresholding(np.zeros((16, 5)), surr_number=1), ValueError, "surr_number = 1"),
    (lambda: graph_utils.probabilistic_thresholding(np.zeros((16, 5)), alpha=1.5), ValueError, "alpha = 1.5"),
    (lambda: graph_utils.probabilistic_thresholding(np.zeros(16)), TypeError, "y must be a real [L, N] array"),
    (lambda: graph_utils.probabilistic_thresholding(np.zeros((16, 5), dtype=complex)), TypeError, "y must be a real"),
])
def test_python_layers_refuse(call, exc, text):
    with pytest.raises(exc) as e:
        call()
    assert text in str(e.value)


def test_facade_signature_is_the_references():
    import inspect
    assert str(inspect.signature(graph_utils.probabilistic_thresholding)) == "(y, surr_number=50, alpha=0.05, conn='corr')"
    assert surrogate.surrogate_slab_bytes(90, 50) == 50 * 4005 * 8


def test_library_validates_without_device_work():
    from nremmodfc_amd import _lib
    L = _lib.lib()
    vp, v8 = ctypes.c_void_p(1 << 20), ctypes.c_void_p((1 << 20) + 8)
    far = [ctypes.c_void_p((k + 2) << 30) for k in range(6)]
    fc = lambda B=2, N=5, Ln=16, S=4, spec=far[0], seeds=far[1], sfc=far[2]: \
        L.wc_surrogate_fc(B, N, Ln, S, spec, seeds, sfc, None)                                    # noqa: E731
    for kw, rc, text in [(dict(B=0), -1, b"B < 1"), (dict(N=1), -1, b"N < 2"), (dict(N=97), -2, b"N = 97 > 96"),
                         (dict(S=1), -1, b"S = 1"), (dict(Ln=15), -1, b"L = 15 is odd"), (dict(Ln=2), -1, b"L = 2 < 4"),
                         (dict(Ln=4098), -2, b"L = 4098 > 4096"), (dict(B=1 << 20, S=1 << 12), -1, b"2^31"),
                         (dict(spec=None), -1, b"NULL"), (dict(spec=v8), -1, b"spec must be 16-byte aligned"),
                         (dict(seeds=ctypes.c_void_p((3 << 30) + 4)), -1, b"seeds must be 8-byte aligned"),
                         (dict(sfc=far[0]), -1, b"sfc must not alias spec")]:
        assert fc(**kw) == rc, kw
        assert text in L.wc_last_error(), (kw, L.wc_last_error())
    ts = lambda B=2, N=5, S=4, alpha=0.05, fcm=far[0], sfc=far[1], pa=far[2], fa=far[3], mu=None, sd=None, p=None: \
        L.wc_surrogate_test(B, N, S, fcm, sfc, alpha, pa, fa, mu, sd, p, None)                    # noqa: E731
    for kw, rc, text in [(dict(B=0), -1, b"B < 1"), (dict(N=97), -2, b"N = 97 > 96"), (dict(S=1), -1, b"S = 1"),
                         (dict(alpha=0.0), -1, b"alpha"), (dict(alpha=1.0), -1, b"alpha"),
                         (dict(alpha=float("nan")), -1, b"alpha"), (dict(pa=None), -1, b"NULL"),
                         (dict(fa=far[2]), -1, b"fc_adj must not alias p_adj"), (dict(pa=far[1]), -1, b"p_adj must not alias sfc"),
                         (dict(mu=far[3]), -1, b"mu must not alias fc_adj"), (dict(p=vp, sd=vp), -1, b"p must not alias sd"),
                         (dict(fcm=ctypes.c_void_p((2 << 30) + 4)), -1, b"fc must be 8-byte aligned")]:
        assert ts(**kw) == rc, kw
        assert text in L.wc_last_error(), (kw, L.wc_last_error())
    assert L.wcsde_abi_version() == 7

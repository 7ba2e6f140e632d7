"""Dynamic FC on the device (wc_fcd, wc_fcd_phase through sigchain.fcd, fcd_from_phasors, fcd_ks,
utils.fcd and run_sweep(want_fcd=...)) against tests/fcd_reference.py, the numpy restatement of the
definitions (np.corrcoef per window, two-pass Pearson between the patterns, explicit cosine matrices).

Deviation: fcd_reference.deviation, the largest |got - want| (every value lies in [-1, 1]); NaN must be
in the same places.  Bounds: fcd, the patterns and fcd_phase 1e-12, the project's fp64 bound; symmetry and
the unit diagonal exact; bit identity exact; fcd_ks 1e-15.

Sizes: N in 3, 16, 17, 64, 65, 90, 96 with (M, W, S) in (12, 3, 1), (12, 12, 1) (one window: fcd = [[1]]),
(40, 10, 3) (rows 37 .. 39 fit no window: poisoned with NaN) and (70, 9, 2); 298 x 90, W = 30, S = 1,
B = 3 (269 windows).  The kernels' own boundaries, a case on either side:
  the 16 x 16 thread grid's cells (N a multiple of 16): N = 32 | 33, 48 | 49, 80 | 81 (16 | 17 and 64 | 65 above)
  rows of a window in LDS at a time, 32: W = 32 | 33
  the 64 x 64 tiles of fcd: nw = 64 | 65, and 129 (three tiles a side)
  pattern entries of a tile in LDS at a time, 32: P = 28 | 36 (N = 8 | 9); the 256 threads of the
    patterns' sums: P = 253 | 276 (N = 23 | 24)
  simulations a chunk (8 with the minimum workspace): B = 8 | 9, B = 19 in three chunks
  the 32 x 32 tiles of fcd_phase: M = 32 | 33, 64 | 65; its nodes in LDS at a time, 32: N = 32 | 33; the
    16 times a workgroup of its norms: M = 16 | 17; the norms' 16 interleaved parts: N = 2 .. 6, 17

Measured on MI355X, largest deviation over the cases of a test (fcd / patterns):
  test_sizes, N = 3 .. 96, four shapes:        3.2e-15 / 4.4e-16
  test_product_shape, 298 x 90, B = 3:         6.8e-15 / 6.7e-16
  test_kernel_boundaries:                      2.3e-15 / 5.6e-16
  test_isolation_of_a_degenerate_window:       2.2e-16 / 4.4e-16
  test_chunks_of_simulations, B = 8, 9, 19:    4.4e-16 / 4.4e-16
  test_phase_sizes (fcd_phase):                4.2e-15 (N = 96, M = 33); N = 2: 0
  test_phase_method_from_a_series:             7.2e-16
No measure needs more than the 1e-12 bound.
"""
import functools

import numpy as np
import pytest
import torch

from nremmodfc_amd import _lib, utils
from nremmodfc_amd import sigchain as wsg
from tests import fcd_reference as ref

pytestmark = pytest.mark.gpu

BOUND = 1e-12
SHAPES = ((12, 3, 1), (12, 12, 1), (40, 10, 3), (70, 9, 2))


def frozen(a):
    a = np.asarray(a)
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def series(M, B, N, seed, W, S):
    return frozen(ref.make_input(M, B, N, seed, W, S))


@functools.lru_cache(maxsize=None)
def reference(M, B, N, seed, W, S):
    """fcd_reference.fcd_batch of series(...), computed once, read only."""
    f, v = ref.fcd_batch(series(M, B, N, seed, W, S), W, S)
    return frozen(f), frozen(v)


def device(x, W, S, **kw):
    f, v = wsg.fcd(torch.from_numpy(np.array(x)).cuda(), W, S, want_windows=True, **kw)
    return f.cpu().numpy(), v.cpu().numpy()


def check(got, want, tag):
    """The bounds of the module docstring on (fcd, patterns) of a batch; prints the deviations."""
    (f, v), (wf, wv) = got, want
    dev = ref.deviation(f, wf), ref.deviation(v, wv)
    print(f"{tag}: fcd {dev[0]:.1e}  patterns {dev[1]:.1e}")
    assert dev[0] <= BOUND and dev[1] <= BOUND, (tag, dev)
    for m in f:
        np.testing.assert_array_equal(m, m.T)                                # NaN in the same places too
        d = np.diag(m)
        assert ((d == 1.0) | np.isnan(d)).all()
    return dev


@pytest.mark.parametrize("M,W,S", SHAPES)
@pytest.mark.parametrize("n", [3, 16, 17, 64, 65, 90, 96])
def test_sizes(n, M, W, S):
    x, want = series(M, 1, n, n + M, W, S), reference(M, 1, n, n + M, W, S)
    nw = (M - W) // S + 1
    if (M - W) % S:                                              # the tail rows fit no window: never read
        x = np.array(x)
        x[(nw - 1) * S + W:] = np.nan
    got = device(x, W, S)
    assert got[0].shape == (1, nw, nw) and got[1].shape == (1, nw, n * (n - 1) // 2)
    assert np.isfinite(got[0]).all() and np.isfinite(got[1]).all()
    check(got, want, f"N={n} M={M} W={W} S={S}")
    if nw == 1:
        assert got[0].tolist() == [[[1.0]]]
    single = wsg.fcd(torch.from_numpy(np.array(x[:, 0])).cuda(), W, S)       # [M][N] in, no batch axis out
    np.testing.assert_array_equal(single.cpu().numpy(), got[0][0])


def test_product_shape():
    x, want = series(298, 3, 90, 298, 30, 1), reference(298, 3, 90, 298, 30, 1)
    got = device(x, 30, 1)
    assert got[0].shape == (3, 269, 269) and got[1].shape == (3, 269, 4005)
    check(got, want, "298 x 90, W=30, S=1, B=3")
    only = wsg.fcd(torch.from_numpy(np.array(x)).cuda(), 30)                 # without the patterns: the same bits
    np.testing.assert_array_equal(only.cpu().numpy(), got[0])


@pytest.mark.parametrize("n,M,W,S", [
    (32, 20, 6, 2), (33, 20, 6, 2), (48, 20, 6, 2), (49, 20, 6, 2), (80, 20, 6, 2), (81, 20, 6, 2),  # thread-grid cells
    (5, 40, 32, 1), (5, 40, 33, 1),                                            # rows of a window in LDS
    (5, 67, 4, 1), (5, 68, 4, 1), (5, 132, 4, 1),                              # nw = 64 | 65, 129
    (8, 20, 6, 2), (9, 20, 6, 2), (23, 20, 6, 2), (24, 20, 6, 2),              # P = 28 | 36, 253 | 276
])
def test_kernel_boundaries(n, M, W, S):
    seed = 7 * n + M
    check(device(series(M, 1, n, seed, W, S), W, S), reference(M, 1, n, seed, W, S), f"N={n} M={M} W={W} S={S}")


def test_isolation_of_a_degenerate_window():
    """Simulation 2 of 5 has column 4 constant over rows 20 .. 29, exactly window 2 of (40, 10, 10)."""
    M, W, S, B, N = 40, 10, 10, 5, 17
    clean = series(M, B, N, 40, W, S)
    x = np.array(clean)
    x[20:30, 2, 4] = 3.25
    got = device(x, W, S)
    want = ref.fcd_batch(x, W, S)
    assert np.isnan(want[0][2, 2]).all() and np.isnan(want[0][2, :, 2]).all() and np.isnan(want[0]).sum() == 7
    assert np.isnan(want[1]).sum() == N - 1                      # the entries of pattern 2 that involve column 4
    check(got, want, "B=5, window 2 of simulation 2 degenerate")              # NaN in the same places, the rest 1e-12
    assert np.isnan(got[0][2, 2, 2])                             # the diagonal too
    untouched = device(clean, W, S)
    for b in (0, 1, 3, 4):                                       # the other simulations: the same bits
        np.testing.assert_array_equal(got[0][b], untouched[0][b])
        np.testing.assert_array_equal(got[1][b], untouched[1][b])
    keep = np.array([0, 1, 3])                                   # and the other windows of simulation 2
    np.testing.assert_array_equal(got[0][2][np.ix_(keep, keep)], untouched[0][2][np.ix_(keep, keep)])
    np.testing.assert_array_equal(got[1][2][keep], untouched[1][2][keep])


def test_bit_identity_across_batch_position_and_workspace():
    M, W, S, N = 70, 9, 2, 17
    x = series(M, 7, N, 70, W, S)
    need = _lib.lib().wc_fcd_workspace_size(7, N, M, W, S)
    base = device(x, W, S, ws_bytes=need)
    for ws in (4 * need, None):
        for a, b in zip(device(x, W, S, ws_bytes=ws), base):
            np.testing.assert_array_equal(a, b)
    alone = device(x[:, 3:4], W, S)
    twice = np.array(x)
    twice[:, 6] = x[:, 3]                                        # the same simulation at positions 3 and 6
    both = device(twice, W, S)
    for k in range(2):
        np.testing.assert_array_equal(alone[k][0], base[k][3])
        np.testing.assert_array_equal(both[k][3], alone[k][0])
        np.testing.assert_array_equal(both[k][6], alone[k][0])
    with pytest.raises(_lib.WCSDEError, match="EWORKSPACE"):
        device(x, W, S, ws_bytes=need - 8)


@pytest.mark.parametrize("B", [8, 9, 19])
def test_chunks_of_simulations(B):
    """The minimum workspace holds 8 simulations: B = 9 and 19 go through it in two and three chunks."""
    M, W, S, N = 40, 10, 3, 9
    x, want = series(M, B, N, B, W, S), reference(M, B, N, B, W, S)
    need = _lib.lib().wc_fcd_workspace_size(B, N, M, W, S)
    assert need == min(B, 8) * (11 * 36 + 11) * 8
    got = device(x, W, S, ws_bytes=need)
    check(got, want, f"B={B}, minimum workspace")
    for a, b in zip(device(x, W, S), got):                      # the default workspace takes all B at once
        np.testing.assert_array_equal(a, b)


def phasors(M, B, N, seed):
    rng = np.random.default_rng(seed)
    th = np.cumsum(rng.uniform(0.05, 0.6, size=(M, B, N)), axis=0) + rng.uniform(-np.pi, np.pi, size=(1, B, N))
    return np.stack((np.cos(th), np.sin(th)), axis=-1)


@pytest.mark.parametrize("n,M", [(2, 12), (3, 12), (4, 33), (5, 32), (6, 65), (17, 64), (32, 16), (33, 17), (64, 40),
                                 (65, 40), (90, 70), (96, 33)])
def test_phase_sizes(n, M):
    ph = phasors(M, 2, n, n + M)
    got = wsg.fcd_from_phasors(torch.from_numpy(ph).cuda()).cpu().numpy()
    assert got.shape == (2, M, M)
    dev = max(ref.deviation(got[b], ref.fcd_phase(ph[:, b])) for b in range(2))
    print(f"phase N={n} M={M}: {dev:.1e}")
    assert dev <= BOUND
    for m in got:
        np.testing.assert_array_equal(m, m.T)
        assert (np.diag(m) == 1.0).all()
    single = wsg.fcd_from_phasors(torch.from_numpy(np.array(ph[:, 1])).cuda()).cpu().numpy()
    np.testing.assert_array_equal(single, got[1])


def test_phase_zero_norm_and_bits():
    ph = phasors(40, 3, 2, 5)
    ph[7, 1] = [[0.6, 0.8], [-0.8, 0.6]]                         # simulation 1, time 7: pi / 2 apart, d = 0 exactly
    got = wsg.fcd_from_phasors(torch.from_numpy(ph).cuda()).cpu().numpy()
    want = np.stack([ref.fcd_phase(ph[:, b]) for b in range(3)])
    assert np.isnan(want[1, 7]).all() and np.isnan(want[1, :, 7]).all() and np.isnan(want).sum() == 79
    assert ref.deviation(got, want) <= BOUND
    alone = wsg.fcd_from_phasors(torch.from_numpy(np.array(ph[:, 2:3])).cuda()).cpu().numpy()
    np.testing.assert_array_equal(alone[0], got[2])


def test_phase_method_from_a_series():
    """sigchain.fcd(method="phase", trim=2) is the restatement applied to hilbert_phase's own phasors."""
    M, B, N = 70, 2, 17
    x = torch.from_numpy(np.array(series(M, B, N, 71, 9, 2))).cuda()
    x = x - x.mean(dim=0, keepdim=True)
    got = wsg.fcd(x, method="phase", trim=2).cpu().numpy()
    ph = wsg.hilbert_phase(x.reshape(M, B * N).contiguous()).view(M, B, N, 2).cpu().numpy()[2:-2]
    assert got.shape == (B, M - 4, M - 4)
    dev = max(ref.deviation(got[b], ref.fcd_phase(ph[:, b])) for b in range(B))
    print(f"fcd(method='phase', trim=2): {dev:.1e}")
    assert dev <= BOUND
    np.testing.assert_array_equal(wsg.fcd(x[:, 1].contiguous(), method="phase", trim=2).cpu().numpy(), got[1])
    np.testing.assert_array_equal(utils.fcd(x.cpu().numpy(), method="phase", trim=2), got)


def test_fcd_ks_on_device_output():
    M, W, S, B, N = 70, 9, 2, 3, 17
    f = wsg.fcd(torch.from_numpy(np.array(series(M, B, N, 70, W, S)[:, :B])).cuda(), W, S)
    emp = np.random.default_rng(1).uniform(-0.5, 1.0, 301)
    host = f.cpu().numpy()
    for lag in (1, W // S):
        got = wsg.fcd_ks(f, emp, lag).cpu().numpy()
        want = np.array([ref.fcd_ks(m, emp, lag) for m in host])
        assert got.shape == (B,) and np.abs(got - want).max() <= 1e-15
    f[1, 2, 20] = float("nan")
    got = wsg.fcd_ks(f, emp, 1).cpu().numpy()
    assert np.isnan(got[1]) and np.isfinite(got[[0, 2]]).all()


def test_utils_fcd_round_trips_float32():
    x32 = np.array(series(40, 2, 9, 41, 10, 3), dtype=np.float32)
    got = utils.fcd(x32, window=10, step=3)
    assert got.dtype == np.float64 and got.shape == (2, 11, 11)
    want, _ = ref.fcd_batch(x32.astype(np.float64), 10, 3)
    assert ref.deviation(got, want) <= BOUND
    one = utils.fcd(x32[:, 0], window=10, step=3)
    np.testing.assert_array_equal(one, got[0])


def test_run_sweep_want_fcd(sc90):
    from nremmodfc_amd.model import Schedule, sim_keys
    from nremmodfc_amd.pipeline import run_sweep
    sch = Schedule(n_trans1=200, n_trans2=2000, n_sim=100_000)   # 5000 recorded samples: M = 30 at bold_downsamp 100
    G, S, keys = np.array([0.16, 0.22]), np.array([7.68, 7.80]), sim_keys([0, 1], [0, 5])
    res = run_sweep(sc90, G, S, keys, {}, sch, bold_downsamp=100, want_bold=True, want_fcd=(8, 2))
    M = res.bold.shape[0]
    assert M >= 12 and res.fcd.shape == (2, (M - 8) // 2 + 1, (M - 8) // 2 + 1)
    want = wsg.fcd(torch.from_numpy(res.bold).cuda(), 8, 2).cpu().numpy()
    np.testing.assert_array_equal(res.fcd, want)
    assert np.isfinite(res.fcd).all()
    plain = run_sweep(sc90, G, S, keys, {}, sch, bold_downsamp=100, want_bold=True)
    assert plain.fcd is None
    np.testing.assert_array_equal(plain.bold, res.bold)

"""Phase and envelope connectivity on the device (wc_phase_conn, sigchain.phase_connectivity,
utils.connectivity) against tests/conn_reference.py, a numpy loop over the columns from
scipy.signal.hilbert that test_connectivity_cpu.py pins.

Deviation: max |got - want| over the off-diagonal entries.  Bounds.  pli: exactly equal (an integer
sum over T; every compared case asserts that no sample of the reference has |s| < 1e-10, and the
device's phasors are within 4.6e-15 of SciPy's).  plv, wpli, aec: 1e-12, the project's fp64 bound
(means of products of two phasors are within about 1e-14).  aec is also bit-equal, in its entries
i < j, to sigchain.corrcoef of sigchain.hilbert_envelope.  aec_orth, a Pearson coefficient of a
derived series: 10x the largest deviation measured over these cases (4.7e-14), ORTH_BOUND.

Time blocks are 4096 samples (BLOCK): 4096 x 4 is exactly one, 8193 x 3 two and a remainder of one
sample, 20,000 x 6 four and a remainder.  Tiles are 32 columns: 1000 x 33, 4100 x 90, 300 x 130.

Measured on MI355X (plv / wpli / aec / aec_orth; pli exact everywhere):
  3 x 3: 2.2e-16 / 1.7e-16 / 1.3e-15 / 9.0e-15       64 x 7: 2.2e-16 / 3.3e-16 / 5.6e-16 / 1.2e-14
  257 x 7: 2.2e-16 / 7.8e-16 / 4.4e-16 / 1.3e-14     1000 x 33: 7.8e-16 / 1.4e-15 / 1.8e-15 / 1.7e-14
  2049 x 5: 4.2e-16 / 6.1e-16 / 5.6e-16 / 1.2e-14    4100 x 90: 1.3e-15 / 2.0e-15 / 3.7e-15 / 4.2e-14
  8193 x 3: 1.2e-16 / 4.2e-16 / 7.8e-16 / 5.2e-15    20000 x 6: 2.8e-15 / 1.4e-15 / 4.2e-15 / 7.1e-15
  4096 x 4: 1.1e-16 / 3.2e-16 / 1.3e-15 / 2.2e-14    8192 x 3: 1.8e-16 / 3.9e-16 / 7.8e-16 / 7.4e-15
  300 x 130: 6.7e-16 / 1.4e-15 / 1.4e-15 / 4.4e-14   64 x 1: the diagonals alone
  [298][3][90], worst simulation: 1.0e-15 / 2.0e-15 / 1.6e-15 / 4.7e-14
  utils.connectivity 6000 x 90, 8-13 Hz: 4.3e-15 / 5.4e-15 / 3.9e-15 / 3.4e-14 (the same with freqs=None on
    SciPy's band-passed array: the device's band-pass is bit-equal to SciPy's)
  a duplicated column: plv - 1 = 0 at 4100 x 6 and 300 x 130

aec beyond 96 columns is corrcoef of the envelopes of every pair of 48-column groups, so that an entry
depends on its two columns only, as for the four measures of wc_phase_conn (one wc_corrcoef call on 130
columns takes another kernel and differed from the 2-column call by 3.3e-16).
"""
import functools

import numpy as np
import pytest
import torch
from scipy import signal

from nremmodfc_amd import _lib, utils
from nremmodfc_amd import sigchain as wsg
from tests import conn_reference as ref

pytestmark = pytest.mark.gpu

BLOCK = 4096          # wc_phaseconn.hip's kBlk
BOUND = 1e-12
ORTH_BOUND = 4.7e-13  # 10x the largest measured deviation (4.7e-14, [298][3][90]); the cap would be 1e-9
SHAPES = [(3, 3), (64, 7), (257, 7), (1000, 33), (2049, 5), (4100, 90), (8193, 3), (20000, 6),
          (64, 1), (BLOCK, 4), (8192, 3), (300, 130)]
SEED = 1              # conn_reference.make meets the |s| >= 1e-10 condition with it at every shape here


def frozen(a):
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def case(T, C):
    """(x, reference dict, count of near-zero lags, smallest |s|): computed once per shape, read only."""
    x = frozen(ref.make(T, C, SEED))
    want = {m: frozen(v) for m, v in ref.connectivity(x).items()}
    n, least = ref.near_zero_lags(x) if C > 1 else (0, np.inf)
    return x, want, n, least


@functools.lru_cache(maxsize=None)
def device_case(T, C):
    """The device's five matrices of case(T, C) as numpy arrays."""
    got = wsg.phase_connectivity(torch.from_numpy(np.array(case(T, C)[0])).cuda())
    return {m: frozen(v.cpu().numpy()) for m, v in got.items()}


def check(got, want, tag):
    """Asserts the bounds of the module docstring; prints every deviation."""
    C = want["plv"].shape[-1]
    dev = {m: ref.deviation(got[m], want[m]) for m in ref.MEASURES}
    print(f"{tag}: " + "  ".join(f"{m} {dev[m]:.1e}" for m in ref.MEASURES))
    for m in ref.MEASURES:
        assert got[m].shape == want[m].shape
        np.testing.assert_array_equal(got[m], np.swapaxes(got[m], -1, -2))
        np.testing.assert_array_equal(np.diagonal(got[m], axis1=-2, axis2=-1), ref.DIAGONAL[m])
        if C > 1:
            assert np.abs(ref.off_diagonal(got[m])).max() <= 1.0
    assert dev["pli"] == 0.0
    assert dev["plv"] <= BOUND and dev["wpli"] <= BOUND and dev["aec"] <= BOUND
    assert dev["aec_orth"] <= ORTH_BOUND
    return dev


@pytest.mark.parametrize("T,C", SHAPES)
def test_against_reference(T, C):
    x, want, n, least = case(T, C)
    assert n == 0, f"{n} samples of the reference with |s| < 1e-10 (smallest {least:.1e}): change the seed"
    check(device_case(T, C), want, f"{T} x {C} (smallest |s| {least:.1e})")


def test_hilbert_boundary_takes_both_kernels():
    """8193 samples go through the long Hilbert kernel, 8192 through the direct one."""
    assert wsg.HILBERT_DIRECT_MAX_M == 8192
    for T in (8192, 8193):
        check(device_case(T, 3), case(T, 3)[1], f"{T} x 3")


def test_aec_is_corrcoef_of_the_envelope():
    """Bit-equal to sigchain.corrcoef(sigchain.hilbert_envelope(x)) in the entries i < j.  wc_corrcoef keeps
    np.corrcoef's division order in either triangle (c / sd_i / sd_j against c / sd_j / sd_i) and a computed
    diagonal, so its own matrix is symmetric and 1 on the diagonal only up to the last bit; the contract here
    is exact symmetry and an exact diagonal, so aec is corrcoef's upper triangle, mirrored.

    Beyond 96 columns wc_corrcoef changes kernels, and its entries differ in the last bit from those of a
    narrower call of the same columns; an aec entry must not depend on the other columns, so there aec is
    corrcoef of the envelopes of every pair of 48-column groups (sigchain._aec_corrcoef): checked group pair
    by group pair, with the difference from the 130-column corrcoef printed."""
    T, C = 1000, 33
    xd = torch.from_numpy(np.array(case(T, C)[0])).cuda()
    fc = wsg.corrcoef(wsg.hilbert_envelope(xd).view(T, 1, C), 1, C)[0]
    got = wsg.phase_connectivity(xd, ("aec",))["aec"]
    upper = torch.ones((C, C), dtype=torch.bool, device="cuda").triu(1)
    assert torch.equal(got[upper], fc[upper])
    assert torch.equal(got.t()[upper], fc[upper])
    assert (got.diagonal() == 1.0).all()
    print(f"aec {T} x {C}: corrcoef's lower triangle and diagonal differ from it by {(got - fc).abs().max().item():.1e}")
    np.testing.assert_array_equal(device_case(T, C)["aec"], got.cpu().numpy())

    T, C, G = 300, 130, wsg.AEC_GROUP
    assert G == 48
    xd = torch.from_numpy(np.array(case(T, C)[0])).cuda()
    env = wsg.hilbert_envelope(xd)
    got = wsg.phase_connectivity(xd, ("aec",))["aec"]
    groups = [list(range(g, min(g + G, C))) for g in range(0, C, G)]
    for ka, ga in enumerate(groups):
        for gb in groups[ka:]:
            cols = ga if gb is ga else ga + gb
            fc = wsg.corrcoef(env[:, cols].contiguous().view(T, 1, len(cols)), 1, len(cols))[0]
            sub = got[cols][:, cols]
            up = torch.ones((len(cols), len(cols)), dtype=torch.bool, device="cuda").triu(1)
            assert torch.equal(sub[up], fc[up]) and torch.equal(sub.t()[up], fc[up])
    assert (got.diagonal() == 1.0).all()
    whole = wsg.corrcoef(env.view(T, 1, C), 1, C)[0]
    print(f"aec {T} x {C}: differs from the 130-column corrcoef by {(got - whole).abs().max().item():.1e}")
    assert (got - whole).abs().max().item() <= 1e-14
    np.testing.assert_array_equal(device_case(T, C)["aec"], got.cpu().numpy())


@functools.lru_cache(maxsize=None)
def batched():
    """x [298][3][90] and the device's matrices of the whole and of each simulation."""
    x = frozen(ref.make(298, 270, SEED).reshape(298, 3, 90))
    xd = torch.from_numpy(np.array(x)).cuda()
    whole = {m: v.cpu().numpy() for m, v in wsg.phase_connectivity(xd).items()}
    each = [{m: v.cpu().numpy() for m, v in wsg.phase_connectivity(xd[:, b].contiguous()).items()} for b in range(3)]
    return x, whole, each


def test_batched_against_reference_and_per_simulation_calls():
    x, whole, each = batched()
    for b in range(3):
        n, least = ref.near_zero_lags(x[:, b])
        assert n == 0, f"simulation {b}: {n} samples with |s| < 1e-10 (smallest {least:.1e}): change the seed"
        check({m: whole[m][b] for m in ref.MEASURES}, ref.connectivity(x[:, b]), f"[298][3][90] b = {b}")
        for m in ref.MEASURES:
            assert whole[m].shape == (3, 90, 90)
            np.testing.assert_array_equal(whole[m][b], each[b][m])


@functools.lru_cache(maxsize=None)
def column_pairs():
    """[(i, j, the device's matrices of columns i and j of the 300 x 130 case alone)]: across tiles (3, 70),
    (40, 129), (31, 32), inside one (33, 34), (96, 129), (64, 95), and a diagonal tile's far corner (0, 31)."""
    x = case(300, 130)[0]
    res = []
    for i, j in ((3, 70), (40, 129), (33, 34), (96, 129), (0, 31), (31, 32), (64, 95)):
        two = wsg.phase_connectivity(torch.from_numpy(np.ascontiguousarray(x[:, [i, j]])).cuda())
        res.append((i, j, {m: v.cpu().numpy() for m, v in two.items()}))
    return res


@pytest.mark.parametrize("m", ref.MEASURES)
def test_entry_depends_on_its_two_columns_only(m):
    """An entry of the 130-column call is bit-identical to the 2-column call of its two columns.

    aec is wc_corrcoef of the envelopes, which beyond 96 columns changes kernels; sigchain._aec_corrcoef keeps
    it on the N <= 96 kernels by groups of 48 columns so that this holds for aec too (one wc_corrcoef call on
    130 columns differed from the 2-column call by 3.3e-16, one unit in the last place)."""
    big = device_case(300, 130)
    worst = 0.0
    for i, j, two in column_pairs():
        worst = max(worst, abs(two[m][0, 1] - big[m][i, j]))
    print(f"{m}: 130-column entry against the 2-column call, largest difference {worst:.1e}")
    for i, j, two in column_pairs():
        assert two[m][0, 1].tobytes() == big[m][i, j].tobytes(), (m, i, j, two[m][0, 1], big[m][i, j])
        assert two[m][1, 0].tobytes() == big[m][j, i].tobytes()


def raw_call(ph, amp, bits, ws_factor=1):
    """wc_phase_conn itself on [M][B][N][2] phasors -> out [popcount][B][N][N]."""
    L = _lib.lib()
    M, B, N = ph.shape[:3]
    need = L.wc_phase_conn_workspace_size(B, N, M, bits)
    assert need > 0
    nbytes = need * ws_factor
    ws = torch.full((nbytes // 8,), float("nan"), dtype=torch.float64, device=ph.device)
    out = torch.full((bin(bits).count("1"), B, N, N), float("nan"), dtype=torch.float64, device=ph.device)
    _lib.check(L.wc_phase_conn(B, N, M, _lib.ptr(ph), _lib.ptr(amp), bits, _lib.ptr(out), _lib.ptr(ws), nbytes,
                               _lib.stream_handle()), "wc_phase_conn")
    return out


def test_runs_workspace_and_measure_subsets_give_the_same_bits():
    T, C = 20000, 6                                                     # four time blocks and a remainder
    xd = torch.from_numpy(np.array(case(T, C)[0])).cuda()
    ph = wsg.hilbert_phase(xd).view(T, 1, C, 2)
    amp = wsg.hilbert_envelope(xd).view(T, 1, C)
    full = raw_call(ph, amp, 15)
    assert not torch.isnan(full).any()
    assert torch.equal(full, raw_call(ph, amp, 15))                     # two runs
    assert torch.equal(full, raw_call(ph, amp, 15, ws_factor=4))        # a 4x larger workspace
    assert torch.equal(full[:2], raw_call(ph, None, 3))                 # phase-only: no envelopes, fewer sums
    assert torch.equal(full[:2], raw_call(ph, None, 3, ws_factor=4))
    for bits in range(1, 15):                                           # every subset, in ascending bit order
        rows = [k for k in range(4) if bits & (1 << k)]
        assert torch.equal(full[rows], raw_call(ph, amp, bits)), bits
    got = device_case(T, C)
    for k, m in enumerate(("plv", "pli", "wpli", "aec_orth")):          # the facade is this call
        np.testing.assert_array_equal(full[k, 0].cpu().numpy(), got[m])
    only = wsg.phase_connectivity(xd, ("pli", "plv"))
    assert list(only) == ["pli", "plv"]
    np.testing.assert_array_equal(only["pli"].cpu().numpy(), got["pli"])


def test_duplicated_column():
    """Column 4 repeats column 1 (in another tile: column 40 repeats column 1): s is exactly 0 there."""
    for T, C, dup in ((4100, 6, 4), (300, 130, 40)):
        x = np.array(case(T, C)[0])
        x[:, dup] = x[:, 1]
        got = {m: v.cpu().numpy() for m, v in wsg.phase_connectivity(torch.from_numpy(x).cuda()).items()}
        nan = np.zeros((C, C), dtype=bool)
        nan[1, dup] = nan[dup, 1] = True
        assert got["pli"][1, dup] == 0.0 and got["pli"][dup, 1] == 0.0
        for m in ("wpli", "aec_orth"):
            np.testing.assert_array_equal(np.isnan(got[m]), nan)
        for m in ("plv", "pli", "aec"):
            assert not np.isnan(got[m]).any()
        assert abs(got["plv"][1, dup] - 1.0) <= BOUND
        print(f"duplicated column, {T} x {C}: plv - 1 = {got['plv'][1, dup] - 1.0:.1e}")
        keep = [c for c in range(C) if c != dup]                        # the other pairs: as without the copy
        base = device_case(T, C)
        for m in ref.MEASURES:
            np.testing.assert_array_equal(got[m][np.ix_(keep, keep)], base[m][np.ix_(keep, keep)])


@functools.lru_cache(maxsize=None)
def facade_case():
    """x [6000][90], SciPy's band-passed x (8-13 Hz at dt = 0.002) and the reference of that."""
    x = frozen(ref.make(6000, 90, SEED))
    b, a = signal.bessel(3, [2 * 0.002 * 8, 2 * 0.002 * 13], btype="bandpass")
    v = frozen(signal.filtfilt(b, a, x, axis=0))
    return x, v, ref.connectivity(v)


def test_utils_connectivity_against_scipy_chain():
    """The band-pass is bit-equal to SciPy's (test_envelope_gpu.py), so the bounds are not loosened."""
    x, v, want = facade_case()
    n, least = ref.near_zero_lags(v)
    assert n == 0, f"{n} samples with |s| < 1e-10 (smallest {least:.1e}): change the seed"
    got = utils.connectivity(x, dt=0.002, freqs=[8, 13])
    assert list(got) == list(ref.MEASURES) and all(isinstance(g, np.ndarray) for g in got.values())
    check(got, want, f"utils.connectivity 6000 x 90 (smallest |s| {least:.1e})")


def test_utils_connectivity_options():
    x, v, want = facade_case()
    # freqs=None: the series is taken as band-limited already
    got = utils.connectivity(v, freqs=None)
    check(got, want, "utils.connectivity freqs=None")
    # float32 input is widened exactly
    x32 = x[:, :7].astype(np.float32)
    got32 = utils.connectivity(x32, measures=("plv", "aec_orth"))
    got64 = utils.connectivity(x32.astype(np.float64), measures=("plv", "aec_orth"))
    assert list(got32) == ["plv", "aec_orth"]
    for m in got32:
        np.testing.assert_array_equal(got32[m], got64[m])
    # [time][B][N]: pairs within a simulation only
    x3 = x[:, :24].reshape(6000, 3, 8)
    got3 = utils.connectivity(x3)
    for b in range(3):
        one = utils.connectivity(np.ascontiguousarray(x3[:, b]))
        for m in ref.MEASURES:
            assert got3[m].shape == (3, 8, 8)
            np.testing.assert_array_equal(got3[m][b], one[m])

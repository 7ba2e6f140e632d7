"""What the core chain does with a NaN, an infinity or a constant column ("non-finite
inputs"): wc_fc_metrics, wc_corrcoef, the Hilbert phasors behind wc_kuramoto, wc_hma / wc_hma_modes.

FC, goodness of fit, Kuramoto.  Simulation b = 1 of a batch of three random walks carries a defect:
  const   one column constant at 0.5 (mean and centred values exact, so its standard deviation is
          exactly 0 and np.corrcoef has 2 N - 1 NaN)
  nan     one NaN sample
  inf     one +Inf sample
  allnan  every sample NaN
and the references are numpy and the oracle on the same input (np.corrcoef, oracle.sigchain's
get_all_metrics and kuramoto).  Asserted: isnan of every device output equals isnan of the reference,
element for element; where the reference is finite the device is within the bound the entry point's
own test uses (FC 1e-12 absolute; get_all_metrics rtol 1e-9, atol 1e-12; mean(FC) rtol 1e-12; Kuramoto
rtol 1e-9; test_signal_gpu.py, test_large_n_gpu.py, test_hilbert_long_gpu.py); and every output of
simulations 0 and 2 is bit-identical to a run of the batch with a clean simulation 1.

HMA.  The clip comes first, as in the reference (FC[FC < 0] = 0: -Inf becomes 0, a NaN stays).  A
matrix that then holds a NaN or +Inf has NaN in hin, hse, hin_node, hse_node and sv and -1 in every
clus_num, keeps those entries, and leaves its neighbours in the batch bit-identical to a run without it.
"""
import functools

import numpy as np
import pytest
import torch

import oracle.sigchain as osg
from nremmodfc_amd import HMA, _lib, datasets
from nremmodfc_amd import sigchain as wsg

pytestmark = pytest.mark.gpu

DEFECTS = ("const", "nan", "inf", "allnan")
COL = 2  # the column of simulation 1 that carries the defect


def _walks(M, B, N):
    """Ordinary random-walk simulations [M][B][N], as test_signal_gpu.py's."""
    rng = np.random.default_rng(1000 * M + 10 * N + B)
    return rng.standard_normal((M, B, N)).cumsum(0) + rng.standard_normal((M, B, 1))


def _with_defect(x, kind):
    x = x.copy()
    M = x.shape[0]
    if kind == "const":
        x[:, 1, COL] = 0.5
    elif kind == "nan":
        x[M // 3, 1, COL] = np.nan
    elif kind == "inf":
        x[M // 3, 1, COL] = np.inf
    elif kind == "allnan":
        x[:, 1, :] = np.nan
    else:
        raise ValueError(kind)
    return x


def _emp(N):
    """Two empirical matrices: the project's own at N = 90, correlation matrices of noise elsewhere."""
    if N == 90:
        return np.stack([datasets.load_empfc(s) for s in ("W", "N3")])
    rng = np.random.default_rng(N)
    return np.stack([np.corrcoef(rng.standard_normal((3 * N, N)).T + 0.3 * k) for k in range(2)])


@functools.lru_cache(maxsize=None)
def _reference(M, B, N, kind):
    """(x, fc [B][N][N], metrics [B][2][4], extra [B][3]) of numpy and the oracle: computed once per
    case, read only."""
    x = _with_defect(_walks(M, B, N), kind)
    emp = _emp(N)
    with np.errstate(all="ignore"):
        fc = np.stack([np.corrcoef(x[:, b, :].T) for b in range(B)])
        met = np.array([[osg.get_all_metrics(fc[b], e, 1) for e in emp] for b in range(B)])
        kur = [osg.kuramoto(x[:, b, :]) for b in range(B)]
        extra = np.array([[fc[b].mean(), kur[b][0], kur[b][1]] for b in range(B)])
    for a in (x, fc, met, extra):
        a.setflags(write=False)
    return x, fc, met, extra


def _check(got, want, rtol, atol, what):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    np.testing.assert_array_equal(np.isnan(got), np.isnan(want), err_msg=f"{what}: NaN pattern")
    ok = ~np.isnan(want)
    np.testing.assert_allclose(got[ok], want[ok], rtol=rtol, atol=atol, err_msg=what)


def _check_fc_metrics(got, want, kuramoto=True):
    fc, met, extra = (None if t is None else t.cpu().numpy() for t in got)
    wfc, wmet, wextra = want
    if fc is not None:
        _check(fc, wfc, 0, 1e-12, "FC")
    for b in range(met.shape[0]):
        for k in range(met.shape[1]):
            _check(met[b, k], wmet[b, k], 1e-9, 1e-12, f"get_all_metrics b={b} k={k}")
    _check(extra[:, 0], wextra[:, 0], 1e-12, 0, "mean(FC)")
    if kuramoto:
        _check(extra[:, 1:], wextra[:, 1:], 1e-9, 0, "kuramoto")


def _neighbours_equal(got, clean):
    for g, c in zip(got, clean):
        if g is not None:
            assert torch.equal(g[0], c[0]) and torch.equal(g[2], c[2])


def test_reference_has_the_nan_the_contract_speaks_of():
    """No GPU in this one: the defects do to numpy what the module docstring says."""
    _, fc, met, extra = _reference(40, 3, 90, "const")
    assert np.isnan(fc[1]).sum() == 2 * 90 - 1 and not np.isnan(fc[[0, 2]]).any()
    assert np.isnan(met[1]).all() and np.isnan(extra[1, 0]) and np.isfinite(extra[1, 1:]).all()
    for kind in ("nan", "inf", "allnan"):
        _, fc, met, extra = _reference(40, 3, 90, kind)
        assert np.isnan(fc[1]).sum() == (90 * 90 if kind == "allnan" else 2 * 90 - 1)
        assert np.isnan(met[1]).all() and np.isnan(extra[1]).all() and np.isfinite(extra[[0, 2]]).all()


@pytest.mark.parametrize("kind", DEFECTS)
@pytest.mark.parametrize("M,B,N", [(40, 3, 8), (40, 3, 90), (40, 3, 97)])
def test_fc_metrics_from_series(cuda, M, B, N, kind):
    """The fused kernel (N <= 96) and wc_fc_large.hip (N = 97), with want_fc, two empirical matrices
    and Kuramoto through the direct transform."""
    x, *want = _reference(M, B, N, kind)
    emp = _emp(N)
    got = wsg.fc_metrics(torch.tensor(x, device=cuda), B, N, emp, kuramoto=True, want_fc=True)
    _check_fc_metrics(got, want)
    clean = wsg.fc_metrics(torch.from_numpy(_walks(M, B, N)).to(cuda), B, N, emp, kuramoto=True, want_fc=True)
    _neighbours_equal(got, clean)
    assert not any(bool(torch.isnan(t).any()) for t in clean)


@pytest.mark.parametrize("N", [90, 97])
def test_fc_metrics_fc_in_with_a_nan_entry(cuda, N):
    """fc_in mode: one NaN placed in the FC of simulation 1 itself."""
    B = 3
    x = _walks(40, B, N)
    emp = _emp(N)
    fcs = np.stack([np.corrcoef(x[:, b, :].T) for b in range(B)])
    bad = fcs.copy()
    bad[1, 4, N - 5] = np.nan  # upper triangle, inside the SSIM interior
    with np.errstate(all="ignore"):
        wmet = np.array([[osg.get_all_metrics(bad[b], e, 1) for e in emp] for b in range(B)])
        wextra = np.array([[bad[b].mean(), 0.0, 0.0] for b in range(B)])
    assert np.isnan(wmet[1]).all() and np.isnan(wextra[1, 0])
    got = wsg.fc_metrics(fc_in=torch.from_numpy(bad).to(cuda), empfc=emp)
    _check_fc_metrics(got, (None, wmet, wextra), kuramoto=False)
    clean = wsg.fc_metrics(fc_in=torch.from_numpy(fcs).to(cuda), empfc=emp)
    _neighbours_equal(got[1:], clean[1:])


@pytest.mark.parametrize("kind", DEFECTS)
@pytest.mark.parametrize("M,B,N", [(130, 3, 7), (5, 3, 97)])
def test_corrcoef(cuda, M, B, N, kind):
    """wc_corrcoef: split over 3 time blocks (wc_corr.hip), and N > 96 (wc_fc_large.hip)."""
    x = _with_defect(_walks(M, B, N), kind)
    with np.errstate(all="ignore"):
        want = np.stack([np.corrcoef(x[:, b, :].T) for b in range(B)])
    assert np.isnan(want[1]).sum() == (N * N if kind == "allnan" else 2 * N - 1)
    got = wsg.corrcoef(torch.tensor(x, device=cuda), B, N)
    _check(got.cpu().numpy(), want, 0, 1e-12, "corrcoef")
    clean = wsg.corrcoef(torch.from_numpy(_walks(M, B, N)).to(cuda), B, N)
    assert torch.equal(got[0], clean[0]) and torch.equal(got[2], clean[2])


def _kuramoto_long(x, B, N):
    """wc_kuramoto of wc_hilbert_phase_long's phasors (sigchain.kuramoto would take the direct
    transform below M = 8193)."""
    M = x.shape[0]
    ph = wsg.hilbert_phase_long(x.reshape(M, B * N).contiguous())
    out = torch.empty((B, 2), dtype=torch.float64, device=x.device)
    _lib.check(_lib.lib().wc_kuramoto(B, N, M, _lib.ptr(ph), _lib.ptr(out), _lib.stream_handle()), "wc_kuramoto")
    return out


@pytest.mark.parametrize("kind", DEFECTS)
@pytest.mark.parametrize("M", [40, 8193])
def test_kuramoto_through_the_long_transform(cuda, M, kind):
    """A constant column keeps the oracle's finite value (its analytic signal is 0.5 + 0 i, and
    angle(0) = 0 stays as it is); a NaN or an infinity in a column makes sync and meta NaN."""
    B, N = 3, 8
    x = _with_defect(_walks(M, B, N), kind)
    with np.errstate(all="ignore"):
        want = np.array([osg.kuramoto(x[:, b, :]) for b in range(B)])
    assert np.isnan(want[1]).all() == (kind != "const") and np.isfinite(want[[0, 2]]).all()
    got = _kuramoto_long(torch.tensor(x, device=cuda), B, N)
    _check(got.cpu().numpy(), want, 1e-9, 0, "kuramoto")
    clean = _kuramoto_long(torch.from_numpy(_walks(M, B, N)).to(cuda), B, N)
    assert torch.equal(got[0], clean[0]) and torch.equal(got[2], clean[2])


def test_zero_column_has_phase_zero(cuda):
    """angle(0) = 0: a column of zeros is a column of phasors (1, 0) in both transforms."""
    x = _walks(40, 1, 8)[:, 0, :]
    x[:, COL] = 0.0
    xt = torch.tensor(x, device=cuda)
    for ph in (wsg.hilbert_phase(xt), wsg.hilbert_phase_long(xt)):
        col = ph[:, COL].cpu().numpy()
        assert (col[:, 0] == 1.0).all() and (col[:, 1] == 0.0).all()
        assert not bool(torch.isnan(ph).any())


# ---------------- HMA ----------------
HMA_KEYS = ("hin", "hse", "hin_node", "hse_node", "sv")


def _signed_fc(B, N, seed):
    """Correlation matrices of short white series: about half the entries negative before the clip."""
    rng = np.random.default_rng(seed)
    return np.stack([np.corrcoef(rng.standard_normal((40, N)).T) for _ in range(B)])


def _assert_hma_nan(r, b):
    for k in HMA_KEYS:
        assert bool(torch.isnan(r[k][b]).all()), k
    assert bool((r["clus_num"][b] == -1).all())


def _assert_hma_neighbours(r, clean):
    for k in HMA_KEYS + ("clus_num",):
        assert torch.equal(r[k][0], clean[k][0]) and torch.equal(r[k][2], clean[k][2]), k
        assert not bool(torch.isnan(clean[k].double()).any()), k


@pytest.mark.parametrize("bad", [np.nan, np.inf], ids=["nan", "inf"])
@pytest.mark.parametrize("N", [8, 90, 97])
def test_hma_nan_or_inf_after_the_clip(cuda, N, bad):
    """wc_hma (N = 8, 90) and the eigensolver path with wc_hma_modes (N = 97), which must neither
    raise nor hand a non-finite matrix to the eigensolver."""
    fcs = _signed_fc(3, N, N)
    assert (fcs < 0).sum() > N  # the clip has work to do
    dirty = fcs.copy()
    dirty[1, 1, N - 2] = bad       # one entry, so the input is not symmetric either
    dirty[1, N - 1, 0] = -np.inf   # clipped to 0 as any negative entry
    t = torch.from_numpy(dirty).to(cuda)
    r = wsg.hma(t, want_clus_num=True)
    _assert_hma_nan(r, 1)
    np.testing.assert_array_equal(t.cpu().numpy(), np.where(dirty < 0, 0.0, dirty))  # NaN / +Inf stay
    clean = wsg.hma(torch.from_numpy(fcs).to(cuda), want_clus_num=True)
    _assert_hma_neighbours(r, clean)


@pytest.mark.parametrize("N", [8, 90, 97])
def test_hma_minus_inf_is_clipped_like_any_negative_entry(cuda, N):
    fcs = _signed_fc(3, N, N + 1)
    fcs[1, 2, 1] = -1.0
    dirty = fcs.copy()
    dirty[1, 2, 1] = -np.inf
    t = torch.from_numpy(dirty).to(cuda)
    r = wsg.hma(t, want_clus_num=True)
    clean = wsg.hma(torch.from_numpy(fcs).to(cuda), want_clus_num=True)
    for k in HMA_KEYS + ("clus_num",):
        assert torch.equal(r[k], clean[k]), k
    assert bool(torch.isfinite(t).all()) and t[1, 2, 1].item() == 0.0


@pytest.mark.parametrize("N", [8, 90])
def test_hma_modes_with_a_nan_eigenvalue(cuda, N):
    """wc_hma_modes called directly: a NaN in lam of matrix 1."""
    fcs = _signed_fc(3, N, N + 2)
    f = np.where(fcs < 0, 0.0, fcs)
    lam, V = np.linalg.eigh((f + f.transpose(0, 2, 1)) / 2)
    vt = np.ascontiguousarray(V.transpose(0, 2, 1))

    def run(lam):
        B = lam.shape[0]
        out = {k: torch.empty(s, dtype=torch.float64, device=cuda)
               for k, s in (("hin", (B,)), ("hse", (B,)), ("hin_node", (B, N)), ("hse_node", (B, N)), ("sv", (B, N)))}
        out["clus_num"] = torch.empty((B, N - 1), dtype=torch.int32, device=cuda)
        lt, vtt = torch.from_numpy(lam).to(cuda), torch.from_numpy(vt).to(cuda)
        _lib.check(_lib.lib().wc_hma_modes(B, N, _lib.ptr(lt), _lib.ptr(vtt), _lib.ptr(out["hin"]),
                                           _lib.ptr(out["hse"]), _lib.ptr(out["hin_node"]),
                                           _lib.ptr(out["hse_node"]), _lib.ptr(out["clus_num"]),
                                           _lib.ptr(out["sv"]), _lib.stream_handle()), "wc_hma_modes")
        return out

    dirty = lam.copy()
    dirty[1, N // 2] = np.nan
    r = run(dirty)
    _assert_hma_nan(r, 1)
    _assert_hma_neighbours(r, run(lam))


def test_integration_segregation_batch_returns_nan(cuda):
    """The batch function returns the NaN values; the per-matrix host functions raise, as the
    reference's SVD does (tests/test_hma.py)."""
    fcs = _signed_fc(3, 8, 5)
    fcs[1, 3, 4] = np.nan
    res = HMA.integration_segregation_batch(fcs, device=cuda)
    assert np.isnan(res[1]["Hin_sim"]) and np.isnan(res[1]["Hse_sim"])
    assert np.isnan(res[1]["Hin_node_sim"]).all() and np.isnan(res[1]["Hse_node_sim"]).all()
    assert np.isnan(res[1]["sFC"][3, 4]) and (np.nan_to_num(res[1]["sFC"]) >= 0).all()
    for b in (0, 2):
        want = HMA.integration_segregation(fcs[b].copy())
        np.testing.assert_allclose(res[b]["Hin_sim"], want["Hin_sim"], rtol=1e-12)
        np.testing.assert_allclose(res[b]["Hse_sim"], want["Hse_sim"], rtol=1e-11)


def test_chain_constant_column_to_hma(cuda):
    """fc_metrics(want_fc=True), then hma: the constant column's NaN row reaches hma as NaN, and the
    other simulations equal the host facade (test_hma_gpu.py's bounds)."""
    M, B, N = 40, 3, 8
    x = _reference(M, B, N, "const")[0]
    fc, _, _ = wsg.fc_metrics(torch.tensor(x, device=cuda), B, N, None, kuramoto=False, want_fc=True)
    r = wsg.hma(fc, want_clus_num=True)
    _assert_hma_nan(r, 1)
    assert int(torch.isnan(fc[1]).sum()) == 2 * N - 1
    for b in (0, 2):
        f = fc[b].cpu().numpy()  # the device's own FC (clipped already; the facade clips again)
        cn, cs, _ = HMA.Functional_HP(f)
        hin, hse = HMA.Balance(f, cn, cs)
        hin_n, hse_n = HMA.nodal_measures(f, cn, cs)
        np.testing.assert_array_equal(r["clus_num"][b].cpu().numpy(), cn)
        np.testing.assert_allclose(r["hin"][b].item(), hin, rtol=1e-12)
        np.testing.assert_allclose(r["hse"][b].item(), hse, rtol=1e-11)
        np.testing.assert_allclose(r["hin_node"][b].cpu().numpy(), hin_n, rtol=1e-10, atol=1e-15)
        np.testing.assert_allclose(r["hse_node"][b].cpu().numpy(), hse_n, rtol=1e-9, atol=1e-15)

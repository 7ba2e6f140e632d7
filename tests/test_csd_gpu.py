"""Cross-spectral matrix and coherence on the device (wc_csd, sigchain.csd / coherence, utils.csd,
utils.coherence, utils.csd_matrix, utils.coherence_matrix) against the host reference of
tests/csd_reference.py (a numpy loop over segments that test_csd_cpu.py ties to scipy.signal.csd /
coherence), and the pair modes against SciPy directly.

Cross spectrum, per element over every bin:  |got - want| <= 2e-12 sqrt(max_f P_ii max_f P_jj): the
project's 1e-12 amplitude-domain Bluestein bound (test_welch_psd_gpu.py) carried through a product
of two spectra, dP <= |X_i| dX_j + |X_j| dX_i.
Coherence:  |got - want| <= 8e-12 max(r_i[f], r_j[f]),  r = max_f P / P[f]: from
dC <= eps (2 sqrt(r_i r_j) + r_i + r_j); on this signal r reaches about 2e8 in SciPy's own result, so a
flat bound would mean nothing.  Also 0 <= C <= 1 + 1e-12 and the diagonal within 1e-15 of 1.
Every case prints its measured maximum in those units as a `TOL csd-... dev=` line.

Measured on MI355X (380 printed figures; none reaches a tenth of its bound):
  cross spectrum, worst over noverlap and segment count per nperseg, C = 7:  2: 2.8e-16   3: 9.6e-15   5: 3.3e-14
    8: 8.5e-15   15: 6.8e-15   16: 6.3e-15   64: 5.5e-15   100: 2.5e-15   200: 3.9e-15   400: 1.5e-15   1000: 8.6e-16
    1025: 8.2e-16   2049: 1.2e-15   4096: 5.4e-16  (the largest at nperseg = 5, as in the PSD tests: the detrended segment of an offset column
    is 1e-3 of its mean)
  coherence, the same cases:  2: 5.6e-16   3: 4.1e-15   5: 1.7e-14   8: 2.7e-15   15: 5.0e-15   16: 5.5e-15
    64: 3.1e-15   100: 1.2e-15   200: 1.0e-15   400: 4.4e-16   1000: 1.8e-16   1025: 2.2e-16   2049: 3.5e-16   4096: 2.2e-16
  C = 1 / 2 / 33 / 90 / 130, cross spectrum:  nperseg 15: 8.0e-16 / 4.6e-16 / 3.1e-15 / 4.7e-15 / 5.8e-15
    1000: 4.7e-16 / 1.5e-16 / 4.9e-16 / 6.7e-16 / 7.6e-16;  coherence:  15: 0 / 2.2e-16 / 1.7e-15 / 2.6e-15 / 2.7e-15
    1000: 0 / 2.3e-17 / 6.8e-16 / 8.9e-16 / 1.0e-15
  diagonal against sigchain.welch (amplitude units):  15: 2.9e-16   1000: 1.8e-16   4096: 1.8e-16
  20,000 x 33 / 400: 1.4e-15, coherence 6.7e-16   30,000 x 90 / 400: 2.1e-15, coherence 1.8e-15
  pair modes against SciPy:  6,000 x 7 / 400: 2.7e-16, coherence 1.1e-16   300 x 64 / 15: 2.7e-15, coherence 7.8e-16;
    against the matrix mode of [x | y]: exactly equal
  options:  detrend False 5.7e-16   spectrum 9.5e-16   tukey 7.0e-16   array window 8.8e-16   defaults 8.2e-16
    clamped nperseg 2.3e-15   float32 input 3.6e-16   zero column 2.3e-15 (15), 1.8e-15 (400)
"""
import functools
import warnings

import numpy as np
import pytest
import torch
from scipy import signal

from nremmodfc_amd import _lib, utils
from nremmodfc_amd import sigchain as wsg
from tests import csd_reference as ref

pytestmark = pytest.mark.gpu

CSD_BOUND = 2e-12
COH_BOUND = 8e-12
PSD_BOUND = 1e-12
NPERSEG = [2, 3, 5, 8, 15, 16, 64, 100, 200, 400, 1000, 1025, 2049, 4096]


def make_signal(M, C):
    """test_welch_psd_gpu.py's recipe: amplitude-modulated 2-12 Hz carriers at 500 Hz plus a little
    noise; even columns sit on a 0.2 offset (E-like: the detrend has work to do), odd columns
    rotate through every phase."""
    rng = np.random.default_rng(M)
    t = np.arange(M)[:, None] * 0.002
    f = rng.uniform(2, 12, C)
    p = rng.uniform(0, 2 * np.pi, C)
    g = rng.uniform(0.05, 0.2, C)
    x = (1 + 0.3 * np.sin(2 * np.pi * g * t)) * np.cos(2 * np.pi * f * t + p) + 0.01 * rng.standard_normal((M, C))
    x[:, ::2] = 0.2 + 0.05 * x[:, ::2]
    return np.ascontiguousarray(x)


@functools.lru_cache(maxsize=None)
def sig(M, C):
    """Computed once per shape, read only; shorter series are its leading rows."""
    x = make_signal(M, C)
    x.setflags(write=False)
    return x


def dev(x, cuda):
    return torch.tensor(np.ascontiguousarray(x), device=cuda)  # a copy: the shared cases are read only


def diag(P):
    return np.einsum("fii->fi", P).real


def check_csd(tag, got, want, pi, pj=None):
    d = ref.csd_deviation(got, want, pi, pj)
    print(f"TOL csd-{tag} dev={d:.3e}")
    assert d <= CSD_BOUND
    return d


def check_coh(tag, got, want, pi, pj=None):
    d = ref.coherence_deviation(got, want, pi, pj)
    print(f"TOL csd-coherence-{tag} dev={d:.3e}")
    assert d <= COH_BOUND
    ok = ~np.isnan(got)
    assert (got[ok] >= 0).all() and (got[ok] <= 1 + 1e-12).all()
    if got.ndim == 3:
        dg = np.einsum("fii->fi", got)
        assert (np.abs(dg[~np.isnan(dg)] - 1) <= 1e-15).all()
    return d


def check_matrix(tag, x, cuda, n, nov, **kw):
    """sigchain.csd and coherence of x against the reference; returns the device matrix (numpy)."""
    rkw = {k: v for k, v in kw.items() if k != "ws_bytes"}
    fw, want = ref.csd_matrix(x, 500.0, nperseg=n, noverlap=nov, **{"window": "hann", **rkw})
    xt = dev(x, cuda)
    fg, got = wsg.csd(xt, None, 500.0, nperseg=n, noverlap=nov, **kw)
    C = x.shape[1]
    assert got.is_cuda and got.dtype == torch.complex128 and got.shape == (n // 2 + 1, C, C)
    np.testing.assert_array_equal(fg, fw)
    got = got.cpu().numpy()
    worst = check_csd(tag, got, want, diag(want))
    ckw = {k: v for k, v in kw.items() if k != "scaling"}
    fc, coh = wsg.coherence(xt, None, 500.0, nperseg=n, noverlap=nov, **ckw)
    assert coh.dtype == torch.float64 and coh.shape == got.shape
    np.testing.assert_array_equal(fc, fw)
    coh = coh.cpu().numpy()
    np.testing.assert_array_equal(coh, np.swapaxes(coh, 1, 2))
    return got, worst, check_coh(tag, coh, ref.coherence_of(want), diag(want))


@pytest.mark.parametrize("n", NPERSEG)
def test_segment_lengths_overlaps_and_counts(cuda, n):
    """Every L class with odd and even nperseg x noverlap (0, n / 2, 3 n / 4) x segment counts 1
    (coherence is 1), 2, 3 (the odd last segment rides alone) and 7 (several segment blocks, also run
    through the minimum workspace); C = 7."""
    C, wp, wc = 7, 0.0, 0.0
    x = sig(7 * n, C)
    for nov in sorted({0, n // 2, 3 * n // 4}):
        step = n - nov
        for nseg in (1, 2, 3, 7):
            T = n + (nseg - 1) * step
            got, dp, dc = check_matrix(f"n{n}-nov{nov}-nseg{nseg}", x[:T], cuda, n, nov)
            wp, wc = max(wp, dp), max(wc, dc)
            if nseg == 7:  # four chunks of one segment block (the last of one segment) against the single chunk
                need = _lib.lib().wc_csd_workspace_size(C, T, n, nov)
                again = wsg.csd(dev(x[:T], cuda), None, 500.0, nperseg=n, noverlap=nov, ws_bytes=need)[1]
                np.testing.assert_array_equal(again.cpu().numpy(), got)
    print(f"TOL csd-n{n}-worst dev={wp:.3e}")
    print(f"TOL csd-coherence-n{n}-worst dev={wc:.3e}")


def test_single_segment_coherence_is_one(cuda):
    x = sig(400, 7)
    coh = wsg.coherence(dev(x, cuda), None, 500.0, nperseg=400, noverlap=200)[1].cpu().numpy()
    r = diag(ref.csd_matrix(x, 500.0, nperseg=400, noverlap=200)[1])
    r = r.max(axis=0) / r
    assert (np.abs(coh - 1) <= COH_BOUND * np.maximum(r[:, :, None], r[:, None, :])).all()


@pytest.mark.parametrize("n", [15, 1000])
@pytest.mark.parametrize("C", [1, 2, 33, 90, 130])
def test_column_tiling(cuda, n, C):
    """One column, two, a ragged 32-tile, cortex_run.py's width (three tiles, more columns than a
    pass-1 workgroup holds), five tiles; eight segments."""
    step = n - n // 2
    check_matrix(f"C{C}-n{n}", sig(n + 7 * step, C), cuda, n, n // 2)


@pytest.mark.parametrize("n", [15, 1000, 4096])
def test_diagonal_is_the_psd_kernel(cuda, n):
    """The matrix's real diagonal against sigchain.welch on the same input, in the PSD test's
    amplitude-domain units (not bit-equal: the PSD kernel never splits its segment pairs)."""
    x = dev(sig(n + 7 * (n - n // 2), 7), cuda)
    P = wsg.csd(x, None, 500.0, nperseg=n)[1].cpu().numpy()
    psd = wsg.welch(x, 500.0, nperseg=n)[1].cpu().numpy()
    d = float((np.abs(np.sqrt(diag(P)) - np.sqrt(psd)).max(axis=0) / np.sqrt(psd.max(axis=0))).max())
    print(f"TOL csd-diagonal-vs-welch-n{n} dev={d:.3e}")
    assert d <= PSD_BOUND


@pytest.mark.parametrize("n", [15, 1000])
def test_exact_structure(cuda, n):
    """Exactly Hermitian with an exactly real diagonal, and an entry depends on its two columns only:
    bit-identical in the 130-column call and in a 2-column call."""
    x = sig(n + 7 * (n - n // 2), 130)
    P = wsg.csd(dev(x, cuda), None, 500.0, nperseg=n)[1].cpu().numpy()
    np.testing.assert_array_equal(P, np.conj(np.swapaxes(P, 1, 2)))
    assert (np.einsum("fii->fi", P).imag == 0).all()
    coh = wsg.coherence(dev(x, cuda), None, 500.0, nperseg=n)[1].cpu().numpy()
    for i, j in ((0, 129), (5, 64), (31, 32), (100, 101)):
        two = dev(x[:, [i, j]], cuda)
        P2 = wsg.csd(two, None, 500.0, nperseg=n)[1].cpu().numpy()
        np.testing.assert_array_equal(P2, P[:, [i, j]][:, :, [i, j]])
        c2 = wsg.coherence(two, None, 500.0, nperseg=n)[1].cpu().numpy()
        np.testing.assert_array_equal(c2, coh[:, [i, j]][:, :, [i, j]])


def test_workspace_invariance(cuda):
    """20,000 x 33 at nperseg 400: 99 segments; the minimum workspace (50 chunks of one segment block),
    one holding three segment blocks (17 chunks, the last of three segments) and the default (one chunk)
    are bit-identical in every mode, and so are two runs."""
    T, C, n = 20_000, 33, 400
    x = sig(T, C + 1)
    xt, yt = dev(x[:, :C], cuda), dev(x[:, 1:], cuda)
    need = _lib.lib().wc_csd_workspace_size(C, T, n, n // 2)
    block = 2 * (n // 2 + 1) * C * 16
    P = wsg.csd(xt, None, 500.0, nperseg=n)[1]
    coh = wsg.coherence(xt, None, 500.0, nperseg=n)[1]
    fw, want = ref.csd_matrix(x[:, :C], 500.0, nperseg=n)
    check_csd("invariance-20000x33-n400", P.cpu().numpy(), want, diag(want))
    check_coh("invariance-20000x33-n400", coh.cpu().numpy(), ref.coherence_of(want), diag(want))
    assert torch.equal(wsg.csd(xt, None, 500.0, nperseg=n)[1].view(torch.float64), P.view(torch.float64))
    assert torch.equal(wsg.coherence(xt, None, 500.0, nperseg=n)[1], coh)
    for ws_bytes in (need, need + 2 * block):
        assert torch.equal(wsg.csd(xt, None, 500.0, nperseg=n, ws_bytes=ws_bytes)[1].view(torch.float64),
                           P.view(torch.float64))
        assert torch.equal(wsg.coherence(xt, None, 500.0, nperseg=n, ws_bytes=ws_bytes)[1], coh)
    need2 = _lib.lib().wc_csd_workspace_size(2 * C, T, n, n // 2)
    Pp = wsg.csd(xt, yt, 500.0, nperseg=n)[1]
    cp = wsg.coherence(xt, yt, 500.0, nperseg=n)[1]
    for ws_bytes in (need2, need2 + 4 * block, None):
        assert torch.equal(wsg.csd(xt, yt, 500.0, nperseg=n, ws_bytes=ws_bytes)[1].view(torch.float64),
                           Pp.view(torch.float64))
        assert torch.equal(wsg.coherence(xt, yt, 500.0, nperseg=n, ws_bytes=ws_bytes)[1], cp)
    with pytest.raises(_lib.WCSDEError, match=str(need)):
        wsg.csd(xt, None, 500.0, nperseg=n, ws_bytes=need - 16)


@pytest.mark.parametrize("T,C,n", [(6000, 7, 400), (300, 64, 15)])
def test_pair_modes(cuda, T, C, n):
    """sigchain.csd(x, y) and coherence(x, y) against scipy.signal.csd / coherence(x, y, axis=0), and
    against the matching off-diagonal entries of the matrix mode of [x | y]."""
    z = sig(T, 2 * C)
    x, y = z[:, :C], z[:, C:]
    xt, yt = dev(x, cuda), dev(y, cuda)
    fw, want = signal.csd(x, y, 500.0, nperseg=n, axis=0)
    px, py = signal.welch(x, 500.0, nperseg=n, axis=0)[1], signal.welch(y, 500.0, nperseg=n, axis=0)[1]
    fg, got = wsg.csd(xt, yt, 500.0, nperseg=n)
    assert got.dtype == torch.complex128 and got.shape == (n // 2 + 1, C)
    np.testing.assert_array_equal(fg, fw)
    got = got.cpu().numpy()
    check_csd(f"pairs-T{T}-n{n}", got, want, px, py)
    fc, cw = signal.coherence(x, y, 500.0, nperseg=n, axis=0)
    fg, coh = wsg.coherence(xt, yt, 500.0, nperseg=n)
    assert coh.dtype == torch.float64 and coh.shape == (n // 2 + 1, C)
    np.testing.assert_array_equal(fg, fc)
    coh = coh.cpu().numpy()
    check_coh(f"pairs-T{T}-n{n}", coh, cw, px, py)
    i = np.arange(C)
    full = wsg.csd(dev(z, cuda), None, 500.0, nperseg=n)[1].cpu().numpy()
    check_csd(f"pairs-vs-matrix-T{T}-n{n}", got, full[:, i, i + C], px, py)
    cfull = wsg.coherence(dev(z, cuda), None, 500.0, nperseg=n)[1].cpu().numpy()
    check_coh(f"pairs-vs-matrix-T{T}-n{n}", coh, cfull[:, i, i + C], px, py)
    with pytest.raises(TypeError, match="shape"):
        wsg.csd(xt, yt[:, :C - 1], 500.0, nperseg=n)


def test_options(cuda):
    """detrend False, scaling='spectrum', a Tukey tuple window, an array window (nperseg from its
    length), SciPy's defaults (nperseg 256), the clamped-nperseg warning, float32 input through utils."""
    n, T = 400, 400 + 6 * 200
    x = sig(T, 7)
    check_matrix("n400-detrend-False", x, cuda, n, n // 2, detrend=False)
    check_matrix("n400-spectrum", x, cuda, n, n // 2, scaling="spectrum")
    check_matrix("n400-detrend-False-spectrum", x, cuda, n, n // 2, detrend=False, scaling="spectrum")
    check_matrix("n400-tukey", x, cuda, n, n // 2, window=("tukey", 0.25))
    w = np.blackman(n) + 0.1
    check_matrix("n400-array-window", x, cuda, n, n // 2, window=w)
    xt = dev(x, cuda)
    fw, want = ref.csd_matrix(x, 500.0, w, n)
    fg, got = wsg.csd(xt, None, 500.0, w)                                # nperseg and noverlap from the window
    np.testing.assert_array_equal(fg, fw)
    check_csd("n400-array-window-defaults", got.cpu().numpy(), want, diag(want))
    fw, want = ref.csd_matrix(x)                                         # fs = 1, nperseg = 256, noverlap = 128
    fg, got = wsg.csd(xt)
    np.testing.assert_array_equal(fg, fw)
    check_csd("defaults", got.cpu().numpy(), want, diag(want))
    fg, coh = wsg.coherence(xt)
    check_coh("defaults", coh.cpu().numpy(), ref.coherence_of(want), diag(want))
    fw, want = signal.csd(x, x[:, ::-1], axis=0)
    fg, got = wsg.csd(xt, dev(x[:, ::-1], cuda))
    np.testing.assert_array_equal(fg, fw)
    pw = signal.welch(x, axis=0)[1]
    check_csd("pairs-defaults", got.cpu().numpy(), want, pw, pw[:, ::-1])
    # a named window longer than the series: SciPy's warning and SciPy's clamped result
    short = x[:200]
    with pytest.warns(UserWarning, match="nperseg = 256 is greater than input length"):
        fg, got = utils.csd(short, short[:, ::-1], 500.0, axis=0)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        fw, want = signal.csd(short, short[:, ::-1], 500.0, axis=0)
        pw = signal.welch(short, 500.0, axis=0)[1]
    np.testing.assert_array_equal(fg, fw)
    check_csd("clamped-nperseg", got, want, pw, pw[:, ::-1])
    with pytest.warns(UserWarning, match="nperseg = 256 is greater than input length"):
        wsg.coherence(dev(short, cuda))
    x32 = x.astype(np.float32)
    fw, want = ref.csd_matrix(x32.astype(np.float64), 500.0, nperseg=n)
    fg, got = utils.csd_matrix(x32, 500.0, nperseg=n)
    np.testing.assert_array_equal(fg, fw)
    check_csd("float32-input", got, want, diag(want))
    fg, got = utils.csd(x32, x32[:, ::-1], 500.0, nperseg=n, nfft=n, axis=0)
    check_csd("float32-input-pairs", got, want[:, np.arange(7), np.arange(7)[::-1]], diag(want), diag(want)[:, ::-1])
    with pytest.raises(ValueError, match="longer"):
        wsg.csd(xt[:300], None, 500.0, w)
    with pytest.raises(ValueError, match="noverlap"):
        wsg.coherence(xt, None, 500.0, "hann", n, n)
    with pytest.raises(NotImplementedError, match="detrend"):
        wsg.csd(xt, None, 500.0, detrend="linear")
    with pytest.raises(_lib.WCSDEError, match="4096"):
        wsg.csd(dev(sig(5000, 2), cuda), None, 500.0, nperseg=4097)
    with pytest.raises(TypeError, match="fp64"):
        wsg.csd(xt.float())


@pytest.mark.parametrize("n", [15, 400])
def test_all_zero_column(cuda, n):
    """A column without power: NaN coherence in its row and column (the diagonal included), exactly
    where the reference has NaN, finite elsewhere; the cross spectrum's row and column are 0."""
    x = np.array(sig(n + 7 * (n - n // 2), 7))
    x[:, 3] = 0.0
    got, _, _ = check_matrix(f"zero-column-n{n}", x, cuda, n, n // 2)
    assert (got[:, 3, :] == 0).all() and (got[:, :, 3] == 0).all()
    coh = wsg.coherence(dev(x, cuda), None, 500.0, nperseg=n)[1].cpu().numpy()
    nan = np.isnan(coh)
    assert nan[:, 3, :].all() and nan[:, :, 3].all()
    keep = [0, 1, 2, 4, 5, 6]
    assert np.isfinite(coh[:, keep][:, :, keep]).all()
    y = np.ascontiguousarray(x[:, ::-1])
    cp = wsg.coherence(dev(x, cuda), dev(y, cuda), 500.0, nperseg=n)[1].cpu().numpy()
    assert np.isnan(cp[:, 3]).all() and np.isfinite(cp[:, [0, 1, 2, 4, 5, 6]]).all()


def test_facades(cuda):
    """utils.csd / utils.coherence return SciPy's shapes along axis 0 and -1 and for one series;
    utils.coherence_matrix at 30,000 x 90 / 400 against the reference."""
    x = sig(30_000, 90)
    a, b = x[:5000, :6], x[:5000, 6:12]
    fw, want = signal.csd(a, b, 500.0, nperseg=400, axis=0)
    pa, pb = signal.welch(a, 500.0, nperseg=400, axis=0)[1], signal.welch(b, 500.0, nperseg=400, axis=0)[1]
    f0, p0 = utils.csd(a, b, 500.0, nperseg=400, axis=0)
    assert isinstance(p0, np.ndarray) and p0.dtype == np.complex128 and p0.shape == want.shape == (201, 6)
    np.testing.assert_array_equal(f0, fw)
    check_csd("facade-axis0", p0, want, pa, pb)
    f1, p1 = utils.csd(np.ascontiguousarray(a.T), np.ascontiguousarray(b.T), 500.0, nperseg=400)   # axis = -1
    assert p1.shape == signal.csd(a.T, b.T, 500.0, nperseg=400)[1].shape == (6, 201)
    np.testing.assert_array_equal(p1, p0.T)
    f2, p2 = utils.csd(a[:, 3], b[:, 3], 500.0, nperseg=400)             # one series each
    assert p2.shape == (201,)
    np.testing.assert_array_equal(p2, p0[:, 3])
    cw = signal.coherence(a, b, 500.0, nperseg=400, axis=0)[1]
    f0, c0 = utils.coherence(a, b, 500.0, nperseg=400, axis=0)
    assert c0.dtype == np.float64 and c0.shape == cw.shape
    check_coh("facade-axis0", c0, cw, pa, pb)
    f1, c1 = utils.coherence(np.ascontiguousarray(a.T), np.ascontiguousarray(b.T), 500.0, nperseg=400)
    np.testing.assert_array_equal(c1, c0.T)
    cube = a.reshape(5000, 2, 3)
    f3, c3 = utils.coherence(cube, b.reshape(5000, 2, 3), 500.0, nperseg=400, axis=0)
    assert c3.shape == (201, 2, 3)
    np.testing.assert_array_equal(c3.reshape(201, 6), c0)

    fw, want = ref.csd_matrix(x, 500.0, nperseg=400)
    fg, coh = utils.coherence_matrix(x, 500.0, nperseg=400)
    assert isinstance(coh, np.ndarray) and coh.shape == (201, 90, 90)
    np.testing.assert_array_equal(fg, fw)
    check_coh("facade-coherence-matrix-30000x90-n400", coh, ref.coherence_of(want), diag(want))
    fg, P = utils.csd_matrix(x, 500.0, nperseg=400)
    assert P.dtype == np.complex128 and P.shape == (201, 90, 90)
    check_csd("facade-csd-matrix-30000x90-n400", P, want, diag(want))


@pytest.mark.parametrize("kwargs,word", [
    (dict(nfft=2048), "nfft"),
    (dict(return_onesided=False), "return_onesided"),
    (dict(average="median"), "average"),
    (dict(detrend="linear"), "detrend"),
])
def test_facades_refuse(cuda, kwargs, word):
    x = sig(1000, 3)
    with pytest.raises(NotImplementedError, match=word):
        utils.csd(x, x[:, ::-1], 500.0, axis=0, **kwargs)
    if "nfft" in kwargs or "detrend" in kwargs:
        with pytest.raises(NotImplementedError, match=word):
            utils.coherence(x, x[:, ::-1], 500.0, axis=0, **kwargs)
    with pytest.raises(NotImplementedError, match="shapes"):
        utils.csd(x, x[:900], 500.0, axis=0)
    with pytest.raises(NotImplementedError, match="complex"):
        utils.coherence(x * 1j, x, 500.0, axis=0)
    with pytest.raises(NotImplementedError, match="detrend"):
        utils.coherence_matrix(x, 500.0, detrend="linear")

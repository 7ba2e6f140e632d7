"""Host reference of the cross-spectral tests (test_csd_cpu.py checks it against SciPy, test_csd_gpu.py
checks the device against it): a numpy loop over Welch's segments with np.fft.rfft, SciPy's window,
constant detrend, scaling and one-sided doubling -- scipy.signal.csd(x[:, :, None], x[:, None, :],
axis=0) without the time x columns x columns array that form materialises -- and the scaled
deviations both test files assert on."""
import numpy as np
from scipy import signal


def _segments(x, window, nperseg, noverlap, detrend):
    """Yields the windowed one-sided spectra [F][C] of x [T][C], segment by segment."""
    win = signal.get_window(window, nperseg) if isinstance(window, (str, tuple)) else np.asarray(window, float)
    assert win.shape == (nperseg,)
    step = nperseg - noverlap
    for s in range((x.shape[0] - nperseg) // step + 1):
        seg = x[s * step:s * step + nperseg]
        if detrend:
            seg = seg - seg.mean(axis=0)
        yield np.fft.rfft(seg * win[:, None], axis=0)


def _scale(P, nseg, fs, window, nperseg, scaling):
    win = signal.get_window(window, nperseg) if isinstance(window, (str, tuple)) else np.asarray(window, float)
    P *= (1.0 / (fs * (win * win).sum()) if scaling == "density" else 1.0 / win.sum() ** 2) / nseg
    if nperseg % 2:
        P[1:] *= 2
    else:
        P[1:-1] *= 2
    return np.fft.rfftfreq(nperseg, 1 / fs), P


def csd_matrix(x, fs=1.0, window="hann", nperseg=256, noverlap=None, detrend="constant", scaling="density"):
    """(freqs, P [F][C][C]): P[f][i][j] = mean over segments of conj(X_i[f]) X_j[f], scaled as SciPy."""
    x = np.asarray(x, dtype=np.float64)
    noverlap = nperseg // 2 if noverlap is None else noverlap
    P = np.zeros((nperseg // 2 + 1, x.shape[1], x.shape[1]), dtype=np.complex128)
    nseg = 0
    for X in _segments(x, window, nperseg, noverlap, detrend):
        P += np.conj(X)[:, :, None] * X[:, None, :]
        nseg += 1
    return _scale(P, nseg, fs, window, nperseg, scaling)


def csd_pairs(x, y, fs=1.0, window="hann", nperseg=256, noverlap=None, detrend="constant", scaling="density"):
    """(freqs, P [F][C]) = scipy.signal.csd(x, y, axis=0) of equally shaped x and y."""
    f, P = csd_matrix(np.concatenate((x, y), axis=1), fs, window, nperseg, noverlap, detrend, scaling)
    C = x.shape[1]
    i = np.arange(C)
    return f, P[:, i, i + C]


def coherence_of(P):
    """|P_ij|^2 / (P_ii P_jj) of a cross-spectral matrix [F][C][C]; NaN where a column has no power."""
    d = np.einsum("fii->fi", P).real
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.abs(P) ** 2 / (d[:, :, None] * d[:, None, :])


def csd_deviation(got, want, pi, pj=None):
    """max |got - want| / sqrt(max_f P_ii max_f P_jj): got, want [F][C][C] with pi = pj the PSDs [F][C]
    of the columns, or [F][C] with pi, pj those of the two sides.  A column without power must be
    exact (its entries are 0)."""
    pj = pi if pj is None else pj
    si, sj = np.sqrt(pi.max(axis=0)), np.sqrt(pj.max(axis=0))
    scale = si[:, None] * sj[None, :] if got.ndim == 3 else si * sj
    err = np.abs(got - want)
    assert np.isfinite(err).all()
    dead = np.broadcast_to(scale == 0, err.shape)
    assert (err[dead] == 0).all()
    return float((err / np.where(scale == 0, 1.0, scale))[~dead].max()) if (~dead).any() else 0.0


def coherence_deviation(got, want, pi, pj=None):
    """max |got - want| / max(r_i[f], r_j[f]), r = max_f P / P[f]; NaN exactly where want has NaN."""
    pj = pi if pj is None else pj
    with np.errstate(invalid="ignore", divide="ignore"):
        ri, rj = pi.max(axis=0) / pi, pj.max(axis=0) / pj
    r = np.maximum(ri[:, :, None], rj[:, None, :]) if got.ndim == 3 else np.maximum(ri, rj)
    nan = np.isnan(want)
    np.testing.assert_array_equal(np.isnan(got), nan)
    if nan.all():
        return 0.0
    return float((np.abs(got - want)[~nan] / r[~nan]).max())

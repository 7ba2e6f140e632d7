"""Drop-in for utils.py's observables and matrix helpers (utils.py:18-74, 134-154).

get_all_metrics, kuramoto and envelope run in libwcsde.so (wc_fc_metrics,
wc_hilbert_phase / wc_hilbert_phase_long + wc_kuramoto, wc_filtfilt +
wc_hilbert_envelope), and so does welch, a stand-in for the scipy.signal.welch
that cortex_run.py:203-209 calls next to them (wc_welch_psd), with csd, coherence, csd_matrix and coherence_matrix for
the coupling between regions per frequency (wc_csd), spectrogram for the spectra over time
(wc_spectrogram) and connectivity for the coupling between regions in a band, from phases and
envelopes (wc_phase_conn); the small array helpers the reference defines next to
them (flat_FC, new_metric, cohen_d, sub_weight, cortex_mat, scale_mat and the
thal / sub / cortex index lists) are host numpy for callers that import them.
Not mirrored: RSN_profile_FC and fill_missing (they cannot run upstream: the
RSN index table is commented out, DataFrame.append is gone from pandas) and
the pandas / plot helpers find_extreme and xy2plotcor.
"""
import numpy as np
import torch

from . import _args, sigchain

device = "cuda"


def cohen_d(x, y):
    """utils.py:18-22 -- effect size between two samples."""
    nx, ny = len(x), len(y)
    dof = nx + ny - 2
    return (np.mean(x) - np.mean(y)) / np.sqrt(((nx - 1) * np.std(x, ddof=1) ** 2 + (ny - 1) * np.std(y, ddof=1) ** 2)
                                               / dof)


def flat_FC(FC):
    """utils.py:24-26 -- strict upper triangle, row-major."""
    n = len(FC)
    return np.concatenate([FC[i, i + 1:] for i in range(n)])


def new_metric(flat1, flat2):
    """utils.py:28-31."""
    return 1 - np.corrcoef(flat1, flat2)[0, 1] + (flat1.mean() - flat2.mean()) ** 2


thal = [38, 51]
not_thal = [i for i in range(90) if i not in thal]
subL, subR = [35, 36, 37, 38], [51, 52, 53, 54]
sub = subL + subR
cortex = [i for i in range(90) if i not in sub]


def sub_weight(struct, prop=1):
    """utils.py:58-67 -- the subcortical rows and columns of struct times prop (a proportion of
    the original), the links among subcortical areas left as they are."""
    struct = np.asarray(struct)
    is_sub = np.zeros(len(struct), dtype=bool)
    is_sub[sub] = True
    one_end = is_sub[:, None] ^ is_sub[None, :]  # cortex <-> subcortex links, either direction
    out = np.copy(struct)
    out[one_end] = (prop * struct)[one_end]
    return out


def cortex_mat(mat90):
    """utils.py:70-74 -- the 82 x 82 cortical block of a 90 x 90 AAL matrix."""
    return np.asarray(mat90)[np.ix_(cortex, cortex)]


def scale_mat(struct, G, subG):
    """utils.py:137-143 -- thalamic columns of struct times subG, every other column times G
    (scalars, or vectors over the rows)."""
    struct = np.asarray(struct)
    out = np.copy(struct)
    for area in range(struct.shape[1]):
        out[:, area] = (subG if area in thal else G) * struct[:, area]
    return out


def envelope(series, dt=0.002, freqs=[8, 13], fcut=None):
    """utils.py:145-154: band-limited amplitude envelope of series (time, rois): Bessel order-3
    band-pass filtfilt over freqs, |hilbert| along time and, for a truthy fcut, a Bessel order-3
    low-pass filtfilt at fcut.  numpy in, numpy out; a 1-D series gives a 1-D envelope.
    22 <= time <= 524288 (the order-6 band-pass's padlen is 21)."""
    x = np.ascontiguousarray(series, dtype=np.float64)
    if x.ndim not in (1, 2):
        raise ValueError("series must be (time,) or (time, rois)")
    xt = torch.as_tensor(x.reshape(x.shape[0], -1)).to(device)
    return sigchain.envelope(xt, dt, tuple(freqs), fcut).cpu().numpy().reshape(x.shape)


def _refuse_nfft(name, x, window, nperseg, nfft, axis):
    """nfft may only restate the segment length SciPy would use."""
    if nfft is None:
        return
    named = isinstance(window, (str, tuple))
    seg = int(nperseg) if nperseg is not None else (256 if named else len(window))
    if named:
        seg = min(seg, np.shape(x)[axis])  # SciPy clamps a named window's nperseg to the input
    if int(nfft) != seg:
        raise NotImplementedError(f"{name}: nfft other than nperseg (zero padding) does not run on the device")


def _refuse_detrend(name, detrend):
    if not (detrend is False or (isinstance(detrend, str) and detrend == 'constant')):
        raise NotImplementedError(f"{name}: detrend = {detrend!r} (only 'constant' and False run on the device)")


def _refuse_options(name, return_onesided, average, detrend):
    if not return_onesided:
        raise NotImplementedError(f"{name}: return_onesided=False does not run on the device")
    if average != 'mean':
        raise NotImplementedError(f"{name}: average = {average!r} (only 'mean' runs on the device)")
    _refuse_detrend(name, detrend)


def _real_input(name, x, noun="input"):
    x = np.asarray(x)
    if np.iscomplexobj(x):
        raise NotImplementedError(f"{name}: complex {noun} does not run on the device")
    return x


def _not_empty(name, x):
    if x.ndim < 1 or x.size == 0:
        raise ValueError(f"{name}: x must have at least one sample")


def _upload(a, to=None):
    """a as a contiguous fp64 tensor on the module's device, or on `to`."""
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to(device if to is None else to)


def _time_major(x, axis):
    """x with `axis` first and the others flattened, on the device as fp64, and the others' shape."""
    xt = np.moveaxis(x, axis, 0)
    return _upload(xt.reshape(xt.shape[0], -1)), xt.shape[1:]


def _from_time_major(out, rest, axis):
    p = out.cpu().numpy().reshape((out.shape[0],) + rest)
    return np.moveaxis(p, 0, axis) if rest else p


def welch(x, fs=1.0, window='hann', nperseg=None, noverlap=None, nfft=None, detrend='constant',
          return_onesided=True, scaling='density', axis=-1, average='mean'):
    """scipy.signal.welch with its parameter order and defaults, on the device (wc_welch_psd), for
    what cortex_run.py:203-209 asks of it: real input, one-sided, mean over segments, no nfft
    padding, detrend 'constant' or False, 2 <= nperseg <= 4096.  numpy in, numpy (freqs, Pxx) out,
    shaped as SciPy's; anything else SciPy's welch offers raises NotImplementedError."""
    _refuse_nfft("welch", x, window, nperseg, nfft, axis)
    _refuse_options("welch", return_onesided, average, detrend)
    x = _real_input("welch", x, "input x")
    _not_empty("welch", x)
    xd, rest = _time_major(x, axis)
    freqs, psd = sigchain.welch(xd, fs, window, nperseg, noverlap, detrend, scaling)
    return freqs, _from_time_major(psd, rest, axis)


def spectrogram(x, fs=1.0, window=('tukey', .25), nperseg=None, noverlap=None, nfft=None, detrend='constant',
                return_onesided=True, scaling='density', axis=-1, mode='psd'):
    """scipy.signal.spectrogram with its parameter order and defaults, on the device
    (wc_spectrogram), under welch's restrictions: real input, one-sided, no nfft padding, detrend
    'constant' or False, 2 <= nperseg <= 4096.  numpy in, numpy (f, t, Sxx) out, shaped as SciPy's
    (the frequencies where axis was, the segments last); anything else SciPy's spectrogram offers
    raises NotImplementedError.  mode 'phase' is np.unwrap, on the host, of the device's angles
    along the last axis, the segments: each bin's phase is continuous over time.  (SciPy 1.15
    passes its adjusted data axis to np.unwrap, which is the frequency axis of its result; the
    two agree up to multiples of 2 pi.)"""
    modes = ['psd', 'complex', 'magnitude', 'angle', 'phase']
    if mode not in modes:
        raise ValueError(f'unknown value for mode {mode}, must be one of {modes}')
    _refuse_nfft("spectrogram", x, window, nperseg, nfft, axis)
    _refuse_options("spectrogram", return_onesided, 'mean', detrend)
    x = _real_input("spectrogram", x, "input x")
    _not_empty("spectrogram", x)
    xd, rest = _time_major(x, axis)
    freqs, times, sxx = sigchain.spectrogram(xd, fs, window, nperseg, noverlap, detrend, scaling,
                                             'angle' if mode == 'phase' else mode)
    sxx = sxx.cpu().numpy().reshape((sxx.shape[0],) + rest + (sxx.shape[-1],))
    if mode == 'phase':
        sxx = np.unwrap(sxx, axis=-1)
    if rest:  # the segments are a new last axis: a negative data axis counts from one further back
        sxx = np.moveaxis(sxx, 0, axis - 1 if axis < 0 else axis)
    return freqs, times, sxx


def _cross_input(name, x, y, window, nperseg, nfft, detrend, axis, return_onesided=True, average='mean'):
    """What csd and coherence refuse before they touch the device, and x, y as (time, columns)
    device tensors with the shape of the remaining axes."""
    x, y = _real_input(name, x), _real_input(name, y)
    if x.shape != y.shape:
        raise NotImplementedError(f"{name}: x and y of different shapes or lengths (broadcasting, zero padding of the "
                                  "shorter) do not run on the device")
    _not_empty(name, x)
    _refuse_nfft(name, x, window, nperseg, nfft, axis)
    _refuse_options(name, return_onesided, average, detrend)
    (xd, rest), (yd, _) = _time_major(x, axis), _time_major(y, axis)
    return xd, yd, rest


def csd(x, y, fs=1.0, window='hann', nperseg=None, noverlap=None, nfft=None, detrend='constant',
        return_onesided=True, scaling='density', axis=-1, average='mean'):
    """scipy.signal.csd with its parameter order and defaults, on the device (wc_csd's pair mode),
    for equally shaped real x and y: one-sided, mean over segments, no nfft padding, detrend
    'constant' or False, 2 <= nperseg <= 4096.  numpy in, numpy (freqs, Pxy) out, complex, shaped as
    SciPy's; anything else SciPy's csd offers raises NotImplementedError."""
    xd, yd, rest = _cross_input("csd", x, y, window, nperseg, nfft, detrend, axis, return_onesided, average)
    freqs, p = sigchain.csd(xd, yd, fs, window, nperseg, noverlap, detrend, scaling)
    return freqs, _from_time_major(p, rest, axis)


def coherence(x, y, fs=1.0, window='hann', nperseg=None, noverlap=None, nfft=None, detrend='constant', axis=-1):
    """scipy.signal.coherence with its parameter order and defaults, on the device (wc_csd's pair
    mode), under csd's restrictions.  numpy in, numpy (freqs, Cxy) out."""
    xd, yd, rest = _cross_input("coherence", x, y, window, nperseg, nfft, detrend, axis)
    freqs, c = sigchain.coherence(xd, yd, fs, window, nperseg, noverlap, detrend)
    return freqs, _from_time_major(c, rest, axis)


def _matrix_input(name, x, detrend):
    x = _real_input(name, x)
    _refuse_detrend(name, detrend)
    if x.ndim != 2 or x.size == 0:
        raise ValueError(f"{name}: x must be (time, rois)")
    return _upload(x)


def csd_matrix(x, fs=1.0, window='hann', nperseg=None, noverlap=None, detrend='constant', scaling='density'):
    """The cross-spectral matrix of x (time, rois), rois <= 1024: (freqs, P) with P [F][rois][rois]
    complex, P[f][i][j] = scipy.signal.csd(x[:, i], x[:, j], ...)[1][f] -- SciPy's broadcast form
    csd(x[:, :, None], x[:, None, :], axis=0) without its time x rois x rois intermediate."""
    freqs, p = sigchain.csd(_matrix_input("csd_matrix", x, detrend), None, fs, window, nperseg, noverlap, detrend,
                            scaling)
    return freqs, p.cpu().numpy()


def coherence_matrix(x, fs=1.0, window='hann', nperseg=None, noverlap=None, detrend='constant'):
    """The magnitude-squared coherence between the columns of x (time, rois): (freqs, C) with
    C [F][rois][rois] real, symmetric, the spectral counterpart of the FC matrix."""
    freqs, c = sigchain.coherence(_matrix_input("coherence_matrix", x, detrend), None, fs, window, nperseg, noverlap,
                                  detrend)
    return freqs, c.cpu().numpy()


def _series(name, series, freqs=None):
    """series as a host array of real numbers, (time, rois) or (time, B, N), not empty; freqs, if given, a band."""
    x = np.asarray(series)
    if x.dtype.kind not in "fiub":
        raise TypeError(f"{name}: series must be real numbers, not {x.dtype}")
    if x.ndim not in (2, 3) or x.size == 0:
        raise ValueError("series must be (time, rois) or (time, B, N)")
    if freqs is not None and len(freqs) != 2:
        raise ValueError("freqs must be [fmin, fmax] or None")
    return x


def _band_limited(xt, dt, freqs):
    """utils.envelope's Bessel order-3 band-pass filtfilt over freqs; freqs None: xt as it is."""
    if freqs is None:
        return xt
    (bb, ba), _ = sigchain.envelope_filters(float(dt), float(freqs[0]), float(freqs[1]), None)
    return sigchain.filtfilt(bb, ba, xt)


def connectivity(series, dt=0.002, freqs=[8, 13], measures=("plv", "pli", "wpli", "aec", "aec_orth"),
                 device="cuda"):
    """Phase and envelope connectivity of series (time, rois) or (time, B, N) in a band: utils.envelope's
    Bessel order-3 band-pass filtfilt over freqs (Hz, at sampling step dt; freqs=None: series is taken
    as band-limited already), then, from the analytic signal along time, the matrices between the
    columns of each simulation: "plv" phase-locking value, "pli" phase-lag index, "wpli" weighted
    phase-lag index, "aec" amplitude-envelope correlation and "aec_orth" its pairwise
    orthogonalised form (sigchain.phase_connectivity).  numpy in (float32 accepted), a dict of
    numpy arrays (rois, rois) or (B, N, N) out.  time <= 524288 (with a band-pass: >= 22, the
    order-6 filter's padlen is 21), N <= 1024."""
    names = _args.names("connectivity", measures, sigchain.CONN_MEASURES)
    xt = _band_limited(_upload(_series("connectivity", series, freqs), device), dt, freqs)
    return {m: v.cpu().numpy() for m, v in sigchain.phase_connectivity(xt, names).items()}


def fcd(series, window=30, step=1, method="corr", trim=0, device="cuda"):
    """Functional connectivity dynamics of series (time, rois) or (time, B, N) on the device
    (sigchain.fcd).  method="corr": the correlations between the FC patterns of sliding windows of
    `window` samples every `step` -> (nw, nw) or (B, nw, nw), nw = (time - window) // step + 1.
    method="phase": the cosine similarities between the instantaneous phase-coherence patterns of an
    already band-limited series, less `trim` samples at either end -> (time - 2 trim, time - 2 trim)
    or with a leading B; window and step are not used.  numpy in (float32 accepted), numpy out.
    3 <= N <= 96 (phase: 2), nw and time - 2 trim <= 4096."""
    x = _series("fcd", series)
    if method not in sigchain.FCD_METHODS:
        raise ValueError(f"fcd: unknown method {method!r}, must be one of {list(sigchain.FCD_METHODS)}")
    xt = _upload(x, device)
    if method == "phase":
        return sigchain.fcd(xt, method="phase", trim=trim).cpu().numpy()
    return sigchain.fcd(xt, window, step).cpu().numpy()


def leida(series, dt, freqs, centroids=None, k=None, trim=0, metric="cosine", device="cuda"):
    """LEiDA (Cabral et al. 2017) of series (time, rois) or (time, B, N) on the device: utils.envelope's
    Bessel order-3 band-pass filtfilt over freqs (Hz, at sampling step dt; freqs=None: series is taken
    as band-limited already), then sigchain.leida: the leading eigenvector of every instantaneous
    phase-coherence matrix, less `trim` samples at either end.  numpy in (float32 accepted), a dict of
    numpy arrays out: "vec" (time - 2 trim, [B,] N) and "share" (time - 2 trim[, B]).  With centroids
    (K, N) also sigchain.leida_states' "labels", "occupancy", "dwell" and "trans"; with an integer k
    instead, the eigenvectors of all simulations and times are clustered first (sigchain.kmeans, seed 0)
    and "centroids", "inertia" and "n_iter" are returned too.  2 <= N <= 1024, K <= 32."""
    x = _series("leida", series, freqs)
    if metric not in sigchain.KMEANS_METRICS:
        raise ValueError(f"leida: unknown metric {metric!r}, must be one of {list(sigchain.KMEANS_METRICS)}")
    if centroids is not None and k is not None:
        raise ValueError("leida: give centroids or k, not both")
    if k is not None and not 1 <= int(k) <= sigchain.KMEANS_MAX_K:
        raise ValueError(f"leida: K = {k}: needs 1 <= K <= {sigchain.KMEANS_MAX_K}")
    N = x.shape[-1]
    if centroids is not None:
        centroids = np.array(centroids, dtype=np.float64, order="C")
        if centroids.ndim != 2 or centroids.shape[1] != N or not 1 <= centroids.shape[0] <= sigchain.KMEANS_MAX_K:
            raise ValueError(f"leida: centroids must be (K, N = {N}) with 1 <= K <= {sigchain.KMEANS_MAX_K}")
    if N < 2 or N > sigchain.LEIDA_MAX_N or int(trim) < 0 or x.shape[0] - 2 * int(trim) < 1:
        raise ValueError(f"leida: needs 2 <= N <= {sigchain.LEIDA_MAX_N}, trim >= 0 and time - 2 trim >= 1 "
                         f"(N = {N}, time = {x.shape[0]}, trim = {trim})")
    vec, share = sigchain.leida(_band_limited(_upload(x, device), dt, freqs), trim)
    res = dict(vec=vec, share=share)
    if k is not None:
        cent, _, inertia, n_iter = sigchain.kmeans(vec, int(k), metric)
        res.update(centroids=cent)
    elif centroids is not None:
        cent = torch.from_numpy(centroids).to(device)
    if k is not None or centroids is not None:
        res.update(sigchain.leida_states(vec, cent, metric))
    res = {n: v.cpu().numpy() for n, v in res.items()}
    if k is not None:
        res.update(inertia=inertia, n_iter=n_iter)
    return res


def kuramoto(sign):
    """utils.py:34-40: (sync, meta) of the Kuramoto order parameter of sign (T x N)
    from the phases of its analytic signal (hilbert along axis 0).

    2 <= T <= 524288: series of up to 8192 samples take the direct convolution
    (wc_hilbert_phase), longer ones the FFT path (wc_hilbert_phase_long), e.g.
    cortex_run.py's 29,800-sample BOLD and 300,000-sample E_t."""
    x = torch.as_tensor(np.ascontiguousarray(sign, dtype=np.float64)).to(device)
    if x.ndim != 2:
        raise ValueError("sign must be (time, nodes)")
    out = sigchain.kuramoto(x, B=1, N=x.shape[1]).cpu().numpy()[0]
    return out[0], out[1]


def get_all_metrics(sFC, empFC, data_range=1):
    """utils.py:42-50 -> (corr, euc, ssim, new_metric) of sFC against empFC:
    Pearson and Euclidean distance of the strict upper triangles, skimage SSIM
    (7x7 uniform window, sample covariance), and new_metric."""
    s = np.asarray(sFC, dtype=np.float64)
    e = np.asarray(empFC, dtype=np.float64)
    if s.shape != e.shape or s.ndim != 2 or s.shape[0] != s.shape[1]:
        raise ValueError("sFC and empFC must be square matrices of the same shape")
    fc = torch.as_tensor(np.ascontiguousarray(s)).to(device)[None]
    _, met, _ = sigchain.fc_metrics(fc_in=fc, empfc=e[None], data_range=data_range)
    corr, euc, ssim, newm = met[0, 0].cpu().numpy()
    return corr, euc, ssim, newm

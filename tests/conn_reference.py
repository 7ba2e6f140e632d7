"""Host reference of the connectivity tests (test_connectivity_cpu.py pins it, test_connectivity_gpu.py
checks the device against it): the test signal, and a numpy loop over the columns for the five
measures of wc_phase_conn / sigchain.phase_connectivity from scipy.signal.hilbert.

With z = hilbert(x, axis=0), a = |z| and u = z / a, for columns i != j
  c = u_i.x u_j.x + u_i.y u_j.y
  s = u_i.y u_j.x - u_i.x u_j.y      two rounded products and one subtraction: numpy's complex product
                                     u_i conj(u_j) may contract one of them into an FMA, and then a
                                     duplicated column has the product's rounding residue for s, not 0
  plv = sqrt((sum c)^2 + (sum s)^2) / T       pli = |sum sign(s)| / T
  wpli = |sum a_i a_j s| / sum |a_i a_j s|    aec = corr(a_i, a_j)
  aec_orth = (corr(a_i |s|, a_j) + corr(a_j |s|, a_i)) / 2
and the diagonals 1 (plv, aec) and 0.  A zero denominator gives NaN."""
import numpy as np
from scipy import signal

MEASURES = ("plv", "pli", "wpli", "aec", "aec_orth")
DIAGONAL = {"plv": 1.0, "pli": 0.0, "wpli": 0.0, "aec": 1.0, "aec_orth": 0.0}


def make(T, C, seed):
    """[T][C]: per column an amplitude-modulated sinusoid of its own frequency near 10 Hz (at 500 Hz),
    plus a modulated component all columns share, plus 0.2 white noise, plus an offset of 0.2."""
    rng = np.random.default_rng(seed)
    t = np.arange(T)[:, None] * 0.002
    f = 10.0 + rng.uniform(-0.6, 0.6, C)
    p = rng.uniform(0, 2 * np.pi, C)
    g = rng.uniform(0.3, 1.1, C)
    q = rng.uniform(0, 2 * np.pi, C)
    own = (1 + 0.4 * np.sin(2 * np.pi * g * t + q)) * np.cos(2 * np.pi * f * t + p)
    shared = (1 + 0.5 * np.sin(2 * np.pi * 0.7 * t)) * np.cos(2 * np.pi * 10.2 * t + 0.3)
    x = own + rng.uniform(0.2, 0.6, C) * shared + 0.2 * rng.standard_normal((T, C)) + 0.2
    return np.ascontiguousarray(x)


def analytic(x):
    """(u [T][C] complex unit phasors, a [T][C] envelopes) of hilbert(x, axis=0)."""
    z = signal.hilbert(np.asarray(x, dtype=np.float64), axis=0)
    a = np.abs(z)
    return z / a, a


def lag(u, i):
    """s [T][C] of column i against every column j, in the explicit real form."""
    return u[:, i:i + 1].imag * u.real - u[:, i:i + 1].real * u.imag


def _corr(p, a):
    """Pearson's r of the columns of p with those of a (both [T][C]); NaN where either is constant."""
    dp, da = p - p.mean(axis=0), a - a.mean(axis=0)
    with np.errstate(invalid="ignore", divide="ignore"):
        return (dp * da).sum(axis=0) / np.sqrt((dp * dp).sum(axis=0) * (da * da).sum(axis=0))


def from_analytic(u, a):
    """The five [C][C] matrices from unit phasors u (complex) and envelopes a, column by column."""
    T, C = u.shape
    out = {m: np.empty((C, C)) for m in MEASURES}
    for i in range(C):
        ui = u[:, i:i + 1]
        c = ui.real * u.real + ui.imag * u.imag
        s = lag(u, i)
        w = (a[:, i:i + 1] * a) * s
        out["plv"][i] = np.sqrt(c.sum(axis=0) ** 2 + s.sum(axis=0) ** 2) / T
        out["pli"][i] = np.abs(np.sign(s).sum(axis=0)) / T
        with np.errstate(invalid="ignore", divide="ignore"):
            out["wpli"][i] = np.abs(w.sum(axis=0)) / np.abs(w).sum(axis=0)
        ai = np.broadcast_to(a[:, i:i + 1], a.shape)
        out["aec"][i] = _corr(ai, a)
        out["aec_orth"][i] = 0.5 * (_corr(ai * np.abs(s), a) + _corr(a * np.abs(s), ai))
    for m in MEASURES:
        np.fill_diagonal(out[m], DIAGONAL[m])
    return out


def connectivity(x):
    """The five matrices of a real [T][C] array, as a dict of [C][C] arrays."""
    return from_analytic(*analytic(x))


def near_zero_lags(x, eps=1e-10):
    """How many (t, i < j) have |s_ij(t)| < eps (pli is discontinuous there), and the smallest |s|."""
    u, _ = analytic(x)
    n, least = 0, np.inf
    for i in range(u.shape[1] - 1):
        s = np.abs(lag(u, i)[:, i + 1:])
        n += int((s < eps).sum())
        least = min(least, float(s.min()))
    return n, least


def off_diagonal(m):
    """The off-diagonal entries of a [C][C] (or [B][C][C]) array, flattened."""
    C = m.shape[-1]
    return m[..., ~np.eye(C, dtype=bool)]


def deviation(got, want):
    """max |got - want| over the off-diagonal entries (0 without any); NaN must sit where want's does."""
    g, w = off_diagonal(np.asarray(got)), off_diagonal(np.asarray(want))
    nan = np.isnan(w)
    np.testing.assert_array_equal(np.isnan(g), nan)
    return float(np.abs(g - w)[~nan].max()) if (~nan).any() else 0.0

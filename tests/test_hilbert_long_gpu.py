"""wc_hilbert_phase_long (Bluestein over a four-step power-of-two FFT, wc_hilbert.hip) against the
oracle's scipy-style hilbert / kuramoto, at the lengths where each mechanism can break.

Bounds: phasors to 1e-12 absolute (a NumPy restatement of the algorithm is 3.3e-15 .. 5.4e-15 from
the oracle at these shapes; the rest is room for device sincospi over 20 butterfly stages), Kuramoto
(sync, meta) to the project's rtol 1e-9 (test_signal_gpu.py).

Measured on MI355X, max |phasor - oracle phasor| (min |analytic| of the recipe):
  (8193, 6) 4.0e-15 (0.134)   (16384, 6) 3.0e-15 (0.134)   (16385, 6) 3.0e-15 (0.134)
  (29800, 90) 4.6e-15 (0.133)   (300000, 90) 4.3e-15 (0.107)
  long entry point at M = 2 / 3 / 298 / 4000: 1.3e-16 / 3.7e-16 / 2.4e-15 / 2.5e-15 from the oracle,
  8.4e-17 / 3.4e-16 / 3.3e-15 / 1.3e-14 from wc_hilbert_phase.
All below 1e-13, so no stage needs singling out.
"""
import functools

import numpy as np
import pytest
import torch

import oracle.sigchain as osg
from nremmodfc_amd import _lib, datasets, utils
from nremmodfc_amd import sigchain as wsg

pytestmark = pytest.mark.gpu

# (M, C): first length past the dispatch (odd); 2 M - 1 = L - 1, the tightest fit; L doubles;
# cortex_run.py's BOLD (prime factor 149); cortex_run.py's E_t (L = 2^20)
SHAPES = [(8193, 6), (16384, 6), (16385, 6), (29800, 90), (300_000, 90)]


def make_signal(M, C):
    """Amplitude-modulated 2-12 Hz carriers at 500 Hz plus a little noise; even columns are shifted
    positive (E-like), odd columns rotate through every phase."""
    rng = np.random.default_rng(M)
    t = np.arange(M)[:, None] * 0.002
    f = rng.uniform(2, 12, C)
    p = rng.uniform(0, 2 * np.pi, C)
    g = rng.uniform(0.05, 0.2, C)
    x = (1 + 0.3 * np.sin(2 * np.pi * g * t)) * np.cos(2 * np.pi * f * t + p) + 0.01 * rng.standard_normal((M, C))
    x[:, ::2] = 0.2 + 0.05 * x[:, ::2]
    return np.ascontiguousarray(x)


@functools.lru_cache(maxsize=None)
def case(M, C):
    """(x, oracle phasors, min |analytic|, oracle (sync, meta)): computed once per shape, read only."""
    x = make_signal(M, C)
    an = osg.hilbert(x)
    mag = np.abs(an)
    ph = an / mag
    R = np.abs(ph.mean(axis=1))
    ph.setflags(write=False)
    return x, ph, float(mag.min()), (R.mean(), R.std())


def as_complex(ph):
    ph = ph.cpu().numpy()
    return ph[..., 0] + 1j * ph[..., 1]


@pytest.mark.parametrize("M,C", SHAPES)
def test_phasors_vs_oracle(cuda, M, C):
    x, want, minmag, _ = case(M, C)
    assert minmag >= 0.1, minmag  # the phase is well conditioned
    got = as_complex(wsg.hilbert_phase(torch.from_numpy(x).to(cuda)))
    err = np.abs(got - want).max()
    print(f"hilbert_phase ({M}, {C}): min |analytic| = {minmag:.3f}, max |dphasor| = {err:.3e}")
    assert err <= 1e-12, err


@pytest.mark.parametrize("M,C", SHAPES)
def test_kuramoto_vs_oracle(cuda, M, C):
    x, _, _, want = case(M, C)
    if C == 90:  # the facade, as cortex_run.py calls it
        got = utils.kuramoto(x)
    else:
        got = wsg.kuramoto(torch.from_numpy(x).to(cuda))[0].cpu().numpy()
    print(f"kuramoto ({M}, {C}): {got[0]!r}, {got[1]!r} vs {want[0]!r}, {want[1]!r}")
    np.testing.assert_allclose(got, want, rtol=1e-9)


@pytest.mark.parametrize("M", [2, 3, 298, 4000])
def test_small_m_through_the_long_entry_point(cuda, M):
    """Below the dispatch the long kernel is called directly: scipy's h for odd and even M, and the
    padding to L = 2^15; against the oracle and against wc_hilbert_phase."""
    C = 7
    x = make_signal(M, C)
    xt = torch.from_numpy(x).to(cuda)
    want = osg.hilbert(x)
    want = want / np.abs(want)
    got = as_complex(wsg.hilbert_phase_long(xt))
    direct = as_complex(wsg.hilbert_phase(xt))
    e_or, e_di = np.abs(got - want).max(), np.abs(got - direct).max()
    print(f"long entry point M = {M}: vs oracle {e_or:.3e}, vs wc_hilbert_phase {e_di:.3e}")
    assert e_or <= 1e-12
    assert e_di <= 1e-12


def test_tile_invariance(cuda):
    """Minimum workspace (one column per pass), five more columns' worth (ragged last tile of
    37 = 6 * 6 + 1), and room for all: bit-identical phasors."""
    M, C = 16385, 37
    xt = torch.from_numpy(make_signal(M, C)).to(cuda)
    need = _lib.lib().wc_hilbert_long_workspace_size(C, M)
    per_col = 32 * (1 << 16)  # two [L] complex buffers, L = nextpow2(2 M - 1) = 2^16
    outs = [wsg.hilbert_phase_long(xt, ws_bytes=n) for n in (need, need + 5 * per_col, need + (C - 1) * per_col)]
    assert torch.equal(outs[0], outs[1])
    assert torch.equal(outs[0], outs[2])
    assert torch.isfinite(outs[0]).all()


def test_pipeline_epilogue_takes_the_long_path(cuda, sc90):
    """run_sweep at bold_downsamp = 10: 85,000 recorded samples -> M = 8,300 BOLD samples, past the
    direct kernel's range, so sync/meta come from wc_hilbert_phase_long."""
    from nremmodfc_amd.model import Schedule, sim_keys
    from nremmodfc_amd.pipeline import run_sweep
    sch = Schedule.from_seconds(0.01, 0.1, 170.0)
    G = np.array([0.16, 0.22])
    S = np.array([7.68, 7.80])
    keys = sim_keys([0, 1], [0, 5])
    emp = {s: datasets.load_empfc(s) for s in datasets.STATES}
    res = run_sweep(sc90, G, S, keys, emp, sch, bold_downsamp=10, want_bold=True)
    assert res.bold.shape == (8300, 2, 90)
    assert res.bold.shape[0] > wsg.HILBERT_DIRECT_MAX_M
    for b in range(2):
        want = osg.kuramoto(res.bold[:, b, :])
        print(f"pipeline b = {b}: {res.sync[b]!r}, {res.meta[b]!r} vs {want[0]!r}, {want[1]!r}")
        np.testing.assert_allclose((res.sync[b], res.meta[b]), want, rtol=1e-9)
    for name, v in res.columns().items():
        assert np.isfinite(v).all(), name

"""utils.envelope on the device (wc_filtfilt at odd orders, wc_hilbert_envelope, sigchain.envelope)
against SciPy: signal.filtfilt, np.abs(signal.hilbert(., axis=0)) and the reference's expression
(utils.py:145-154) built from them.

Bounds.  filtfilt: bit-equal (the kernel's claim: SciPy's DF2T recursion in SciPy's association
order, FMA contraction off).  Hilbert modulus: 1e-12 * scale, scale = max |SciPy envelope| of the
array: the phasor bound of test_hilbert_long_gpu.py, the arithmetic being the same up to the final
normalisation.  End to end: 10x the deviation measured on MI355X per fcut (the low-pass amplifies
its input's 1e-15-level differences: about 9x at fcut = 2.0, 230x at fcut = 0.5 in (b, a) form),
never above the project's signal-chain rtol 1e-9; E2E_BOUND below.

Measured on MI355X (max |got - SciPy| / scale):
  modulus, direct / long / direct vs long, C = 7:  M = 2: 1.2e-16 / 5.9e-17 / 1.2e-16   3: 2.3e-16 / 3.5e-16 /
    3.5e-16   298: 1.4e-15 / 1.2e-15 / 1.6e-15   4000: 5.9e-15 / 1.2e-15 / 5.9e-15
  modulus, long:  (8193, 6) 1.9e-15   (16385, 6) 1.4e-15   (29800, 90) 1.2e-15
  modulus, auto:  (2047, 7) 2.8e-15 (direct)   (2048, 7) 5.5e-16 (long)
  envelope of SciPy's band-passed array:  (22, 5) 2.2e-16   (298, 7) 9.8e-16   (4000, 7) 1.3e-15
  end to end, fcut = None / 2.0 / 0.5:  (298, 7) 9.8e-16 / 1.9e-12 / 4.6e-11   (8193, 6) 1.9e-15 / 4.4e-12 /
    1.3e-10   (29800, 90) 2.2e-15 / 6.0e-12 / 2.0e-10   utils.envelope (300000, 90), fcut = 2.0: 7.5e-12
  so the maxima per fcut are 2.2e-15 / 7.5e-12 / 2.0e-10, and 10x the last would pass 1e-9: capped there.
"""
import functools

import numpy as np
import pytest
import torch
from scipy import signal

from nremmodfc_amd import _lib, utils
from nremmodfc_amd import sigchain as wsg

pytestmark = pytest.mark.gpu

AUTO_LONG_M = 2048   # wc_hilbert_envelope's method 0: direct below, long from here on (docs/CHANGELOG.md)
E2E_BOUND = {None: 2.2e-14, 2.0: 7.5e-11, 0.5: 1e-9}  # x scale; 10x the measured maxima above, at most 1e-9


def make_signal(M, C):
    """Amplitude-modulated 2-12 Hz carriers at 500 Hz plus a little noise; even columns are shifted
    positive (E-like), odd columns rotate through every phase (test_hilbert_long_gpu.py's recipe)."""
    rng = np.random.default_rng(M)
    t = np.arange(M)[:, None] * 0.002
    f = rng.uniform(2, 12, C)
    p = rng.uniform(0, 2 * np.pi, C)
    g = rng.uniform(0.05, 0.2, C)
    x = (1 + 0.3 * np.sin(2 * np.pi * g * t)) * np.cos(2 * np.pi * f * t + p) + 0.01 * rng.standard_normal((M, C))
    x[:, ::2] = 0.2 + 0.05 * x[:, ::2]
    return np.ascontiguousarray(x)


def frozen(a):
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def modulus_case(M, C):
    """(x, |scipy hilbert|, scale): computed once per shape, read only."""
    x = frozen(make_signal(M, C))
    env = frozen(np.abs(signal.hilbert(x, axis=0)))
    return x, env, float(env.max())


@functools.lru_cache(maxsize=None)
def chain_case(M, C, dt=0.002, freqs=(8, 13)):
    """SciPy's intermediates of utils.envelope: (x, band-passed x, its envelope)."""
    x = frozen(make_signal(M, C))
    b, a = signal.bessel(3, [2 * dt * freqs[0], 2 * dt * freqs[1]], btype="bandpass")
    v = frozen(signal.filtfilt(b, a, x, axis=0))
    env = frozen(np.abs(signal.hilbert(v, axis=0)))
    return x, v, env


@functools.lru_cache(maxsize=None)
def chain_lowpass(M, C, fcut, dt=0.002):
    """The reference's result for a truthy fcut: the low-passed envelope of chain_case."""
    b, a = signal.bessel(3, [2 * dt * fcut], btype="low")
    return frozen(signal.filtfilt(b, a, chain_case(M, C)[2], axis=0))


def reference_envelope(M, C, fcut):
    return chain_lowpass(M, C, fcut) if fcut else chain_case(M, C)[2]


def dev(x, cuda):
    return torch.tensor(np.ascontiguousarray(x), device=cuda)  # a copy: the shared cases are read only


ODD_FILTERS = {
    "bessel3_low": lambda: signal.bessel(3, 0.004, "low"),
    "butter1": lambda: signal.butter(1, 0.1),
    "bessel5": lambda: signal.bessel(5, 0.1),
    "bessel7": lambda: signal.bessel(7, 0.2),
}


@pytest.mark.parametrize("tail", [1, 17, None])
@pytest.mark.parametrize("name", list(ODD_FILTERS))
def test_odd_order_filtfilt_is_bit_equal_to_scipy(cuda, name, tail):
    """T = padlen + 1 (the shortest legal series), padlen + 17 (one 16-sample batch and a tail),
    1001 (many batches, odd tail); C = 5 and 300 (two workgroups)."""
    b, a = ODD_FILTERS[name]()
    K = len(a) - 1
    assert K % 2 == 1
    T = 1001 if tail is None else 3 * (K + 1) + tail
    for C in (5, 300):
        x = np.random.default_rng(100 * K + C).standard_normal((T, C)).cumsum(0) * 0.01
        got = wsg.filtfilt(b, a, dev(x, cuda)).cpu().numpy()
        np.testing.assert_array_equal(got, signal.filtfilt(b, a, x, axis=0))


def test_filtfilt_wrapper_shapes_and_errors(cuda):
    b, a = signal.bessel(3, 0.1, "low")
    x = np.random.default_rng(1).standard_normal((50, 3, 4))
    got = wsg.filtfilt(b, a, dev(x, cuda))
    assert got.shape == (50, 3, 4)
    np.testing.assert_array_equal(got.cpu().numpy(), signal.filtfilt(b, a, x, axis=0))
    with pytest.raises(_lib.WCSDEError, match="padlen"):
        wsg.filtfilt(b, a, dev(x[:12], cuda))
    b9, a9 = signal.butter(9, 0.3)
    with pytest.raises(_lib.WCSDEError, match="order"):
        wsg.filtfilt(b9, a9, dev(x, cuda))


@pytest.mark.parametrize("M", [2, 3, 298, 4000])
def test_modulus_both_methods(cuda, M):
    x, want, scale = modulus_case(M, 7)
    xt = dev(x, cuda)
    direct = wsg.hilbert_envelope(xt, method=1).cpu().numpy()
    long_ = wsg.hilbert_envelope(xt, method=2).cpu().numpy()
    e1, e2, e12 = (np.abs(direct - want).max() / scale, np.abs(long_ - want).max() / scale,
                   np.abs(direct - long_).max() / scale)
    print(f"modulus ({M}, 7): direct {e1:.3e}, long {e2:.3e}, direct vs long {e12:.3e} (x scale {scale:.3f})")
    assert e1 <= 1e-12 and e2 <= 1e-12 and e12 <= 1e-12


@pytest.mark.parametrize("M,C", [(8193, 6), (16385, 6), (29800, 90)])
def test_modulus_long(cuda, M, C):
    x, want, scale = modulus_case(M, C)
    got = wsg.hilbert_envelope(dev(x, cuda), method=2).cpu().numpy()
    err = np.abs(got - want).max() / scale
    print(f"modulus ({M}, {C}): long {err:.3e} (x scale {scale:.3f})")
    assert err <= 1e-12
    if M == 8193:
        with pytest.raises(_lib.WCSDEError, match="8192"):
            wsg.hilbert_envelope(dev(x, cuda), method=1)


@pytest.mark.parametrize("M,method", [(AUTO_LONG_M - 1, 1), (AUTO_LONG_M, 2)])
def test_modulus_auto_dispatch(cuda, M, method):
    """Either side of the threshold: within the bound, and the bits of the method it names."""
    x, want, scale = modulus_case(M, 7)
    xt = dev(x, cuda)
    auto = wsg.hilbert_envelope(xt)
    err = np.abs(auto.cpu().numpy() - want).max() / scale
    print(f"modulus ({M}, 7): auto {err:.3e} (x scale {scale:.3f})")
    assert err <= 1e-12
    assert torch.equal(auto, wsg.hilbert_envelope(xt, method=method))


def test_modulus_tile_invariance(cuda):
    """Minimum workspace (one column per pass), five more columns' worth (ragged last tile of
    37 = 6 * 6 + 1), and room for all: bit-identical envelopes."""
    M, C = 16385, 37
    xt = dev(make_signal(M, C), cuda)
    need = _lib.lib().wc_hilbert_envelope_workspace_size(C, M, 2)
    per_col = 32 * (1 << 16)  # two [L] complex buffers, L = nextpow2(2 M - 1) = 2^16
    outs = [wsg.hilbert_envelope(xt, method=2, ws_bytes=n)
            for n in (need, need + 5 * per_col, need + (C - 1) * per_col)]
    assert torch.equal(outs[0], outs[1])
    assert torch.equal(outs[0], outs[2])
    assert torch.isfinite(outs[0]).all() and (outs[0] > 0).all()


@pytest.mark.parametrize("M,C", [(22, 5), (298, 7), (4000, 7)])
def test_chain_stage_by_stage(cuda, M, C):
    """Each stage on SciPy's own intermediate; (22, 5) is the shortest series the order-6 band-pass takes."""
    x, v, env = chain_case(M, C)
    (bb, ba), (lb, la) = wsg.envelope_filters(0.002, 8.0, 13.0, 2.0)
    np.testing.assert_array_equal(wsg.filtfilt(bb, ba, dev(x, cuda)).cpu().numpy(), v)
    scale = float(env.max())
    got = wsg.hilbert_envelope(dev(v, cuda)).cpu().numpy()
    err = np.abs(got - env).max() / scale
    print(f"chain ({M}, {C}): envelope of SciPy's band-pass {err:.3e} (x scale {scale:.3e})")
    assert err <= 1e-12
    np.testing.assert_array_equal(wsg.filtfilt(lb, la, dev(env, cuda)).cpu().numpy(), chain_lowpass(M, C, 2.0))


@pytest.mark.parametrize("fcut", [None, 2.0, 0.5])
@pytest.mark.parametrize("M,C", [(298, 7), (8193, 6), (29800, 90)])
def test_envelope_end_to_end(cuda, M, C, fcut):
    x = chain_case(M, C)[0]
    want = reference_envelope(M, C, fcut)
    scale = float(np.abs(want).max())
    got = wsg.envelope(dev(x, cuda), freqs=[8, 13], fcut=fcut)
    assert got.is_cuda and got.shape == (M, C)
    err = np.abs(got.cpu().numpy() - want).max() / scale
    print(f"envelope ({M}, {C}) fcut = {fcut}: {err:.3e} (x scale {scale:.3e})")
    assert err <= E2E_BOUND[fcut]
    facade = utils.envelope(x, freqs=[8, 13], fcut=fcut)
    assert isinstance(facade, np.ndarray) and facade.shape == (M, C)
    np.testing.assert_array_equal(facade, got.cpu().numpy())


def test_utils_envelope_cortex_run_shape(cuda):
    """cortex_run.py's E_t: 300,000 samples of 90 nodes at dt = 0.002."""
    M, C, fcut = 300_000, 90, 2.0
    x = chain_case(M, C)[0]
    want = reference_envelope(M, C, fcut)
    scale = float(np.abs(want).max())
    got = utils.envelope(x, fcut=fcut)
    err = np.abs(got - want).max() / scale
    print(f"utils.envelope ({M}, {C}) fcut = {fcut}: {err:.3e} (x scale {scale:.3e})")
    assert err <= E2E_BOUND[fcut]


def test_envelope_one_dimensional_input_and_zero_fcut(cuda):
    M, C = 298, 7
    x = chain_case(M, C)[0]
    full = utils.envelope(x, fcut=2.0)
    one = utils.envelope(x[:, 3], fcut=2.0)
    assert one.shape == (M,)
    np.testing.assert_array_equal(one, full[:, 3])   # a column's arithmetic does not depend on C
    np.testing.assert_array_equal(utils.envelope(x, fcut=0), utils.envelope(x, fcut=None))
    np.testing.assert_array_equal(utils.envelope(x, fcut=0), utils.envelope(x))
    x3 = dev(x[:, :6], cuda).reshape(M, 2, 3)
    got3 = wsg.envelope(x3, fcut=0.5)
    assert got3.shape == (M, 2, 3)
    assert torch.equal(got3.reshape(M, 6), wsg.envelope(dev(x[:, :6], cuda), fcut=0.5))

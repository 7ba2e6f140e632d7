"""utils.envelope's entry points validate before any device work, and the pure-numpy matrix
helpers of utils.py (sub_weight, cortex_mat, scale_mat) do what utils.py:52-74, 134-143 do (no GPU)."""
import ctypes

import numpy as np


def _dp(*v):
    return (ctypes.c_double * len(v))(*v)


def test_filtfilt_orders_validate_without_device_work():
    from nremmodfc_amd import _lib
    L = _lib.lib()
    vp, vq = ctypes.c_void_p(16), ctypes.c_void_p(4096)
    b3, a3, zi3 = _dp(0.1, 0.2, 0.2, 0.1), _dp(1.0, 0.1, 0.1, 0.1), _dp(0.0, 0.0, 0.0)
    assert L.wc_filtfilt(3, b3, a3, zi3, 12, 5, vp, vq, None) == -1  # T must exceed padlen = 3 (3 + 1)
    assert b"padlen" in L.wc_last_error()
    b9, a9, zi9 = _dp(*([0.1] * 10)), _dp(1.0, *([0.1] * 9)), _dp(*([0.0] * 9))
    assert L.wc_filtfilt(9, b9, a9, zi9, 1000, 5, vp, vq, None) == -2
    assert L.wc_filtfilt(0, b3, a3, zi3, 1000, 5, vp, vq, None) == -2
    assert L.wc_filtfilt(3, b3, a3, zi3, 1000, 5, vp, vp, None) == -1  # y aliasing x


def test_hilbert_envelope_validates_without_device_work():
    from nremmodfc_amd import _lib
    L = _lib.lib()
    x, env, ws = ctypes.c_void_p(4096), ctypes.c_void_p(8192), ctypes.c_void_p(1 << 20)
    big = 1 << 40
    assert L.wc_hilbert_envelope(7, 1, x, env, 0, ws, big, None) == -1          # M < 2
    assert L.wc_hilbert_envelope(0, 298, x, env, 0, ws, big, None) == -1        # no columns
    assert L.wc_hilbert_envelope(7, 298, None, env, 0, ws, big, None) == -1
    assert L.wc_hilbert_envelope(7, 298, x, None, 0, ws, big, None) == -1
    assert L.wc_hilbert_envelope(7, 298, x, x, 0, ws, big, None) == -1          # env aliasing x
    assert L.wc_hilbert_envelope(7, 298, x, env, 3, ws, big, None) == -1        # method
    assert L.wc_hilbert_envelope(7, 298, x, env, -1, ws, big, None) == -1
    assert L.wc_hilbert_envelope(7, 298, x, ctypes.c_void_p(8196), 1, ws, big, None) == -1  # misaligned env
    assert L.wc_hilbert_envelope(7, 298, x, env, 2, ctypes.c_void_p((1 << 20) + 8), big, None) == -1  # workspace
    assert L.wc_hilbert_envelope(7, 524289, x, env, 0, ws, big, None) == -2
    assert L.wc_hilbert_envelope(7, 524289, x, env, 2, ws, big, None) == -2
    assert b"524288" in L.wc_last_error()
    assert L.wc_hilbert_envelope(7, 8193, x, env, 1, ws, big, None) == -2       # the direct kernel's range
    assert L.wc_hilbert_envelope_workspace_size(7, 524289, 0) == 0
    assert L.wc_hilbert_envelope_workspace_size(7, 8193, 1) == 0
    assert L.wc_hilbert_envelope_workspace_size(7, 1, 0) == 0
    assert L.wc_hilbert_envelope_workspace_size(0, 298, 0) == 0
    assert L.wc_hilbert_envelope_workspace_size(7, 298, 3) == 0
    # direct: M doubles; long: wc_hilbert_long_workspace_size's minimum
    assert L.wc_hilbert_envelope_workspace_size(7, 298, 1) == 298 * 8
    for M in (298, 8193, 524288):
        need = L.wc_hilbert_envelope_workspace_size(7, M, 2)
        assert need == L.wc_hilbert_long_workspace_size(7, M) > 0
        assert L.wc_hilbert_envelope(7, M, x, env, 2, ws, need - 8, None) == -3
        assert b"workspace" in L.wc_last_error()
    assert L.wc_hilbert_envelope(7, 298, x, env, 1, ws, 298 * 8 - 8, None) == -3
    assert L.wc_hilbert_envelope(7, 298, x, env, 1, None, 0, None) == -3
    # auto is one of the two methods at every length
    for M in (2, 298, 4000, 8192, 8193):
        assert L.wc_hilbert_envelope_workspace_size(7, M, 0) in (M * 8, L.wc_hilbert_long_workspace_size(7, M))
    assert L.wc_hilbert_envelope_workspace_size(7, 8193, 0) == L.wc_hilbert_long_workspace_size(7, 8193)


def test_matrix_helpers():
    from nremmodfc_amd import utils
    assert utils.thal == [38, 51]
    assert utils.sub == [35, 36, 37, 38, 51, 52, 53, 54]
    assert utils.cortex == [i for i in range(90) if i not in utils.sub] and len(utils.cortex) == 82
    m = np.random.default_rng(3).uniform(0.1, 1.0, (90, 90))
    keep = m.copy()

    assert np.array_equal(utils.sub_weight(m), m)
    assert np.array_equal(utils.sub_weight(m, 1), m)
    h = utils.sub_weight(m, 0.5)
    is_sub = np.zeros(90, bool)
    is_sub[utils.sub] = True
    touched = is_sub[:, None] ^ is_sub[None, :]   # a subcortical row or column, but not the 8 x 8 block
    want = np.where(touched, 0.5 * m, m)
    assert np.array_equal(h, want)
    assert np.array_equal(h[np.ix_(utils.sub, utils.sub)], m[np.ix_(utils.sub, utils.sub)])
    assert np.array_equal(h[35, :35], 0.5 * m[35, :35]) and np.array_equal(h[:35, 54], 0.5 * m[:35, 54])
    assert touched.sum() == 2 * 8 * 82

    c = utils.cortex_mat(m)
    assert c.shape == (82, 82)
    assert c[0, 0] == m[0, 0] and c[34, 35] == m[34, 39] and c[46, 47] == m[50, 55] and c[81, 81] == m[89, 89]

    s = utils.scale_mat(m, 0.3, 2.0)
    col = np.full(90, 0.3)
    col[utils.thal] = 2.0
    assert np.array_equal(s, m * col[None, :])
    v = np.linspace(1.0, 2.0, 90)            # subG as a vector runs down the thalamic columns
    sv = utils.scale_mat(m, 0.3, v)
    assert np.array_equal(sv[:, 38], v * m[:, 38]) and np.array_equal(sv[:, 51], v * m[:, 51])
    assert np.array_equal(np.delete(sv, utils.thal, axis=1), np.delete(s, utils.thal, axis=1))
    assert np.array_equal(m, keep)           # none of them writes to its argument

"""numpy facade of surrogate.fc_surrogate_test with the reference's signature (graph_utils.py:220-265);
graph_utils imports it by name, so graph_utils.probabilistic_thresholding is a drop-in.  torch and the
device modules are imported on first use."""
import numpy as np


def probabilistic_thresholding(y, surr_number=50, alpha=0.05, conn='corr'):
    """[FC_adjusted, p_matrix]: the FC of the series y [L, N] with the entries removed whose
    Benjamini-Hochberg adjusted p-value against surr_number phase-randomised surrogates is not below
    alpha, and the adjusted p-values; both symmetric with a zero diagonal (graph_utils.py:220-265).
    conn must be 'corr'; anything else raises KeyError('invalid connectivity metric'), as the reference.
    y may be a [B, L, N] stack, which gives [B, N, N] results from one batched run.  L must be even
    (the reference raises for an odd one), 4 <= L <= 4096, 2 <= N <= 96.  Surrogate i has seed i + 1
    as in the reference, but the phases are the engine's Philox stream (include/wcsde.h), not numpy's
    Mersenne Twister: the surrogates are other draws of the same law.  The adjustment is
    scipy.stats.false_discovery_control's."""
    if conn != 'corr':
        raise KeyError('invalid connectivity metric')
    a = np.asarray(y)
    if a.ndim not in (2, 3) or a.dtype.kind not in "fiu":
        raise TypeError(f"probabilistic_thresholding: y must be a real [L, N] array or a [B, L, N] stack, got "
                        f"shape {a.shape}, dtype {a.dtype}")
    import torch

    from . import surrogate
    a = np.ascontiguousarray(a, dtype=np.float64)
    x = torch.from_numpy(a)
    x = x if a.ndim == 2 else x.permute(1, 0, 2).contiguous()     # time-major [L][B][N]
    surrogate._test_args("probabilistic_thresholding", x, surr_number, alpha, None, None)   # before the device is touched
    fc_adj, p_adj = surrogate.fc_surrogate_test(x.cuda(), surr_number=surr_number, alpha=alpha)
    return [fc_adj.cpu().numpy(), p_adj.cpu().numpy()]

"""Surrogate-tested functional connectivity on the device (wc_surrogate.hip): the reference's
probabilistic_thresholding (graph_utils.py:220-265) for a batch.  From a BOLD batch [L][B][N] it gives
the matrices the graph kernels take: the FC entries whose upper-tail p-value against phase-randomised
surrogates, Benjamini-Hochberg adjusted, lies below alpha.  No surrogate series and no inverse FFT is
made: a surrogate's FC is a normalised Gram product of the rotated spectrum (include/wcsde.h).

Device tensors in and out; surrogate_np holds the numpy facade that graph_utils re-exports.
"""
import torch

from . import _args, _lib, sigchain

SURROGATE_MAX_L = 4096            # wc_spectrogram's longest segment
SURROGATE_WS_CAP = 1 << 30        # default cap on the surrogate FCs of a chunk of simulations, in bytes


def surrogate_slab_bytes(N, S):
    """The surrogate FCs of one simulation, S N (N - 1) / 2 fp64."""
    return 8 * S * (N * (N - 1) // 2)


def _series(name, x):
    """(x [L][B][N] contiguous, single, B, N, L) of a [L][N] or time-major [L][B][N] fp64 tensor."""
    x, single, B, N = _args.stack(name, "x must be a [L][N] or time-major [L][B][N] fp64 device tensor", x, batch=1)
    L = x.shape[0]
    if L < 4 or L % 2:
        raise ValueError(f"{name}: L = {L}, needs an even number of samples, at least 4 (the reference's stacked "
                         "phases need an even length)")
    if L > SURROGATE_MAX_L:
        raise ValueError(f"{name}: L = {L} > {SURROGATE_MAX_L} (one transform per workgroup, in LDS)")
    if N < 2 or N > sigchain.GRAPH_MAX_N or B < 1:
        raise ValueError(f"{name}: N = {N}, B = {B}: needs B >= 1 and 2 <= N <= {sigchain.GRAPH_MAX_N} "
                         "(the result feeds the graph kernels)")
    return x.reshape(L, B, N), single, B, N, L


def _spectrum(x):
    """x [L][b][N] contiguous -> the DFT of its mean-free columns at bins 0 .. L/2, complex [L/2 + 1][b N]."""
    L, C = x.shape[0], x.shape[1] * x.shape[2]
    lib = _lib.lib()
    ws_bytes = lib.wc_spectrogram_workspace_size(L)
    ws = _args.workspace(ws_bytes, x.device)
    ones = torch.ones(L, dtype=torch.float64, device=x.device)
    spec = torch.empty((L // 2 + 1, C), dtype=torch.complex128, device=x.device)
    _lib.check(lib.wc_spectrogram(C, L, _lib.ptr(x), L, 0, _lib.ptr(ones), 1, 1.0, sigchain.SPEC_MODES["complex"],
                                  _lib.ptr(spec), _lib.ptr(ws), ws_bytes, _lib.stream_handle()), "wc_spectrogram")
    return spec


def _surrogate_fc(x, seeds_dev, S):
    """x [L][b][N] contiguous -> sfc [b][S][P]."""
    L, b, N = x.shape
    spec = _spectrum(x)
    sfc = torch.empty((b, S, N * (N - 1) // 2), dtype=torch.float64, device=x.device)
    _lib.check(_lib.lib().wc_surrogate_fc(b, N, L, S, _lib.ptr(spec), _lib.ptr(seeds_dev), _lib.ptr(sfc),
                                          _lib.stream_handle()), "wc_surrogate_fc")
    return sfc


def _fc_group(L):
    """The most simulations a wc_corrcoef call may take here: it cuts the series into min(ceil(512 / B),
    ceil(L / 64)) time blocks, and up to this B that is ceil(L / 64), what a simulation alone gets (127 at
    L = 298, 8 at L = 4096, no bound up to L = 64)."""
    most = -(-L // 64)
    return 511 // (most - 1) if most > 1 else None


def _fc(x):
    """x [L][b][N] -> np.corrcoef per simulation [b][N][N], _fc_group(L) simulations a call, so that a
    simulation's FC has the same bits in any batch and any chunk."""
    L, b, N = x.shape
    group = min(b, _fc_group(L) or b)
    parts = [sigchain.corrcoef(x[:, g:g + group].contiguous(), min(group, b - g), N) for g in range(0, b, group)]
    return parts[0] if len(parts) == 1 else torch.cat(parts)


def surrogate_fc(x, seeds):
    """The FC of phase-randomised surrogates on the device (wc_surrogate_fc): x [L][N] or time-major
    [L][B][N] fp64 device tensor (the layout of bold), L even, 4 <= L <= 4096, 2 <= N <= 96; seeds a
    sequence of S >= 2 ints in [0, 2^64) -> sfc [B][S][P] (or [S][P]), the strict upper triangle,
    row-major (get_uptri's order), of np.corrcoef of surrogate s of simulation b.  The phases of a
    surrogate are the engine's Philox stream of its seed (include/wcsde.h) and do not depend on the
    simulation.  A (simulation, seed) pair gives the same bits in any batch.  The whole of sfc is one
    tensor: B S P doubles; fc_surrogate_test walks a large batch in chunks."""
    name = "surrogate_fc"
    x, single, B, N, L = _series(name, x)
    arr, scalar = _args.seeds(name, seeds)
    if scalar or len(arr) < 2:
        raise ValueError(f"{name}: seeds must be a sequence of at least 2 ints in [0, 2^64), got {seeds!r}")
    return _args.unbatch(single, _surrogate_fc(x, _args.upload_seeds(arr, x.device), len(arr)))


def _test_args(name, x, surr_number, alpha, seeds, ws_bytes):
    """What fc_surrogate_test refuses, before the device is touched -> (x [L][B][N], single, B, N, S, seeds
    uint64 [S], slab bytes, ws_bytes)."""
    S = _args.integer(name, f"surr_number = {surr_number!r}, must be an int of at least 2", surr_number, 2)
    _args.real(name, f"alpha = {alpha!r}, must lie in (0, 1)", alpha, lambda a: 0 < a < 1)
    what = f"seeds must be a sequence of surr_number = {S} ints in [0, 2^64), got {seeds!r}"
    arr = _args.seed_list(name, what, seeds, S, first=1)        # None: 1 .. S, the reference's np.random.seed(i + 1)
    x, single, B, N, L = _series(name, x)
    slab = surrogate_slab_bytes(N, S)
    what = f"ws_bytes = {ws_bytes!r}, needs at least one simulation's slab of 8 S P = {slab} bytes"
    return x, single, B, N, S, arr, slab, _args.slot_ws_bytes(name, what, ws_bytes, slab, B * slab, SURROGATE_WS_CAP)


def fc_surrogate_test(x, surr_number=50, alpha=0.05, seeds=None, want_stats=False, ws_bytes=None):
    """The reference's probabilistic_thresholding on the device: x [L][N] or time-major [L][B][N] fp64
    device tensor, L even, 4 <= L <= 4096, 2 <= N <= 96 -> (fc_adj, p_adj), [B][N][N] or [N][N]:
    p_adj the Benjamini-Hochberg adjusted upper-tail p-values of the FC against a normal law fitted per
    pair to the FC of surr_number surrogates, fc_adj = fc (p_adj < alpha); both symmetric with a zero
    diagonal.  seeds: one per surrogate, 1 .. surr_number by default as the reference's
    np.random.seed(i + 1); the phases are the engine's, not numpy's (include/wcsde.h).
    want_stats=True adds a dict of "mu", "sd", "p", each [B][P]: the pairs' surrogate mean, population
    deviation and unadjusted p.

    A simulation with a constant or non-finite column, or a pair whose surrogate values all coincide,
    has NaN throughout its fc_adj and p_adj; the others are not affected.

    ws_bytes caps the surrogate FCs held at a time (S P doubles a simulation; a 20,000-simulation sweep
    at S = 50, N = 90 would need 32 GB): the batch is walked in chunks of ws_bytes / slab simulations.
    None: 1 GiB, or one slab where that is more.  Less than one slab (surrogate_slab_bytes) is refused.
    The result is the same bits for every cap."""
    x, single, B, N, S, arr, slab, ws_bytes = _test_args("fc_surrogate_test", x, surr_number, alpha, seeds, ws_bytes)
    dev, P = x.device, N * (N - 1) // 2
    per = min(B, ws_bytes // slab)
    seeds_dev = _args.upload_seeds(arr, dev)
    fc_adj = torch.empty((B, N, N), dtype=torch.float64, device=dev)
    p_adj = torch.empty((B, N, N), dtype=torch.float64, device=dev)
    stats = {k: torch.empty((B, P), dtype=torch.float64, device=dev) for k in ("mu", "sd", "p")} if want_stats else None
    for b0 in range(0, B, per):
        nb = min(per, B - b0)
        xc = x if nb == B else x[:, b0:b0 + nb].contiguous()
        sfc = _surrogate_fc(xc, seeds_dev, S)
        fc = _fc(xc)
        opt = [_lib.ptr(stats[k][b0:b0 + nb]) if want_stats else None for k in ("mu", "sd", "p")]
        _lib.check(_lib.lib().wc_surrogate_test(nb, N, S, _lib.ptr(fc), _lib.ptr(sfc), float(alpha),
                                                _lib.ptr(p_adj[b0:b0 + nb]), _lib.ptr(fc_adj[b0:b0 + nb]), *opt,
                                                _lib.stream_handle()), "wc_surrogate_test")
    res = (fc_adj, p_adj) + ((stats,) if want_stats else ())
    return _args.unbatch(single, res)

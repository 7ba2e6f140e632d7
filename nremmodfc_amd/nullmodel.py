"""Degree- and strength-preserving null models on the device (wc_nullmodel.hip): the reference's
randmio_und_signed, null_model_und_sign and participation_coef_norm for a batch.  With
partition.graph_consensus a stack of thresholded FC matrices goes from matrix to consensus partition
to the participation coefficient normalised against its own null models (Pedersen et al. 2020) on the
device.

Device tensors in and out; nullmodel_np holds the numpy facades that graph_utils re-exports.
"""
import numpy as np
import torch

from . import _args, _lib, sigchain

NULL_MODEL_MIN_N = 4        # a rewiring takes four distinct nodes
NULL_MODEL_SLOTS = 4096     # default workspace: a slot for each run, at most this many (150 MB at N = 96)
NULL_MODEL_MAX_PERIOD = 64  # wc_graph_null_model's period
NEGATIVE_MODES = ("reference", "bct")   # wc_graph_null_model's neg_mode 0, 1
PARTICIPATION_NORM_BYTES = 1 << 28      # participation_norm: null models alive at a time


def null_model_slot_bytes(N):
    """One workgroup's slot of the workspace of wc_graph_rewire and wc_graph_null_model: the sorted
    weights of both signs, N (N - 1) / 2 fp64."""
    return 4 * N * (N - 1)


def _stack(name, w):
    w, single, B, N = sigchain._graph_stack(name, w)
    if N < NULL_MODEL_MIN_N:
        raise ValueError(f"{name}: N = {N}, a rewiring takes four distinct nodes: needs N >= {NULL_MODEL_MIN_N}")
    return w, single, B, N


def _swaps(name, bin_swaps, N):
    bin_swaps = _args.integer(name, f"bin_swaps = {bin_swaps!r}, must be an int >= 0", bin_swaps, 0)
    attempts = int(np.round(N / 2)) + 1
    if bin_swaps * (N * (N - 1) // 2) * attempts >= 1 << 31:
        raise ValueError(f"{name}: bin_swaps = {bin_swaps}: its iterations times {attempts} attempts reach 2^31")
    return bin_swaps


def _ws_bytes(name, ws_bytes, N, runs):
    slot = null_model_slot_bytes(N)
    return _args.slot_ws_bytes(name, f"ws_bytes = {ws_bytes!r}, needs at least one slot of 4 N (N - 1) = {slot} bytes",
                               ws_bytes, slot, runs * slot, NULL_MODEL_SLOTS * slot)


def period_of(name, wei_freq):
    """round(1 / wei_freq) as the reference takes it (np.round; graph_utils.py:2297), 0 for wei_freq 0."""
    _args.real(name, f"wei_freq = {wei_freq!r}, must be a number in [0, 1]", wei_freq, lambda f: 0 <= f <= 1)
    if wei_freq == 0:
        return 0
    period = int(np.round(1 / wei_freq))
    if period > NULL_MODEL_MAX_PERIOD:
        raise ValueError(f"{name}: wei_freq = {wei_freq!r} is a period of {period} > {NULL_MODEL_MAX_PERIOD}; "
                         "0 sorts once")
    return period


def graph_rewire(w, bin_swaps=5, seeds=0, want_info=False, ws_bytes=None):
    """Sign-preserving rewiring on the device (wc_graph_rewire; the reference's randmio_und_signed):
    w [B][N][N] or [N][N] fp64 device tensor, exactly symmetric, 4 <= N <= 96 -> wr [B][R][N][N], the
    matrix after bin_swaps N (N - 1) / 2 iterations, every node keeping its number of positive and of
    negative edges; the diagonal is cleared.  seeds is an int or a sequence of R ints; an int gives no R
    axis, as an [N][N] input gives no batch axis.  Every (matrix, seed) pair is an independent run in
    one launch.  The nodes an attempt takes are the engine's Philox stream (include/wcsde.h), not
    numpy's: a seed gives the reference's algorithm under those draws, the same bits in every call and
    every batch.

    want_info=True adds info int32 [B][R][3]: effective rewirings, draws consumed, status.  A matrix
    with a NaN or inf (status 3) or that is not symmetric (status 2) has wr NaN and 0 rewirings.
    ws_bytes as graph_null_model's."""
    name = "graph_rewire"
    seed_arr, scalar = _args.seeds(name, seeds)
    w, single, B, N = _stack(name, w)
    bin_swaps = _swaps(name, bin_swaps, N)
    R = len(seed_arr)
    ws_bytes = _ws_bytes(name, ws_bytes, N, B * R)
    dev = w.device
    ws, seeds_dev = _args.workspace(ws_bytes, dev), _args.upload_seeds(seed_arr, dev)
    wr = torch.empty((B, R, N, N), dtype=torch.float64, device=dev)
    info = torch.empty((B, R, 3), dtype=torch.int32, device=dev) if want_info else None
    _lib.check(_lib.lib().wc_graph_rewire(B, R, N, _lib.ptr(w), bin_swaps, _lib.ptr(seeds_dev), _lib.ptr(wr),
                                          _lib.ptr(info), _lib.ptr(ws), ws_bytes, _lib.stream_handle()),
               "wc_graph_rewire")
    res = _args.unrun(scalar, single, (wr, info) if want_info else (wr,))
    return res if want_info else res[0]


def graph_null_model(w, seeds=0, bin_swaps=5, wei_freq=0.1, negative="bct", want_stats=False, ws_bytes=None):
    """Null models that keep every node's degrees and, approximately, its strengths, per sign, on the
    device (wc_graph_null_model; the reference's null_model_und_sign, Rubinov & Sporns 2011): w
    [B][N][N] or [N][N] fp64 device tensor, exactly symmetric, 4 <= N <= 96 -> w0 [B][R][N][N].  seeds
    is an int or a sequence of R ints; an int gives no R axis, as an [N][N] input gives no batch axis.
    The pattern is rewired as graph_rewire does (not at all where every off-diagonal entry is
    positive); then per sign the weights are given to the rewired edges in the order of the expected
    products of strengths, which are re-sorted every round(1 / wei_freq) weights (wei_freq 0: sorted
    once; the period may not pass 64).

    negative="bct" is the definition (BCT's null_model_und_sign.m): the negative weights are dealt by
    magnitude and stay negative.  negative="reference" is the reference's Python as written: its
    negative half sorts and sums w instead of -w and writes the result with the wrong sign, so every
    negative weight of w comes back POSITIVE and the negative strengths are lost; on a non-negative
    matrix the two agree.  The random choices are the engine's Philox stream (include/wcsde.h).

    want_stats=True returns (w0, r, info): r [B][R][2], the correlation of the positive and of the
    negative strengths of w and w0 (NaN for a constant sequence), and info int32 [B][R][3]: effective
    rewirings, draws consumed, status.  Status 3, a NaN or inf in the matrix, and 2, not symmetric,
    give NaN in w0 and r for all runs of that matrix; status 1, a strength that reaches exactly 0 where
    the reference would divide by it, gives NaN in w0 and r of that run.

    ws_bytes: the sorted weights of a run lie in global memory, in one slot of 4 N (N - 1) bytes per
    workgroup; the launch has min(B R, ws_bytes / slot) workgroups, which stride over the runs.  None
    takes a slot per run, at most 4096.  The result does not depend on it, bit for bit."""
    name = "graph_null_model"
    if not isinstance(negative, str) or negative not in NEGATIVE_MODES:
        raise ValueError(f"{name}: negative = {negative!r}, must be one of {list(NEGATIVE_MODES)}")
    period = period_of(name, wei_freq)
    seed_arr, scalar = _args.seeds(name, seeds)
    w, single, B, N = _stack(name, w)
    bin_swaps = _swaps(name, bin_swaps, N)
    R = len(seed_arr)
    ws_bytes = _ws_bytes(name, ws_bytes, N, B * R)
    dev = w.device
    ws, seeds_dev = _args.workspace(ws_bytes, dev), _args.upload_seeds(seed_arr, dev)
    w0 = torch.empty((B, R, N, N), dtype=torch.float64, device=dev)
    r = torch.empty((B, R, 2), dtype=torch.float64, device=dev) if want_stats else None
    info = torch.empty((B, R, 3), dtype=torch.int32, device=dev) if want_stats else None
    _lib.check(_lib.lib().wc_graph_null_model(B, R, N, _lib.ptr(w), bin_swaps, period, NEGATIVE_MODES.index(negative),
                                              _lib.ptr(seeds_dev), _lib.ptr(w0), _lib.ptr(r), _lib.ptr(info),
                                              _lib.ptr(ws), ws_bytes, _lib.stream_handle()),
               "wc_graph_null_model")
    res = _args.unrun(scalar, single, (w0, r, info) if want_stats else (w0,))
    return res if want_stats else res[0]


def _module_strengths(x, onehot):
    """x [B][...][N][N], onehot [B][N][K] bool -> [B][...][N][K]: row sums over the members of each
    module, by elementwise operations alone (the same bits for any leading shape)."""
    extra = x.dim() - 3
    cols = []
    for m in range(onehot.shape[2]):
        mask = onehot[:, :, m].to(x.dtype).reshape(onehot.shape[0], *([1] * extra), 1, onehot.shape[1])
        cols.append(sigchain._halving_sum(x * mask))
    return torch.stack(cols, dim=-1)


def participation_norm(w, ci, reps=100, seeds=None, bin_swaps=5, wei_freq=0.1, negative="bct",
                       max_bytes=PARTICIPATION_NORM_BYTES):
    """The participation coefficient normalised against null models (the reference's
    participation_coef_norm, :2341-2393; Pedersen et al. 2020) on the device: w [B][N][N] or [N][N]
    fp64 device tensor, ci integer labels [N] or [B][N] (any integers, a tensor or an array) ->
    (mean, std), each [B][N] or [N].  For each of reps null models w0 of a matrix (graph_null_model,
    seeds 0 .. reps-1 by default, the reference's np.random.seed(rand)),
        Kc2_i = sum_m ((sum_{j in m} w_ij - sum_{j in m} w0_ij) / Ko_i)^2,  Ko_i = sum_j w_ij,
        P_i = 1 - sqrt(Kc2_i / 2), 0 where Ko_i == 0 and 0 where it would be negative,
    and the result is the mean and the population standard deviation of P over the reps.  w enters
    with its own diagonal, the null models have none.

    The null models are made in chunks of reps, so that no more than max_bytes of w0 is alive (one rep
    of every matrix at least); every sum is taken in an order that the chunking does not change, so
    the result is the same bits for any max_bytes.  A matrix of which any run has a non-zero status
    (graph_null_model) has NaN in its rows of mean and std; one flag per matrix stays on the device."""
    name = "participation_norm"
    reps = _args.integer(name, f"reps = {reps!r}, must be a positive int", reps, 1)
    max_bytes = _args.integer(name, f"max_bytes = {max_bytes!r}, must be a positive int", max_bytes, 1)
    base = _args.seed_list(name, f"seeds must be a sequence of length reps = {reps}, or None", seeds, reps)
    if not isinstance(negative, str) or negative not in NEGATIVE_MODES:
        raise ValueError(f"{name}: negative = {negative!r}, must be one of {list(NEGATIVE_MODES)}")
    period_of(name, wei_freq)
    w, single, B, N = _stack(name, w)
    _swaps(name, bin_swaps, N)
    dev = w.device
    lab = sigchain._louvain_labels(name, ci, B, N, dev).long()                 # [B][N] in [0, N)
    K = int(lab.max()) + 1                                                     # one readback
    onehot = lab[:, :, None] == torch.arange(K, device=dev)[None, None, :]     # [B][N][K]
    w = w.reshape(B, N, N)
    ko = sigchain._halving_sum(w)                                              # [B][N]
    km = _module_strengths(w, onehot)                                          # [B][N][K]
    chunk = max(1, min(reps, max_bytes // (8 * B * N * N)))
    p_all = torch.empty((B, reps, N), dtype=torch.float64, device=dev)
    bad = torch.zeros((B,), dtype=torch.bool, device=dev)
    for r0 in range(0, reps, chunk):
        run_seeds = [int(s) for s in base[r0:r0 + chunk]]
        w0, _, info = graph_null_model(w, seeds=run_seeds, bin_swaps=bin_swaps, wei_freq=wei_freq, negative=negative,
                                       want_stats=True)
        km0 = _module_strengths(w0, onehot)                                    # [B][r][N][K]
        kc2 = sigchain._halving_sum(((km[:, None] - km0) / ko[:, None, :, None]) ** 2)
        p = 1.0 - torch.sqrt(0.5 * kc2)
        p = torch.where(ko[:, None, :] == 0, torch.zeros_like(p), p)
        p_all[:, r0:r0 + chunk] = torch.where(p < 0, torch.zeros_like(p), p)
        bad |= (info[:, :, 2] != 0).any(dim=1)
        del w0, km0
    pt = p_all.transpose(1, 2)                                                 # [B][N][reps]
    mean = sigchain._halving_sum(pt) / reps
    std = torch.sqrt(sigchain._halving_sum((pt - mean[:, :, None]) ** 2) / reps)
    nan = torch.full_like(mean, float("nan"))
    mean = torch.where(bad[:, None], nan, mean)
    std = torch.where(bad[:, None], nan, std)
    return _args.unbatch(single, (mean, std))

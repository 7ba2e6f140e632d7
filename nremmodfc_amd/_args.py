"""What the wrappers of sigchain, utils and graph_utils do to their arguments before and after a library
call, once: the tensor gate, the [B] axis a single matrix or series lacks, measure names, workspaces.
Plain functions; every message is the caller's own sentence, passed in.
"""
import torch


def tensor(name, what, t, dtype, dims=None, last=None, shapes=None, device=None):
    """The gate: t is a tensor of dtype, with one of `dims` dimensions, a trailing axis of `last`, one of
    the `shapes` and on `device`, as far as each is given; else TypeError(f"{name}: {what}").  Returns t."""
    ok = isinstance(t, torch.Tensor) and t.dtype == dtype and (dims is None or t.dim() in dims)
    ok = ok and (last is None or t.shape[-1] == last) and (shapes is None or tuple(t.shape) in shapes)
    if not ok or (device is not None and t.device != device):
        raise TypeError(f"{name}: {what}")
    return t


def stack(name, what, t, dtype=torch.float64, ndim=3, batch=0, last=None, square=False):
    """(t contiguous, single, B, N) of a tensor with `ndim` dimensions, or with ndim - 1 where the batch
    axis (`batch`, counted in the full shape) is left out: single, B = 1.  [B][N][N] | [N][N] is the default
    (square=True: both N equal); batch=1 is the time-major [M][B][N] | [M][C]; last=2 the phasors
    [M][B][N][2] | [M][C][2], whose N is the axis before.  The gate's TypeError where t is none of these."""
    tensor(name, what, t, dtype, (ndim - 1, ndim), last)
    if square and t.shape[-1] != t.shape[-2]:
        raise TypeError(f"{name}: {what}")
    single = t.dim() == ndim - 1
    return t.contiguous(), single, (1 if single else t.shape[batch]), t.shape[-1 if last is None else -2]


def unbatch(single, value):
    """value without its leading [B] axis where single: a tensor, or a tuple or dict of them (None stays)."""
    if not single or value is None:
        return value
    if isinstance(value, dict):
        return {k: unbatch(single, v) for k, v in value.items()}
    if isinstance(value, (tuple, list)):
        return tuple(unbatch(single, v) for v in value)
    return value[0]


def names(name, asked, known, noun="measure"):
    """The names asked for, a string or a sequence, as a tuple of known ones, each once, not empty."""
    got = (asked,) if isinstance(asked, str) else tuple(asked)
    for m in got:
        if m not in known:
            raise ValueError(f"{name}: unknown {noun} {m!r}, must be one of {list(known)}")
    if not got:
        raise ValueError(f"{name}: no {noun} asked for, choose from {list(known)}")
    return tuple(dict.fromkeys(got))


def ws_default(need, want, cap):
    """The default ws_bytes: what the whole input wants, at most cap, never below the minimum."""
    return max(need, min(want, cap))


def workspace(nbytes, device):
    """An fp64 device buffer of at least nbytes, never empty (the library refuses a NULL workspace)."""
    return torch.empty(max((nbytes + 7) // 8, 1), dtype=torch.float64, device=device)

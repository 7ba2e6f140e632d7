"""What the wrappers do to their arguments before and after a library call, once: the tensor and number
gates, the [B] axis a single matrix or series lacks, measure names, workspaces, a seeded run's seeds and
[R] axis.  Plain functions; every message is the caller's own sentence, passed in.
"""
import numpy as np
import torch


def tensor(name, what, t, dtype, dims=None, last=None, shapes=None, device=None):
    """The gate: t is a tensor of dtype, with one of `dims` dimensions, a trailing axis of `last`, one of
    the `shapes` and on `device`, as far as each is given; else TypeError(f"{name}: {what}").  Returns t."""
    ok = isinstance(t, torch.Tensor) and t.dtype == dtype and (dims is None or t.dim() in dims)
    ok = ok and (last is None or t.shape[-1] == last) and (shapes is None or tuple(t.shape) in shapes)
    if not ok or (device is not None and t.device != device):
        raise TypeError(f"{name}: {what}")
    return t


def integer(name, what, x, lo=None):
    """int(x) of a Python or numpy integer, no bool, at least lo where given; else ValueError(f"{name}: {what}")."""
    if isinstance(x, bool) or not isinstance(x, (int, np.integer)) or (lo is not None and x < lo):
        raise ValueError(f"{name}: {what}")
    return int(x)


def real(name, what, x, ok=None):
    """x, a Python or numpy integer or float, no bool, with ok(x) where given; else ValueError(f"{name}: {what}")."""
    if isinstance(x, bool) or not isinstance(x, (int, float, np.integer, np.floating)) or not (ok is None or ok(x)):
        raise ValueError(f"{name}: {what}")
    return x


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


def slot_ws_bytes(name, what, ws_bytes, slot, want, cap):
    """ws_bytes of a workspace of slots (or slabs): None is ws_default, else an int of at least one slot."""
    return ws_default(slot, want, cap) if ws_bytes is None else integer(name, what, ws_bytes, slot)


def seeds(name, given):
    """(host uint64 array [R], scalar) of an int or a non-empty sequence of ints in [0, 2^64)."""
    scalar = isinstance(given, (int, np.integer)) and not isinstance(given, bool)
    vals = [given] if scalar else (list(given) if isinstance(given, (list, tuple, range, np.ndarray)) else None)
    if not vals or any(isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not 0 <= int(v) < 1 << 64
                       for v in vals):
        raise ValueError(f"{name}: seeds must be an int or a non-empty sequence of ints in [0, 2^64), got {given!r}")
    return np.array([int(v) for v in vals], dtype=np.uint64), scalar


def seed_list(name, what, given, count, first=0):
    """Host uint64 array of count seeds, first .. first + count - 1 for None; else ValueError(f"{name}: {what}")."""
    arr, scalar = seeds(name, range(first, first + count) if given is None else given)
    if scalar or len(arr) != count:
        raise ValueError(f"{name}: {what}")
    return arr


def upload_seeds(arr, device):
    """The uint64 seeds on the device, as the int64 tensor of the same bits (torch has no uint64 arithmetic)."""
    return torch.from_numpy(arr.view(np.int64)).to(device)


def unrun(scalar, single, res):
    """A tuple of [B][R]... tensors without the R axis for a scalar seed and without the B axis where single."""
    return unbatch(single, tuple(t[:, 0] for t in res) if scalar else res)

"""numpy facades of nullmodel.graph_rewire, graph_null_model and participation_norm with the reference's
signatures (graph_utils.py:2165-2217, :2219-2338, :2341-2393) plus seed=None; graph_utils imports them
by name, so graph_utils.randmio_und_signed, null_model_und_sign and participation_coef_norm are
drop-ins.  torch and the device modules are imported on first use."""
import os

import numpy as np

NULL_MODEL_MIN_N, NULL_MODEL_MAX_N = 4, 96


def _matrix(name, W):
    a = np.ascontiguousarray(W, dtype=np.float64)
    if a.ndim != 2 or a.shape[0] != a.shape[1]:
        raise ValueError(f"{name}: needs an N x N matrix, got shape {a.shape}")
    N = a.shape[0]
    if N < NULL_MODEL_MIN_N or N > NULL_MODEL_MAX_N:
        raise ValueError(f"{name}: N = {N}, the device kernel takes {NULL_MODEL_MIN_N} <= N <= {NULL_MODEL_MAX_N}")
    return a


def _seed(seed):
    return int.from_bytes(os.urandom(8), "little") if seed is None else int(seed)


def _device(fn, a, **kw):
    import torch

    from . import nullmodel
    out = getattr(nullmodel, fn)(torch.from_numpy(a).cuda(), **kw)
    return tuple(t.cpu().numpy() for t in out)


def _refused(name, a, status):
    if status == 3:
        raise ValueError(f"{name}: the matrix holds NaN or inf")
    if status == 2:
        raise TypeError("Input must be undirected")
    if status == 1:
        raise ZeroDivisionError(f"{name}: a strength reached exactly 0 where the reference divides by it")


def randmio_und_signed(R, itr, seed=None):
    """(R, eff): the matrix R rewired with every node keeping its numbers of positive and of negative
    edges, itr the rewirings per edge, and the number of rewirings made (graph_utils.py:2165-2217).
    seed None draws one from os.urandom.  The diagonal comes back as given.  The nodes of an attempt
    are the engine's Philox stream (nullmodel.graph_rewire), not numpy's.  The device works on
    symmetric matrices: an asymmetric R raises TypeError, a non-finite one ValueError."""
    a = _matrix("randmio_und_signed", R)
    if isinstance(itr, bool) or int(itr) != itr or itr < 0:
        raise ValueError(f"randmio_und_signed: itr = {itr!r}, must be an int >= 0")
    wr, info = _device("graph_rewire", a, bin_swaps=int(itr), seeds=_seed(seed), want_info=True)
    _refused("randmio_und_signed", a, int(info[2]))
    np.fill_diagonal(wr, np.diagonal(a))
    return wr, int(info[0])


def null_model_und_sign(W, bin_swaps=5, wei_freq=.1, seed=None):
    """(W0, (rpos_in, rpos_out, rneg_in, rneg_out)): a random matrix with the degrees and, nearly, the
    strengths of W, per sign, and the correlations of the strength sequences (graph_utils.py:2219-2338);
    the in and out values coincide, W being symmetric.  seed None draws one from os.urandom.  This is
    the reference as written (nullmodel.graph_null_model with negative="reference"): on a matrix with
    negative weights they come back positive and rneg is NaN; negative="bct" there gives the
    definition.  Raises TypeError("Input must be undirected") for an asymmetric W, as the reference."""
    a = _matrix("null_model_und_sign", W)
    if not np.all(a == a.T) and np.isfinite(a).all():
        raise TypeError("Input must be undirected")
    w0, r, info = _device("graph_null_model", a, seeds=_seed(seed), bin_swaps=bin_swaps, wei_freq=wei_freq,
                          negative="reference", want_stats=True)
    _refused("null_model_und_sign", a, int(info[2]))
    return w0, (float(r[0]), float(r[0]), float(r[1]), float(r[1]))


def participation_coef_norm(W, ci, degree='undirected', BA_iters=100):
    """(P_mean, P_std): the participation coefficient of every node for the partition ci against
    BA_iters null models of W with seeds 0 .. BA_iters-1, its mean and population standard deviation
    over them (graph_utils.py:2341-2393; Pedersen et al. 2020).  Labels as given, any integers.  The
    null models are null_model_und_sign's, so W must be symmetric and degree changes nothing ('in'
    transposes W, as the reference).  The reference's print of every iteration is left out."""
    if degree not in ("undirected", "in", "out"):
        raise ValueError(f"participation_coef_norm: degree {degree!r}, must be 'undirected', 'in' or 'out'")
    a = _matrix("participation_coef_norm", W)
    if degree == 'in':
        a = np.ascontiguousarray(a.T)
    if np.isfinite(a).all() and not np.all(a == a.T):
        raise TypeError("Input must be undirected")
    lab = np.asarray(ci)
    if lab.shape != (a.shape[0],):
        raise ValueError(f"participation_coef_norm: ci needs one label per node, got shape {lab.shape}")
    lab = np.unique(lab, return_inverse=True)[1].reshape(-1).astype(np.int64)
    mean, std = _device("participation_norm", a, ci=lab, reps=int(BA_iters), negative="reference")
    if np.isnan(mean).any():
        raise ValueError("participation_coef_norm: a null model was refused (NaN or inf in W, or a strength "
                         "that reached exactly 0)")
    return mean, std

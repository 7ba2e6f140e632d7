"""numpy facades of hubs.graph_rich_club, graph_assortativity and graph_score with the reference's
signatures (graph_utils.py:2396-2609, :1808-1926); graph_utils imports them by name, so
graph_utils.rich_club_wu, rich_club_wd, rich_club_bu, rich_club_bd, assortativity_wei, assortativity_bin
and score_wu are drop-ins.  As the other facades they also take a [B, N, N] stack, one launch for all
of it.  torch and the device modules are imported on first use."""
import numpy as np


def _device(fn, a, *args, **kw):
    import torch

    from . import hubs
    out = getattr(hubs, fn)(torch.from_numpy(a).cuda(), *args, **kw)
    if isinstance(out, dict):
        return {k: t.cpu().numpy() for k, t in out.items()}
    return tuple(t.cpu().numpy() for t in out)


def _matrices(name, W):
    from .graph_utils import _matrices
    return _matrices(name, W, False)


def _curves(name, CIJ, klevel, directed, kind, keys):
    """The curves `keys` of every matrix, cut at klevel or at the matrix's own largest degree, as float
    arrays: one tuple for a matrix, for a stack a list of them (klevel None: each its own length)."""
    a = _matrices(name, CIJ)
    if klevel is not None and (isinstance(klevel, bool) or not isinstance(klevel, (int, np.integer)) or klevel < 1):
        raise ValueError(f"{name}: klevel = {klevel!r}, must be None or an int >= 1")
    kmax = (2 if directed else 1) * a.shape[-1]
    got = _device("graph_rich_club", a, kinds=(kind,), klevel=None if klevel is None else min(int(klevel), kmax),
                  directed=directed)
    maxdeg = np.atleast_1d(got["maxdeg"])
    if (maxdeg < 0).any():
        raise ValueError(f"{name}: the matrix holds NaN or inf")
    rows = []
    for b, m in enumerate(maxdeg):
        n = int(m) if klevel is None else int(klevel)
        row = []
        for key in keys:
            v = np.asarray(got[key] if a.ndim == 2 else got[key][b], dtype=np.float64)[:n]
            # past the largest possible degree nothing is kept: 0 nodes, 0 edges, 0 / 0
            pad = np.full(n - len(v), 0.0 if key in ("nk", "ek") else np.nan)
            row.append(np.concatenate([v, pad]))
        rows.append(tuple(row))
    if a.ndim == 2:
        return rows[0]
    return rows if klevel is None else tuple(np.stack(c) for c in zip(*rows))


def rich_club_wu(CIJ, klevel=None):
    """Rw: the weighted rich-club coefficient for the degrees 1 .. klevel, by default up to the largest
    degree (graph_utils.py:2528-2570); NaN at a level below every node's degree, as in the reference.
    A [B, N, N] stack gives [B, klevel], or with klevel None a list of B arrays."""
    got = _curves("rich_club_wu", CIJ, klevel, False, "weighted", ("rw",))
    return [r[0] for r in got] if isinstance(got, list) else got[0]


def rich_club_wd(CIJ, klevel=None):
    """Rw of a directed matrix, the degree being in plus out (graph_utils.py:2482-2525)."""
    got = _curves("rich_club_wd", CIJ, klevel, True, "weighted", ("rw",))
    return [r[0] for r in got] if isinstance(got, list) else got[0]


def rich_club_bu(CIJ, klevel=None):
    """(R, Nk, Ek): the rich-club coefficient, the number of nodes of degree > k and the sum of their
    entries, for k = 1 .. klevel, by default up to the largest degree (graph_utils.py:2440-2479).  As in
    the reference CIJ is not binarised for Ek."""
    return _curves("rich_club_bu", CIJ, klevel, False, "binary", ("rb", "nk", "ek"))


def rich_club_bd(CIJ, klevel=None):
    """(R, Nk, Ek) of a directed matrix, the degree being in plus out (graph_utils.py:2396-2437)."""
    return _curves("rich_club_bd", CIJ, klevel, True, "binary", ("rb", "nk", "ek"))


def _assortativity(name, CIJ, flag, which):
    if isinstance(flag, bool) or flag not in (0, 1, 2, 3, 4):
        raise ValueError('Flag must be 0-4')
    a = _matrices(name, CIJ)
    r = _device("graph_assortativity", a, flag=int(flag))[which]
    return float(r) if a.ndim == 2 else r


def assortativity_wei(CIJ, flag=0):
    """The correlation of the strengths at the two ends of an edge (graph_utils.py:1869-1926): flag 0
    undirected, 1 out/in, 2 in/out, 3 out/out, and 4 in/out as well: the reference reads ist[i], ost[j]
    for flag 4 although its docstring says in/in, and this gives what it gives."""
    return _assortativity("assortativity_wei", CIJ, flag, 0)


def assortativity_bin(CIJ, flag=0):
    """The correlation of the degrees at the two ends of an edge (graph_utils.py:1808-1866): flag 0
    undirected, 1 out/in, 2 in/out, 3 out/out, 4 in/in.  NaN for a regular graph, as in the reference."""
    return _assortativity("assortativity_bin", CIJ, flag, 1)


def score_wu(CIJ, s):
    """(CIJscore, sn): the s-core, the largest subnetwork of nodes with a strength of at least s, as
    the matrix with every other node's row and column cleared, and its size (graph_utils.py:2573-2609).
    A [B, N, N] stack gives [B, N, N] and [B]."""
    a = _matrices("score_wu", CIJ)
    if isinstance(s, bool) or not isinstance(s, (int, float, np.integer, np.floating)):
        raise ValueError(f"score_wu: s = {s!r}, must be a number")
    member, sn, _, core = _device("graph_score", a, float(s), want_matrix=True)
    if (sn < 0).any():
        raise ValueError("score_wu: the matrix holds NaN or inf")
    return (core, int(sn)) if a.ndim == 2 else (core, sn.astype(np.int64))

"""Hub organisation on the device (wc_hubs.hip): the reference's rich-club curves, assortativity
coefficients and s-core for a batch, and the rich club normalised against its own null models
(nullmodel.graph_null_model, graph_rewire), the curves of all B x reps null models taken where the null
models lie.

Device tensors in and out; hubs_np holds the numpy facades that graph_utils re-exports.
"""
import numpy as np
import torch

from . import _args, _lib, nullmodel, sigchain

RICH_CLUB_KINDS = ("weighted", "binary")
RICH_CLUB_NORM_BYTES = 1 << 28      # rich_club_norm: null models alive at a time


def _levels(name, klevel, N, directed):
    kmax = 2 * N if directed else N
    if klevel is None:
        return kmax
    what = f"klevel = {klevel!r}, must be None or an int in [1, {kmax}] ({'2 N' if directed else 'N'}, the largest degree)"
    klevel = _args.integer(name, what, klevel, 1)
    if klevel > kmax:
        raise ValueError(f"{name}: {what}")
    return klevel


def _rich_club(B, N, w, directed, K, kinds):
    """The library call on w [B][N][N], contiguous: the outputs of the kinds and maxdeg."""
    dev = w.device
    out = {}
    if "weighted" in kinds:
        out["rw"] = torch.empty((B, K), dtype=torch.float64, device=dev)
    if "binary" in kinds:
        out["rb"] = torch.empty((B, K), dtype=torch.float64, device=dev)
        out["nk"] = torch.empty((B, K), dtype=torch.int32, device=dev)
        out["ek"] = torch.empty((B, K), dtype=torch.float64, device=dev)
    out["maxdeg"] = torch.empty((B,), dtype=torch.int32, device=dev)
    p = {k: _lib.ptr(out.get(k)) for k in ("rw", "rb", "nk", "ek", "maxdeg")}
    _lib.check(_lib.lib().wc_graph_rich_club(B, N, _lib.ptr(w), int(directed), K, p["rw"], p["rb"], p["nk"], p["ek"],
                                             p["maxdeg"], _lib.stream_handle()), "wc_graph_rich_club")
    return out


def graph_rich_club(w, kinds=RICH_CLUB_KINDS, klevel=None, directed=False):
    """Rich-club curves of B matrices on the device (wc_graph_rich_club; the reference's rich_club_wu,
    rich_club_wd, rich_club_bu and rich_club_bd): w [B][N][N] or [N][N] fp64 device tensor,
    2 <= N <= 96, no symmetry assumed, the diagonal as given -> a dict of [B][K] tensors ([K] for a
    single matrix) and maxdeg [B] int32.  The degree of a node is the number of non-zeros of its
    column, with directed=True plus those of its row.  klevel=None writes K = N levels (2 N with
    directed) for the degrees 1 .. K, of which the reference returns the first maxdeg; an int writes
    that many.

    kinds "weighted": rw, over the nodes of degree >= l the sum of all entries among them over the sum
    of as many of the largest entries of the whole matrix as there are non-zero ones among them; NaN
    where no node has a smaller degree (the reference's `continue`) and where nothing is kept.
    "binary": rb = ek / (nk (nk - 1)) over the nodes of degree > l, nk int32 their number and ek the
    sum of their entries of w as given (the reference does not binarise).  A matrix with a NaN or inf
    has NaN in rw, rb and ek and -1 in nk and maxdeg.  The same matrix gives the same bits in any
    batch."""
    name = "graph_rich_club"
    kinds = _args.names(name, kinds, RICH_CLUB_KINDS, "kind")
    w, single, B, N = sigchain._graph_stack(name, w)
    K = _levels(name, klevel, N, bool(directed))
    return _args.unbatch(single, _rich_club(B, N, w, bool(directed), K, kinds))


def graph_assortativity(w, flag=0):
    """Assortativity coefficients of B matrices on the device (wc_graph_assortativity; the reference's
    assortativity_wei and assortativity_bin): w [B][N][N] or [N][N] fp64 device tensor, 2 <= N <= 96
    -> (r_wei, r_bin), each [B] or a 0-d tensor: the correlation of the strengths, and of the degrees,
    at the two ends of an edge.  flag 0 takes the edges i < j with w_ij > 0 and the column sums and
    column counts at both ends; flags 1 .. 4 take every w_ij > 0 with out/in, in/out, out/out and in/in
    (in: columns, out: rows).  r_wei with flag 4 is in/out, the same as flag 2: the reference's
    assortativity_wei reads ist[i], ost[j] there although its docstring says in/in, and this does as it
    is written.  A regular graph has r_bin NaN (an exact 0 / 0), a matrix without an edge or with a NaN
    or inf NaN in both."""
    name = "graph_assortativity"
    what = f"flag = {flag!r}, must be 0, 1, 2, 3 or 4"
    if _args.integer(name, what, flag, 0) > 4:
        raise ValueError(f"{name}: {what}")
    w, single, B, N = sigchain._graph_stack(name, w)
    r_wei = torch.empty((B,), dtype=torch.float64, device=w.device)
    r_bin = torch.empty((B,), dtype=torch.float64, device=w.device)
    _lib.check(_lib.lib().wc_graph_assortativity(B, N, _lib.ptr(w), int(flag), _lib.ptr(r_wei), _lib.ptr(r_bin),
                                                 _lib.stream_handle()), "wc_graph_assortativity")
    return _args.unbatch(single, (r_wei, r_bin))


def _score_levels(name, s, B, single, dev):
    """s as a [B][S] fp64 device tensor and whether it came without its S axis."""
    what = f"s must be a number, [S] or [B][S] = [{B}][S] numbers, S >= 1"
    t = None
    if isinstance(s, torch.Tensor):
        if not s.dtype.is_complex and s.dtype != torch.bool:
            t = s.to(device=dev, dtype=torch.float64)
    elif not isinstance(s, (bool, str)):
        try:
            a = np.asarray(s)
            if a.dtype.kind in "iuf":
                t = torch.from_numpy(a.astype(np.float64)).to(dev)
        except (TypeError, ValueError):
            pass
    if t is None or t.dim() > 2 or t.numel() == 0 or (t.dim() == 2 and (single or t.shape[0] != B)):
        raise ValueError(f"{name}: {what}")
    scalar = t.dim() == 0
    if t.dim() < 2:
        t = t.reshape(1, -1).expand(B, -1)
    return t.contiguous(), scalar


def graph_score(w, s, want_matrix=False):
    """s-cores of B matrices on the device (wc_graph_score; the reference's score_wu): w [B][N][N] or
    [N][N] fp64 device tensor, 2 <= N <= 96; s the levels: a number (no S axis in the results), [S]
    for all matrices or [B][S] -> (member int32 [B][S][N], sn int32 [B][S], rounds int32 [B][S]).
    The strengths are the column sums; all nodes with 0 < strength < s are peeled together, their rows
    and columns cleared, until none is left to peel.  member is 1 where the node was not peeled, sn
    the number of nodes with a positive strength at the end, rounds the passes that peeled something.
    Every comparison is the reference's own: a column is added up in row order, as numpy does it.

    want_matrix=True adds the core matrices [B][S][N][N], w with the peeled rows and columns cleared.
    A matrix with a NaN or inf has -1 in member, sn and rounds and a NaN core."""
    name = "graph_score"
    w, single, B, N = sigchain._graph_stack(name, w)
    w = w.reshape(B, N, N)
    lev, scalar = _score_levels(name, s, B, single, w.device)
    S = lev.shape[1]
    if B * S >= 1 << 31:
        raise ValueError(f"{name}: B S = {B * S} cores, needs fewer than 2^31")
    member = torch.empty((B, S, N), dtype=torch.int32, device=w.device)
    sn = torch.empty((B, S), dtype=torch.int32, device=w.device)
    rounds = torch.empty((B, S), dtype=torch.int32, device=w.device)
    _lib.check(_lib.lib().wc_graph_score(B, N, S, _lib.ptr(w), _lib.ptr(lev), _lib.ptr(member), _lib.ptr(sn),
                                         _lib.ptr(rounds), _lib.stream_handle()), "wc_graph_score")
    res = (member, sn, rounds)
    if want_matrix:
        keep = (member[:, :, :, None] == 1) & (member[:, :, None, :] == 1)
        core = torch.where(keep, w[:, None], torch.zeros((), dtype=torch.float64, device=w.device))
        core = torch.where((sn < 0)[:, :, None, None], torch.full_like(core, float("nan")), core)
        res += (core,)
    return _args.unrun(scalar, single, res)


def rich_club_norm(w, kind="weighted", reps=100, seeds=None, bin_swaps=5, wei_freq=0.1, negative="bct",
                   max_bytes=RICH_CLUB_NORM_BYTES):
    """The rich-club curve over its expectation under null models that keep the degrees, on the
    device: w [B][N][N] or [N][N] fp64 device tensor, symmetric, 4 <= N <= 96 -> a dict of [B][N]
    tensors ([N] for a single matrix), level k for the degree k + 1:
        phi        the curve of w: rw of graph_rich_club for kind "weighted", rb of (w != 0) for "binary";
        null_mean, null_std   mean and population standard deviation of the curves of reps null models
                   of the matrix: graph_null_model of w for "weighted" (degrees and, nearly, strengths
                   kept), graph_rewire of (w != 0) for "binary" (degrees kept); seeds 0 .. reps-1 by
                   default; bin_swaps, wei_freq and negative are theirs;
        norm       phi / null_mean;
        p          (1 + the number of null models with a value >= phi) / (1 + reps).
    w enters with its own diagonal, the null models have none.  A level at which phi or any null model
    is NaN has NaN in null_mean, null_std, norm and p.

    The null models are made in chunks of reps, so that no more than max_bytes of them is alive (one rep
    of every matrix at least), and each chunk goes to wc_graph_rich_club as one [B r][N][N] stack where
    it lies; every sum is taken in an order that the chunking does not change, so the result is the
    same bits for any max_bytes.  A matrix of which any run has a non-zero status (not symmetric, a NaN
    or inf, a strength that reaches exactly 0: graph_null_model) has NaN throughout; one flag per
    matrix stays on the device."""
    name = "rich_club_norm"
    if not isinstance(kind, str) or kind not in RICH_CLUB_KINDS:
        raise ValueError(f"{name}: kind = {kind!r}, must be one of {list(RICH_CLUB_KINDS)}")
    reps = _args.integer(name, f"reps = {reps!r}, must be a positive int", reps, 1)
    max_bytes = _args.integer(name, f"max_bytes = {max_bytes!r}, must be a positive int", max_bytes, 1)
    base = _args.seed_list(name, f"seeds must be a sequence of length reps = {reps}, or None", seeds, reps)
    if not isinstance(negative, str) or negative not in nullmodel.NEGATIVE_MODES:
        raise ValueError(f"{name}: negative = {negative!r}, must be one of {list(nullmodel.NEGATIVE_MODES)}")
    nullmodel.period_of(name, wei_freq)
    w, single, B, N = nullmodel._stack(name, w)
    nullmodel._swaps(name, bin_swaps, N)
    dev = w.device
    w = w.reshape(B, N, N)
    key = "rw" if kind == "weighted" else "rb"
    bad = ~torch.isfinite(w).reshape(B, -1).all(dim=1)                          # (NaN != 0) would pass for an edge
    if kind == "binary":
        w = (w != 0).to(torch.float64)
    phi = _rich_club(B, N, w, False, N, (kind,))[key]                           # [B][N]
    chunk = max(1, min(reps, max_bytes // (8 * B * N * N)))
    nulls = torch.empty((B, reps, N), dtype=torch.float64, device=dev)
    for r0 in range(0, reps, chunk):
        run_seeds = [int(s) for s in base[r0:r0 + chunk]]
        if kind == "weighted":
            w0, _, info = nullmodel.graph_null_model(w, seeds=run_seeds, bin_swaps=bin_swaps, wei_freq=wei_freq,
                                                     negative=negative, want_stats=True)
        else:
            w0, info = nullmodel.graph_rewire(w, bin_swaps=bin_swaps, seeds=run_seeds, want_info=True)
        r = len(run_seeds)
        nulls[:, r0:r0 + r] = _rich_club(B * r, N, w0.view(B * r, N, N), False, N, (kind,))[key].view(B, r, N)
        bad |= (info[:, :, 2] != 0).any(dim=1)
        del w0
    nt = nulls.transpose(1, 2)                                                  # [B][N][reps]
    mean = sigchain._halving_sum(nt) / reps
    std = torch.sqrt(sigchain._halving_sum((nt - mean[:, :, None]) ** 2) / reps)
    count = (nt >= phi[:, :, None]).sum(dim=2)                                  # integers: exact in any order
    p = (1.0 + count.to(torch.float64)) / (1.0 + reps)
    nan = torch.full_like(mean, float("nan"))
    void = torch.isnan(phi) | torch.isnan(nt).any(dim=2) | bad[:, None]
    out = {"phi": torch.where(bad[:, None], nan, phi), "null_mean": torch.where(void, nan, mean),
           "null_std": torch.where(void, nan, std), "norm": torch.where(void, nan, phi / mean),
           "p": torch.where(void, nan, p)}
    return _args.unbatch(single, out)

"""Device HMA (wc_hma) vs the reference HMA.py outputs (golden_hma.npz) and vs the
host facade nremmodfc_amd.HMA on random FC-like matrices, odd N included.

Those matrices have hardly a negative entry, no negative eigenvalue and are symmetric.  The second half
of the file puts matrices with structure through both kernels (tests/hma_reference.py: zero_diag,
signed_fc, asym; N = 3 .. 96) against 40-digit arithmetic (tests/golden/golden_hma_hp.npz): clus_num and
the clipped matrix exact, every floating output within the larger of 8 x the host facade's (LAPACK's)
recorded deviation for that case and output and N 2^-52 x the output's largest magnitude.  The Jacobi
stops at an off-diagonal mass of 1e-30 of the total, which puts its errors in LAPACK's order; 8 covers the
differing constants.  Printed as TOL lines; measured on MI355X, worst err / bound (err of that case):

                              hin             hse             hin_node        hse_node        sv
  wc_hma          N <= 5      0.26 (2.8e-17)  0.12 (5.6e-17)  0.50 (1.1e-16)  0.28 (1.7e-15)  0.25 (2.2e-16)
                  N 16 .. 33  0.12 (1.0e-17)  0.06 (1.1e-16)  0.25 (6.3e-17)  0.12 (8.9e-16)  0.06 (3.6e-15)
                  N 64 .. 96  0.10 (1.5e-16)  0.01 (8.9e-16)  0.24 (5.7e-16)  0.32 (1.7e-14)  0.05 (1.4e-14)
  wc_hma_modes    5,33,65,96  0.22 (2.8e-17)  0.50 (2.2e-16)  0.83 (2.8e-16)  0.22 (3.9e-16)  0.25 (8.9e-16)
  node permutation  17, 90    0.18 (8.3e-17)  0.06 (1.1e-16)  0.21 (8.0e-16)  0.15 (1.2e-15)  0.08 (1.8e-15)

With the rotation in its plain form (c g - s h, two-sided update of the 2 x 2 block) wc_hma was beyond the
bound in 135 of 330 figures, worst 2.37 / 1.55 / 3.06 / 2.50 / 1.34: the kernel now rotates in
Rutishauser's form (docs/CHANGELOG.md)."""
import functools
import os

import numpy as np
import pytest
import torch

from nremmodfc_amd import HMA, _lib, datasets, sigchain
from tests import hma_reference as hr
from tests.golden.make_golden import inputs

pytestmark = pytest.mark.gpu
G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "golden_hma.npz")


def _fc_like(rng, B, N, T=298):
    """corrcoef of correlated random series: one large mode plus structure, as simulated FC."""
    out = []
    for _ in range(B):
        common = rng.standard_normal((T, 1))
        mods = rng.standard_normal((T, 4))[:, rng.integers(0, 4, N)]
        x = 0.6 * common + 0.5 * mods + rng.standard_normal((T, N))
        out.append(np.corrcoef(x.T))
    return np.stack(out)


def test_hma_matches_reference_golden(cuda):
    g = np.load(G)
    emps = [datasets.load_empfc(s) for s in ("W", "N1", "N2", "N3")]
    fcs = np.stack(inputs()["fcs"] + emps)
    t = torch.from_numpy(fcs.copy()).to(cuda)
    r = sigchain.hma(t, want_clus_num=True)
    cn = r["clus_num"].cpu().numpy()
    for i in range(len(fcs)):
        np.testing.assert_array_equal(cn[i], g[f"clus_num{i}"])
        np.testing.assert_allclose(r["hin"][i].item(), g[f"hin{i}"], rtol=1e-12)
        np.testing.assert_allclose(r["hse"][i].item(), g[f"hse{i}"], rtol=1e-12)
        np.testing.assert_allclose(r["hin_node"][i].cpu().numpy(), g[f"hin_node{i}"], rtol=1e-10, atol=1e-15)
        np.testing.assert_allclose(r["hse_node"][i].cpu().numpy(), g[f"hse_node{i}"], rtol=1e-10, atol=1e-15)
        np.testing.assert_array_equal(t[i].cpu().numpy(), g[f"clipped{i}"])  # in-place clip (HMA.py:55)


@pytest.mark.parametrize("N,B", [(90, 40), (89, 7), (17, 5), (96, 3), (3, 2)])
def test_hma_matches_host_facade(cuda, N, B):
    rng = np.random.default_rng(N * 100 + B)
    fcs = _fc_like(rng, B, N)
    r = sigchain.hma(torch.from_numpy(fcs.copy()).to(cuda), want_clus_num=True)
    for b in range(B):
        f = fcs[b].copy()
        cn, cs, _ = HMA.Functional_HP(f)
        hin, hse = HMA.Balance(f, cn, cs)
        hin_n, hse_n = HMA.nodal_measures(f, cn, cs)
        np.testing.assert_array_equal(r["clus_num"][b].cpu().numpy(), cn)
        np.testing.assert_allclose(r["hin"][b].item(), hin, rtol=1e-12)
        np.testing.assert_allclose(r["hse"][b].item(), hse, rtol=1e-11)
        np.testing.assert_allclose(r["hin_node"][b].cpu().numpy(), hin_n, rtol=1e-10, atol=1e-15)
        np.testing.assert_allclose(r["hse_node"][b].cpu().numpy(), hse_n, rtol=1e-9, atol=1e-15)
        sv = np.linalg.svd(np.where(fcs[b] < 0, 0, fcs[b]), compute_uv=False)
        np.testing.assert_allclose(r["sv"][b].cpu().numpy(), sv, rtol=1e-11, atol=1e-13)


@pytest.mark.parametrize("N,B", [(97, 3), (150, 2), (301, 2)])
def test_hma_large_n_matches_host_facade(cuda, N, B):
    """N > 96 (HMA.py has no N cap): the device eigensolver + wc_hma_modes vs the host facade
    (the reference's algorithm, numpy SVD)."""
    rng = np.random.default_rng(N * 7 + B)
    fcs = _fc_like(rng, B, N)
    t = torch.from_numpy(fcs.copy()).to(cuda)
    r = sigchain.hma(t, want_clus_num=True)
    for b in range(B):
        f = fcs[b].copy()
        cn, cs, _ = HMA.Functional_HP(f)
        hin, hse = HMA.Balance(f, cn, cs)
        hin_n, hse_n = HMA.nodal_measures(f, cn, cs)
        np.testing.assert_array_equal(r["clus_num"][b].cpu().numpy(), cn)
        np.testing.assert_allclose(r["hin"][b].item(), hin, rtol=1e-11)
        np.testing.assert_allclose(r["hse"][b].item(), hse, rtol=1e-10)
        np.testing.assert_allclose(r["hin_node"][b].cpu().numpy(), hin_n, rtol=1e-9, atol=1e-14)
        np.testing.assert_allclose(r["hse_node"][b].cpu().numpy(), hse_n, rtol=1e-8, atol=1e-14)
        np.testing.assert_array_equal(t[b].cpu().numpy(), f)  # clipped in place, as HMA.py:55


def test_hma_batch_is_order_independent(cuda):
    rng = np.random.default_rng(5)
    fcs = _fc_like(rng, 6, 90)
    a = sigchain.hma(torch.from_numpy(fcs.copy()).to(cuda))
    b = sigchain.hma(torch.from_numpy(fcs[::-1].copy()).to(cuda))
    assert torch.equal(a["hin"], b["hin"].flip(0)) and torch.equal(a["hse_node"], b["hse_node"].flip(0))


# ---------------- against 40-digit arithmetic, on matrices with structure (tests/hma_reference.py) ----------------
KEYS = hr.FLOAT_OUTPUTS + ("clus_num",)


@functools.lru_cache(maxsize=None)
def _hp_cases(N):
    """[(case, input, golden reference)] of the six matrices of size N: built once, read only."""
    golden = hr.load_golden()
    out = []
    for case in hr.cases():
        if case[1] == N:
            F = hr.checked_input(*case, golden[case])
            F.setflags(write=False)
            out.append((case, F, golden[case]))
    return out


def _run(fcs, dev):
    """sigchain.hma of a stack of matrices -> ({key: numpy array}, the clipped matrices)."""
    t = torch.tensor(np.asarray(fcs), device=dev)
    r = sigchain.hma(t, want_clus_num=True)
    return {k: r[k].cpu().numpy() for k in KEYS}, t.cpu().numpy()


def _check_hp(got, b, case, ref, what):
    """Matrix b of a device result against the golden reference of `case`: clus_num exact, every
    floating output within hr.bound(..., 8).  Prints the observed figures as TOL lines and returns the
    outputs beyond their bound (the caller asserts there are none, after every line is out)."""
    N = case[1]
    np.testing.assert_array_equal(got["clus_num"][b], ref["clus_num"], err_msg=f"{what} {hr.key(*case)}")
    over = []
    for name in hr.FLOAT_OUTPUTS:
        err = float(np.abs(got[name][b] - ref[name]).max())
        bnd = hr.bound(ref, name, N, 8)
        print(f"TOL {what} {hr.key(*case)} {name}: err {err:.2e} bound {bnd:.2e} ratio {err / bnd:.2f} "
              f"(host {ref['dev_' + name]:.2e})")
        if not err <= bnd:
            over.append((what, hr.key(*case), name, err, bnd))
    return over


@pytest.mark.parametrize("N", hr.SIZES)
def test_hma_matches_high_precision_golden(cuda, N):
    """wc_hma on negative entries, eigenvalues of both signs and asymmetric inputs."""
    cases = _hp_cases(N)
    got, clipped = _run([F for _, F, _ in cases], cuda)
    over = []
    for b, (case, F, ref) in enumerate(cases):
        np.testing.assert_array_equal(clipped[b], hr.clipped(F))
        over += _check_hp(got, b, case, ref, "wc_hma")
    assert not over, over


@pytest.mark.parametrize("N", [5, 33, 65, 96])
def test_hma_modes_direct_matches_high_precision_golden(cuda, N):
    """wc_hma_modes called directly with numpy's eigh of the golden inputs: negative eigenvalues
    through the |lambda| ranking, and more than 64 candidate labels through the ballot compaction."""
    cases = _hp_cases(N)
    f = np.stack([hr.clipped(F) for _, F, _ in cases])
    lam, V = np.linalg.eigh((f + f.transpose(0, 2, 1)) / 2)
    assert (lam < 0).any() and (lam > 0).any()
    B = len(cases)
    lt = torch.tensor(lam, device=cuda)
    vt = torch.tensor(np.ascontiguousarray(V.transpose(0, 2, 1)), device=cuda)  # row j = eigenvector j
    out = {k: torch.empty(s, dtype=torch.float64, device=cuda)
           for k, s in (("hin", (B,)), ("hse", (B,)), ("hin_node", (B, N)), ("hse_node", (B, N)), ("sv", (B, N)))}
    out["clus_num"] = torch.empty((B, N - 1), dtype=torch.int32, device=cuda)
    _lib.check(_lib.lib().wc_hma_modes(B, N, _lib.ptr(lt), _lib.ptr(vt), _lib.ptr(out["hin"]), _lib.ptr(out["hse"]),
                                       _lib.ptr(out["hin_node"]), _lib.ptr(out["hse_node"]),
                                       _lib.ptr(out["clus_num"]), _lib.ptr(out["sv"]), _lib.stream_handle()),
               "wc_hma_modes")
    got = {k: out[k].cpu().numpy() for k in KEYS}
    over = []
    for b, (case, _, ref) in enumerate(cases):
        over += _check_hp(got, b, case, ref, "wc_hma_modes")
    assert not over, over


@pytest.mark.parametrize("N", [97, 130])
def test_hma_large_n_structured_matches_host_facade(cuda, N):
    """N > 96 through sigchain.hma (device eigensolver + wc_hma_modes) on zero_diag and asym, with
    test_hma_large_n_matches_host_facade's bounds.  There is no 40-digit reference at these sizes; the
    admission condition is checked here in fp64, far above fp64's own resolution."""
    fcs = np.stack([hr.make_input(fam, N, i) for fam in ("zero_diag", "asym") for i in range(2)])
    for F in fcs:
        f = hr.clipped(F)
        lam, V = np.linalg.eigh((f + f.T) / 2)
        order = np.argsort(-np.abs(lam))
        s = np.abs(lam)[order]
        assert (s[:-1] - s[1:]).min() >= hr.MIN_GAP * s[0] and np.abs(V[:, order[1:N - 1]]).min() >= hr.MIN_U
        assert (lam < 0).sum() > N // 3
    got, clipped = _run(fcs, cuda)
    for b, F in enumerate(fcs):
        want = hr.host_facade(F)
        np.testing.assert_array_equal(got["clus_num"][b], want["clus_num"])
        np.testing.assert_allclose(got["hin"][b], want["hin"], rtol=1e-11)
        np.testing.assert_allclose(got["hse"][b], want["hse"], rtol=1e-10)
        np.testing.assert_allclose(got["hin_node"][b], want["hin_node"], rtol=1e-9, atol=1e-14)
        np.testing.assert_allclose(got["hse_node"][b], want["hse_node"], rtol=1e-8, atol=1e-14)
        np.testing.assert_array_equal(clipped[b], want["clipped"])


@pytest.mark.parametrize("N", [5, 17, 64, 96])
def test_hma_of_the_transpose_is_bit_identical(cuda, N):
    """F enters only as (clip(F) + clip(F)^T) / 2: hma(F^T) is hma(F) bit for bit, and its clipped
    matrix the transpose."""
    fcs = np.stack([F for case, F, _ in _hp_cases(N) if case[0] == "asym"])
    assert not (fcs == fcs.transpose(0, 2, 1)).all()
    a, ca = _run(fcs, cuda)
    b, cb = _run(np.ascontiguousarray(fcs.transpose(0, 2, 1)), cuda)
    for k in KEYS:
        np.testing.assert_array_equal(a[k], b[k], err_msg=k)
    np.testing.assert_array_equal(cb, ca.transpose(0, 2, 1))


@pytest.mark.parametrize("k", [-20, 20])
@pytest.mark.parametrize("N", [33, 90])
def test_hma_scales_exactly_with_powers_of_two(cuda, N, k):
    """hma(2^k F): sv scales by 2^k, hin / hse and the nodal values by 4^k, bit for bit (rotation
    angles and the stopping test are ratios); clus_num is unchanged."""
    fcs = np.stack([F for _, F, _ in _hp_cases(N)])
    a, _ = _run(fcs, cuda)
    b, _ = _run(fcs * 2.0 ** k, cuda)
    np.testing.assert_array_equal(b["sv"], a["sv"] * 2.0 ** k)
    for name in ("hin", "hse", "hin_node", "hse_node"):
        np.testing.assert_array_equal(b[name], a[name] * 4.0 ** k, err_msg=name)
    np.testing.assert_array_equal(b["clus_num"], a["clus_num"])


@pytest.mark.parametrize("N", [17, 90])
def test_hma_node_permutation(cuda, N):
    """P F P^T: hin_node / hse_node are permuted, everything else is unchanged, all within the golden
    bounds; clus_num is equal."""
    cases = _hp_cases(N)
    perm = np.random.default_rng(N).permutation(N)
    got, _ = _run([F[np.ix_(perm, perm)] for _, F, _ in cases], cuda)
    over = []
    for b, (case, _, ref) in enumerate(cases):
        pref = dict(ref, hin_node=ref["hin_node"][perm], hse_node=ref["hse_node"][perm])
        over += _check_hp(got, b, case, pref, "permuted")
    assert not over, over


def test_hma_more_workgroups_than_cus(cuda):
    """B = 300 copies of one matrix: 300 identical rows."""
    F = _hp_cases(90)[0][1]
    got, clipped = _run(np.broadcast_to(F, (300, 90, 90)).copy(), cuda)
    for k in KEYS:
        assert (got[k] == got[k][0]).all(), k
    assert (clipped == clipped[0]).all()

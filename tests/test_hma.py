"""nremmodfc_amd.HMA vs the reference HMA.py outputs (tests/golden/golden_hma.npz), no GPU."""
import os

import numpy as np
import pytest

from nremmodfc_amd import HMA, datasets
from tests import hma_reference as hr
from tests.golden.make_golden import inputs

G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "golden_hma.npz")


def test_hma_matches_reference():
    g = np.load(G)
    emps = [datasets.load_empfc(s) for s in ("W", "N1", "N2", "N3")]
    fcs = inputs()["fcs"] + emps
    assert int(g["n"]) == len(fcs)
    for i, fc in enumerate(fcs):
        f = fc.copy()
        cn, cs, h_all = HMA.Functional_HP(f)
        np.testing.assert_array_equal(np.array(cn), g[f"clus_num{i}"])
        np.testing.assert_array_equal(f, g[f"clipped{i}"])  # in-place clip, as HMA.py:55
        hin, hse = HMA.Balance(f, cn, cs)
        hin_n, hse_n = HMA.nodal_measures(f, cn, cs)
        np.testing.assert_allclose(hin, g[f"hin{i}"], rtol=1e-13)
        np.testing.assert_allclose(hse, g[f"hse{i}"], rtol=1e-13)
        np.testing.assert_allclose(hin_n, g[f"hin_node{i}"], rtol=1e-12, atol=1e-16)
        np.testing.assert_allclose(hse_n, g[f"hse_node{i}"], rtol=1e-12, atol=1e-16)
        assert len(h_all) == fc.shape[0] - 1


def test_integration_segregation_dict_keys():
    d = HMA.integration_segregation(datasets.load_empfc("W").copy())
    assert set(d) == {"Hin_sim", "Hse_sim", "Hin_node_sim", "Hse_node_sim", "sFC"}
    assert (d["sFC"] >= 0).all()


def test_host_facade_matches_high_precision_golden():
    """The host facade (numpy fp64 SVD) against 40-digit arithmetic (tests/hma_reference.py) on matrices
    with negative entries, negative eigenvalues and no symmetry: clus_num and the in-place clip exact,
    every floating output within 8 x the deviation recorded when the golden file was written (another
    LAPACK build has other constants) or N 2^-52 of the output's largest magnitude."""
    golden = hr.load_golden()
    for (family, N, i), ref in golden.items():
        F = hr.checked_input(family, N, i, ref)
        got = hr.host_facade(F)
        np.testing.assert_array_equal(got["clus_num"], ref["clus_num"], err_msg=hr.key(family, N, i))
        np.testing.assert_array_equal(got["clipped"], hr.clipped(F))
        for name in hr.FLOAT_OUTPUTS:
            err = float(np.abs(np.asarray(got[name]) - ref[name]).max())
            assert err <= hr.bound(ref, name, N, 8), (family, N, i, name, err, hr.bound(ref, name, N, 8))


def test_host_functions_raise_on_nan_as_the_reference():
    """The per-matrix functions keep the reference's behaviour on a NaN entry (numpy's SVD does not
    converge); the batch function returns NaN values instead (tests/test_nonfinite_gpu.py)."""
    f = hr.make_input("signed_fc", 8, 0)
    cn, cs, _ = HMA.Functional_HP(f.copy())
    f[2, 5] = np.nan
    with pytest.raises(np.linalg.LinAlgError):
        HMA.Functional_HP(f.copy())
    with pytest.raises(np.linalg.LinAlgError):
        HMA.Balance(f.copy(), cn, cs)
    with pytest.raises(np.linalg.LinAlgError):
        HMA.nodal_measures(f.copy(), cn, cs)

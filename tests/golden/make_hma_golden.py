#!/usr/bin/env python3
"""golden_hma_hp.npz: HMA in 40-digit arithmetic on matrices with structure (needs mpmath; run once,
minutes; the tests never call mpmath).

For every case of tests/hma_reference.py:cases() -- three input families (zero_diag, signed_fc, asym),
two matrices each at N = 3, 4, 5, 16, 17, 33, 64, 65, 90, 95, 96, generated unclipped -- the file holds
(packed into two arrays, hma_reference.pack):

  hin, hse, hin_node, hse_node, sv, clus_num   hma_reference.hma_mp (mpmath.eigsy at dps = 40), rounded
                                               to fp64 at the end
  dev_hin, ... dev_sv                          max |host facade (numpy fp64 SVD) - the above|, per output
  pins                                         the input's sum and four of its entries
  gap, min_u                                   the admission figures

Inputs are not stored.  A case is admitted only if, on the reference alone, consecutive |lambda| differ by
at least MIN_GAP = 1e-6 of the largest and the smallest |u| over the splitting modes is at least
MIN_U = 1e-7: the ordering and the sign splits are only defined away from ties.  If a case fails, the script
aborts and a different seed goes into hma_reference.SEEDS; no case is skipped at test time.  The host
facade's clus_num must equal the reference's (asserted here).

  python tests/golden/make_hma_golden.py [processes]
"""
import os
import sys
import time
from multiprocessing import Pool

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
from tests import hma_reference as hr  # noqa: E402


def one(case):
    f, N, i = case
    t0 = time.time()
    F = hr.make_input(f, N, i)
    ref, gap, min_u = hr.hma_mp(F)
    host = hr.host_facade(F)
    k = hr.key(f, N, i)
    out = {n: ref[n] for n in hr.FLOAT_OUTPUTS + ("clus_num",)}
    for n in hr.FLOAT_OUTPUTS:
        out[f"dev_{n}"] = float(np.abs(np.asarray(host[n]) - ref[n]).max())
    out["pins"], out["gap"], out["min_u"] = hr.pins(F), gap, min_u
    same = bool((host["clus_num"] == ref["clus_num"]).all())
    Fc = hr.clipped(F)
    neg = int((np.linalg.eigvalsh((Fc + Fc.T) / 2) < 0).sum())
    line = (f"{k}: gap {gap:.1e} min|u| {min_u:.1e} negative entries {int((F < 0).sum())} eigenvalues {neg} "
            f"clus_num[-1] {int(ref['clus_num'][-1])} host dev "
            + " ".join(f"{n} {out[f'dev_{n}']:.1e}" for n in hr.FLOAT_OUTPUTS)
            + f" {time.time() - t0:.0f} s")
    return out, line, gap >= hr.MIN_GAP and min_u >= hr.MIN_U, same


def main():
    procs = int(sys.argv[1]) if len(sys.argv) > 1 else min(16, os.cpu_count() or 1)
    cases = sorted(hr.cases(), key=lambda c: -c[1])  # the long ones first
    out, failed = {}, []
    with Pool(procs) as pool:
        for (o, line, admitted, same), case in zip(pool.imap(one, cases), cases):
            print(line, "" if admitted else "NOT ADMITTED", "" if same else "HOST clus_num DIFFERS", flush=True)
            out[case] = o
            if not (admitted and same):
                failed.append(case)
    if failed:
        sys.exit(f"not admitted (put another seed into hma_reference.SEEDS): {failed}")
    np.savez_compressed(hr.GOLDEN, **hr.pack(out))
    size = os.path.getsize(hr.GOLDEN)
    print(hr.GOLDEN, size, "bytes")
    assert size < 200 * 1024
    got = hr.load_golden()
    for case, o in out.items():
        for n, v in o.items():
            assert (np.asarray(got[case][n]) == np.asarray(v)).all(), (case, n)


if __name__ == "__main__":
    main()

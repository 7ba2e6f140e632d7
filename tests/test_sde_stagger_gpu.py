"""Wave roles of the large-batch fp32 integrator (V_STAG): some waves of a workgroup
draw the step's normals before their coupling phase, the others inside the update.  The role only
reorders independent instructions, so every result is bit-identical to the register-resident
kernel's, whatever the role mask (WCSDE_STAGGER, read per call), the chunking or the record layout.

The large-batch kernels are chosen by groups of 16 simulations per CU (more than 3 CUs' worth:
four groups per workgroup, more than 4: five), so the batch sizes follow the device's CU count.
"""
import numpy as np
import pytest
import torch

from nremmodfc_amd.model import Batch, sim_keys

pytestmark = pytest.mark.gpu

ALL_A, ALL_B = "0", "7fff"


def cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def b_sg5():
    return 16 * (4 * cus() + 1)  # 4 CUs + 1 groups: five groups per workgroup


def b_sg4():
    return 16 * (3 * cus() + 1) - 7  # 3 CUs + 1 groups, the last one ragged (9 simulations)


def inputs(B):
    rng = np.random.default_rng(B)
    G = 0.16 + rng.uniform(-0.1, 0.3, B)
    S = 7.68 + rng.uniform(-0.2, 0.2, B)
    return G, S, sim_keys(np.arange(B) % 50, np.arange(B) // 50)


def run(sc, G, S, keys):
    """integrate(5, 0.05), then 45 recorded steps: records at steps 0, 20, 40 (not the last step)."""
    bt = Batch(sc, G, S, keys, precision="f32")
    B = len(keys)
    rec = [torch.empty((3, B, 90), dtype=torch.float32, device="cuda") for _ in range(3)]
    bt.integrate(5, 0.05)
    bt.integrate(45, 2.0, 20, *rec)
    torch.cuda.synchronize()
    return rec + [bt.E, bt.I, bt.A]


_cache = {}


def run_sg5_default(sc):
    """The SG = 5 batch under the default mask, computed once for the tests that compare against it."""
    if "sg5" not in _cache:
        _cache["sg5"] = run(sc, *inputs(b_sg5()))
    return _cache["sg5"]


@pytest.mark.parametrize("size", ["sg5", "sg4"])
def test_staggered_kernel_matches_register_kernel(cuda, sc90, monkeypatch, size):
    monkeypatch.delenv("WCSDE_STAGGER", raising=False)
    B = b_sg5() if size == "sg5" else b_sg4()
    G, S, keys = inputs(B)
    big = run_sg5_default(sc90) if size == "sg5" else run(sc90, G, S, keys)
    for sl in (slice(0, 40), slice(B - 24, B)):
        small = run(sc90, G[sl], S[sl], keys[sl])
        for k, (x, y) in enumerate(zip(big, small)):
            xs = x[:, sl] if k < 3 else x[sl]
            assert torch.equal(xs, y), (size, sl, k)


def test_role_mask_does_not_change_results(cuda, sc90, monkeypatch):
    monkeypatch.delenv("WCSDE_STAGGER", raising=False)
    ref = run_sg5_default(sc90)
    G, S, keys = inputs(b_sg5())
    for mask in (ALL_A, ALL_B):
        monkeypatch.setenv("WCSDE_STAGGER", mask)
        got = run(sc90, G, S, keys)
        for k, (x, y) in enumerate(zip(ref, got)):
            assert torch.equal(x, y), (mask, k)


def test_chunked_calls_equal_one_call(cuda, sc90, monkeypatch):
    """Two calls of 30 steps against one of 60, a record every 10 steps: the second call starts on
    a record, and its hoisted draws take the step counter where the first call left it."""
    monkeypatch.delenv("WCSDE_STAGGER", raising=False)
    B = b_sg5()
    G, S, keys = inputs(B)
    one = Batch(sc90, G, S, keys, precision="f32")
    two = Batch(sc90, G, S, keys, precision="f32")
    r1 = torch.empty((6, B, 90), dtype=torch.float32, device="cuda")
    r2 = torch.empty((6, B, 90), dtype=torch.float32, device="cuda")
    one.integrate(60, 2.0, 10, r1)
    two.integrate(30, 2.0, 10, r2[:3])
    two.integrate(30, 2.0, 10, r2[3:])
    torch.cuda.synchronize()
    assert torch.equal(r1, r2)
    assert torch.equal(one.E, two.E) and torch.equal(one.I, two.I) and torch.equal(one.A, two.A)


def test_node_major_ring_equals_time_major(cuda, sc90, monkeypatch):
    monkeypatch.delenv("WCSDE_STAGGER", raising=False)
    B = b_sg5()
    G, S, keys = inputs(B)
    nsteps, ld = 50, 32
    n_rec = -(-nsteps // 20)
    a = Batch(sc90, G, S, keys, precision="f32")
    b = Batch(sc90, G, S, keys, precision="f32")
    tm = torch.empty((n_rec, B, 90), dtype=torch.float32, device="cuda")
    ring = torch.full((B * 90 * ld,), float("nan"), dtype=torch.float32, device="cuda")
    a.integrate(nsteps, 2.0, 20, tm)
    b.integrate(nsteps, 2.0, 20, ring[4:], rec_ld=ld)
    torch.cuda.synchronize()
    nm = ring.view(B * 90, ld)[:, 4:4 + n_rec].reshape(B, 90, n_rec).permute(2, 0, 1)
    assert torch.equal(nm, tm)
    assert torch.isnan(ring.view(B * 90, ld)[:, 4 + n_rec:]).all()  # nothing written past the last record
    assert torch.isnan(ring.view(B * 90, ld)[:, :4]).all()
    assert torch.equal(a.E, b.E) and torch.equal(a.A, b.A)

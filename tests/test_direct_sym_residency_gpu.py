"""Where the symmetric Direct kernel keeps a lane's fp64 I-side sums changes no bit of the result.

At 16 bodies per lane tuning variant 3 (and the automatic choice) keeps the sums of bodies 0..11 in LDS and those of
bodies 12..15 in registers (two workgroups per CU); variant 4 keeps all 16 in LDS (one workgroup per CU, the form the
project ran before).  Every addition and its order are the same, so the deterministic form must agree bit for bit; the
atomic form, whose order of additions is not reproducible, is held to the oracle in both residencies."""
import numpy as np
import pytest
import torch

from gpu_util import packed, rel_err, to_device
from nbody_amd._lib import FIELDS
from test_direct_gpu import TOL

pytestmark = pytest.mark.gpu
EPS2 = 1e-6


def _ic(nb, n, masses):
    ic = nb.ic.plummer(n, seed=n)
    if masses == "general":  # the general-mass instantiation (the equal-mass one exits on the device flag)
        ic["mass"] = (ic["mass"] * np.random.default_rng(n).uniform(0.2, 3.0, n)).astype(np.float32)
        ic["mass"][::97] = 0.0
    return ic


# 8,193: NB = 3 with ONE body in the last superblock; 16,384: NB = 4, even -- the half ring skips the upper half's
# partner at d = NB/2; 20,000: NB = 5, ragged; 90,001: the size of test_symmetric_kernel_vs_oracle.
# s = 5 at 20,000 bodies: shares of 39 chunks -- the tail fold with nchunks % 4 != 0, shares that start inside a partner.
@pytest.mark.parametrize("s", [0, 1, 5])
@pytest.mark.parametrize("masses", ["equal", "general"])
@pytest.mark.parametrize("n", [8193, 16384, 20000, 90001])
def test_residency_bit_identity_deterministic(nb, ctx, n, masses, s):
    p = packed(_ic(nb, n, masses))
    out = {}
    try:
        ctx.deterministic(2)  # slot planes required: no silent switch to the atomics
        for variant in (3, 4, 3, 4):  # each form twice
            ctx.tuning(variant, 16, s)
            a = nb.direct_forces_packed(ctx, p, p, 1.0, EPS2)
            info = ctx.directInfo(n, EPS2)
            assert info["last_kernel"] == 2 and info["bodies_per_lane_equal"] == 16 and info["bodies_per_lane_general"] == 16
            out.setdefault(variant, []).append(a.cpu().numpy())
    finally:
        ctx.deterministic(True)
        ctx.tuning()
    assert np.all(np.isfinite(out[3][0])) and np.any(out[3][0][:, :3] != 0)
    assert np.array_equal(out[3][0], out[3][1]), "two-workgroup form: launch after launch"
    assert np.array_equal(out[4][0], out[4][1]), "all-LDS form: launch after launch"
    assert np.array_equal(out[3][0], out[4][0]), "the two residencies differ"


@pytest.mark.parametrize("variant", [3, 4])
@pytest.mark.parametrize("masses", ["equal", "general"])
@pytest.mark.parametrize("n", [20000, 90001])
def test_residency_atomic_vs_oracle(nb, oracle, ctx, n, masses, variant):
    ic = _ic(nb, n, masses)
    p = packed(ic)
    try:
        ctx.deterministic(False)
        ctx.tuning(variant, 16, 0)
        a = nb.direct_forces_packed(ctx, p, p, 1.0, EPS2).cpu().numpy()
        assert ctx.directInfo()["last_kernel"] == 1
    finally:
        ctx.deterministic(True)
        ctx.tuning()
    # the sample of test_symmetric_kernel_vs_oracle
    rng = np.random.default_rng(1)
    r = np.sqrt(ic["pos_x"] ** 2 + ic["pos_y"] ** 2 + ic["pos_z"] ** 2)
    idx = np.unique(np.concatenate([rng.choice(n, 1024, replace=False), np.argsort(r)[:128],
                                    np.arange(n - 300, n), np.arange(300)]))
    ref = np.stack(oracle.direct_forces_indexed(ic["pos_x"], ic["pos_y"], ic["pos_z"], ic["mass"], idx,
                                                1.0, EPS2, 1), 1)
    assert rel_err(a[idx, :3], ref).max() < TOL


# the atomic two-set form at 16 bodies per lane takes the same two residencies (ragged sets, >= 49,152 bodies each);
# reference: the one-sided kernel, itself held to the oracle in test_direct_gpu.py
@pytest.mark.parametrize("variant", [-1, 4])
@pytest.mark.parametrize("masses", ["equal", "general"])
def test_residency_atomic_pair_kernel(nb, ctx, masses, variant):
    na, nb_ = 55001, 50002
    p = packed(_ic(nb, na + nb_, masses))
    a, b = p[:na].contiguous(), p[na:].contiguous()
    acc_a = torch.full((na, 4), 3.0, device="cuda")
    acc_b = torch.full((nb_, 4), 3.0, device="cuda")
    try:
        ctx.deterministic(False)
        ctx.tuning(variant, 16, 0)
        nb.direct_forces_pair_packed(ctx, a, b, 1.0, EPS2, acc_a, acc_b)
        assert ctx.directInfo()["last_kernel"] == 1
        ctx.tuning(1, 4, 0)
        ra = nb.direct_forces_packed(ctx, a, b, 1.0, EPS2)
        rb = nb.direct_forces_packed(ctx, b, a, 1.0, EPS2)
    finally:
        ctx.deterministic(True)
        ctx.tuning()
    assert rel_err(acc_a.cpu().numpy()[:, :3], ra.cpu().numpy()[:, :3]).max() < TOL
    assert rel_err(acc_b.cpu().numpy()[:, :3], rb.cpu().numpy()[:, :3]).max() < TOL


# the finalize pass with the fused Velocity-Verlet kick reads the same slots
def test_residency_fused_kick(nb, ctx):
    n = 20000
    ic = nb.ic.plummer(n, seed=8)
    fc = nb.DirectForceCalculator()
    fc.setSofteningParameter(0.01)
    integ = nb.Integrator()

    def run(variant):
        d, _ = to_device(nb, ic)
        try:
            ctx.tuning(variant, 16, 0)
            fc.computeForces(d)
            for _ in range(3):
                integ.integrate(d, fc, 1e-3)
            assert ctx.directInfo()["last_kernel"] == 2
            torch.cuda.synchronize()
        finally:
            ctx.tuning()
        return {f: getattr(d, f).cpu().numpy().copy() for f in FIELDS}

    new, old = run(3), run(4)
    assert len(new) == 13
    for f in FIELDS:
        assert np.array_equal(new[f], old[f]), f
    assert np.any(new["vel_x"] != ic["vel_x"])

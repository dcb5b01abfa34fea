"""One Context taken through the host state machine of the Direct N^2 calls (csrc/direct_plan.h) on the
exact integer lattice of direct_lattice_ref.py: every expected force is an integer times 2^-60, so every comparison is
torch.equal and no tolerance is involved.  The steps are data; test_direct_sequences_gpu.py runs them.

After every call that succeeds the output equals the lattice formula and nbody_hip_direct_info, asked BEFORE the call
what it will run, names the kernel that then ran: the two answers come from one plan function."""
import re

import numpy as np
import pytest
import torch

import direct_lattice_ref as L

SIZES = (2049, 513)
BUDGET = 1  # bytes: no slot plane fits

REQUIRED = ("deterministic Direct sums were required but their slot planes ({wanted} bytes for {n} bodies) exceed the budget "
            "({budget} bytes and a quarter of the free device memory)")
PACKED_NEEDS = "packed variant needs targets_per_lane >= 2"
PAIR_NEEDS = "pair evaluation needs eps2 >= 1e-12 (use the one-sided entry point)"


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


class Run:
    """the bodies of one size on the device, their expected rows, and the checked force call"""

    def __init__(self, nb, ctx, n):
        self.nb, self.ctx, self.n = nb, ctx, n
        self.lat = L.lattice(n, "permuted", "g0123")
        self.p = dev(self.lat.packed)
        self.ref = L.expect_all_pairs(self.lat)
        self.want = dev(L.acc_rows(self.ref))

    def forces(self, kernel, tag):
        """a force call over all pairs: the plan asked first, then the call, then what ran"""
        plan = self.ctx.directInfo(self.n, L.EPS2)
        a = self.nb.direct_forces_packed(self.ctx, self.p, self.p, L.G, L.EPS2)
        ran = self.ctx.directInfo()["last_kernel"]
        assert plan["kernel"] == ran == kernel, f"{tag}, n = {self.n}: planned {plan['kernel']}, ran {ran}, expected {kernel}"
        if not torch.equal(a, self.want):
            R = plan["bodies_per_lane_equal"] or 2
            pytest.fail(f"{tag}, n = {self.n}\n" + L.describe(self.lat, L.units(a.cpu().numpy()), self.ref, R))
        return plan

    def refused(self, exc, text, tag):
        with pytest.raises(exc, match=re.escape(text)):
            self.nb.direct_forces_packed(self.ctx, self.p, self.p, L.G, L.EPS2)
        assert self.ctx.handle, tag


def run_sequence(nb, ctx, n):
    r = Run(nb, ctx, n)
    try:
        r.forces(0, "1 default tuning: one-sided")
        ctx.tuning(3, 2)
        plan = r.forces(2, "2 tuning(3, 2): symmetric with slots")
        assert plan["bodies_per_lane_equal"] == 2 and plan["workspace_bytes_needed"] == plan["slot_bytes_wanted"] > 0
        ctx.deterministic(0)
        plan = r.forces(1, "3 deterministic(0): atomics")
        assert plan["slot_bytes_wanted"] == 0 and plan["reaction_slots"] == 0 and plan["iside_slots"] == 1
        ctx.deterministic(1)
        ctx.slotBudget(BUDGET)
        plan = r.forces(1, "4 deterministic(1), slotBudget(1): atomics")
        assert plan["slot_bytes_wanted"] > BUDGET and plan["workspace_bytes_needed"] < plan["slot_bytes_wanted"]
        ctx.deterministic(2)
        assert ctx.directInfo(n, L.EPS2)["kernel"] == 1
        r.refused(nb.ResourceException, REQUIRED.format(wanted=plan["slot_bytes_wanted"], n=n, budget=BUDGET),
                  "5 deterministic(2) with that budget")
        assert ctx.directInfo()["last_kernel"] == 1  # (the refused call ran nothing)
        ctx.slotBudget(0)
        r.forces(2, "6 slotBudget(0): slots again, the context is usable after the refusal")
        ctx.tuning(1, 1)
        assert ctx.directInfo(n, L.EPS2)["kernel"] == 0
        r.refused(nb.ValidationException, PACKED_NEEDS, "7 tuning(1, 1)")
        ctx.tuning()
        r.forces(0, "8 tuning(): back to automatic")
        # 9 the two-set entry refuses tiny softening before it plans anything
        half = n // 2
        a, b = r.p[:half].contiguous(), r.p[half:].contiguous()
        with pytest.raises(nb.ValidationException, match=re.escape(PAIR_NEEDS)):
            nb.direct_forces_pair_packed(ctx, a, b, L.G, 0.0, torch.empty_like(a), torch.empty_like(b))
        assert ctx.directInfo()["last_kernel"] == 0
        r.forces(0, "after the refusals")
    finally:
        ctx.slotBudget(0)
        ctx.deterministic(True)
        ctx.tuning()
    return r


def run_field(nb, ctx, r, d):
    """10 the field call on both sides of the four-points-per-lane threshold (32,768 points); d: r's bodies as particle
    data.  It takes the automatic shape whatever the context's tuning says, and is no force call: last_kernel stays."""
    fc = nb.DirectForceCalculator()
    fc.setGravitationalConstant(L.G)
    fc.setSofteningParameter(L.EPS)
    before = ctx.directInfo()["last_kernel"]
    try:
        for tuning in ((), (0, 1, 3)):
            ctx.tuning(*tuning)
            for count in L.FIELD_POINTS:
                pts2 = L.field_points2(count, r.lat)
                u2, msum = L.expect_points(pts2, r.lat)
                want = L.acc_rows(u2, scale=L.UNIT / 2)
                want[:, 3] = np.float32(-L.G * L.PHI_UNIT * msum)
                out = fc.computeField(d, dev((pts2 / 2.0).astype(np.float32)))
                assert torch.equal(out, dev(want)), f"10 field at {count} points against {r.n} bodies, tuning {tuning}"
                assert ctx.directInfo()["last_kernel"] == before
    finally:
        ctx.tuning()


def run_two_bodies_without_softening(nb, ctx):
    """the two-body known answer (a_0 = (1, 0, 0)) at eps = 0: tuning(3, 2) asks for the symmetric kernel, the plan
    answers with the guarded one-sided one -- the same bits as with default tuning"""
    p = dev(np.array([[0, 0, 0, 1], [1, 0, 0, 1]], np.float32))
    try:
        assert ctx.directInfo(2, 0.0)["kernel"] == 0
        ref = nb.direct_forces_packed(ctx, p, p, 1.0, 0.0)
        assert ctx.directInfo()["last_kernel"] == 0
        r = ref.cpu().numpy()
        assert abs(r[0, 0] - 1.0) < 1e-5 and abs(r[1, 0] + 1.0) < 1e-5 and np.all(r[:, 1:] == 0)  # (as test_edge_cases)
        ctx.tuning(3, 2)
        assert ctx.directInfo(2, 0.0)["kernel"] == 0 and ctx.directInfo(2, 1e-6)["kernel"] == 2
        a = nb.direct_forces_packed(ctx, p, p, 1.0, 0.0)
        assert ctx.directInfo()["last_kernel"] == 0
        assert torch.equal(a, ref)
    finally:
        ctx.tuning()

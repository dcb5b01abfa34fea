"""The host state machine of the Direct N^2 calls, one Context through every transition (direct_sequence.py): tuning,
deterministic mode, slot budget, the refusals and the fallback to atomics, on the exact integer lattice -- and after every
successful call nbody_hip_direct_info's plan names the kernel that ran (csrc/direct_plan.h: one plan function for both)."""
import numpy as np
import pytest

import direct_lattice_ref as L
import direct_sequence as S
from gpu_util import to_device

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("n", S.SIZES)
def test_one_context_through_its_states(nb, ctx, n):
    r = S.run_sequence(nb, ctx, n)
    z = np.zeros(n, np.float32)
    d, _ = to_device(nb, dict(pos_x=r.lat.p[:, 0].astype(np.float32), pos_y=r.lat.p[:, 1].astype(np.float32),
                              pos_z=r.lat.p[:, 2].astype(np.float32), vel_x=z, vel_y=z, vel_z=z,
                              mass=r.lat.m.astype(np.float32)))
    S.run_field(nb, ctx, r, d)
    info = ctx.directInfo(n, L.EPS2)
    assert info["deterministic_mode"] == 1 and info["kernel"] == 0  # the context is back in its default state


def test_two_bodies_without_softening_take_the_one_sided_kernel(nb, ctx):
    S.run_two_bodies_without_softening(nb, ctx)

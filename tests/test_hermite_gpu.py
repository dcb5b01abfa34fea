"""Direct force-and-jerk (nbody_hip_direct_acc_jerk) and the fourth-order Hermite integrator (nbody_hip_hermite_*) on a
real GPU: evaluation parity against fp64, ten steps against the restatement, the order of the scheme, determinism, the
time-step hint, refusals, ParticleSystem's scheme switch and the facade.  Restatements: tests/hermite_ref.py."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import hermite_handle_cases as hc
import hermite_ref as hr
from gpu_util import U, rel_err, to_device

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = ("pos_x", "pos_y", "pos_z", "vel_x", "vel_y", "vel_z", "acc_x", "acc_y", "acc_z", "acc_old_x", "acc_old_y", "acc_old_z")

# ---- the a-priori bound of the jerk against fp64 (the pattern of tests/test_field_gpu.py) ------------------------------
# |dj_i| <= max(1e-5 |j_i|, C u S_i), S_i = G sum_j m_j (|w| + 3 |d.w| |d| / h) h^-3/2 the sum of the term magnitudes
# (hermite_ref.acc_jerk), u = 2^-24.  A term is t = m f (w + q d), f = h^-3/2, q = -3 (d.w) / h.  Per term, first order
# in u, csrc/hermite.hip jerk_pk against the fp64 formula on the same fp32 inputs:
#   f:  d = fl(r_j - r_i) puts <= 2u on d^2, the three fused multiply-adds of h <= 3u more: 5u on h, 7.5u on h^-3/2;
#       v_rsq_f32 (<= 1 ulp = 2u) cubed 6u; the three roundings of (m inv) (inv inv) 3u                          => 16.5u
#   the |w| part:  f 16.5u, w = fl(v_j - v_i) 1u, the rounding of fma(q, d, w) 1u, and the ABSOLUTE error of the fp32
#       dot product -- d.w may cancel: <= (2u inputs + 3u roundings) |d| |w|, times 3 |d| / h <= 3 / |d|: 15u |w| => 33.5u
#   the |d.w| part:  f 16.5u, h^-1 5u, rsq squared 4u, the roundings of inv^2, (d.w) inv^2, the product with -3: 3u,
#       d 1u, the rounding of fma(q, d, w) 1u                                                                   => 30.5u
#                                                                                                     C_TERMS = 34
# Accumulation, as for the force: a term enters its fp32 tile sum through an FMA and passes at most TS = 256 roundings
# (constexpr TS in hermite.hip) before the fold into fp64; the split sums are rounded to fp32 once more.  A component's
# error is <= (TS + 1) u sum |t_x| <= (TS + 1) u S; three components -> sqrt(3).  The final rounding: 1.
#   C_JERK = 34 + sqrt(3) (256 + 1) + 1 = 480.1
# Worst cases, every rounding at its limit with the same sign; nothing here is fitted to the data.
TS = 256
C_TERMS = 34
C_JERK = C_TERMS + np.sqrt(3.0) * (TS + 1) + 1
# Regression tier, MEASURED on an MI355X, not derived: the margins max err / (u S_j) of the three 4,096-body sets of
# test_evaluation_parity were 11.06 (eps 0.01), 9.03 (eps 0.05) and 7.18 (general masses, G = 1.7) -- forty times inside
# the worst case; max |dj| / |j| 4.9e-6, 8.5e-6 and 5.6e-6, no body above 1e-5.  1.6 x the largest is held.
JERK_MARGIN_MEASURED = 11.06


def _arrays(ic):
    pos = np.stack([ic["pos_x"], ic["pos_y"], ic["pos_z"]], 1)
    vel = np.stack([ic["vel_x"], ic["vel_y"], ic["vel_z"]], 1)
    return pos, vel, ic["mass"]


def _general_masses(ic, seed=5):
    ic = dict(ic)
    ic["mass"] = (ic["mass"] * np.random.default_rng(seed).uniform(0.5, 2.0, ic["mass"].size)).astype(np.float32)
    return ic


def _direct(nb, G, eps):
    c = nb.DirectForceCalculator()
    c.setGravitationalConstant(G)
    c.setSofteningParameter(eps)
    return c


def _state(d):
    return {k: getattr(d, k).cpu().numpy().copy() for k in F}


def _xv(d):
    s = _state(d)
    return (np.stack([s["pos_x"], s["pos_y"], s["pos_z"]], 1).astype(np.float64),
            np.stack([s["vel_x"], s["vel_y"], s["vel_z"]], 1).astype(np.float64))


def _ref_eval(pos, vel, m, G, eps, targets=None, chunk=256):
    """hr.acc_jerk in fp64 on the device: (a, j, S_a, S_j) as numpy"""
    p = torch.from_numpy(np.ascontiguousarray(pos, np.float64)).cuda()
    v = torch.from_numpy(np.ascontiguousarray(vel, np.float64)).cuda()
    mm = torch.from_numpy(np.asarray(m, np.float64)).cuda()
    idx = torch.arange(len(p), device="cuda") if targets is None else torch.as_tensor(np.asarray(targets), device="cuda")
    e2 = hr.eps2_of(eps)
    out = [[], [], [], []]
    for b in range(0, len(idx), chunk):
        t = idx[b:b + chunk]
        d = p[None, :, :] - p[t, None, :]
        w = v[None, :, :] - v[t, None, :]
        d2 = (d * d).sum(-1)
        ok = (d2 > 0) if e2 < 1e-12 else torch.ones_like(d2, dtype=torch.bool)
        h = torch.where(ok, d2 + e2, torch.ones_like(d2))
        f = torch.where(ok, mm[None, :] * h ** -1.5, torch.zeros_like(d2))
        dw = (d * w).sum(-1)
        q = -3.0 * dw / h
        out[0].append(G * (f[:, :, None] * d).sum(1))
        out[1].append(G * (f[:, :, None] * (w + q[:, :, None] * d)).sum(1))
        out[2].append(G * (f * d2.sqrt()).sum(1))
        out[3].append(G * (f * ((w * w).sum(-1).sqrt() + 3.0 * dw.abs() * d2.sqrt() / h)).sum(1))
    return tuple(torch.cat(o).cpu().numpy() for o in out)


def _gpu_eval(nb, ctx, d, G, eps):
    acc, jerk = nb.direct_acc_jerk(ctx, d, G, eps)
    assert tuple(acc.shape) == (d.count, 4) and tuple(jerk.shape) == (d.count, 4)
    acc, jerk = acc.cpu().numpy(), jerk.cpu().numpy()
    assert not acc[:, 3].any() and not jerk[:, 3].any()
    return acc[:, :3].astype(np.float64), jerk[:, :3].astype(np.float64)


def _parity(tag, a, j, ref, rows=None):
    """the criterion: a per body within 1e-5; |dj| <= max(1e-5 |j|, C_JERK u S_j).  -> the margin max err / (u S_j)"""
    a_ref, j_ref, _, sj = ref
    if rows is not None:
        a, j = a[rows], j[rows]
    ea = rel_err(a, a_ref)
    err = np.linalg.norm(j - j_ref, axis=1)
    bound = np.maximum(1e-5 * np.linalg.norm(j_ref, axis=1), C_JERK * U * sj)
    margin = float((err / np.maximum(U * sj, 1e-300)).max())
    print(f"{tag}: max |da| / |a| {ea.max():.3e}; max |dj| / |j| {rel_err(j, j_ref).max():.3e}, bodies above 1e-5: "
          f"{int((rel_err(j, j_ref) > 1e-5).sum())} of {len(j)}, margin max err / (u S_j) {margin:.2f} (C = {C_JERK:.1f})",
          flush=True)
    assert ea.max() <= 1e-5, (tag, ea.max())
    assert np.all(err <= bound), (tag, int(np.argmax(err / np.maximum(bound, 1e-300))))
    return margin


# ---- evaluation parity -------------------------------------------------------------------------------------------------
def test_device_reference_is_the_restatement(nb, ctx):
    pos, vel, m = _arrays(_general_masses(nb.ic.plummer(700, seed=3)))
    for eps in (0.05, 0.0):
        if eps == 0.0:
            pos[1] = pos[0]  # a coincident pair under the guard convention
        got = _ref_eval(pos, vel, m, 1.7, eps)
        want = hr.acc_jerk(pos, vel, m, 1.7, eps)
        for g, w, s in zip(got, want, (want[2], want[3], want[2], want[3])):
            assert np.allclose(g, w, rtol=1e-11, atol=1e-12 * s.max())
    sub = _ref_eval(pos, vel, m, 1.7, 0.05, targets=[5, 699, 0])
    full = _ref_eval(pos, vel, m, 1.7, 0.05)
    assert all(np.allclose(s, f[[5, 699, 0]], rtol=1e-13, atol=0) for s, f in zip(sub, full))


SETS = {"eps0.01": (0.01, 1.0, False), "eps0.05": (0.05, 1.0, False), "general_masses_G1.7": (0.05, 1.7, True)}


@pytest.fixture(scope="module")
def plummer4096(nb):
    return nb.ic.plummer(4096, seed=42)


@pytest.mark.parametrize("name", list(SETS))
def test_evaluation_parity(nb, ctx, plummer4096, name):
    eps, G, general = SETS[name]
    ic = _general_masses(plummer4096) if general else plummer4096
    pos, vel, m = _arrays(ic)
    d, _ = to_device(nb, ic)
    a, j = _gpu_eval(nb, ctx, d, G, eps)
    margin = _parity(f"4,096 bodies, {name}", a, j, _ref_eval(pos, vel, m, G, eps))
    assert margin <= 1.6 * JERK_MARGIN_MEASURED, (name, margin, JERK_MARGIN_MEASURED)


@pytest.mark.parametrize("n", [1, 2, 255, 257, 1000, 12289])
def test_evaluation_sizes(nb, ctx, n):
    """padding, a ragged last tile, the split choice (12,289 bodies: 25 target blocks, 49 tiles in 49 splits)"""
    ic = _general_masses(nb.ic.plummer(n, seed=42))
    pos, vel, m = _arrays(ic)
    d, _ = to_device(nb, ic)
    a, j = _gpu_eval(nb, ctx, d, 1.7, 0.05)
    if n == 1:
        assert not a.any() and not j.any()
        return
    _parity(f"{n} bodies", a, j, _ref_eval(pos, vel, m, 1.7, 0.05))


def test_guard_instantiation_with_a_coincident_pair(nb, ctx):
    ic = _general_masses(nb.ic.plummer(257, seed=42))
    for k in ("pos_x", "pos_y", "pos_z"):
        ic[k][200] = ic[k][3]  # two bodies at one place, different velocities
    pos, vel, m = _arrays(ic)
    d, _ = to_device(nb, ic)
    a, j = _gpu_eval(nb, ctx, d, 1.7, 0.0)
    assert np.isfinite(a).all() and np.isfinite(j).all()
    _parity("eps = 0, 257 bodies, one coincident pair", a, j, _ref_eval(pos, vel, m, 1.7, 0.0))
    # with softening the pair adds m w / eps^3 to the jerk (the derivative of the softened kernel) and nothing to a
    a2, j2 = _gpu_eval(nb, ctx, d, 1.7, 0.05)
    _parity("eps = 0.05, the same bodies", a2, j2, _ref_eval(pos, vel, m, 1.7, 0.05))


def test_evaluation_65536_sampled(nb, ctx):
    ic = nb.ic.plummer(65536, seed=42)
    pos, vel, m = _arrays(ic)
    d, _ = to_device(nb, ic)
    a, j = _gpu_eval(nb, ctx, d, 1.0, 0.01)
    rows = np.random.default_rng(7).choice(65536, 2048, replace=False)
    _parity("65,536 bodies, 2,048 sampled", a, j, _ref_eval(pos, vel, m, 1.0, 0.01, targets=rows, chunk=64), rows=rows)


def test_standalone_call_leaves_acc_alone_and_prime_keeps_the_same_jerk(nb, ctx, plummer4096):
    d, _ = to_device(nb, plummer4096)
    d.acc_x.fill_(3.0)
    d.acc_old_y.fill_(-2.0)
    before = _state(d)
    acc, jerk = nb.direct_acc_jerk(ctx, d, 1.0, 0.05)
    after = _state(d)
    for k in F:
        assert np.array_equal(before[k], after[k]), k
    fc = _direct(nb, 1.0, 0.05)
    h = nb.HermiteIntegrator()
    h.prime(d, fc)
    assert torch.equal(h.getJerk(), jerk)
    assert torch.equal(torch.stack([d.acc_x, d.acc_y, d.acc_z], 1), acc[:, :3])
    assert np.array_equal(d.acc_old_y.cpu().numpy(), before["acc_old_y"])  # priming writes acc_* only
    none, jerk2 = nb.direct_acc_jerk(ctx, d, 1.0, 0.05, write_acc=True)  # acc_out == NULL: into acc_*
    assert none is None and torch.equal(jerk2, jerk)
    assert torch.equal(torch.stack([d.acc_x, d.acc_y, d.acc_z], 1), acc[:, :3])


# ---- ten steps against the restatement ---------------------------------------------------------------------------------
def test_ten_steps_against_the_restatement(nb, ctx, plummer4096):
    G, eps, dt = 1.0, 0.05, 1e-3
    pos, vel, m = _arrays(plummer4096)
    d, _ = to_device(nb, plummer4096)
    fc = _direct(nb, G, eps)
    h = nb.HermiteIntegrator()
    h.integrate_steps(d, fc, dt, 10)
    ref = hr.hermite_steps(pos, vel, m, G, eps, dt, 10, np.float32, evaluate=lambda x, v: _ref_eval(x, v, m, G, eps))
    x, v = _xv(d)
    print(f"ten steps: max |dx| {np.abs(x - ref['pos']).max():.3e}, max |dv| {np.abs(v - ref['vel']).max():.3e}")
    # the bar of tests/test_integrator_gpu.py for ten Velocity-Verlet steps against its fixture
    assert np.allclose(x, ref["pos"], rtol=2e-5, atol=2e-6)
    assert np.allclose(v, ref["vel"], rtol=2e-5, atol=2e-6)
    s = _state(d)
    acc = np.stack([s["acc_x"], s["acc_y"], s["acc_z"]], 1)
    acc_old = np.stack([s["acc_old_x"], s["acc_old_y"], s["acc_old_z"]], 1)
    assert rel_err(acc, ref["acc"]).max() <= 1e-5        # a(t10), evaluated at the predicted state
    assert rel_err(acc_old, ref["acc_old"]).max() <= 1e-5  # a(t9)
    assert rel_err(acc, ref["acc_old"]).max() > 1e-5     # (the two differ by more than the bar: the check can tell)
    # the jerk on the handle: the parity criterion against fp64 at the restatement's own predicted state
    steps9 = hr.hermite_steps(pos, vel, m, G, eps, dt, 9, np.float32, evaluate=lambda x, v: _ref_eval(x, v, m, G, eps))
    hh = float(np.float32(dt))
    xp = (steps9["pos"] + steps9["vel"] * hh + steps9["acc"] * (0.5 * hh * hh) + steps9["jerk"] * (hh ** 3 / 6)).astype(np.float32)
    vp = (steps9["vel"] + steps9["acc"] * hh + steps9["jerk"] * (0.5 * hh * hh)).astype(np.float32)
    a_ref, j_ref, sa, sj = _ref_eval(xp, vp, m, G, eps)
    j = h.getJerk().cpu().numpy()[:, :3].astype(np.float64)
    err = np.linalg.norm(j - j_ref, axis=1)
    # (the engine's predicted state differs from the restatement's by the rounding of ten steps: that moves j by a few
    # 1e-6 relative, inside the 1e-5 term of the criterion; C u S_j covers the bodies whose jerk cancels)
    assert np.all(err <= np.maximum(1e-5 * np.linalg.norm(j_ref, axis=1), C_JERK * U * sj))


# ---- the order of the scheme -------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def binary_reference():
    pos, vel, m = hr.binary()
    return hr.hermite_steps(pos, vel, m, 1.0, 0.01, 6.25 / 65536, 65536, np.float64)["pos"]


def _ic_of(pos, vel, m):
    return dict(pos_x=pos[:, 0].copy(), pos_y=pos[:, 1].copy(), pos_z=pos[:, 2].copy(), vel_x=vel[:, 0].copy(),
                vel_y=vel[:, 1].copy(), vel_z=vel[:, 2].copy(), mass=np.asarray(m, np.float32).copy())


def _run(nb, ic, G, eps, dt, steps, scheme):
    d, _ = to_device(nb, ic)
    fc = _direct(nb, G, eps)
    if scheme == "hermite4":
        integ = nb.HermiteIntegrator()
    else:
        integ = nb.Integrator()
        fc.computeForces(d)
    e0 = integ.computeEnergiesF64(d, G, eps)
    integ.integrate_steps(d, fc, dt, steps)
    e1 = integ.computeEnergiesF64(d, G, eps)
    return _xv(d)[0], abs(sum(e1) - sum(e0)) / abs(e0[1])


def test_order_on_the_binary(nb, ctx, binary_reference):
    ic = _ic_of(*hr.binary())
    T, eps = 6.25, 0.01
    err = {}
    for n in (50, 100, 200):
        err["hermite4", n] = np.abs(_run(nb, ic, 1.0, eps, T / n, n, "hermite4")[0] - binary_reference).max()
    err["vv", 200] = np.abs(_run(nb, ic, 1.0, eps, T / 200, 200, "velocity-verlet")[0] - binary_reference).max()
    print({k: f"{v:.3e}" for k, v in err.items()})
    # 8 = the geometric mean of second order's 4 and fourth order's 16; the restatement with fp32 state gives 19.4
    assert err["hermite4", 50] / err["hermite4", 100] >= 8
    assert err["hermite4", 200] <= err["vv", 200] / 16  # the restatement: 1 / 66


def test_order_on_a_plummer_sphere(nb, ctx):
    ic = nb.ic.plummer(256, seed=42)
    pos, vel, m = _arrays(ic)
    G, eps, T = 1.0, 0.1, 1.0
    ref = hr.hermite_steps(pos, vel, m, G, eps, T / 512, 512, np.float64,
                           evaluate=lambda x, v: _ref_eval(x, v, m, G, eps))["pos"]
    err, drift = {}, {}
    for k in (8, 16, 32):
        x, drift["hermite4", k] = _run(nb, ic, G, eps, T / k, k, "hermite4")
        err["hermite4", k] = np.abs(x - ref).max()
    x, drift["vv", 32] = _run(nb, ic, G, eps, T / 32, 32, "velocity-verlet")
    err["vv", 32] = np.abs(x - ref).max()
    print({k: f"{v:.3e}" for k, v in err.items()}, {k: f"{v:.3e}" for k, v in drift.items()})
    assert err["hermite4", 8] / err["hermite4", 16] >= 8         # the restatement: 21
    assert drift["hermite4", 32] <= 0.25 * drift["vv", 32]       # |dE| / |PE0|; the restatement: 1 / 13


# ---- determinism -------------------------------------------------------------------------------------------------------
def _bits(d):
    return np.concatenate([v.view(np.uint32) for v in _state(d).values()])


def test_bitwise_reproducible_and_steps_compose(nb, ctx):
    ic = _general_masses(nb.ic.plummer(12289, seed=42))
    fc = _direct(nb, 1.7, 0.05)
    runs = []
    for plan in ((5,), (5,), (1, 1, 1, 1, 1), (2, 3)):
        d, _ = to_device(nb, ic)
        h = nb.HermiteIntegrator()
        for k in plan:
            if k == 1:
                h.integrate(d, fc, 2e-3)
            else:
                h.integrate_steps(d, fc, 2e-3, k)
        runs.append((_bits(d), h.getJerk().cpu().numpy().view(np.uint32)))
    for bits, jerk in runs[1:]:
        assert np.array_equal(bits, runs[0][0]) and np.array_equal(jerk, runs[0][1])


def test_invalidate_then_step_is_prime_then_step(nb, ctx):
    ic = nb.ic.plummer(1000, seed=42)
    fc = _direct(nb, 1.0, 0.05)
    out = []
    for how in ("invalidate", "prime", "neither"):
        d, _ = to_device(nb, ic)
        h = nb.HermiteIntegrator()
        h.integrate_steps(d, fc, 1e-2, 3)
        d.vel_x.mul_(0.5)  # the caller changes the state behind the handle
        if how == "invalidate":
            h.invalidate()
        elif how == "prime":
            h.prime(d, fc)
        h.integrate_steps(d, fc, 1e-2, 2)
        out.append(_bits(d))
    assert np.array_equal(out[0], out[1])
    assert not np.array_equal(out[0], out[2])  # (without either the stale (a, j) are used: the check can tell)


# ---- the time-step hint ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(SETS))
def test_time_step_hint(nb, ctx, plummer4096, name):
    eps, G, general = SETS[name]
    ic = _general_masses(plummer4096) if general else plummer4096
    pos, vel, m = _arrays(ic)
    d, _ = to_device(nb, ic)
    h = nb.HermiteIntegrator()
    with pytest.raises(nb.StateException):
        h.suggestTimeStep()
    h.prime(d, _direct(nb, G, eps))
    a_ref, j_ref, _, _ = _ref_eval(pos, vel, m, G, eps)
    for eta in (0.02, 0.01):
        want = hr.suggest_dt(a_ref, j_ref, eta)
        got = h.suggestTimeStep(eta)
        assert abs(got - want) <= 1e-4 * want, (got, want)
    assert h.suggestTimeStep() == h.suggestTimeStep(0.02)
    with pytest.raises(nb.ValidationException):
        h.suggestTimeStep(0.0)


def test_hint_needs_priming_at_the_c_abi(nb, ctx):
    lib = nb._lib.load()
    h = C.c_void_p()
    nb._lib.check(lib.nbody_hip_hermite_create(ctx.handle, 16, C.byref(h)))
    try:
        out = C.c_float()
        with pytest.raises(nb.StateException):
            nb._lib.check(lib.nbody_hip_hermite_suggest_dt(h, 0.02, C.byref(out)))
        buf = torch.zeros((16, 4), dtype=torch.float32, device="cuda")
        with pytest.raises(nb.StateException):
            nb._lib.check(lib.nbody_hip_hermite_jerk(h, buf.data_ptr()))
    finally:
        lib.nbody_hip_hermite_destroy(h)


# ---- refusals ----------------------------------------------------------------------------------------------------------
def test_refusals(nb, ctx):
    class Sub(nb.DirectForceCalculator):
        pass

    ic = nb.ic.plummer(64, seed=42)
    d, _ = to_device(nb, ic)
    before = _state(d)
    h = nb.HermiteIntegrator()
    for calc in (nb.BarnesHutCalculator(0.5), nb.SpatialHashCalculator(1.0, 2.0), Sub()):
        with pytest.raises(ValueError, match=r"HermiteIntegrator\.integrate: the Hermite scheme is Direct-only"):
            h.integrate(d, calc, 1e-3)
    fc = _direct(nb, 1.0, 0.05)
    for dt, msg in ((0.0, "Time step must be positive"), (-1e-3, "Time step must be positive"),
                    (float("nan"), "Time step must be a finite number"), (float("inf"), "Time step must be a finite number")):
        with pytest.raises(nb.ValidationException, match=msg):
            h.integrate(d, fc, dt)
    for k in F:  # nothing was touched by the refused calls
        assert np.array_equal(before[k], _state(d)[k]), k
    # a count above the capacity, at the C ABI (the Python class sizes its handle from the first count and grows it)
    lib = nb._lib.load()
    small = C.c_void_p()
    nb._lib.check(lib.nbody_hip_hermite_create(ctx.handle, 16, C.byref(small)))
    try:
        s = d.struct()
        with pytest.raises(nb.ValidationException, match="exceeds the integrator's capacity"):
            nb._lib.check(lib.nbody_hip_hermite_prime(small, C.byref(s), 1.0, 0.05))
        with pytest.raises(nb.ValidationException, match="exceeds the integrator's capacity"):
            nb._lib.check(lib.nbody_hip_hermite_step(small, C.byref(s), 1.0, 0.05, 1e-3, 1))
        with pytest.raises(nb.ValidationException, match="steps must be at least 1"):
            s.count = 16
            nb._lib.check(lib.nbody_hip_hermite_step(small, C.byref(s), 1.0, 0.05, 1e-3, 0))
        with pytest.raises(nb.StateException):
            nb._lib.check(lib.nbody_hip_hermite_step(small, None, 1.0, 0.05, 1e-3, 1))
        with pytest.raises(nb.ValidationException):
            s.count = 0
            nb._lib.check(lib.nbody_hip_hermite_step(small, C.byref(s), 1.0, 0.05, 1e-3, 1))
    finally:
        lib.nbody_hip_hermite_destroy(small)
    h.integrate(d, fc, 1e-3)  # and the integrator still works; a larger system re-sizes its handle
    big, _ = to_device(nb, nb.ic.plummer(300, seed=1))
    h.integrate(big, fc, 1e-3)
    assert tuple(h.getJerk().shape) == (300, 4)


# ---- ParticleSystem ----------------------------------------------------------------------------------------------------
def _system(nb, ic, scheme=None, dt=0.01):
    ps = nb.ParticleSystem()
    if scheme is not None:
        ps.setIntegrationScheme(scheme)
    cfg = nb.SimulationConfig(particle_count=ic["mass"].size, force_method=nb.ForceMethod.DIRECT_N2, dt=dt, G=1.0,
                              softening=0.1)
    ps.initialize(cfg, ic)
    return ps


def test_handle_refusals_at_the_c_abi(nb, ctx):
    """null state arrays, a count above the capacity, the precision read back (tests/hermite_handle_cases.py)"""
    d, _ = to_device(nb, nb.ic.plummer(8, seed=1))
    hc.raw_refusals(nb, ctx, d, "", "integrator's")


def test_particle_system_hermite4(nb, ctx):
    ic = nb.ic.plummer(256, seed=42)
    ps = _system(nb, ic, "hermite4")
    integ = nb.Integrator()
    e0 = integ.computeEnergiesF64(ps.getDeviceData(), 1.0, 0.1)
    energies = []
    for s in range(100):
        ps.update(0.01)
        if s % 10 == 9:
            energies.append(sum(integ.computeEnergiesF64(ps.getDeviceData(), 1.0, 0.1)))
    drift = max(abs(e - sum(e0)) for e in energies) / abs(e0[1])
    print(f"hermite4, 256 bodies, 100 steps of 0.01: max |dE| / |PE0| {drift:.3e}")
    # truncation at dt = 0.01 is below the 6.6e-7 the restatement has at dt = 1/32 over the same time; the rounding of the
    # fp32 state over 100 steps random-walks to about sqrt(100) u: an order of magnitude above both
    assert drift <= 1e-5
    assert ps.getSimulationTime() == pytest.approx(1.0, rel=1e-4)
    # setState mid-run re-primes: the trajectory after it is that of a fresh system started from that state
    st = ps.getState()
    ps.setState(st)
    fresh = _system(nb, {k: getattr(st, k) for k in ("pos_x", "pos_y", "pos_z", "vel_x", "vel_y", "vel_z", "mass")},
                    "hermite4")
    for _ in range(5):
        ps.update(0.01)
        fresh.update(0.01)
    assert np.array_equal(_bits(ps.getDeviceData()), _bits(fresh.getDeviceData()))
    # a parameter change re-primes too (G and eps come from the calculator)
    ps.setGravitationalConstant(1.5)
    ps.update(0.01)
    st2 = fresh.getState()
    other = _system(nb, {k: getattr(st2, k) for k in ("pos_x", "pos_y", "pos_z", "vel_x", "vel_y", "vel_z", "mass")},
                    "hermite4")
    other.setGravitationalConstant(1.5)
    other.update(0.01)
    x = ps.getState()
    y = other.getState()
    for k in ("pos_x", "pos_y", "pos_z", "vel_x", "vel_y", "vel_z"):
        assert np.array_equal(getattr(x, k), getattr(y, k)), k
    # the force method cannot leave Direct while the scheme is selected
    with pytest.raises(nb.ValidationException, match="Direct-only"):
        ps.setForceMethod(nb.ForceMethod.BARNES_HUT)


def test_default_scheme_is_untouched(nb, ctx):
    ic = nb.ic.plummer(1000, seed=42)
    a = _system(nb, ic)                                # never touches the new setter
    b = _system(nb, ic, "velocity-verlet")
    c = nb.ParticleSystem()
    c.setIntegrationScheme("hermite4")
    c.setIntegrationScheme("velocity-verlet")
    c.initialize(a.config_, ic)
    d, _ = to_device(nb, ic)                           # the parent's path spelled out: Integrator on the Direct calculator
    fc = _direct(nb, 1.0, 0.1)
    fc.computeForces(d)
    integ = nb.Integrator()
    for _ in range(10):
        for ps in (a, b, c):
            ps.update(0.01)
        integ.integrate(d, fc, 0.01)
    assert a.getIntegrationScheme() == "velocity-verlet" and a.hermite_ is None
    for ps in (b, c):
        assert np.array_equal(_bits(a.getDeviceData()), _bits(ps.getDeviceData()))
    assert np.array_equal(_bits(a.getDeviceData()), _bits(d))


# ---- the facade's program ----------------------------------------------------------------------------------------------
def test_facade_hermite_program(nb, ctx):
    exe = os.path.join(ROOT, "n-body_amd", "lib", "hermite_tests")
    assert os.path.exists(exe), "build with __graft_entry__.build()"
    env = dict(os.environ)
    env["LD_LIBRARY_PATH"] = os.path.dirname(exe) + os.pathsep + env.get("LD_LIBRARY_PATH", "")
    r = subprocess.run([exe], cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    print(r.stdout)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    got = dict(re.findall(r"^hermite (\S+) (\S+)$", r.stdout, re.M))
    # the same ten steps through the Python host: the same bits
    n = 1000
    hst = nb.ParticleData()
    nb.ParticleDataManager.allocateHost(hst, n)
    nb.ParticleInitializer.initUniform(hst, nb.UniformDistParams((-1, -1, -1), (1, 1, 1), 0.5, 1.5), 7)
    hst.vel_x[:] = np.float32(0.1) * hst.pos_y
    hst.vel_y[:] = np.float32(-0.1) * hst.pos_x
    d = nb.ParticleData()
    nb.ParticleDataManager.allocateDevice(d, n)
    nb.ParticleDataManager.copyToDevice(d, hst)
    fc = _direct(nb, float(np.float32(1.7)), float(np.float32(0.05)))
    h = nb.HermiteIntegrator()
    h.integrate_steps(d, fc, 1e-3, 4)
    for _ in range(6):
        h.integrate(d, fc, 1e-3)
    fnv = 1469598103934665603
    for k in F[:6]:
        for b in getattr(d, k).cpu().numpy().tobytes():
            fnv = ((fnv ^ b) * 1099511628211) & 0xFFFFFFFFFFFFFFFF
    assert got["fnv"] == f"{fnv:016x}"
    assert float(got["dt"]) == pytest.approx(h.suggestTimeStep(0.02), rel=1e-7)
    assert float(got["ke"]) == pytest.approx(h.computeKineticEnergy(d), rel=1e-6)

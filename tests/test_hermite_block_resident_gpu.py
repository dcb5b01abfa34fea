"""Resident scheduling of the block-step Hermite integrator (nbody_hip_hermite_block_set_scheduling) on a real GPU.

The oracle is the host-scheduled integrator held to the narrow kernel form (setTuning(1 << 30)): the resident form runs
the same bodies in the same order, so every array of the particle data, the residuals, the jerk, the levels, the ticks,
want and the counters must agree BIT FOR BIT.  "reference" below is that run.  narrow_launches / wide_launches count
host-form launches, so a handle that ran only the resident form reports 0 for both.
Restatement of the scheme itself: tests/hermite_block_ref.py (tests/test_hermite_block_gpu.py holds the host form to it)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import hermite_block_ref as br
from gpu_util import to_device

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = ("pos_x", "pos_y", "pos_z", "vel_x", "vel_y", "vel_z", "acc_x", "acc_y", "acc_z", "acc_old_x", "acc_old_y", "acc_old_z",
     "mass")
ALWAYS_NARROW = 1 << 30
COUNTERS = ("block_steps", "body_steps", "level_steps", "floor_hits", "macro_steps", "current_tick", "last_n_active",
            "max_level")
G, DT = 1.7, 1.0 / 16


def _general_masses(ic, seed=5):
    ic = dict(ic)
    ic["mass"] = (ic["mass"] * np.random.default_rng(seed).uniform(0.5, 2.0, ic["mass"].size)).astype(np.float32)
    return ic


def _ic_of(pos, vel, m):
    return dict(pos_x=pos[:, 0].copy(), pos_y=pos[:, 1].copy(), pos_z=pos[:, 2].copy(), vel_x=vel[:, 0].copy(),
                vel_y=vel[:, 1].copy(), vel_z=vel[:, 2].copy(), mass=np.asarray(m, np.float32).copy())


def _direct(nb, g, eps):
    c = nb.DirectForceCalculator()
    c.setGravitationalConstant(g)
    c.setSofteningParameter(eps)
    return c


def _integ(nb, scheduling, precision="fp32", max_level=16, eta=0.02):
    """scheduling "reference": the host form held to the narrow kernel"""
    b = nb.BlockHermiteIntegrator()
    b.setParameters(eta, 0.01, max_level)
    b.setStatePrecision(precision)
    if scheduling == "reference":
        b.setTuning(ALWAYS_NARROW)
    else:
        b.setScheduling(scheduling)
    return b


def _snap(d, integ):
    """everything "equal" compares: the particle data, getState(), the extended state and the counters"""
    out = {k: getattr(d, k).cpu().numpy().view(np.uint32).copy() for k in F}
    st = integ.getState()
    out.update(jerk=st["jerk"].view(np.uint32).copy(), levels=st["levels"].copy(), ticks=st["ticks"].copy(),
               want=st["want"].view(np.uint32).copy())
    if integ.getStatePrecision() == "extended":
        x, v = integ.getExtendedState(d)
        out.update(X=x.view(np.uint64).copy(), V=v.view(np.uint64).copy())
    info = integ.info()
    out["info"] = {k: info[k] for k in COUNTERS}
    out["launches"] = (info["narrow_launches"], info["wide_launches"])
    return out


def _assert_equal(tag, got, ref):
    assert got.keys() == ref.keys(), tag
    for k in ref:
        if k == "launches":
            continue
        if k == "info":
            assert got[k] == ref[k], (tag, got[k], ref[k])
        else:
            bad = np.flatnonzero((got[k] != ref[k]).reshape(len(ref[k]), -1).any(axis=1))
            assert bad.size == 0, (tag, k, f"{bad.size} bodies differ, first {bad[:5]}")


_REF = {}


def _reference(nb, n, eps, precision, macro=2):
    """two macro steps of the Plummer case by the reference, computed once per shape and shared"""
    key = (n, eps, precision, macro)
    if key not in _REF:
        ic = _general_masses(nb.ic.plummer(n, seed=42))
        d, _ = to_device(nb, ic)
        b = _integ(nb, "reference", precision)
        b.advance(d, _direct(nb, G, eps), DT, macro)
        _REF[key] = (ic, _snap(d, b))
        assert _REF[key][1]["launches"][1] == 0  # (the reference really took the narrow form throughout)
    return _REF[key]


# ---- 1. bit equality over the edge shapes ------------------------------------------------------------------------------
# n = 1: no partner, |j| = 0, want = +inf; 4 / 5: the four-target group; 255-257: the lane block; 1023-1025: a second
# source block holding one body; 2049: three source blocks on four sub-blocks; 4096: the cap
@pytest.mark.parametrize("precision", ["fp32", "extended"])
@pytest.mark.parametrize("eps", [0.05, 0.0], ids=["packed", "guard"])
@pytest.mark.parametrize("n", [1, 2, 3, 4, 5, 255, 256, 257, 1023, 1024, 1025, 2049, 4096])
def test_resident_equals_the_narrow_host_form(nb, ctx, n, eps, precision):
    ic, ref = _reference(nb, n, eps, precision)
    d, _ = to_device(nb, ic)
    b = _integ(nb, "resident", precision)
    b.advance(d, _direct(nb, G, eps), DT, 2)
    got = _snap(d, b)
    print(f"n {n} eps {eps} {precision}: {got['info']['block_steps']} block steps, {got['info']['body_steps']} body steps")
    _assert_equal((n, eps, precision), got, ref)
    assert got["launches"] == (0, 0)
    assert got["info"]["macro_steps"] == 2 and got["info"]["current_tick"] == 0
    assert b.getScheduling() == ("resident", "resident")


# ---- 2. forced active sets ---------------------------------------------------------------------------------------------
def _forced_sets(n):
    """(tag, indices of the bodies active in the first block step): |A| in {1, 4, 5, n - 1, n}, first / last / strided"""
    out = []
    for k in sorted({1, 4, 5, n - 1, n}):
        if not 1 <= k <= n:
            continue
        out.append((f"{k} first", np.arange(k)))
        if k < n:
            out.append((f"{k} last", np.arange(n - k, n)))
            stride = max(1, n // k)
            out.append((f"{k} strided", (np.arange(k) * stride) % n))
    return out


@pytest.mark.parametrize("precision", ["fp32", "extended"])
@pytest.mark.parametrize("n", [5, 257, 1025])
def test_forced_active_sets(nb, ctx, n, precision):
    ic = _general_masses(nb.ic.plummer(n, seed=42))
    fc = _direct(nb, G, 0.05)
    L = 3
    for tag, active in _forced_sets(n):
        assert len(set(active.tolist())) == len(active)
        levels = np.full(n, L - 1, np.int32)  # first correction at tick 2 ...
        levels[active] = L                    # ... and these at tick 1: the first block step corrects exactly them
        snaps = []
        for scheduling in ("reference", "resident"):
            d, _ = to_device(nb, ic)
            b = _integ(nb, scheduling, precision, max_level=L)
            b.prime(d, fc, DT)
            b.setLevels(levels)
            b.block_step(d, fc, DT, 1)
            first = _snap(d, b)
            b.advance(d, fc, DT, 1)  # finishes the macro step
            snaps.append((first, _snap(d, b)))
        (r1, r2), (g1, g2) = snaps
        assert r1["info"]["last_n_active"] == len(active) and r1["info"]["current_tick"] == 1, tag
        assert np.array_equal(np.flatnonzero(r1["ticks"] == 1), np.sort(active)), tag
        _assert_equal((n, tag, "first block step"), g1, r1)
        _assert_equal((n, tag, "macro step"), g2, r2)
        assert g2["info"]["macro_steps"] == 1 and g2["info"]["current_tick"] == 0 and g2["launches"] == (0, 0), tag


# ---- 3. level traffic --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("max_level", [br.BINARY["L"], 2], ids=["deep", "floor"])
def test_binary_level_traffic(nb, ctx, max_level):
    c = br.BINARY
    ic = _ic_of(*br.binary_case())
    fc = _direct(nb, 1.0, c["eps"])
    snaps = []
    for scheduling in ("reference", "resident"):
        d, _ = to_device(nb, ic)
        b = _integ(nb, scheduling, max_level=max_level)
        b.advance(d, fc, c["T"] / c["macro"], c["macro"])
        snaps.append(_snap(d, b))
    ref, got = snaps
    populated = [k for k, v in enumerate(ref["info"]["level_steps"]) if v]
    print(f"binary, max_level {max_level}: levels {populated}, {ref['info']['block_steps']} block steps, "
          f"{ref['info']['floor_hits']} floor hits")
    # the run exercises what it is here for (asserted on the reference's own counters)
    if max_level == 2:
        assert ref["info"]["floor_hits"] > 0 and sum(ref["info"]["level_steps"][3:]) == 0
    else:
        assert len(populated) >= 6 and ref["info"]["floor_hits"] == 0
    assert ref["info"]["macro_steps"] == c["macro"]
    _assert_equal(("binary", max_level), got, ref)
    assert got["launches"] == (0, 0)


# ---- 4. step semantics -------------------------------------------------------------------------------------------------
def test_block_step_by_block_step(nb, ctx):
    n, L = 257, 5
    ic = _general_masses(nb.ic.plummer(n, seed=42))
    fc = _direct(nb, G, 0.05)
    # the reference, one block step at a time
    dr, _ = to_device(nb, ic)
    r = _integ(nb, "reference", max_level=L)
    ref_steps = []
    while True:
        r.block_step(dr, fc, DT, 1)
        ref_steps.append(_snap(dr, r))
        if ref_steps[-1]["info"]["current_tick"] == 0:
            break
    assert len(ref_steps) >= 3 and ref_steps[0]["info"]["current_tick"] != 0
    # resident, one block step at a time: the state in the middle of the macro step is the reference's
    d1, _ = to_device(nb, ic)
    b1 = _integ(nb, "resident", max_level=L)
    for k, ref in enumerate(ref_steps):
        b1.block_step(d1, fc, DT, 1)
        _assert_equal(("block step", k), _snap(d1, b1), ref)
    assert b1.info()["current_tick"] == 0 and b1.info()["macro_steps"] == 1
    # ... which is advance(1)
    d2, _ = to_device(nb, ic)
    b2 = _integ(nb, "resident", max_level=L)
    b2.advance(d2, fc, DT, 1)
    _assert_equal("advance(1)", _snap(d2, b2), ref_steps[-1])
    # a budget of several block steps; one larger than the remainder stops at the boundary
    d3, _ = to_device(nb, ic)
    b3 = _integ(nb, "resident", max_level=L)
    b3.block_step(d3, fc, DT, 2)
    _assert_equal("block_step(2)", _snap(d3, b3), ref_steps[1])
    b3.block_step(d3, fc, DT, 10 ** 6)
    _assert_equal("block_step(10^6)", _snap(d3, b3), ref_steps[-1])
    assert b3.info()["macro_steps"] == 1 and b3.info()["block_steps"] == len(ref_steps)


# ---- 5. switching forms at a boundary ----------------------------------------------------------------------------------
def test_switch_at_a_macro_boundary(nb, ctx):
    ic, ref = _reference(nb, 257, 0.05, "fp32")
    fc = _direct(nb, G, 0.05)
    d, _ = to_device(nb, ic)
    b = _integ(nb, "reference")
    b.advance(d, fc, DT, 1)
    assert b.getScheduling() == ("host", "host")
    b.setScheduling("resident")
    b.advance(d, fc, DT, 1)
    got = _snap(d, b)
    assert got["info"]["macro_steps"] == 2  # (not primed again)
    _assert_equal("host then resident", got, ref)
    assert b.getScheduling() == ("resident", "resident")
    assert 0 < sum(got["launches"]) < got["info"]["block_steps"]
    # and back: resident, then host
    d2, _ = to_device(nb, ic)
    b2 = _integ(nb, "resident")
    b2.setTuning(ALWAYS_NARROW)
    b2.advance(d2, fc, DT, 1)
    b2.setScheduling("host")
    b2.advance(d2, fc, DT, 1)
    _assert_equal("resident then host", _snap(d2, b2), ref)


# ---- 6. capture --------------------------------------------------------------------------------------------------------
def test_resident_macro_step_in_a_step_graph(nb, ctx):
    ic, ref = _reference(nb, 257, 0.05, "fp32", macro=4)
    fc = _direct(nb, G, 0.05)
    d, _ = to_device(nb, ic)
    b = _integ(nb, "resident")
    b.advance(d, fc, DT, 1)  # eagerly first
    with ctx.capture() as rec:
        b.advance(d, fc, DT, 1)  # (7. no hidden read: a call that read from the device could not be recorded)
    assert b.getScheduling() == ("resident", "resident")
    rec.graph.launch(3)
    got = _snap(d, b)
    _assert_equal("1 eager + 3 replayed", got, ref)
    assert got["info"]["macro_steps"] == 4 and got["launches"] == (0, 0)
    rec.graph.close()
    # an unprimed handle, a handle that has not run yet, and the host form cannot be recorded
    d2, _ = to_device(nb, ic)
    b2 = _integ(nb, "resident")
    b2.prime(d2, fc, DT)
    with pytest.raises(nb.StateException, match="step graph"):
        with ctx.capture():
            b2.advance(d2, fc, DT, 1)
    b2.invalidate()
    with pytest.raises(nb.StateException, match="cannot be recorded into a step graph"):
        with ctx.capture():
            b2.advance(d2, fc, DT, 1)
    b2.advance(d2, fc, DT, 1)
    b2.setScheduling("host")
    with pytest.raises(nb.StateException, match="cannot be recorded into a step graph"):
        with ctx.capture():
            b2.advance(d2, fc, DT, 1)


# ---- 7. automatic choice -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [256, 4096])
def test_automatic_choice_follows_the_crossover(nb, ctx, n):
    from nbody_amd import api
    ic, ref = _reference(nb, n, 0.05, "fp32")
    d, _ = to_device(nb, ic)
    b = _integ(nb, "auto")
    b.setTuning(ALWAYS_NARROW)
    assert b.getScheduling() == ("auto", None)
    b.advance(d, _direct(nb, G, 0.05), DT, 2)
    resident = n < api.HERMITE_BLOCK_RESIDENT_BELOW and n <= api.HERMITE_BLOCK_RESIDENT_MAX
    assert b.getScheduling() == ("auto", "resident" if resident else "host")
    got = _snap(d, b)
    _assert_equal(("auto", n), got, ref)
    assert (got["launches"] == (0, 0)) == resident


# ---- 8. refusals -------------------------------------------------------------------------------------------------------
def test_refusals(nb, ctx):
    from nbody_amd import api
    fc = _direct(nb, G, 0.05)
    # more bodies than the resident form takes
    big, _ = to_device(nb, nb.ic.plummer(api.HERMITE_BLOCK_RESIDENT_MAX + 1, seed=1))
    b = _integ(nb, "resident")
    with pytest.raises(nb.ValidationException, match=str(api.HERMITE_BLOCK_RESIDENT_MAX)):
        b.advance(big, fc, DT, 1)
    with pytest.raises(nb.ValidationException, match=str(api.HERMITE_BLOCK_RESIDENT_MAX)):
        b.block_step(big, fc, DT, 1)
    # a mode outside 0..2 at the C ABI
    lib = nb._lib.load()
    for bad in (-1, 3):
        assert lib.nbody_hip_hermite_block_set_scheduling(b._h, bad) == nb._lib.ERR_VALIDATION
    assert b.getScheduling() == ("resident", None)
    # in the middle of a resident macro step: no switch, no other dt_max; the state stays
    ic = _general_masses(nb.ic.plummer(300, seed=42))
    d, _ = to_device(nb, ic)
    b = _integ(nb, "resident", max_level=8)
    b.block_step(d, fc, DT, 1)
    assert b.info()["current_tick"] != 0
    mid = _snap(d, b)
    with pytest.raises(nb.StateException, match="middle of a macro step"):
        b.setScheduling("host")
    with pytest.raises(nb.StateException, match="changed in the middle of a macro step"):
        b.block_step(d, fc, DT / 2, 1)
    with pytest.raises(nb.StateException, match="changed in the middle of a macro step"):
        b.advance(d, fc, DT / 2, 1)
    with pytest.raises(nb.StateException, match="only be set at tick 0"):
        b.setLevels(np.zeros(300, np.int32))
    assert b.getScheduling()[0] == "resident"
    _assert_equal("after the refusals", _snap(d, b), mid)
    b.advance(d, fc, DT, 1)
    assert b.info()["current_tick"] == 0 and b.info()["macro_steps"] == 1
    b.setScheduling("host")  # at the boundary it goes through


# ---- 9. hosts ----------------------------------------------------------------------------------------------------------
def _system(nb, ic, scheduling=None):
    ps = nb.ParticleSystem()
    ps.setIntegrationScheme("hermite4-block")
    if scheduling is not None:
        ps.setHermiteBlockScheduling(scheduling)
    cfg = nb.SimulationConfig(particle_count=ic["mass"].size, force_method=nb.ForceMethod.DIRECT_N2, dt=DT, G=G,
                              softening=0.05)
    ps.initialize(cfg, ic)
    return ps


def test_particle_system_resident(nb, ctx):
    ic, ref = _reference(nb, 257, 0.05, "fp32")
    ps = _system(nb, ic, "resident")
    assert ps.getHermiteBlockScheduling() == "resident"
    ps.update(DT)
    ps.update(DT)
    got = _snap(ps.getDeviceData(), ps.hermite_block_)
    _assert_equal("ParticleSystem, resident", got, ref)
    assert got["launches"] == (0, 0) and ps.hermite_block_.getScheduling() == ("resident", "resident")
    # a switch between two update() calls goes through (every update ends at a macro boundary)
    ps.setHermiteBlockScheduling("host")
    ps.update(DT)
    assert ps.hermite_block_.getScheduling() == ("host", "host") and ps.hermite_block_.info()["macro_steps"] == 3


def test_default_system_keeps_the_host_form(nb, ctx):
    ic = _general_masses(nb.ic.plummer(257, seed=42))
    ps = _system(nb, ic)
    assert ps.getHermiteBlockScheduling() == "host"
    ps.update(DT)
    ps.update(DT)
    d, _ = to_device(nb, ic)
    alone = nb.BlockHermiteIntegrator()
    alone.advance(d, _direct(nb, G, 0.05), DT, 2)
    assert alone.getScheduling() == ("host", "host") and ps.hermite_block_.getScheduling() == ("host", "host")
    _assert_equal("default system", _snap(ps.getDeviceData(), ps.hermite_block_), _snap(d, alone))
    assert sum(_snap(d, alone)["launches"]) == alone.info()["block_steps"]


def test_facade_resident_program(nb, ctx):
    exe = os.path.join(ROOT, "n-body_amd", "lib", "hermite_block_resident_tests")
    assert os.path.exists(exe), "build with __graft_entry__.build()"
    env = dict(os.environ)
    env["LD_LIBRARY_PATH"] = os.path.dirname(exe) + os.pathsep + env.get("LD_LIBRARY_PATH", "")
    r = subprocess.run([exe], cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    print(r.stdout)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    h = subprocess.run([exe, "hash"], cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert h.returncode == 0, h.stdout[-3000:] + h.stderr[-2000:]
    got = re.findall(r"^hermite_block_resident fnv (\S+)$", h.stdout, re.M)
    assert len(got) == 1 and got == re.findall(r"^hermite_block_resident fnv (\S+)$", r.stdout, re.M)
    # the same two resident macro steps through the Python host: the same bits
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
    blk = _integ(nb, "resident")
    blk.integrate(d, fc, 1.0 / 64)
    blk.advance(d, fc, 1.0 / 64, 1)
    fnv = 1469598103934665603
    for k in F[:6]:
        for byte in getattr(d, k).cpu().numpy().tobytes():
            fnv = ((fnv ^ byte) * 1099511628211) & 0xFFFFFFFFFFFFFFFF
    assert got[0] == f"{fnv:016x}"

"""The block-step Hermite ENSEMBLE (nbody_hip_hermite_batch_*, BlockHermiteEnsemble) on a real GPU.

The oracle is bit equality: system s of an ensemble run against the "reference", a single-system BlockHermiteIntegrator in
"resident" scheduling on that system's bodies alone, with the same parameters and number of macro steps.  "Snapshot" is
the _snap set of tests/test_hermite_block_resident_gpu.py cut to the system: the 13 arrays of the particle data, jerk,
levels, ticks, want, X / V in extended precision, and the counters.  Every comparison is for equality of the bits.
G = 1.7, Plummer spheres with general masses and two macro steps unless a test says otherwise."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import hermite_batch_cases as bc
import hermite_block_ref as br
import hermite_handle_cases as hc
from gpu_util import to_device

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = ("pos_x", "pos_y", "pos_z", "vel_x", "vel_y", "vel_z", "acc_x", "acc_y", "acc_z", "acc_old_x", "acc_old_y", "acc_old_z",
     "mass")
COUNTERS = ("block_steps", "body_steps", "level_steps", "floor_hits", "macro_steps", "current_tick", "last_n_active",
            "max_level")
G, DT = 1.7, 1.0 / 16
# (state precision, eps): the packed pair body in fp32, the guarded one (eps^2 < 1e-12) on the extended state
FORMS = [("fp32", 0.05), ("extended", 0.0)]
FORM_IDS = ["fp32-packed", "extended-guard"]


def _plummer(nb, n, seed=42):
    ic = dict(nb.ic.plummer(n, seed=seed))
    ic["mass"] = (ic["mass"] * np.random.default_rng(5 + seed).uniform(0.5, 2.0, ic["mass"].size)).astype(np.float32)
    return ic


def _direct(nb, g, eps):
    c = nb.DirectForceCalculator()
    c.setGravitationalConstant(g)
    c.setSofteningParameter(eps)
    return c


def _snap_one(d, integ):
    """the snapshot of a single-system integrator"""
    out = {k: getattr(d, k).cpu().numpy().view(np.uint32).copy() for k in F}
    st = integ.getState()
    out.update(jerk=st["jerk"].view(np.uint32).copy(), levels=st["levels"].copy(), ticks=st["ticks"].copy(),
               want=st["want"].view(np.uint32).copy())
    if integ.getStatePrecision() == "extended":
        x, v = integ.getExtendedState(d)
        out.update(X=x.view(np.uint64).copy(), V=v.view(np.uint64).copy())
    info = integ.info()
    out["info"] = {k: info[k] for k in COUNTERS}
    assert (info["narrow_launches"], info["wide_launches"]) == (0, 0)  # (the reference ran the resident form only)
    return out


def _snaps(d, ens, offsets):
    """the snapshots of all systems of an ensemble, cut from one read-out"""
    whole = {k: getattr(d, k).cpu().numpy().view(np.uint32) for k in F}
    st = ens.getState()
    whole.update(jerk=st["jerk"].view(np.uint32), levels=st["levels"], ticks=st["ticks"], want=st["want"].view(np.uint32))
    if ens.getStatePrecision() == "extended":
        x, v = ens.getExtendedState(d)
        whole.update(X=x.view(np.uint64), V=v.view(np.uint64))
    out = []
    for s in range(len(offsets) - 1):
        a, b = int(offsets[s]), int(offsets[s + 1])
        one = {k: v[a:b].copy() for k, v in whole.items()}
        info = ens.info(s)
        one["info"] = {k: info[k] for k in COUNTERS}
        assert (info["narrow_launches"], info["wide_launches"], info["narrow_below"]) == (0, 0, 0)
        out.append(one)
    return out


def _assert_equal(tag, got, ref):
    assert got.keys() == ref.keys(), tag
    for k in ref:
        if k == "info":
            assert got[k] == ref[k], (tag, got[k], ref[k])
        else:
            assert got[k].shape == ref[k].shape, (tag, k)
            bad = np.flatnonzero((got[k] != ref[k]).reshape(len(ref[k]), -1).any(axis=1))
            assert bad.size == 0, (tag, k, f"{bad.size} bodies differ, first {bad[:5]}")


_REF = {}


def _reference(nb, key, ic, eps, precision, dt=DT, macro=2, max_level=16, g=G):
    """the reference run of one system, computed once per (key, parameters) and shared; macro = 0: primed only"""
    key = (key, eps, precision, float(np.float32(dt)), macro, max_level, g)
    if key not in _REF:
        d, _ = to_device(nb, ic)
        b = nb.BlockHermiteIntegrator()
        b.setParameters(0.02, 0.01, max_level)
        b.setStatePrecision(precision)
        b.setScheduling("resident")
        fc = _direct(nb, g, eps)
        if macro:
            b.advance(d, fc, dt, macro)
        else:
            b.prime(d, fc, dt)
        _REF[key] = _snap_one(d, b)
        b.close()
    return _REF[key]


def _ensemble(nb, ics, eps, precision, dt=DT, max_level=16, g=G):
    """-> (d, ens, offsets), primed"""
    ic, offsets = nb.ic.concat(ics)
    d, _ = to_device(nb, ic)
    ens = nb.BlockHermiteEnsemble()
    ens.setParameters(0.02, 0.01, max_level)
    ens.setStatePrecision(precision)
    ens.setLayout(offsets)
    ens.prime(d, _direct(nb, g, eps), dt)
    return d, ens, offsets


# ---- 1. priming --------------------------------------------------------------------------------------------------------
# no partner; the packed pair; inside one target block; the tile edge 255 / 256 / 257 (two tiles); the target-block edge
# 513; 1025: a second 1,024-source block holding one body
PRIME_SIZES = [1, 2, 5, 255, 256, 257, 513, 1025]


@pytest.mark.parametrize("precision,eps", FORMS, ids=FORM_IDS)
def test_priming_equals_the_single_system_priming(nb, ctx, precision, eps):
    ics = [_plummer(nb, n) for n in PRIME_SIZES]
    d, ens, off = _ensemble(nb, ics, eps, precision)
    got = _snaps(d, ens, off)
    for s, n in enumerate(PRIME_SIZES):
        ref = _reference(nb, ("plummer", n, 42), ics[s], eps, precision, macro=0)
        _assert_equal(("prime", n, precision), got[s], ref)  # acc, jerk, want, levels, ticks -- and everything else
        assert not got[s]["ticks"].any() and got[s]["info"]["block_steps"] == 0
    if eps > 0:
        assert np.isinf(got[0]["want"].view(np.float32)).all()  # (n = 1: |j| = 0)


# ---- 2. one system -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision,eps", FORMS, ids=FORM_IDS)
@pytest.mark.parametrize("n", [1, 5, 257, 1025, 4096])
def test_one_system(nb, ctx, n, precision, eps):
    ic = _plummer(nb, n)
    ref = _reference(nb, ("plummer", n, 42), ic, eps, precision)
    d, ens, off = _ensemble(nb, [ic], eps, precision)
    ens.advance(d, 2)
    got = _snaps(d, ens, off)[0]
    print(f"n {n} {precision}: {got['info']['block_steps']} block steps, {got['info']['body_steps']} body steps")
    _assert_equal((n, precision), got, ref)
    assert got["info"]["macro_steps"] == 2 and got["info"]["current_tick"] == 0


# ---- 3. mixed sizes, offsets that are no multiples of 4, 64 or 256; the order of the systems -----------------------------
MIXED = [3, 257, 5, 1025, 64, 1]


@pytest.mark.parametrize("precision,eps", FORMS, ids=FORM_IDS)
def test_mixed_sizes_and_their_order(nb, ctx, precision, eps):
    ics = [_plummer(nb, n, seed=100 + k) for k, n in enumerate(MIXED)]
    refs = [_reference(nb, ("plummer", n, 100 + k), ics[k], eps, precision) for k, n in enumerate(MIXED)]
    d, ens, off = _ensemble(nb, ics, eps, precision)
    assert [int(o) for o in off] == [0, 3, 260, 265, 1290, 1354, 1355]
    ens.advance(d, 2)
    for k, got in enumerate(_snaps(d, ens, off)):
        _assert_equal(("mixed", k, MIXED[k], precision), got, refs[k])
    d2, ens2, off2 = _ensemble(nb, ics[::-1], eps, precision)
    ens2.advance(d2, 2)
    for k, got in enumerate(_snaps(d2, ens2, off2)):
        _assert_equal(("reversed", k, precision), got, refs[len(MIXED) - 1 - k])


# ---- 4. dt_max per system ----------------------------------------------------------------------------------------------
def test_dt_max_per_system(nb, ctx):
    ic = _plummer(nb, 16)
    dts = [1.0 / 16, 1.0 / 32, 1.0 / 8, 1.0 / 16]
    d, ens, off = _ensemble(nb, [ic] * 4, 0.05, "fp32", dt=np.array(dts, np.float32))
    ens.advance(d, 2)
    got = _snaps(d, ens, off)
    for k, dt in enumerate(dts):
        _assert_equal(("dt_max", k, dt), got[k], _reference(nb, ("plummer", 16, 42), ic, 0.05, "fp32", dt=dt))
    _assert_equal("copies 0 and 3", got[0], got[3])
    assert any((got[0][k] != got[1][k]).any() for k in ("pos_x", "vel_x"))  # (another dt_max is another run)


# ---- 5. more workgroups than compute units -----------------------------------------------------------------------------
def test_more_systems_than_compute_units(nb, ctx):
    c = bc.TRIPLE
    ics = bc.triples(c["systems"])
    assert len(ics) == 300
    d, ens, off = _ensemble(nb, ics, c["eps"], "fp32", dt=c["dt_max"], max_level=c["max_level"], g=c["G"])
    ens.advance(d, 2)
    got = _snaps(d, ens, off)
    for s, ic in enumerate(ics):
        ref = _reference(nb, ("triple", s), ic, c["eps"], "fp32", dt=c["dt_max"], max_level=c["max_level"], g=c["G"])
        _assert_equal(("triple", s), got[s], ref)
    # the schedules differ from system to system (checked on the inputs with tests/hermite_block_ref.py before the seed
    # was fixed: tests/test_hermite_batch_cpu.py): the case is not 300 times the same schedule
    steps = sorted({g["info"]["block_steps"] for g in got})
    print(f"block steps per system: {steps}")
    assert len(steps) >= 2
    total = ens.info()
    for k in ("block_steps", "body_steps", "floor_hits", "macro_steps"):
        assert total[k] == sum(g["info"][k] for g in got), k
    assert total["level_steps"] == [sum(g["info"]["level_steps"][lv] for g in got) for lv in range(21)]
    assert total["macro_steps"] == 600 and total["current_tick"] == 0 and total["last_n_active"] == 0
    assert (total["narrow_launches"], total["wide_launches"], total["narrow_below"]) == (0, 0, 0)


# ---- 6. the macro-step loop inside the launch --------------------------------------------------------------------------
def test_macro_steps_inside_one_launch(nb, ctx):
    ics = [_plummer(nb, n, seed=100 + k) for k, n in enumerate([257, 5])]
    refs = [_reference(nb, ("plummer", n, 100 + k), ics[k], 0.05, "fp32", macro=4) for k, n in enumerate([257, 5])]
    d, ens, off = _ensemble(nb, ics, 0.05, "fp32")
    ens.advance(d, 4)
    one = _snaps(d, ens, off)
    d2, ens2, off2 = _ensemble(nb, ics, 0.05, "fp32")
    for _ in range(4):
        ens2.advance(d2, 1)
    four = _snaps(d2, ens2, off2)
    for k in range(2):
        _assert_equal(("advance(4)", k), one[k], refs[k])
        _assert_equal(("4 x advance(1)", k), four[k], refs[k])
        assert one[k]["info"]["macro_steps"] == 4


# ---- 7. step graph -----------------------------------------------------------------------------------------------------
def test_advance_in_a_step_graph(nb, ctx):
    """One eager advance(1), one more recorded and replayed three times.  Recording runs nothing in this library (the
    recorded launch executes only at the replays: tests/test_hermite_block_resident_gpu.py counts the same way), so the
    replays leave the ensemble at FOUR macro steps; one further eager advance(1) takes it to the five macro steps of the
    reference, which also shows that an eager call continues a replayed one."""
    ics = [_plummer(nb, n, seed=100 + k) for k, n in enumerate([257, 5])]
    d, ens, off = _ensemble(nb, ics, 0.05, "fp32")
    ens.advance(d, 1)  # eagerly first
    with ctx.capture() as rec:
        ens.advance(d, 1)  # (no hidden read: a call that read from the device could not be recorded)
    rec.graph.launch(3)
    for k, got in enumerate(_snaps(d, ens, off)):
        _assert_equal(("1 eager + 3 replayed", k), got,
                      _reference(nb, ("plummer", [257, 5][k], 100 + k), ics[k], 0.05, "fp32", macro=4))
    ens.advance(d, 1)
    for k, got in enumerate(_snaps(d, ens, off)):
        _assert_equal(("... + 1 eager", k), got,
                      _reference(nb, ("plummer", [257, 5][k], 100 + k), ics[k], 0.05, "fp32", macro=5))
        assert got["info"]["macro_steps"] == 5
    rec.graph.close()
    # a handle that has not run eagerly since its priming cannot be recorded
    d2, ens2, _ = _ensemble(nb, ics, 0.05, "fp32")
    with pytest.raises(nb.StateException, match="step graph"):
        with ctx.capture():
            ens2.advance(d2, 1)
    ens2.advance(d2, 1)  # (and the refusal left it usable)
    assert ens2.info()["macro_steps"] == 2


# ---- 8. floor hits -----------------------------------------------------------------------------------------------------
def test_floor_hits(nb, ctx):
    """the e = 0.9 binary of tests/hermite_block_ref.py with max_level = 4, over the EIGHT macro steps of period / 16 that
    take it to pericentre (two would not reach the floor: 0 floor hits in the restatement, 32 after eight)"""
    c = br.BINARY
    ic = bc.ic_of(*br.binary_case())
    dt, macro = c["T"] / c["macro"], 8
    ref = _reference(nb, "binary", ic, c["eps"], "fp32", dt=dt, macro=macro, max_level=4, g=1.0)
    d, ens, off = _ensemble(nb, [ic], c["eps"], "fp32", dt=dt, max_level=4, g=1.0)
    ens.advance(d, macro)
    got = _snaps(d, ens, off)[0]
    print(f"floor hits {got['info']['floor_hits']}, levels {[k for k, v in enumerate(got['info']['level_steps']) if v]}")
    assert got["info"]["floor_hits"] > 0 and sum(got["info"]["level_steps"][5:]) == 0
    _assert_equal("floor", got, ref)


# ---- 9. errors ---------------------------------------------------------------------------------------------------------
def test_refusals(nb, ctx):
    ic = _plummer(nb, 16)
    fc = _direct(nb, G, 0.05)
    d, _ = to_device(nb, ic)

    def fresh(offsets):
        e = nb.BlockHermiteEnsemble()
        e.setLayout(offsets)
        return e

    # the rules of a layout: ERR_VALIDATION, the message names the system
    for offsets, what in (([0, 8, 8, 16], "system 1 has 0 bodies"), ([0, 4097], "system 0 has 4097 bodies"),
                          ([0, 12, 8, 16], "strictly ascending: system 1"), ([1, 16], r"offsets\[0\] must be 0")):
        with pytest.raises(nb.ValidationException, match=what):
            fresh(offsets).prime(d, fc, DT)
    # more systems than the handle was made for, at the C ABI (the Python host sizes its handle by the layout)
    lib = nb._lib.load()
    h = C.c_void_p()
    nb._lib.check(lib.nbody_hip_hermite_batch_create(ctx.handle, 16, 2, C.byref(h)))
    three = np.array([0, 4, 8, 16], np.uint64)
    assert lib.nbody_hip_hermite_batch_set_layout(h, three.ctypes.data, 3) == nb._lib.ERR_VALIDATION
    assert b"number of systems must be in [1, 2], got 3" in lib.nbody_hip_last_error()
    s = d.struct()
    assert lib.nbody_hip_hermite_batch_advance(h, C.byref(s), 1) == nb._lib.ERR_STATE  # (and nothing was laid out)
    assert b"not primed" in lib.nbody_hip_last_error()
    lib.nbody_hip_hermite_batch_destroy(h)
    # the count at prime
    with pytest.raises(nb.ValidationException, match="particle count 16 differs from the layout's 12 bodies"):
        fresh([0, 4, 12]).prime(d, fc, DT)
    # advance unprimed; a layout after the priming unprimes
    e = fresh([0, 4, 16])
    with pytest.raises(nb.StateException, match="not primed"):
        e.advance(d, 1)
    assert not d.acc_x.cpu().numpy().any()  # (no refusal so far reached a launch: the priming would have written acc)
    e.prime(d, fc, DT)
    primed = {k: getattr(d, k).cpu().numpy().copy() for k in F}
    e.setLayout([0, 10, 16])
    with pytest.raises(nb.StateException, match="not primed"):
        e.advance(d, 1)
    # dt_max, with the existing wordings
    with pytest.raises(nb.ValidationException, match="Time step must be positive"):
        e.prime(d, fc, [DT, 0.0])
    with pytest.raises(nb.ValidationException, match="Time step must be a finite number"):
        e.prime(d, fc, float("inf"))
    # Direct only
    with pytest.raises(ValueError, match="Direct-only"):
        e.prime(d, nb.BarnesHutCalculator(), DT)
    # none of these reached a launch: the arrays are as the one priming left them, and the handle still primes and runs
    assert all(np.array_equal(getattr(d, k).cpu().numpy(), primed[k]) for k in F)
    assert all(np.array_equal(primed[k], np.asarray(ic[k], np.float32)) for k in F[:6])
    e.prime(d, fc, DT)
    e.advance(d, 1)
    assert e.info()["macro_steps"] == 2 and e.info(1)["macro_steps"] == 1


def test_handle_refusals_at_the_c_abi(nb, ctx):
    """null state arrays, a count above the capacity, the precision read back, the three parameter checks
    (tests/hermite_handle_cases.py), on systems of 3 and 5 bodies"""
    d, _ = to_device(nb, _plummer(nb, 8))
    hc.raw_refusals(nb, ctx, d, "batch_", "ensemble's", layout=[0, 3, 8])


# ---- 10. both hosts ----------------------------------------------------------------------------------------------------
def test_facade_program(nb, ctx):
    exe = os.path.join(ROOT, "n-body_amd", "lib", "hermite_batch_tests")
    assert os.path.exists(exe), "build with __graft_entry__.build()"
    env = dict(os.environ)
    env["LD_LIBRARY_PATH"] = os.path.dirname(exe) + os.pathsep + env.get("LD_LIBRARY_PATH", "")
    r = subprocess.run([exe], cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    print(r.stdout)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    h = subprocess.run([exe, "hash"], cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert h.returncode == 0, h.stdout[-3000:] + h.stderr[-2000:]
    got = re.findall(r"^hermite_batch fnv (\S+)$", h.stdout, re.M)
    assert len(got) == 1 and got == re.findall(r"^hermite_batch fnv (\S+)$", r.stdout, re.M)
    # the same ensemble through the Python host: the same bits
    n = 300
    hst = nb.ParticleData()
    nb.ParticleDataManager.allocateHost(hst, n)
    nb.ParticleInitializer.initUniform(hst, nb.UniformDistParams((-1, -1, -1), (1, 1, 1), 0.5, 1.5), 7)
    hst.vel_x[:] = np.float32(0.1) * hst.pos_y
    hst.vel_y[:] = np.float32(-0.1) * hst.pos_x
    d = nb.ParticleData()
    nb.ParticleDataManager.allocateDevice(d, n)
    nb.ParticleDataManager.copyToDevice(d, hst)
    ens = nb.BlockHermiteEnsemble()
    ens.setLayout([0, 3, 260, 300])
    ens.prime(d, _direct(nb, float(np.float32(1.7)), float(np.float32(0.05))), 1.0 / 64)
    ens.advance(d, 2)
    fnv = 1469598103934665603
    for k in F[:6]:
        for byte in getattr(d, k).cpu().numpy().tobytes():
            fnv = ((fnv ^ byte) * 1099511628211) & 0xFFFFFFFFFFFFFFFF
    assert got[0] == f"{fnv:016x}"

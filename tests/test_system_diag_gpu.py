"""The ensemble diagnostics (nbody_hip_systems_diagnostics, nbody_hip_hermite_batch_diagnostics,
nbody_hip_hermite_block_diagnostics; include/nbody_hip.h and nbody_hip_diag.h) on a real GPU.

Values are held against the fp64 restatement tests/system_diag_ref.py, evaluated on the state get_state_f64 returns, with
DERIVED tolerances: a sum S = sum t_k to (L + 32) 2^-53 sum |t_k| (per component for the vectors), L the longest chain of
fp64 additions a term passes through in the kernel's fixed order -- system_diag_ref.chain_pairs(n) <= n^2 / 512 + 10 for the
pair sum, chain_bodies(n) = ceil(n / 256) + 9 for the per-body sums -- and the 32 for the roundings inside a term, on both
sides; the pair quantities to 64 2^-53 relative (min_sep, bind_energy, bind_a) and 64 2^-53 / e absolute (bind_e).  The
indices are compared wherever the reference's runner-up is at least 1e-9 (relative) away from the winner, which the tests
assert of their inputs.  Everything else is equality of bytes."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import hermite_ref as hr
import system_diag_ref as sr
from gpu_util import to_device

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G, DT = float(np.float32(1.7)), 1.0 / 64     # (the model takes G = (double)G of the fp32 argument)
U53 = 2.0 ** -53
GAP = 1e-9
# (state precision, eps, positions shifted to (64, -32, 16) at scale 0.01)
FORMS = [("fp32", 0.05, False), ("extended", 1e-4, True)]
FORM_IDS = ["fp32", "extended-shifted"]


def _direct(nb, g, eps):
    c = nb.DirectForceCalculator()
    c.setGravitationalConstant(g)
    c.setSofteningParameter(eps)
    return c


def _ensemble(nb, systems, precision, eps, prime=True):
    """-> (d, ens, offsets, fc): the systems back to back, the state set through set_state_f64, primed"""
    pos, vel, m, off = sr.concat64(systems)
    d, _ = to_device(nb, sr.ic32(pos, vel, m))
    ens = nb.BlockHermiteEnsemble()
    ens.setStatePrecision(precision)
    ens.setLayout(off)
    fc = _direct(nb, G, eps)
    ens.setExtendedState(d, pos, vel, fc)
    if prime:
        ens.prime(d, fc, DT)
    return d, ens, off, fc


def _lo_rows(nb, d, X, V):
    """the residual rows {lx, ly, lz, 0} of the state (X, V) over the fp32 arrays of d, as device tensors"""
    out = []
    for full, names in ((X, ("pos_x", "pos_y", "pos_z")), (V, ("vel_x", "vel_y", "vel_z"))):
        hi = np.stack([getattr(d, k).cpu().numpy() for k in names], 1).astype(np.float64)
        lo = np.zeros((len(full), 4), np.float32)
        lo[:, :3] = (full - hi).astype(np.float32)
        assert np.array_equal(hi + lo[:, :3].astype(np.float64), full)   # hi + lo is the state, exactly
        out.append(torch.from_numpy(lo).to(d.pos_x.device))
    return out


def _check_values(tag, got, ref, n):
    """every field of one struct against the reference, each within its bound"""
    lb, lp = sr.chain_bodies(n), sr.chain_pairs(n)
    assert lp <= n * n / 512 + 64
    ab = ref["abs"]
    rows = []

    def close(name, g, r, bound):
        err = float(np.max(np.abs(np.asarray(g, np.float64) - np.asarray(r, np.float64)))) if np.all(np.isfinite(r)) else 0.0
        rows.append(f"{name} err {err:.3e} bound {float(np.min(bound)):.3e}")
        assert np.all(np.abs(np.asarray(g) - np.asarray(r)) <= bound), (tag, name, g, r, bound)

    assert got["mass"] == ref["mass"] and got["n"] == n and got["status"] == 0, (tag, got["mass"], ref["mass"])
    if ref["mass"] != 0:
        close("com", got["com"], ref["com"], sr.sum_bound(lb, ab["mx"]) / abs(ref["mass"]))
    close("momentum", got["momentum"], ref["momentum"], sr.sum_bound(lb, ab["momentum"]))
    close("ang_mom", got["ang_mom"], ref["ang_mom"], sr.sum_bound(lb, ab["ang_mom"]))
    close("kinetic", got["kinetic"], ref["kinetic"], sr.sum_bound(lb, ab["kinetic"]))
    close("potential", got["potential"], ref["potential"], sr.sum_bound(lp, ab["potential"]))
    if n == 1:
        assert np.isposinf(got["min_sep"]) and (got["min_i"], got["min_j"], got["bind_i"], got["bind_j"]) == (-1, -1, -1, -1)
    else:
        assert ref["min_gap"] >= GAP and ref["bind_gap"] >= GAP, (tag, ref["min_gap"], ref["bind_gap"])  # (the inputs)
        assert (got["min_i"], got["min_j"]) == (ref["min_i"], ref["min_j"]), tag
        assert (got["bind_i"], got["bind_j"]) == (ref["bind_i"], ref["bind_j"]), tag
        close("min_sep", got["min_sep"], ref["min_sep"], 64 * U53 * ref["min_sep"])
    close("bind_energy", got["bind_energy"], ref["bind_energy"], 64 * U53 * abs(ref["bind_energy"]))
    close("bind_a", got["bind_a"], ref["bind_a"], 64 * U53 * abs(ref["bind_a"]))
    if ref["bind_i"] >= 0:
        assert ref["bind_e"] > 0
        close("bind_e", got["bind_e"], ref["bind_e"], 64 * U53 / ref["bind_e"])
    else:
        assert got["bind_e"] == 0.0
    print(f"  {tag}: " + "; ".join(rows), flush=True)


# ---- 1. values against fp64 ---------------------------------------------------------------------------------------------
_VALUE = {}


def _value_run(nb, precision, eps, shifted):
    """the value ensemble of one form, its structs and its state, run once and shared (test 4 reads it too)"""
    if precision not in _VALUE:
        systems = sr.value_systems(nb, shifted)
        d, ens, off, _ = _ensemble(nb, systems, precision, eps)
        got = ens.diagnostics(d)
        X, V = ens.getExtendedState(d)
        _VALUE[precision] = dict(d=d, ens=ens, off=off, got=got, X=X, V=V, m=d.mass.cpu().numpy(), eps=eps)
    return _VALUE[precision]


@pytest.mark.parametrize("precision,eps,shifted", FORMS, ids=FORM_IDS)
def test_values_against_fp64(nb, ctx, precision, eps, shifted):
    run = _value_run(nb, precision, eps, shifted)
    off, got, X, V, m = run["off"], run["got"], run["X"], run["V"], run["m"]
    sizes = np.diff(off.astype(np.int64))
    assert list(sizes) == [1, 2, 3, 3, 5, 63, 64, 65, 255, 256, 257, 511, 512, 513, 1025, 4096]
    assert all(int(o) % 4 for o in off[3:-1]) and all(int(o) % 64 for o in off[1:-1])  # (no system starts on a tile edge)
    assert got.dtype == nb.SYSTEM_DIAG_DTYPE and got.shape == (16,)
    hi = np.stack([run["d"].pos_x.cpu().numpy(), run["d"].pos_y.cpu().numpy(), run["d"].pos_z.cpu().numpy()], 1).astype(np.float64)
    if precision == "extended":
        assert np.abs(X - hi).max() > 1e-7      # the residuals are there
    else:
        assert np.array_equal(X, hi)
    for s, n in enumerate(sizes):
        a, b = int(off[s]), int(off[s + 1])
        ref = sr.reference(X[a:b], V[a:b], m[a:b], G, eps)
        _check_values((precision, s, int(n)), got[s], ref, int(n))
        if precision == "extended" and 2 <= n <= 1025:
            # a kernel that drops the residuals fails this test: the PE of the hi parts alone is outside the bound
            dropped = hr.energy(hi[a:b], V[a:b], m[a:b], G, eps)[1]
            assert abs(dropped - ref["potential"]) > 100 * sr.sum_bound(sr.chain_pairs(int(n)), ref["abs"]["potential"]), (s, n)


# ---- 2. independence, bit for bit ---------------------------------------------------------------------------------------
def _one_way(nb, systems, precision, eps, macro):
    d, ens, off, fc = _ensemble(nb, systems, precision, eps)
    if macro:
        ens.advance(d, macro)
    return d, ens, off, fc


@pytest.mark.parametrize("macro", [0, 2], ids=["primed", "advanced"])
def test_a_system_is_a_function_of_its_bodies_only(nb, ctx, macro):
    precision, eps = "extended", 1e-4
    systems = sr.small_systems(nb)
    d, ens, off, fc = _one_way(nb, systems, precision, eps, macro)
    whole = ens.diagnostics(d)
    assert (whole["status"] == 0).all() and list(whole["n"]) == [1, 2, 3, 65, 257]
    # the generic call on the same arrays with the same residual rows
    X, V = ens.getExtendedState(d)
    pos_lo, vel_lo = _lo_rows(nb, d, X, V)
    generic = nb.systems_diagnostics(ctx, d, off, G, eps, pos_lo, vel_lo)
    assert generic.tobytes() == whole.tobytes()
    assert np.abs(pos_lo.cpu().numpy()).max() > 0 or macro == 0
    # the reversed ensemble
    dr, er, offr, _ = _one_way(nb, systems[::-1], precision, eps, macro)
    rev = er.diagnostics(dr)
    for s in range(len(systems)):
        assert rev[len(systems) - 1 - s].tobytes() == whole[s].tobytes(), ("reversed", s)
    for s, one in enumerate(systems):
        # an ensemble of one
        d1, e1, _, _ = _one_way(nb, [one], precision, eps, macro)
        assert e1.diagnostics(d1)[0].tobytes() == whole[s].tobytes(), ("ensemble of one", s)
        # the single-system integrator on that system alone
        pos, vel, m, _ = sr.concat64([one])
        db, _ = to_device(nb, sr.ic32(pos, vel, m))
        b = nb.BlockHermiteIntegrator()
        b.setStatePrecision(precision)
        b.setScheduling("resident")
        b.setExtendedState(db, pos, vel, fc)
        if macro:
            b.advance(db, fc, DT, macro)
        else:
            b.prime(db, fc, DT)
        assert b.diagnostics(db, fc)[0].tobytes() == whole[s].tobytes(), ("block integrator", s)
        b.close()
        e1.close()
    er.close()
    ens.close()


# ---- 3. pair edge cases through the generic call, fp32 state ------------------------------------------------------------
def _generic(nb, ctx, rows, g, eps, offsets=None):
    """rows: [[x, y, z, vx, vy, vz, m], ...] (fp32 values) -> the structs"""
    a = np.asarray(rows, np.float64)
    d, _ = to_device(nb, sr.ic32(a[:, 0:3], a[:, 3:6], a[:, 6]))
    return nb.systems_diagnostics(ctx, d, [0, len(a)] if offsets is None else offsets, g, eps)


def test_pair_edge_cases(nb, ctx):
    one = _generic(nb, ctx, [[1, 2, 3, 0.5, 0.25, 0.125, 2]], 1.0, 0.05)[0]
    assert np.isposinf(one["min_sep"]) and (one["min_i"], one["min_j"], one["bind_i"], one["bind_j"]) == (-1, -1, -1, -1)
    assert one["potential"] == 0 and one["n"] == 1 and one["status"] == 0 and one["mass"] == 2
    assert one["kinetic"] == 0.328125 and list(one["com"]) == [1, 2, 3] and list(one["momentum"]) == [1, 0.5, 0.25]
    # a tie in min_sep goes to the smallest (i, j)
    tie = _generic(nb, ctx, [[0, 0, 0, 0, 0, 0, 1], [1, 0, 0, 0, 3, 0, 1], [0, 1, 0, 3, 0, 0, 1]], 1.0, 0.0)[0]
    assert (tie["min_i"], tie["min_j"], tie["min_sep"]) == (0, 1, 1.0) and tie["bind_i"] == -1
    # a coincident pair, eps = 0: min_sep 0 with that pair, nothing added to PE, skipped for binding (at rest relative to
    # each other it would otherwise be the most bound pair); the third body is unbound
    rows = [[0.5, 0.25, 0, 0, 0, 0, 1], [0.5, 0.25, 0, 0, 0, 0, 2], [4.5, 0.25, 0, 0, 9, 0, 1]]
    co = _generic(nb, ctx, rows, 1.0, 0.0)[0]
    assert (co["min_sep"], co["min_i"], co["min_j"]) == (0.0, 0, 1) and co["bind_i"] == -1 and co["bind_energy"] == 0
    assert co["potential"] == -(1 * 1 / 4.0 + 2 * 1 / 4.0)
    # the same pair with eps > 0 adds -G m m / eps
    ce = _generic(nb, ctx, rows[:2], 1.5, 0.25)[0]
    assert ce["potential"] == -1.5 * 1 * 2 / 0.25 and ce["min_sep"] == 0 and ce["bind_i"] == -1
    # all masses 0
    ml = _generic(nb, ctx, [[1, 0, 0, 0, 1, 0, 0], [-1, 0, 0, 0, -1, 0, 0], [0, 2, 0, 1, 0, 0, 0]], 1.0, 0.0)[0]
    assert list(ml["com"]) == [0, 0, 0] and ml["mass"] == 0 and ml["bind_i"] == -1 and ml["bind_j"] == -1 and ml["min_sep"] == 2
    # a hyperbolic pair only
    hy = _generic(nb, ctx, [[-1, 0, 0, 0, -2, 0, 1], [1, 0, 0, 0, 2, 0, 1]], 1.0, 0.0)[0]
    assert (hy["bind_i"], hy["bind_j"], hy["bind_energy"], hy["bind_a"], hy["bind_e"]) == (-1, -1, 0, 0, 0)
    assert (hy["min_i"], hy["min_j"], hy["min_sep"]) == (0, 1, 2.0)
    # two bound pairs with exactly equal E_b (the second is the first mirrored; every coordinate is representable)
    tw = _generic(nb, ctx, [[64.5, 0, 0, 0, 0.5, 0, 1], [65.5, 0, 0, 0, -0.5, 0, 1], [-64.5, 0, 0, 0, -0.5, 0, 1],
                            [-65.5, 0, 0, 0, 0.5, 0, 1]], 1.0, 0.0)[0]
    assert (tw["bind_i"], tw["bind_j"], tw["bind_energy"]) == (0, 1, -0.75) and (tw["min_i"], tw["min_j"]) == (0, 1)
    assert tw["bind_a"] == 1 / 1.5 and tw["bind_e"] == 0.5
    # ... and the pairs in the other order of bodies give the other pair's indices only through the tie rule
    sw = _generic(nb, ctx, [[-64.5, 0, 0, 0, -0.5, 0, 1], [64.5, 0, 0, 0, 0.5, 0, 1], [-65.5, 0, 0, 0, 0.5, 0, 1],
                            [65.5, 0, 0, 0, -0.5, 0, 1]], 1.0, 0.0)[0]
    assert (sw["bind_i"], sw["bind_j"], sw["bind_energy"]) == (0, 2, -0.75)


# ---- 4. illegal ranges --------------------------------------------------------------------------------------------------
def test_illegal_ranges_are_marked_and_touch_nothing(nb, ctx):
    run = _value_run(nb, *FORMS[0])
    d, off, legal = run["d"], [int(o) for o in run["off"]], run["got"]
    count = off[-1]
    assert count == d.count == 7631
    # after the 16 legal systems: descending, 4,097 bodies, a last offset above count, an empty range
    offsets = off + [0, 4097, count + 1, count + 1]
    out = torch.full((len(offsets) - 1, nb.SYSTEM_DIAG_BYTES), 0xAB, dtype=torch.uint8, device=d.pos_x.device)
    nb.systems_diagnostics_into(ctx, d, offsets, G, run["eps"], out)
    ctx.synchronize()
    got = nb.system_diag_array(out)
    assert got[:16].tobytes() == legal.tobytes()                     # the legal systems: the bytes of test 1
    raw = out.cpu().numpy()
    for s in range(16, 20):
        assert (got[s]["status"], got[s]["n"]) == (1, 0), s
        assert (raw[s, :144] == 0xAB).all()                           # nothing else is written
    # a whole call of illegal ranges, offsets far outside the arrays: nothing is indexed by them
    wild = nb.systems_diagnostics(ctx, d, [2 ** 40, 2 ** 41, 5, 2 ** 62], G, run["eps"])
    assert list(wild["status"]) == [1, 1, 1] and list(wild["n"]) == [0, 0, 0]
    assert nb.systems_diagnostics(ctx, d, [0], G, run["eps"]).shape == (0,)   # no system: nothing to do


# ---- 5. step graph ------------------------------------------------------------------------------------------------------
def test_diagnostics_in_a_step_graph(nb, ctx):
    precision, eps = "extended", 1e-4
    systems = sr.small_systems(nb)
    # eager: four rounds of advance(1) + diagnostics
    d, ens, off, _ = _ensemble(nb, systems, precision, eps)
    out = nb.system_diag_tensor(len(systems), d.pos_x.device)
    for _ in range(4):
        ens.advance(d, 1)
        ens.diagnostics_into(d, out)
    ctx.synchronize()
    eager = nb.system_diag_array(out)
    # one eager round, then the round recorded and replayed three times
    d2, ens2, _, _ = _ensemble(nb, systems, precision, eps)
    out2 = nb.system_diag_tensor(len(systems), d2.pos_x.device)
    ens2.advance(d2, 1)
    ens2.diagnostics_into(d2, out2)
    with ctx.capture() as rec:
        ens2.advance(d2, 1)
        ens2.diagnostics_into(d2, out2)
    rec.graph.launch(3)
    ctx.synchronize()
    replayed = nb.system_diag_array(out2)
    assert replayed.tobytes() == eager.tobytes()
    assert ens2.info()["macro_steps"] == 4 * len(systems)
    # the generic call is capturable from its first call (device offsets: nothing is allocated)
    off_dev = torch.from_numpy(off.astype(np.int64)).to(d2.pos_x.device)
    X, V = ens2.getExtendedState(d2)
    pos_lo, vel_lo = _lo_rows(nb, d2, X, V)
    out3 = nb.system_diag_tensor(len(systems), d2.pos_x.device)
    with ctx.capture() as rec3:
        nb.systems_diagnostics_into(ctx, d2, off_dev, G, eps, out3, pos_lo, vel_lo)
    rec3.graph.launch(1)
    ctx.synchronize()
    assert nb.system_diag_array(out3).tobytes() == eager.tobytes()
    rec.graph.close()
    rec3.graph.close()
    ens.close()
    ens2.close()


# ---- 6. refusals --------------------------------------------------------------------------------------------------------
def test_refusals(nb, ctx):
    lib = nb._lib.load()
    systems = sr.small_systems(nb)[:3]
    pos, vel, m, off = sr.concat64(systems)
    d, _ = to_device(nb, sr.ic32(pos, vel, m))
    s = d.struct()
    dev = d.pos_x.device
    out = nb.system_diag_tensor(3, dev)
    off_dev = torch.from_numpy(off.astype(np.int64)).to(dev)
    h = ctx.handle
    call = lib.nbody_hip_systems_diagnostics
    ST, VAL = nb._lib.ERR_STATE, nb._lib.ERR_VALIDATION
    assert call(None, C.byref(s), None, None, off_dev.data_ptr(), 3, G, 0.1, out.data_ptr()) == ST
    assert call(h, None, None, None, off_dev.data_ptr(), 3, G, 0.1, out.data_ptr()) == ST
    assert call(h, C.byref(s), None, None, None, 3, G, 0.1, out.data_ptr()) == ST
    assert call(h, C.byref(s), None, None, off_dev.data_ptr(), 3, G, 0.1, None) == ST
    assert call(h, C.byref(s), None, None, off_dev.data_ptr(), 3, G, -0.1, out.data_ptr()) == VAL
    assert b"Softening parameter must be non-negative" in lib.nbody_hip_last_error()
    assert call(h, C.byref(s), None, None, off_dev.data_ptr(), 0, G, 0.1, out.data_ptr()) == nb._lib.OK
    ctx.synchronize()
    assert not out.cpu().numpy().any()                                # none of these reached a launch
    with pytest.raises(nb.ValidationException, match="Softening"):
        nb.systems_diagnostics(ctx, d, off, G, -1.0)
    # the ensemble handle: no layout, unprimed, another count
    fc = _direct(nb, G, 0.05)
    raw = C.c_void_p()
    assert lib.nbody_hip_hermite_batch_create(h, 16, 4, C.byref(raw)) == 0
    assert lib.nbody_hip_hermite_batch_diagnostics(None, C.byref(s), out.data_ptr()) == ST
    assert lib.nbody_hip_hermite_batch_diagnostics(raw, None, out.data_ptr()) == ST
    assert lib.nbody_hip_hermite_batch_diagnostics(raw, C.byref(s), None) == ST
    assert lib.nbody_hip_hermite_batch_diagnostics(raw, C.byref(s), out.data_ptr()) == ST
    assert b"no layout" in lib.nbody_hip_last_error()
    lib.nbody_hip_hermite_batch_destroy(raw)
    ens = nb.BlockHermiteEnsemble()
    with pytest.raises(nb.StateException, match="not primed"):
        ens.diagnostics(d)
    ens.setLayout(off)
    ens.setExtendedState(d, pos, vel, fc)          # (a handle with a layout, not primed)
    with pytest.raises(nb.StateException, match="not primed"):
        ens.diagnostics(d)
    ens.prime(d, fc, DT)
    other, _ = to_device(nb, sr.ic32(pos[:5], vel[:5], m[:5]))
    with pytest.raises(nb.StateException, match="differ from the primed ones"):
        ens.diagnostics_into(other, out)
    with pytest.raises(nb.ValidationException, match="out must"):
        ens.diagnostics_into(d, nb.system_diag_tensor(2, dev))
    assert ens.diagnostics(d)["status"].tolist() == [0, 0, 0]          # and it still works
    ens.close()
    # the single-system handle: in the middle of a macro step, above 4,096 bodies
    one = sr.small_systems(nb)[3]
    p1, v1, m1, _ = sr.concat64([one])
    d1, _ = to_device(nb, sr.ic32(p1, v1, m1))
    b = nb.BlockHermiteIntegrator()
    b.prime(d1, fc, 1.0)                           # (a macro step long enough for the bodies to sit on several levels)
    assert b.diagnostics(d1, fc)["n"].tolist() == [65]
    b.block_step(d1, fc, 1.0, 1)
    assert b.info()["current_tick"] != 0
    with pytest.raises(nb.StateException, match="middle of a macro step"):
        b.diagnostics(d1, fc)
    b.advance(d1, fc, 1.0, 1)                      # (to the boundary)
    assert b.diagnostics(d1, fc)["status"].tolist() == [0]
    with pytest.raises(ValueError, match="Direct-only"):
        b.diagnostics(d1, nb.BarnesHutCalculator())
    b.close()
    big = nb.ParticleData()
    nb.ParticleDataManager.allocateDevice(big, 4097)
    b2 = nb.BlockHermiteIntegrator()
    with pytest.raises(nb.ValidationException, match="at most 4096 bodies"):
        b2.diagnostics(big, fc)
    assert lib.nbody_hip_hermite_block_diagnostics(None, C.byref(s), G, 0.1, out.data_ptr()) == ST
    b2.close()


# ---- 7. both hosts ------------------------------------------------------------------------------------------------------
def test_facade_program(nb, ctx):
    exe = os.path.join(ROOT, "n-body_amd", "lib", "system_diag_tests")
    assert os.path.exists(exe), "build with __graft_entry__.build()"
    env = dict(os.environ)
    env["LD_LIBRARY_PATH"] = os.path.dirname(exe) + os.pathsep + env.get("LD_LIBRARY_PATH", "")
    r = subprocess.run([exe], cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    print(r.stdout)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    lines = re.findall(r"^system_diag (\d) (.+)$", r.stdout, re.M)
    assert [int(s) for s, _ in lines] == [0, 1, 2]
    # the same ensemble through the Python host (the recipe of tests/test_hermite_batch_gpu.py): the same bits
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
    got = ens.diagnostics(d)
    for s, (_, text) in enumerate(lines):
        words = np.frombuffer(got[s].tobytes()[:128], np.uint64)   # the 16 doubles come first
        ints = [int(got[s][k]) for k in ("min_i", "min_j", "bind_i", "bind_j", "n", "status")]
        mine = " ".join(f"{int(w):016x}" for w in words) + " " + " ".join(str(v) for v in ints)
        assert text.strip() == mine, s
    ens.close()

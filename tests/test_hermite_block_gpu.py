"""The Hermite integrator with individual block time steps (nbody_hip_hermite_block_*) on a real GPU: level 0 against the
shared-step integrator bit for bit, one block step against the restatement, the active-set edge shapes in both kernel
forms, the schedule and its counters, the two accuracy conditions, refusals, ParticleSystem and the facade.
Restatement: tests/hermite_block_ref.py."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import hermite_block_ref as br
import hermite_handle_cases as hc
import hermite_ref as hr
from gpu_util import rel_err, to_device

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = ("pos_x", "pos_y", "pos_z", "vel_x", "vel_y", "vel_z", "acc_x", "acc_y", "acc_z", "acc_old_x", "acc_old_y", "acc_old_z",
     "mass")
U = hr.U  # 2^-24
# The jerk criterion of DESIGN.md section 4.9 (tests/test_hermite_gpu.py), its held regression tier:
# |dj_i| <= max(1e-5 |j_i|, 1.6 x 11.06 u S_j), S_j the sum of the term magnitudes, 11.06 the largest margin measured
# for the one-sided force-and-jerk kernel on an MI355X.  Both kernel forms here sum fewer fp32 roundings per term than
# that kernel or as many (the narrow form folds into fp64 after 4 sources, the wide one after 256), so the tier holds.
JERK_TIER = 1.6 * 11.06
ALWAYS_WIDE, ALWAYS_NARROW = 1, 1 << 30


def _arrays(ic):
    return (np.stack([ic["pos_x"], ic["pos_y"], ic["pos_z"]], 1), np.stack([ic["vel_x"], ic["vel_y"], ic["vel_z"]], 1),
            ic["mass"])


def _ic_of(pos, vel, m):
    return dict(pos_x=pos[:, 0].copy(), pos_y=pos[:, 1].copy(), pos_z=pos[:, 2].copy(), vel_x=vel[:, 0].copy(),
                vel_y=vel[:, 1].copy(), vel_z=vel[:, 2].copy(), mass=np.asarray(m, np.float32).copy())


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


def _vec(s, name):
    return np.stack([s[name + "_x"], s[name + "_y"], s[name + "_z"]], 1).astype(np.float64)


def _bits(d, integ=None):
    parts = [v.view(np.uint32) for v in _state(d).values()]
    if integ is not None:
        st = integ.getState()
        parts += [st["jerk"].view(np.uint32).ravel(), st["levels"].view(np.uint32), st["ticks"], st["want"].view(np.uint32)]
    return np.concatenate(parts)


def _ref_eval(pos, vel, m, G, eps, targets=None, chunk=256):
    """hermite_ref.acc_jerk in fp64 on the device: (a, j, S_a, S_j) as numpy"""
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


def _criterion(tag, a, j, a_ref, j_ref, sj):
    """a per body within 1e-5; |dj| <= max(1e-5 |j|, 1.6 x 11.06 u S_j)"""
    if len(a) == 0:
        return
    ea = rel_err(a, a_ref)
    err = np.linalg.norm(j - j_ref, axis=1)
    bound = np.maximum(1e-5 * np.linalg.norm(j_ref, axis=1), JERK_TIER * U * sj)
    margin = float((err / np.maximum(U * sj, 1e-300)).max())
    print(f"{tag}: {len(a)} bodies, max |da| / |a| {ea.max():.3e}, max |dj| / |j| {rel_err(j, j_ref).max():.3e}, margin "
          f"max err / (u S_j) {margin:.2f} (held: {JERK_TIER:.2f})", flush=True)
    nz = np.linalg.norm(a_ref, axis=1) > 0
    assert ea[nz].max(initial=0.0) <= 1e-5, (tag, ea.max())
    assert np.all(np.abs(a[~nz]) == 0.0)
    assert np.all(err <= bound), (tag, int(np.argmax(err / np.maximum(bound, 1e-300))))


def _block(nb, eta=0.02, eta_start=0.01, max_level=16, narrow_below=0):
    b = nb.BlockHermiteIntegrator()
    b.setParameters(eta, eta_start, max_level)
    b.setTuning(narrow_below)
    return b


# ---- 1. level 0 is the shared step -------------------------------------------------------------------------------------
@pytest.mark.parametrize("eps", [0.05, 0.0], ids=["packed", "guard"])
@pytest.mark.parametrize("n", [1, 2, 257, 4096, 32768])
def test_level_zero_is_the_shared_step(nb, ctx, n, eps):
    """n = 32768: every body active, the gathered sweep with four targets per lane; one step (10^9 pairs a sweep)"""
    ic = _general_masses(nb.ic.plummer(n, seed=42))
    fc = _direct(nb, 1.7, eps)
    dt = 1.0 / 128
    steps = 1 if n == 32768 else 3
    d0, _ = to_device(nb, ic)
    shared = nb.HermiteIntegrator()
    shared.integrate_steps(d0, fc, dt, steps)
    d1, _ = to_device(nb, ic)
    blk = _block(nb, max_level=0)
    blk.advance(d1, fc, dt, steps)
    s0, s1 = _state(d0), _state(d1)
    for k in F:
        assert np.array_equal(s0[k].view(np.uint32), s1[k].view(np.uint32)), k
    assert np.array_equal(shared.getJerk().cpu().numpy().view(np.uint32), blk.getState()["jerk"].view(np.uint32))
    info = blk.info()
    assert info["block_steps"] == steps and info["body_steps"] == steps * n and info["wide_launches"] == steps
    assert info["narrow_launches"] == 0 and info["macro_steps"] == steps and info["level_steps"][0] == steps * n


# ---- 2. one block step against the restatement -------------------------------------------------------------------------
def _one_step_bits(nb, ic, G, eps, dt_max, L, narrow_below, levels):
    d, _ = to_device(nb, ic)
    fc = _direct(nb, G, eps)
    blk = _block(nb, max_level=L, narrow_below=narrow_below)
    blk.prime(d, fc, dt_max)
    blk.setLevels(levels)
    blk.block_step(d, fc, dt_max, 1)
    return _bits(d, blk)


def _check_one_step(nb, tag, ic, G, eps, dt_max, L, narrow_below=0, levels=None, eta=0.02, ref_cache=None):
    """primes, optionally forces the levels, takes ONE block step and holds it against the restatement seeded with the
    engine's own primed a, j and levels.  ref_cache: a dict that keeps the fp64 sums of ALL bodies at the predicted state
    per tick (the cases of one body set that differ in the levels only share them).  -> (bits after the step, A)"""
    pos, vel, m = _arrays(ic)
    n = len(m)
    d, _ = to_device(nb, ic)
    fc = _direct(nb, G, eps)
    blk = _block(nb, eta=eta, max_level=L, narrow_below=narrow_below)
    blk.prime(d, fc, dt_max)
    s0, st0 = _state(d), blk.getState()
    a0, j0 = _vec(s0, "acc"), st0["jerk"][:, :3].astype(np.float64)
    # priming: the levels and want are the fp64 rule on the engine's own fp32 (a, j), exactly
    lv, want = br.prime_levels(a0, j0, 0.01, dt_max, L)
    assert np.array_equal(lv, st0["levels"]) and np.array_equal(want.astype(np.float32), st0["want"])
    assert not st0["ticks"].any()
    if levels is not None:
        blk.setLevels(levels)
        st0["levels"] = np.asarray(levels, np.int32)
    run = br.BlockHermite(pos, vel, m, G, eps, dt_max, eta=eta, max_level=L, acc=a0, jerk=j0, levels=st0["levels"],
                          evaluate=lambda x, v, t: _ref_eval(x, v, m, G, eps, targets=t)[:2])
    t, A = run.schedule()
    blk.block_step(d, fc, dt_max, 1)
    s1, st1, info = _state(d), blk.getState(), blk.info()
    wrapped = t == 2 ** L
    # the active set and t are identical
    assert info["last_n_active"] == len(A) and info["current_tick"] == (0 if wrapped else t)
    assert info["block_steps"] == 1 and info["body_steps"] == len(A)
    moved = np.flatnonzero(st1["ticks"] != st0["ticks"]) if not wrapped else np.arange(n)
    assert np.array_equal(moved, A)
    assert (st1["ticks"][A] == (0 if wrapped else t)).all()
    # bodies outside A: untouched in all 13 arrays, the jerk, the levels, the ticks and want
    rest = np.setdiff1d(np.arange(n), A)
    for k in F:
        assert np.array_equal(s0[k][rest].view(np.uint32), s1[k][rest].view(np.uint32)), k
    assert np.array_equal(s0["mass"].view(np.uint32), s1["mass"].view(np.uint32))
    for k in ("jerk", "levels", "ticks", "want"):
        assert np.array_equal(st0[k][rest], st1[k][rest], equal_nan=True), k
    # a1, j1 of A against fp64 at the restatement's predicted state
    xp, vp = run.predicted(t)
    if ref_cache is None:
        a_ref, j_ref, _, sj = _ref_eval(xp, vp, m, G, eps, targets=A)
    else:  # (every tick is 0: the predicted state depends on t alone)
        assert not st0["ticks"].any()
        if t not in ref_cache:
            ref_cache[t] = _ref_eval(xp, vp, m, G, eps)
        a_ref, j_ref, _, sj = (r[A] for r in ref_cache[t])
    a1, j1 = _vec(s1, "acc")[A], st1["jerk"][A, :3].astype(np.float64)
    assert not st1["jerk"][:, 3].any()
    _criterion(tag, a1, j1, a_ref, j_ref, sj)
    assert np.array_equal(_vec(s1, "acc_old")[A], a0[A])
    # the corrector and the level rule on the engine's own a1, j1
    k_old = run.level[A].copy()
    run.correct(A, t, a1, j1)
    x1, v1 = _vec(s1, "pos")[A], _vec(s1, "vel")[A]
    dv = np.abs(v1 - run.v[A]).max()
    print(f"{tag}: t = {t} of {2 ** L}, {len(A)} active, levels {int(k_old.min())}..{int(k_old.max())} -> "
          f"{int(run.level[A].min())}..{int(run.level[A].max())}, max |dv| {dv:.2e}", flush=True)
    assert np.array_equal(x1.astype(np.float32).view(np.uint32), run.x[A].astype(np.float32).view(np.uint32))
    assert dv <= 6e-8
    assert np.array_equal(st1["levels"][A], run.level[A])
    assert np.array_equal(st1["want"][A].view(np.uint32), run.want[A].astype(np.float32).view(np.uint32))
    assert info["floor_hits"] == run.floor_hits
    assert info["level_steps"] == list(run.level_steps)
    return _bits(d, blk), A


@pytest.mark.parametrize("name", ["plummer", "general_masses_G1.7"])
@pytest.mark.parametrize("n", [2, 255, 257, 1000, 12289])
def test_one_block_step_against_the_restatement(nb, ctx, n, name):
    ic = nb.ic.plummer(n, seed=42)
    G, eps = 1.0, 0.01
    if name != "plummer":
        ic, G, eps = _general_masses(ic), 1.7, 0.05
    _check_one_step(nb, f"{n} bodies, {name}", ic, G, eps, 1.0 / 8, 12)


# ---- 3. active-set edge shapes -----------------------------------------------------------------------------------------
def _placements(n, k):
    """k of n bodies at the start, at the end, and scattered with body n - 1 and a body of the ragged last tile"""
    out = {"start": np.arange(k), "end": np.arange(n - k, n)}
    rng = np.random.default_rng(n * 1000 + k)
    pick = set(rng.choice(n, k, replace=False).tolist()) if k < n else set(range(n))
    must = ([n - 1] + ([(n // 256) * 256] if n % 256 else []))[:k]
    for b in must:
        if b not in pick:
            pick.remove(next(p for p in pick if p not in must))
            pick.add(b)
    out["scattered"] = np.array(sorted(pick))
    return out


@pytest.mark.parametrize("n", [1, 2, 255, 257, 12289])
def test_active_set_edge_shapes(nb, ctx, n):
    """the active set forced with set_levels (its bodies on level 1, the others on level 0: the first block step at tick
    2^(L-1) corrects exactly them), one step each, with the wide and with the narrow form"""
    ic = _general_masses(nb.ic.plummer(n, seed=42))
    lib_default = _block(nb)
    d, _ = to_device(nb, ic)
    lib_default.prime(d, _direct(nb, 1.7, 0.05), 1.0 / 16)
    crossover = lib_default.info()["narrow_below"]
    sizes = sorted({k for k in (1, 2, 63, 64, 65, 255, 256, 257, n - 1, n, crossover - 1, crossover, crossover + 1)
                    if 1 <= k <= n})
    cases, cache = 0, {}
    for k in sizes:
        for where, A in _placements(n, k).items():
            if n > 1000 and where != "scattered" and k not in (1, 257, n - 1, n):
                continue  # (the large size: every placement at the ends of the range, scattered everywhere)
            levels = np.zeros(n, np.int32)
            levels[A] = 1
            for form in (ALWAYS_WIDE, ALWAYS_NARROW):
                tag = f"{n} bodies, {k} active ({where}), {'wide' if form == ALWAYS_WIDE else 'narrow'}"
                first, got = _check_one_step(nb, tag, ic, 1.7, 0.05, 1.0 / 16, 6, narrow_below=form, levels=levels,
                                             ref_cache=cache)
                assert np.array_equal(got, A)
                assert np.array_equal(first, _one_step_bits(nb, ic, 1.7, 0.05, 1.0 / 16, 6, form, levels)), tag
                cases += 1
    print(f"{n} bodies: {cases} cases, crossover {crossover}")


def test_automatic_choice_at_the_crossover(nb, ctx):
    n = 1000
    ic = _general_masses(nb.ic.plummer(n, seed=42))
    fc = _direct(nb, 1.7, 0.05)
    for auto in (True, False):
        for delta in (-1, 0, 1):
            d, _ = to_device(nb, ic)
            blk = _block(nb, max_level=6, narrow_below=0 if auto else 200)
            blk.prime(d, fc, 1.0 / 16)
            cross = blk.info()["narrow_below"]
            assert (auto or cross == 200) and 1 < cross < n
            levels = np.zeros(n, np.int32)
            levels[np.random.default_rng(1).choice(n, cross + delta, replace=False)] = 1
            blk.setLevels(levels)
            blk.block_step(d, fc, 1.0 / 16, 1)
            info = blk.info()
            assert info["last_n_active"] == cross + delta
            assert (info["narrow_launches"], info["wide_launches"]) == ((1, 0) if delta < 0 else (0, 1))
    # every body active: the automatic choice is the wide form whatever the size (the shape of the shared step)
    small = _general_masses(nb.ic.plummer(8, seed=42))
    d, _ = to_device(nb, small)
    blk = _block(nb, max_level=0)
    blk.advance(d, fc, 1.0 / 16, 1)
    assert blk.info()["wide_launches"] == 1 and blk.info()["narrow_launches"] == 0


@pytest.mark.parametrize("form", [ALWAYS_WIDE, ALWAYS_NARROW], ids=["wide", "narrow"])
def test_guard_form_with_a_coincident_pair(nb, ctx, form):
    """eps = 0: two bodies at one place with different velocities, one of them active"""
    n = 257
    ic = _general_masses(nb.ic.plummer(n, seed=42))
    for k in ("pos_x", "pos_y", "pos_z", "vel_x", "vel_y", "vel_z"):
        ic[k][200] = ic[k][3]  # (the same velocity too: they stay together over the predictor; their jerks differ)
    ic["mass"][200] *= 2.0
    levels = np.zeros(n, np.int32)
    levels[[3, 17, 256]] = 1
    bits, A = _check_one_step(nb, f"eps = 0, coincident pair, form {form}", ic, 1.7, 0.0, 1.0 / 16, 6, narrow_below=form,
                              levels=levels)
    assert list(A) == [3, 17, 256] and np.isfinite(bits.view(np.float32)[:12 * n]).all()


# ---- 4. schedule and counters ------------------------------------------------------------------------------------------
def test_schedule_and_counters(nb, ctx):
    n, L, dt_max, G, eps = 1000, 10, 1.0 / 8, 1.0, 0.01
    ic = nb.ic.plummer(n, seed=42)
    fc = _direct(nb, G, eps)
    d, _ = to_device(nb, ic)
    blk = _block(nb, max_level=L)
    blk.prime(d, fc, dt_max)
    st = blk.getState()
    assert len(set(st["levels"])) > 2
    sum_active, macro, steps = 0, 0, 0
    per_step = []
    while macro < 2:
        before = st
        nxt = before["ticks"].astype(np.int64) + 2 ** (L - before["levels"].astype(np.int64))
        t, A = int(nxt.min()), np.flatnonzero(nxt == nxt.min())
        checked = steps < 50 or t == 2 ** L
        before_state = _state(d) if checked else None
        blk.block_step(d, fc, dt_max, 1)
        steps += 1
        info = blk.info()
        sum_active += len(A)
        assert info["last_n_active"] == len(A) and info["body_steps"] == sum_active and info["block_steps"] == steps
        assert sum(info["level_steps"]) == sum_active and info["narrow_launches"] + info["wide_launches"] == steps
        wrapped = t == 2 ** L
        st = blk.getState()
        if checked:  # the restatement's invariants on state()
            after_state = _state(d)
            rest = np.setdiff1d(np.arange(n), A)
            for k in F:
                assert np.array_equal(before_state[k][rest].view(np.uint32), after_state[k][rest].view(np.uint32)), k
            assert np.array_equal(before["jerk"][rest], st["jerk"][rest])
            assert np.array_equal(before["levels"][rest], st["levels"][rest])
            assert ((st["levels"] >= 0) & (st["levels"] <= L)).all()
            if wrapped:
                assert not st["ticks"].any() and len(A) == n  # re-based
            else:
                assert (st["ticks"] <= t).all() and (st["ticks"][A] == t).all()
                assert np.array_equal(before["ticks"][rest], st["ticks"][rest])
                assert (st["ticks"].astype(np.int64) % 2 ** (L - st["levels"].astype(np.int64)) == 0).all()
        if wrapped:
            macro += 1
            assert info["macro_steps"] == macro and info["current_tick"] == 0
            per_step.append(steps)
        else:
            assert info["current_tick"] == t and info["macro_steps"] == macro
    assert info["narrow_launches"] > 0 and info["wide_launches"] > 0
    print(f"1,000 bodies, 2 macro steps: {steps} block steps, {sum_active} body steps, narrow {info['narrow_launches']}, "
          f"wide {info['wide_launches']}, floor hits {info['floor_hits']}")
    by_steps = _bits(d, blk)
    # advance(2) == 2 x advance(1) == the step(1) sequence, bit for bit; two fresh runs are bitwise equal
    runs = []
    for plan in ((2,), (1, 1), (2,)):
        d2, _ = to_device(nb, ic)
        b2 = _block(nb, max_level=L)
        for k in plan:
            b2.advance(d2, fc, dt_max, k)
        assert b2.info()["block_steps"] == steps and b2.info()["body_steps"] == sum_active
        runs.append(_bits(d2, b2))
    for r in runs:
        assert np.array_equal(r, by_steps)
    # block_step with a count stops at the macro boundary
    d3, _ = to_device(nb, ic)
    b3 = _block(nb, max_level=L)
    b3.block_step(d3, fc, dt_max, 10 ** 6)
    assert b3.info()["macro_steps"] == 1 and b3.info()["block_steps"] == per_step[0] and b3.info()["current_tick"] == 0


# ---- 5. accuracy -------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def refs():
    return br.references()


def _run_block(nb, ic, G, eps, dt_max, macro, L, eta=0.02):
    d, _ = to_device(nb, ic)
    blk = _block(nb, eta=eta, max_level=L)
    blk.advance(d, _direct(nb, G, eps), dt_max, macro)
    return _vec(_state(d), "pos"), blk.info()


def test_plummer_condition(nb, ctx, refs):
    """the condition of tests/test_hermite_block_cpu.py::test_plummer_condition on the engine: max |dx| not above the
    shared fp32 run of 512 steps, at most a quarter of its body steps, no floor hit"""
    c = br.PLUMMER
    x, info = _run_block(nb, nb.ic.plummer(c["n"], seed=c["seed"]), 1.0, c["eps"], c["dt_max"], c["macro"], c["L"])
    err = np.abs(x - refs["plummer_ref"]).max()
    print(f"plummer: max |dx| {err:.3e} (shared 512 steps: {refs['plummer_shared_err']:.3e}), {info['body_steps']} body "
          f"steps in {info['block_steps']} block steps, narrow {info['narrow_launches']} wide {info['wide_launches']}")
    assert err <= refs["plummer_shared_err"]
    assert info["body_steps"] <= c["shared_steps"] * c["n"] // 4
    assert info["floor_hits"] == 0 and info["macro_steps"] == c["macro"]


def test_binary_condition(nb, ctx, refs):
    """... and the binary: error not above the shared fp32 run of 4,096 steps, at most an eighth of its body steps"""
    c = br.BINARY
    ic = _ic_of(*br.binary_case())
    x, info = _run_block(nb, ic, 1.0, c["eps"], c["T"] / c["macro"], c["macro"], c["L"])
    err = np.abs(x - refs["binary_ref"]).max()
    print(f"binary: max |dx| {err:.3e} (shared 4,096 steps: {refs['binary_shared_err']:.3e}), {info['body_steps']} body "
          f"steps in {info['block_steps']} block steps, levels {[k for k, v in enumerate(info['level_steps']) if v]}")
    assert err <= refs["binary_shared_err"]
    assert info["body_steps"] <= c["shared_steps"] * 3 // 8
    assert info["floor_hits"] == 0
    _, shallow = _run_block(nb, ic, 1.0, c["eps"], c["T"] / c["macro"], c["macro"], 2)
    assert shallow["floor_hits"] > 0 and sum(shallow["level_steps"][3:]) == 0


# ---- 6. refusals and state errors --------------------------------------------------------------------------------------
def test_refusals_and_state_errors(nb, ctx):
    ic = nb.ic.plummer(300, seed=42)
    d, _ = to_device(nb, ic)
    fc = _direct(nb, 1.0, 0.01)
    before = _state(d)
    blk = _block(nb, max_level=8)
    for dt, msg in ((0.0, "Time step must be positive"), (-1e-3, "Time step must be positive"),
                    (float("nan"), "Time step must be a finite number"), (float("inf"), "Time step must be a finite number")):
        for call in (lambda: blk.integrate(d, fc, dt), lambda: blk.block_step(d, fc, dt, 1), lambda: blk.prime(d, fc, dt)):
            with pytest.raises(nb.ValidationException, match=msg):
                call()
    for k in F:  # nothing was touched by the refused calls
        assert np.array_equal(before[k], _state(d)[k]), k
    # the middle of a macro step: another dt_max, G, eps -> ERR_STATE; set_levels -> ERR_STATE; the same ones go on
    blk.block_step(d, fc, 1.0 / 8, 1)
    assert blk.info()["current_tick"] != 0
    mid = _bits(d, blk)
    with pytest.raises(nb.StateException, match="middle of a macro step"):
        blk.block_step(d, fc, 1.0 / 16, 1)
    with pytest.raises(nb.StateException, match="middle of a macro step"):
        blk.integrate(d, _direct(nb, 2.0, 0.01), 1.0 / 8)
    with pytest.raises(nb.StateException, match="middle of a macro step"):
        blk.integrate(d, _direct(nb, 1.0, 0.02), 1.0 / 8)
    with pytest.raises(nb.StateException, match="only be set at tick 0"):
        blk.setLevels(np.zeros(300, np.int32))
    assert np.array_equal(mid, _bits(d, blk))
    blk.integrate(d, fc, 1.0 / 8)  # finishes the macro step
    assert blk.info()["current_tick"] == 0 and blk.info()["macro_steps"] == 1
    # at tick 0: levels out of range are refused, another dt_max primes again (the counters start over)
    for bad in (-1, 9):
        lv = np.zeros(300, np.int32)
        lv[7] = bad
        with pytest.raises(nb.ValidationException, match="outside"):
            blk.setLevels(lv)
    blk.integrate(d, fc, 1.0 / 16)
    assert blk.info()["macro_steps"] == 1
    # set_params takes effect at the next priming
    blk.setParameters(0.02, 0.01, 3)
    assert blk.info()["max_level"] == 8
    blk.invalidate()
    blk.integrate(d, fc, 1.0 / 16)
    assert blk.info()["max_level"] == 3 and blk.getLevels().max() <= 3
    # capture: none of the calls can be recorded
    lib = nb._lib.load()
    s = d.struct()
    with pytest.raises(nb.StateException, match="cannot be recorded into a step graph"):
        with ctx.capture():
            blk.integrate(d, fc, 1.0 / 16)
    # capacity and count at the C ABI
    small = C.c_void_p()
    nb._lib.check(lib.nbody_hip_hermite_block_create(ctx.handle, 16, C.byref(small)))
    try:
        with pytest.raises(nb.ValidationException, match="exceeds the integrator's capacity"):
            nb._lib.check(lib.nbody_hip_hermite_block_prime(small, C.byref(s), 1.0, 0.05, 0.1))
        with pytest.raises(nb.ValidationException, match="exceeds the integrator's capacity"):
            nb._lib.check(lib.nbody_hip_hermite_block_advance(small, C.byref(s), 1.0, 0.05, 0.1, 1))
        s.count = 16
        with pytest.raises(nb.ValidationException, match="block_steps must be at least 1"):
            nb._lib.check(lib.nbody_hip_hermite_block_step(small, C.byref(s), 1.0, 0.05, 0.1, 0))
        with pytest.raises(nb.ValidationException, match="macro_steps must be at least 1"):
            nb._lib.check(lib.nbody_hip_hermite_block_advance(small, C.byref(s), 1.0, 0.05, 0.1, 0))
        with pytest.raises(nb.ValidationException, match="Softening parameter must be non-negative"):
            nb._lib.check(lib.nbody_hip_hermite_block_advance(small, C.byref(s), 1.0, -0.05, 0.1, 1))
        with pytest.raises(nb.StateException):
            nb._lib.check(lib.nbody_hip_hermite_block_advance(small, None, 1.0, 0.05, 0.1, 1))
        with pytest.raises(nb.StateException, match="not primed"):
            nb._lib.check(lib.nbody_hip_hermite_block_state(small, None, None, None, None))
        with pytest.raises(nb.StateException, match="not primed"):
            nb._lib.check(lib.nbody_hip_hermite_block_set_levels(small, np.zeros(16, np.int32).ctypes.data))
        with pytest.raises(nb.ValidationException):
            nb._lib.check(lib.nbody_hip_hermite_block_set_params(small, 0.02, 0.01, 21))
        with pytest.raises(nb.ValidationException):
            nb._lib.check(lib.nbody_hip_hermite_block_tuning(small, -1))
        s.count = 0
        with pytest.raises(nb.ValidationException):
            nb._lib.check(lib.nbody_hip_hermite_block_advance(small, C.byref(s), 1.0, 0.05, 0.1, 1))
    finally:
        lib.nbody_hip_hermite_block_destroy(small)
    with pytest.raises(nb.ValidationException):
        h = C.c_void_p()
        nb._lib.check(lib.nbody_hip_hermite_block_create(ctx.handle, 0, C.byref(h)))
    # a larger system re-sizes the Python class's handle
    big, _ = to_device(nb, nb.ic.plummer(400, seed=1))
    blk.integrate(big, fc, 1.0 / 16)
    assert blk.getLevels().shape == (400,)


# ---- 7. ParticleSystem and the facade ----------------------------------------------------------------------------------
def _system(nb, ic, scheme=None, dt=1.0 / 16):
    ps = nb.ParticleSystem()
    if scheme is not None:
        ps.setIntegrationScheme(scheme)
    cfg = nb.SimulationConfig(particle_count=ic["mass"].size, force_method=nb.ForceMethod.DIRECT_N2, dt=dt, G=1.0,
                              softening=0.1)
    ps.initialize(cfg, ic)
    return ps


def test_handle_refusals_at_the_c_abi(nb, ctx):
    """null state arrays, a count above the capacity, the precision read back, the three parameter checks
    (tests/hermite_handle_cases.py)"""
    d, _ = to_device(nb, nb.ic.plummer(8, seed=1))
    hc.raw_refusals(nb, ctx, d, "block_", "integrator's")


def test_particle_system_hermite4_block(nb, ctx):
    ic = nb.ic.plummer(256, seed=42)
    ps = _system(nb, ic, "hermite4-block")
    ps.update(1.0 / 16)
    ps.update(1.0 / 16)
    d, _ = to_device(nb, ic)
    blk = nb.BlockHermiteIntegrator()
    blk.advance(d, _direct(nb, 1.0, 0.1), 1.0 / 16, 2)
    a, b = _state(ps.getDeviceData()), _state(d)
    for k in F[:6]:
        assert np.array_equal(a[k].view(np.uint32), b[k].view(np.uint32)), k
    assert ps.getSimulationTime() == pytest.approx(1.0 / 8)
    assert ps.hermite_block_.info()["macro_steps"] == 2 and ps.hermite_ is None
    # saveState / loadState (setState) invalidates: the run after it is that of a fresh system started from that state
    st = ps.getState()
    ps.setState(st)
    fresh = _system(nb, {k: getattr(st, k) for k in ("pos_x", "pos_y", "pos_z", "vel_x", "vel_y", "vel_z", "mass")},
                    "hermite4-block")
    for _ in range(2):
        ps.update(1.0 / 16)
        fresh.update(1.0 / 16)
    assert ps.hermite_block_.info()["macro_steps"] == 2  # (primed again: the counters started over)
    assert np.array_equal(_bits(ps.getDeviceData()), _bits(fresh.getDeviceData()))
    with pytest.raises(nb.ValidationException, match="Direct-only"):
        ps.setForceMethod(nb.ForceMethod.BARNES_HUT)


def test_save_and_load_state_invalidate(nb, ctx, tmp_path):
    ic = nb.ic.plummer(256, seed=42)
    ps = _system(nb, ic, "hermite4-block")
    ps.update(1.0 / 16)
    path = str(tmp_path / "state.nbody")
    ps.saveState(path)
    ps.update(1.0 / 16)
    ps.loadState(path)
    ps.update(1.0 / 16)
    assert ps.hermite_block_.info()["macro_steps"] == 1  # primed again after the load
    other = _system(nb, ic, "hermite4-block")
    other.update(1.0 / 16)
    other.loadState(path)
    other.update(1.0 / 16)
    assert np.array_equal(_bits(ps.getDeviceData()), _bits(other.getDeviceData()))


def test_default_scheme_is_untouched(nb, ctx):
    ic = nb.ic.plummer(1000, seed=42)
    a = _system(nb, ic, dt=0.01)
    c = nb.ParticleSystem()
    c.setIntegrationScheme("hermite4-block")
    c.setIntegrationScheme("velocity-verlet")
    c.initialize(a.config_, ic)
    d, _ = to_device(nb, ic)
    fc = _direct(nb, 1.0, 0.1)
    fc.computeForces(d)
    integ = nb.Integrator()
    for _ in range(10):
        a.update(0.01)
        c.update(0.01)
        integ.integrate(d, fc, 0.01)
    assert a.getIntegrationScheme() == "velocity-verlet" and a.hermite_block_ is None and c.hermite_block_ is None
    assert np.array_equal(_bits(a.getDeviceData()), _bits(c.getDeviceData()))
    assert np.array_equal(_bits(a.getDeviceData()), _bits(d))


def test_facade_hermite_block_program(nb, ctx):
    exe = os.path.join(ROOT, "n-body_amd", "lib", "hermite_block_tests")
    assert os.path.exists(exe), "build with __graft_entry__.build()"
    env = dict(os.environ)
    env["LD_LIBRARY_PATH"] = os.path.dirname(exe) + os.pathsep + env.get("LD_LIBRARY_PATH", "")
    r = subprocess.run([exe], cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    print(r.stdout)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    h = subprocess.run([exe, "hash"], cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert h.returncode == 0, h.stdout[-3000:] + h.stderr[-2000:]
    got = re.findall(r"^hermite_block fnv (\S+)$", h.stdout, re.M)
    assert len(got) == 1 and got == re.findall(r"^hermite_block fnv (\S+)$", r.stdout, re.M)
    # the same two macro steps through the Python host: the same bits
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
    blk = nb.BlockHermiteIntegrator()
    blk.integrate(d, fc, 1.0 / 64)
    blk.advance(d, fc, 1.0 / 64, 1)
    fnv = 1469598103934665603
    for k in F[:6]:
        for b in getattr(d, k).cpu().numpy().tobytes():
            fnv = ((fnv ^ b) * 1099511628211) & 0xFFFFFFFFFFFFFFFF
    assert got[0] == f"{fnv:016x}"

"""Extended state precision of the two Hermite integrators (nbody_hip_hermite[_block]_set_precision,
nbody_hip_direct_acc_jerk_ext) on a real GPU: evaluation parity against fp64 on states that are not fp32-representable,
the block forms, bitwise properties, one step against the restatement, the accuracy the mode is for, state handling and
the facade.  Restatement: tests/hermite_ext_ref.py.  Every comparison is against the fp64 restatement, never against
the engine itself."""
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import hermite_ext_ref as xr
import hermite_ref as hr
from gpu_util import U, rel_err, to_device

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = ("pos_x", "pos_y", "pos_z", "vel_x", "vel_y", "vel_z", "acc_x", "acc_y", "acc_z", "acc_old_x", "acc_old_y", "acc_old_z")

# ---- the a-priori bound of the jerk against fp64, extended mode --------------------------------------------------------
# tests/test_hermite_gpu.py derives, for the fp32 sweep, |dj_i| <= max(1e-5 |j_i|, C u S_i) with C = 34 + sqrt(3) (256 + 1)
# + 1 = 480.1: 34 u per term, the rest for the accumulation and the final rounding.  The extended sweep differs in d only:
#     d = fl( fl(hi_j - hi_i) + fl(lo_j - lo_i) )
# against the fp64 value of (hi_j + lo_j) - (hi_i + lo_i).  The hi difference carries <= 1u of itself (0 for a close
# pair, Sterbenz), the sum one more rounding: 2u on d where the fp32 sweep has 1u -- as long as |hi_j - hi_i| stays
# comparable to |d|, which holds because |lo| <= u |hi|.  The rounding of the lo difference is u |lo_j - lo_i| <=
# 2 u^2 max |x|: relative to d it is u (2^-23 |x| / |d|), below u / 8 for every pair with |x| / |d| <= 2^20, which covers
# every pair of the test geometries that carries weight in S_i (the closest pair of a guard case included: its d is the
# lo difference itself, one rounding).  Following the three lines of that derivation with 2u (+ u / 8) on d:
#   f:  4.25u on d^2, three fused multiply-adds 3u: 7.25u on h, 10.9u on h^-3/2; v_rsq_f32 cubed 6u; three roundings 3u
#                                                                                                               => 19.9u
#   the |w| part: f 19.9u, w 1u, fma 1u; the dot product (2.125u + 1u inputs + 3u roundings) |d| |w| x 3            => 40.3u
#   the |d.w| part: f 19.9u, h^-1 7.25u, rsq squared 4u, three roundings 3u, d 2.125u, fma 1u                      => 37.3u
#                                                                                                     C_TERMS_EXT = 41
# Accumulation and final rounding are unchanged:  C_JERK_EXT = 41 + sqrt(3) (256 + 1) + 1 = 487.1
TS = 256
C_TERMS_EXT = 41
C_JERK_EXT = C_TERMS_EXT + np.sqrt(3.0) * (TS + 1) + 1
# Regression tier, MEASURED on an MI355X, not derived (profiles/r11_hermite_ext_tests.log): the largest margin
# max err / (u S_j) over every evaluation comparison of this file (64 comparisons; seventy times inside the worst case).
# 1.6 x it is held, as JERK_MARGIN_MEASURED is.
EXT_JERK_MARGIN_MEASURED = 6.60   # 1,000 bodies, centred, eps 0.01; the displaced geometries stay below it
_margins = []


def _arrays(ic):
    return (np.stack([ic["pos_x"], ic["pos_y"], ic["pos_z"]], 1), np.stack([ic["vel_x"], ic["vel_y"], ic["vel_z"]], 1),
            ic["mass"])


def _ic_of(pos, vel, m):
    pos, vel = np.asarray(pos, np.float32), np.asarray(vel, np.float32)
    return dict(pos_x=pos[:, 0].copy(), pos_y=pos[:, 1].copy(), pos_z=pos[:, 2].copy(), vel_x=vel[:, 0].copy(),
                vel_y=vel[:, 1].copy(), vel_z=vel[:, 2].copy(), mass=np.asarray(m, np.float32).copy())


def _direct(nb, G, eps):
    c = nb.DirectForceCalculator()
    c.setGravitationalConstant(G)
    c.setSofteningParameter(eps)
    return c


def _state(d):
    return {k: getattr(d, k).cpu().numpy().copy() for k in F}


def _col(s, name):
    return np.stack([s[name + "_x"], s[name + "_y"], s[name + "_z"]], 1).astype(np.float64)


def _cluster(nb, n, geometry, seed=42):
    """a Plummer sphere shrunk and displaced: X, V in fp64 (X not fp32-representable), m"""
    pos, vel, m = _arrays(nb.ic.plummer(n, seed=seed))
    scale, centre = xr.GEOMETRIES[geometry]
    return xr.displaced_cluster(pos, vel, m, scale, centre)


def _lo4(lo):
    out = np.zeros((len(lo), 4), np.float32)
    out[:, :3] = lo
    return torch.from_numpy(out).cuda()


def _ref_eval(pos, vel, m, G, eps, targets=None, chunk=256):
    """hermite_ref.acc_jerk in fp64 on the device (tests/test_hermite_gpu.py pins this form to the numpy one):
    -> (a, j, S_a, S_j) as numpy"""
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


def _parity(tag, a, j, ref):
    """the criterion: a per body within 1e-5; |dj| <= max(1e-5 |j|, C_JERK_EXT u S_j); the regression tier on the margin"""
    a_ref, j_ref, _, sj = ref
    ea = rel_err(a, a_ref)
    err = np.linalg.norm(j - j_ref, axis=1)
    bound = np.maximum(1e-5 * np.linalg.norm(j_ref, axis=1), C_JERK_EXT * U * sj)
    margin = float((err / np.maximum(U * sj, 1e-300)).max())
    _margins.append(margin)
    print(f"ext parity {tag}: max |da| / |a| {ea.max():.3e}; max |dj| / |j| {rel_err(j, j_ref).max():.3e}, margin "
          f"max err / (u S_j) {margin:.2f} (C' = {C_JERK_EXT:.1f}); largest margin so far {max(_margins):.2f}", flush=True)
    assert ea.max() <= 1e-5, (tag, ea.max())
    assert np.all(err <= bound), (tag, int(np.argmax(err / np.maximum(bound, 1e-300))))
    assert margin <= 1.6 * EXT_JERK_MARGIN_MEASURED, (tag, margin, EXT_JERK_MARGIN_MEASURED)
    return margin


def _np4(t):
    t = t.cpu().numpy()
    assert not t[:, 3].any()
    return t[:, :3].astype(np.float64)


def _eval_ext(nb, ctx, X, V, m, G, eps):
    """direct_acc_jerk_ext at the split state: -> (a, j, d, hi, lo, acc4, jerk4)"""
    hi, lo = xr.split(X)
    d, _ = to_device(nb, _ic_of(hi, V, m))
    acc, jerk = nb.direct_acc_jerk_ext(ctx, d, _lo4(lo), G, eps)
    return _np4(acc), _np4(jerk), d, hi, lo, acc, jerk


# ---- 4. evaluation -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("geometry", list(xr.GEOMETRIES))
@pytest.mark.parametrize("n", [1, 2, 255, 257, 1000, 12289])
def test_evaluation_against_fp64(nb, ctx, n, geometry):
    G, eps = 1.0, 0.01
    X, V, m = _cluster(nb, n, geometry)
    a, j, d, hi, lo, acc4, jerk4 = _eval_ext(nb, ctx, X, V, m, G, eps)
    vh = V.astype(np.float32)
    if n == 1:
        assert not a.any() and not j.any()
    else:
        ref = _ref_eval(hi + lo, vh, m, G, eps)
        _parity(f"{n} bodies, {geometry}", a, j, ref)
        if geometry != "centred" and n >= 255:
            # the inputs discriminate: the fp32 mode, from the rounded positions, misses the same bar
            a32 = _np4(nb.direct_acc_jerk(ctx, d, G, eps)[0])
            worst = rel_err(a32, ref[0]).max()
            print(f"   fp32 mode on the same bodies: max |da| / |a| {worst:.3e}")
            assert worst > 1e-5
    # the primed integrators hold the same a and j (one evaluation each), from set_state_f64
    fc = _direct(nb, G, eps)
    for integ, prime in ((nb.HermiteIntegrator(), lambda h, dd: h.prime(dd, fc)),
                         (nb.BlockHermiteIntegrator(), lambda h, dd: h.prime(dd, fc, 1e-3))):
        dd, _ = to_device(nb, _ic_of(np.zeros_like(hi), np.zeros_like(hi), m))
        integ.setStatePrecision("extended")
        integ.setExtendedState(dd, X, V, fc)
        prime(integ, dd)
        assert torch.equal(integ.getJerk(), jerk4)
        assert torch.equal(torch.stack([dd.acc_x, dd.acc_y, dd.acc_z], 1), acc4[:, :3])


@pytest.mark.parametrize("eps", [0.01, 0.0])
def test_evaluation_32768_sampled(nb, ctx, eps):
    """four targets per lane (from 32,768 bodies), packed and GUARD"""
    X, V, m = _cluster(nb, 32768, "scale0.05_at_64")
    a, j, d, hi, lo, _, _ = _eval_ext(nb, ctx, X, V, m, 1.0, eps)
    rows = np.random.default_rng(7).choice(32768, 1024, replace=False)
    _parity(f"32,768 bodies, 1,024 sampled, eps {eps}", a[rows], j[rows],
            _ref_eval(hi + lo, V.astype(np.float32), m, 1.0, eps, targets=rows, chunk=64))


def test_guard_coincident_pair_and_pair_split_by_the_residuals_only(nb, ctx):
    X, V, m = _cluster(nb, 257, "scale0.05_at_64")
    hi, lo = xr.split(X)
    hi[200], lo[200] = hi[3], lo[3]          # two bodies at one place: contributes nothing under the guard convention
    hi[150] = hi[7]                          # the hi parts coincide, the lo parts do not: a distinct pair
    lo[150] = lo[7] + np.float32(2e-6) * np.array([1.0, -0.5, 0.25])
    lo = lo.astype(np.float32).astype(np.float64)
    assert np.array_equal(hi[150], hi[7]) and not np.array_equal(lo[150], lo[7])
    d, _ = to_device(nb, _ic_of(hi, V, m))
    for eps in (0.0, 0.01):
        acc, jerk = nb.direct_acc_jerk_ext(ctx, d, _lo4(lo), 1.0, eps)
        a, j = _np4(acc), _np4(jerk)
        assert np.isfinite(a).all() and np.isfinite(j).all()
        ref = _ref_eval(hi + lo, V.astype(np.float32), m, 1.0, eps)
        _parity(f"257 bodies, a coincident pair and a pair split by lo only, eps {eps}", a, j, ref)
        if eps == 0.0:  # the split pair is seen: it dominates the two bodies' accelerations
            assert np.linalg.norm(a[150]) > 1e3 * np.median(np.linalg.norm(a, axis=1))


# ---- 4 (block forms) and 6: one block step against the restatement -----------------------------------------------------
def _active_set(n, k, where):
    if where == "start":
        return np.arange(k)
    if where == "end":
        return np.arange(n - k, n)
    return np.sort(np.random.default_rng(k).choice(n, k, replace=False))


def _one_block_step(nb, tag, X, V, m, G, eps, A, narrow_below, dt_max=1.0 / 64):
    """levels 1 on A and 0 elsewhere with max_level 1: the first block step corrects exactly A over dt_max / 2"""
    n = len(X)
    fc = _direct(nb, G, eps)
    d, _ = to_device(nb, _ic_of(np.zeros_like(X), np.zeros_like(X), m))
    blk = nb.BlockHermiteIntegrator()
    blk.setParameters(0.02, 0.01, 1)
    blk.setTuning(narrow_below)
    blk.setStatePrecision("extended")
    blk.setExtendedState(d, X, V, fc)
    blk.prime(d, fc, dt_max)
    s0, st0 = _state(d), blk.getState()
    X0, V0 = blk.getExtendedState(d)
    assert np.array_equal(X0, xr.rnd2(X)) and np.array_equal(V0, xr.rnd2(V))
    lv = np.zeros(n, np.int32)
    lv[A] = 1
    if len(A) == n:
        lv[:] = 1
    blk.setLevels(lv)
    blk.block_step(d, fc, dt_max, 1)
    s1, st1 = _state(d), blk.getState()
    X1, V1 = blk.getExtendedState(d)
    info = blk.info()
    assert info["last_n_active"] == len(A)
    assert (info["narrow_launches"], info["wide_launches"]) == ((1, 0) if len(A) < narrow_below else (0, 1))
    a0, j0 = _col(s0, "acc"), st0["jerk"][:, :3].astype(np.float64)
    a1, j1 = _col(s1, "acc")[A], st1["jerk"][A, :3].astype(np.float64)
    # the restatement, seeded with the engine's own (a, j) and handed the engine's own (a1, j1)
    run = xr.BlockHermiteExt(X, V, m, G, eps, dt_max, max_level=1, acc=a0, jerk=j0, levels=lv,
                             evaluate=lambda xp, vp, t: (a1, j1))
    t, A_ref = run.schedule()
    assert t == 1 and np.array_equal(A_ref, A)
    xp, vp = run.predicted(t)
    _parity(tag, a1, j1, _ref_eval(xp, vp, m, G, eps, targets=A))
    h = run.dt_max / 2.0
    run.step()
    # the largest term of each corrector expression
    largest_v = np.maximum(np.abs(V0[A]), np.maximum(np.abs((a0[A] + a1) * (0.5 * h)), np.abs((j0[A] - j1) * (h * h / 12.0))))
    largest_x = np.maximum(np.abs(X0[A]), np.maximum(np.abs((V0[A] + run.v[A]) * (0.5 * h)),
                                                     np.abs((a0[A] - a1) * (h * h / 12.0))))
    # the hi parts bit for bit, hi + lo within 2^-46 of the largest term of the corrector expression
    assert np.array_equal(_col(s1, "pos")[A], run.x_hi[A])
    assert np.array_equal(_col(s1, "vel")[A], run.v_hi[A])
    assert np.all(np.abs(X1[A] - run.x[A]) <= 2.0 ** -46 * largest_x)
    assert np.all(np.abs(V1[A] - run.v[A]) <= 2.0 ** -46 * largest_v)
    assert np.array_equal(_col(s1, "acc_old")[A], a0[A])
    # bodies outside A: untouched in every array, residuals included
    out = np.setdiff1d(np.arange(n), A)
    for k in F:
        assert np.array_equal(s1[k][out], s0[k][out]), k
    assert np.array_equal(X1[out], X0[out]) and np.array_equal(V1[out], V0[out])
    assert np.array_equal(st1["jerk"][out], st0["jerk"][out])


BLOCK_SIZES = {257: (1, 63, 64, 65, 256, 257), 12289: (1, 63, 64, 65, 256, 257, 383, 384, 385, 12289)}


@pytest.mark.parametrize("form", ["wide", "narrow"])
@pytest.mark.parametrize("n", [257, 12289])
def test_block_forms_one_step(nb, ctx, n, form):
    """every active-set size at which a form takes another path (one lane, a wave +- 1, a block +- 1, the automatic
    crossover +- 1, every body), the set at the start, at the end and scattered"""
    X, V, m = _cluster(nb, n, "scale0.05_at_64")
    narrow_below = n + 1 if form == "narrow" else 1
    places = ("start", "end", "scattered")
    for q, k in enumerate(BLOCK_SIZES[n]):
        for where in (places if k == 65 else (places[q % 3],)):
            _one_block_step(nb, f"block {form}, {n} bodies, {k} active at the {where}", X, V, m, 1.0, 0.01,
                            _active_set(n, k, where), narrow_below)


def test_block_forms_guard_and_automatic_choice(nb, ctx):
    X, V, m = _cluster(nb, 1000, "scale0.01_at_1000")
    # dt_max = 2^-16: without softening the closest pairs of this cluster have |j| ~ 1e13, and the hi parts can only be
    # compared bit for bit while the terms of the corrector stay comparable to the result (fp64 contraction moves a sum
    # by 2^-53 of its LARGEST term; at 1 / 64 the jerk term is 1e7 x the velocity and a tie in the rounding to fp32 comes
    # within reach)
    for k, narrow_below in ((65, 1001), (65, 1), (383, 384), (384, 384)):
        _one_block_step(nb, f"block GUARD, 1,000 bodies, {k} active, narrow below {narrow_below}", X, V, m, 1.0, 0.0,
                        _active_set(1000, k, "scattered"), narrow_below, dt_max=2.0 ** -16)


# ---- 6. one shared step against the restatement ------------------------------------------------------------------------
def test_one_shared_step_against_the_restatement(nb, ctx):
    G, eps, dt = 1.0, 0.01, 1.0 / 128
    X, V, m = _cluster(nb, 1000, "scale0.05_at_64")
    fc = _direct(nb, G, eps)
    d, _ = to_device(nb, _ic_of(np.zeros_like(X), np.zeros_like(X), m))
    h = nb.HermiteIntegrator()
    h.setStatePrecision("extended")
    h.setExtendedState(d, X, V, fc)
    h.prime(d, fc)
    a0, j0 = _col(_state(d), "acc"), _np4(h.getJerk())
    h.integrate(d, fc, dt)
    s1 = _state(d)
    a1, j1 = _col(s1, "acc"), _np4(h.getJerk())
    X1, V1 = h.getExtendedState(d)
    seen = {}

    def evaluate(xp, vp):
        seen["xp"], seen["vp"] = xp, vp
        return a1, j1

    ref = xr.hermite_steps_ext(X, V, m, G, eps, dt, 1, evaluate=evaluate, acc=a0, jerk=j0)
    _parity("one shared step, 1,000 bodies: (a1, j1) at the predicted state", a1, j1,
            _ref_eval(seen["xp"], seen["vp"], m, G, eps))
    assert np.array_equal(_col(s1, "pos"), ref["pos_hi"])
    assert np.array_equal(_col(s1, "vel"), ref["vel_hi"])
    hh = float(np.float32(dt))
    assert np.all(np.abs(X1 - ref["pos"]) <= 2.0 ** -46 * ref["largest"])
    largest_v = np.maximum(np.abs(xr.rnd2(V)), np.maximum(np.abs((a0 + a1) * (0.5 * hh)), np.abs((j0 - j1) * (hh * hh / 12.0))))
    assert np.all(np.abs(V1 - ref["vel"]) <= 2.0 ** -46 * largest_v)
    assert np.array_equal(_col(s1, "acc_old"), a0)
    # the representation: pos_* / vel_* are the hi parts, the residuals fp32 numbers of at most half an ulp of them
    for Z, hi in ((X1, _col(s1, "pos")), (V1, _col(s1, "vel"))):
        lo = Z - hi
        assert np.array_equal(lo.astype(np.float32).astype(np.float64), lo)
        assert np.all(np.abs(lo) <= 0.5 * np.spacing(np.abs(hi).astype(np.float32)).astype(np.float64))


# ---- 5. bits -----------------------------------------------------------------------------------------------------------
def _bits_ext(integ, d):
    X, V = integ.getExtendedState(d)
    return np.concatenate([v.view(np.uint32) for v in _state(d).values()] + [X.view(np.uint32).ravel(), V.view(np.uint32).ravel(),
                          integ.getJerk().cpu().numpy().view(np.uint32).ravel()])


def test_shared_steps_reproducible_and_compose(nb, ctx):
    X, V, m = _cluster(nb, 12289, "scale0.05_at_64")
    fc = _direct(nb, 1.0, 0.01)
    runs = []
    for plan in ((4,), (4,), (1, 1, 1, 1), (1, 3)):
        d, _ = to_device(nb, _ic_of(np.zeros_like(X), np.zeros_like(X), m))
        h = nb.HermiteIntegrator()
        h.setStatePrecision("extended")
        h.setExtendedState(d, X, V, fc)
        for k in plan:
            h.integrate_steps(d, fc, 1e-3, k)
        runs.append(_bits_ext(h, d))
    for r in runs[1:]:
        assert np.array_equal(r, runs[0])
    Xe, _ = h.getExtendedState(d)
    assert np.abs(Xe - Xe.astype(np.float32)).max() > 0  # (the residuals are in use)


def test_block_steps_reproducible_and_compose(nb, ctx):
    X, V, m = _cluster(nb, 257, "scale0.05_at_64")
    fc = _direct(nb, 1.0, 0.01)
    runs = []
    for plan in ("advance2", "advance2", "advance1x2", "block_steps"):
        d, _ = to_device(nb, _ic_of(np.zeros_like(X), np.zeros_like(X), m))
        b = nb.BlockHermiteIntegrator()
        b.setParameters(0.02, 0.01, 6)
        b.setStatePrecision("extended")
        b.setExtendedState(d, X, V, fc)
        if plan == "advance2":
            b.advance(d, fc, 1.0 / 64, 2)
        elif plan == "advance1x2":
            b.integrate(d, fc, 1.0 / 64)
            b.integrate(d, fc, 1.0 / 64)
        else:
            b.prime(d, fc, 1.0 / 64)
            while b.info()["macro_steps"] < 2:
                b.block_step(d, fc, 1.0 / 64, 1)
        runs.append(_bits_ext(b, d))
    for r in runs[1:]:
        assert np.array_equal(r, runs[0])
    assert b.info()["block_steps"] > 2  # (levels are in use)


# (n = 32768: every body active, the gathered extended sweep with four targets per lane; one step, 10^9 pairs a sweep)
@pytest.mark.parametrize("n,eps", [(n, eps) for eps in (0.01, 0.0) for n in (1, 2, 257, 4096)] + [(32768, 0.05), (32768, 0.0)])
def test_block_at_max_level_0_is_the_shared_extended_step(nb, ctx, n, eps):
    X, V, m = _cluster(nb, n, "scale0.05_at_64")
    fc = _direct(nb, 1.0, eps)
    out = []
    for kind in ("shared", "block"):
        d, _ = to_device(nb, _ic_of(np.zeros_like(X), np.zeros_like(X), m))
        integ = nb.HermiteIntegrator() if kind == "shared" else nb.BlockHermiteIntegrator()
        if kind == "block":
            integ.setParameters(0.02, 0.01, 0)
        integ.setStatePrecision("extended")
        integ.setExtendedState(d, X, V, fc)
        for _ in range(1 if n == 32768 else 3):
            integ.integrate(d, fc, 1.0 / 256)
        out.append(_bits_ext(integ, d))
    assert np.array_equal(out[0], out[1])


@pytest.mark.parametrize("eps", [0.05, 0.0])
@pytest.mark.parametrize("n", [257, 12289, 32768])
def test_zero_residuals_evaluate_as_the_fp32_mode(nb, ctx, n, eps):
    """an fp32-representable state with residuals 0: the lo differences are exact zeros, a and j those of the fp32 sweep"""
    ic = nb.ic.plummer(n, seed=42)
    d, _ = to_device(nb, ic)
    acc, jerk = nb.direct_acc_jerk(ctx, d, 1.7, eps)
    acc_e, jerk_e = nb.direct_acc_jerk_ext(ctx, d, torch.zeros((n, 4), dtype=torch.float32, device="cuda"), 1.7, eps)
    assert torch.equal(acc.view(torch.int32), acc_e.view(torch.int32))
    assert torch.equal(jerk.view(torch.int32), jerk_e.view(torch.int32))


def test_fp32_mode_is_untouched_by_a_visit_to_extended(nb, ctx):
    ic = nb.ic.plummer(1000, seed=42)
    fc = _direct(nb, 1.0, 0.05)
    out = []
    for visit in (False, True):
        d, _ = to_device(nb, ic)
        h = nb.HermiteIntegrator()
        if visit:
            h.setStatePrecision("extended")
            h.prime(d, fc)
            h.setStatePrecision("fp32")
        assert h.getStatePrecision() == "fp32"
        h.integrate_steps(d, fc, 1e-2, 3)
        out.append(np.concatenate([v.view(np.uint32) for v in _state(d).values()]))
    assert np.array_equal(out[0], out[1])


# ---- 7. the point of it ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def refs():
    return xr.references()


def _run_shared(nb, X, V, m, eps, dt, steps, precision):
    fc = _direct(nb, 1.0, eps)
    d, _ = to_device(nb, _ic_of(X, V, m))
    h = nb.HermiteIntegrator()
    h.setStatePrecision(precision)
    h.setExtendedState(d, X, V, fc)
    h.integrate_steps(d, fc, dt, steps)
    return h.getExtendedState(d)[0]


def test_binary_one_period(nb, ctx, refs):
    """hermite_ref.binary(e = 0.9), eps 1e-4, 25,600 steps over one period, centred and at (20, 10, 0): max |dx| against
    the fp64 run of tests/golden/hermite_ext_refs.npz.  The arithmetic model (tests/test_hermite_ext_cpu.py) gives
    1 / 64 and 1 / 8,400; held: 1 / 10 and 1 / 100.  Measured on an MI355X: centred 4.0e-8 against 1.42e-5 (1 / 353), displaced
    4.5e-8 against 9.34e-4 (1 / 20,900)."""
    c = xr.BINARY
    err = {}
    for displaced, key in ((False, "binary_centred_ref"), (True, "binary_displaced_ref")):
        X, V, m = xr.binary_state(displaced)
        for precision in ("fp32", "extended"):
            x = _run_shared(nb, X, V, m, c["eps"], c["T"] / c["steps"], c["steps"], precision)
            err[displaced, precision] = np.abs(x - refs[key]).max()
    print("binary, one period, max |dx|:", {f"{'displaced' if k[0] else 'centred'} {k[1]}": f"{v:.3e}" for k, v in err.items()},
          flush=True)
    assert err[False, "extended"] <= err[False, "fp32"] / 10
    assert err[True, "extended"] <= err[True, "fp32"] / 100


def test_block_scheme_gains_from_a_smaller_eta_only_in_extended_mode(nb, ctx, refs):
    """section 4.10's binary case (e = 0.9 and the light body, dt_max = T / 16, L = 16) at (20, 10, 0), eta 0.02 and 0.005:
    the error must fall in extended mode and must not fall by more than 2 x in fp32 mode (the restatement shows the pair
    of conditions with these inputs: tests/test_hermite_ext_cpu.py).  Measured on an MI355X: extended 6.12e-6 -> 3.23e-7,
    fp32 9.74e-4 -> 3.18e-3."""
    c = xr.BLOCK
    X, V, m = xr.block_state()
    fc = _direct(nb, 1.0, c["eps"])
    err = {}
    for precision in ("fp32", "extended"):
        for eta in c["etas"]:
            d, _ = to_device(nb, _ic_of(X, V, m))
            b = nb.BlockHermiteIntegrator()
            b.setParameters(eta, 0.01, c["L"])
            b.setStatePrecision(precision)
            b.setExtendedState(d, X, V, fc)
            b.advance(d, fc, c["T"] / c["macro"], c["macro"])
            err[precision, eta] = np.abs(b.getExtendedState(d)[0] - refs["block_displaced_ref"]).max()
    print("block scheme, displaced binary, max |dx|:", {f"{k[0]} eta {k[1]}": f"{v:.3e}" for k, v in err.items()}, flush=True)
    e1, e2 = c["etas"]
    assert err["extended", e2] < err["extended", e1]
    assert err["fp32", e2] >= err["fp32", e1] / 2


# ---- 8. state handling -------------------------------------------------------------------------------------------------
def test_set_get_round_trip_and_fp32_mode_widens(nb, ctx):
    X, V, m = _cluster(nb, 257, "scale0.01_at_1000")
    fc = _direct(nb, 1.0, 0.01)
    for integ in (nb.HermiteIntegrator(), nb.BlockHermiteIntegrator()):
        d, _ = to_device(nb, _ic_of(np.zeros_like(X), np.zeros_like(X), m))
        integ.setStatePrecision("extended")
        integ.setExtendedState(d, X, V, fc)
        Xg, Vg = integ.getExtendedState(d)
        assert np.array_equal(Xg, xr.rnd2(X)) and np.array_equal(Vg, xr.rnd2(V))  # exact to the representation
        assert np.abs(Xg - X).max() <= 2.0 ** -49 * np.abs(X).max()
        s = _state(d)
        assert np.array_equal(_col(s, "pos"), X.astype(np.float32).astype(np.float64))
        integ.setStatePrecision("fp32")
        Xg, Vg = integ.getExtendedState(d)
        assert np.array_equal(Xg, X.astype(np.float32).astype(np.float64))
        assert np.array_equal(Vg, V.astype(np.float32).astype(np.float64))
        integ.setStatePrecision("extended")  # a switch to extended starts with residuals 0
        assert np.array_equal(integ.getExtendedState(d)[0], Xg)
        with pytest.raises(nb.ValidationException):
            integ.setStatePrecision("fp64")
        with pytest.raises(nb.ValidationException):
            integ.setExtendedState(d, X[:-1], V[:-1], fc)
    lib = nb._lib.load()
    with pytest.raises(nb.ValidationException, match="state precision must be 0"):
        nb._lib.check(lib.nbody_hip_hermite_set_precision(integ._h, 2))


def test_invalidate_zeroes_the_residuals_and_parameter_changes_keep_them(nb, ctx):
    X, V, m = _cluster(nb, 257, "scale0.05_at_64")
    for kind in ("shared", "block"):
        fc = _direct(nb, 1.0, 0.01)
        d, _ = to_device(nb, _ic_of(np.zeros_like(X), np.zeros_like(X), m))
        integ = nb.HermiteIntegrator() if kind == "shared" else nb.BlockHermiteIntegrator()
        integ.setStatePrecision("extended")
        integ.setExtendedState(d, X, V, fc)
        integ.integrate(d, fc, 1.0 / 64)
        X1, V1 = integ.getExtendedState(d)
        assert np.abs(X1 - X1.astype(np.float32)).max() > 0
        # G, eps, dt: the step primes again by itself and keeps the residuals -- the run equals one that was handed
        # the extended state afresh
        fc.setGravitationalConstant(1.5)
        fc.setSofteningParameter(0.02)
        integ.integrate(d, fc, 1.0 / 128)
        d2, _ = to_device(nb, _ic_of(np.zeros_like(X), np.zeros_like(X), m))
        other = nb.HermiteIntegrator() if kind == "shared" else nb.BlockHermiteIntegrator()
        other.setStatePrecision("extended")
        other.setExtendedState(d2, X1, V1, fc)
        other.integrate(d2, fc, 1.0 / 128)
        assert np.array_equal(_bits_ext(integ, d), _bits_ext(other, d2))
        # invalidate: the fp32 arrays are the truth
        integ.invalidate()
        Xi, Vi = integ.getExtendedState(d)
        s = _state(d)
        assert np.array_equal(Xi, _col(s, "pos")) and np.array_equal(Vi, _col(s, "vel"))


def test_err_state_in_the_middle_of_a_macro_step(nb, ctx):
    X, V, m = _cluster(nb, 257, "scale0.05_at_64")
    fc = _direct(nb, 1.0, 0.01)
    d, _ = to_device(nb, _ic_of(np.zeros_like(X), np.zeros_like(X), m))
    b = nb.BlockHermiteIntegrator()
    b.setParameters(0.02, 0.01, 6)
    b.setStatePrecision("extended")
    b.setExtendedState(d, X, V, fc)
    b.block_step(d, fc, 1.0 / 16, 1)
    assert b.info()["current_tick"] != 0
    with pytest.raises(nb.StateException, match="middle of a macro step"):
        b.setStatePrecision("fp32")
    with pytest.raises(nb.StateException, match="middle of a macro step"):
        b.setExtendedState(d, X, V, fc)
    assert b.getStatePrecision() == "extended"  # (the refused switch left the mode alone)
    b.advance(d, fc, 1.0 / 16, 1)  # and the macro step can still be finished
    assert b.info()["current_tick"] == 0


def _system(nb, ic, scheme, precision, dt=1.0 / 64, eps=0.01):
    ps = nb.ParticleSystem()
    ps.setIntegrationScheme(scheme)
    ps.setHermiteStatePrecision(precision)
    ps.initialize(nb.SimulationConfig(particle_count=ic["mass"].size, force_method=nb.ForceMethod.DIRECT_N2, dt=dt, G=1.0,
                                      softening=eps), ic)
    return ps


@pytest.mark.parametrize("scheme", ["hermite4", "hermite4-block"])
def test_particle_system(nb, ctx, scheme, tmp_path):
    X, V, m = _cluster(nb, 257, "scale0.05_at_64")
    ic = _ic_of(X, V, m)
    ps = _system(nb, ic, scheme, "extended")
    assert ps.getHermiteStatePrecision() == "extended"
    for _ in range(3):
        ps.update(1.0 / 64)
    Xe, Ve = ps.getExtendedState()
    st = ps.getState()
    pos32, vel32 = np.stack([st.pos_x, st.pos_y, st.pos_z], 1), np.stack([st.vel_x, st.vel_y, st.vel_z], 1)
    assert np.all(np.abs(Xe - pos32) <= 0.5 * np.spacing(np.abs(pos32)))  # pos_* are the hi parts of the extended state
    assert np.all(np.abs(Ve - vel32) <= 0.5 * np.spacing(np.abs(vel32)))
    assert np.abs(Xe - pos32).max() > 0                                   # and the residuals are in use
    # G, eps and dt alone keep the residuals
    ps.setGravitationalConstant(1.5)
    ps.setSofteningParameter(0.02)
    ps.setTimeStep(1.0 / 128)
    assert np.array_equal(ps.getExtendedState()[0], Xe)
    # saveState writes the fp32 arrays; loadState continues from the ROUNDED state: the run of a fresh system started there
    path = str(tmp_path / "state.bin")
    ps.saveState(path)
    ps.loadState(path)
    Xl, Vl = ps.getExtendedState()
    assert np.array_equal(Xl, pos32.astype(np.float64)) and np.array_equal(Vl, vel32.astype(np.float64))
    st = ps.getState()
    fresh = _system(nb, {k: getattr(st, k) for k in ("pos_x", "pos_y", "pos_z", "vel_x", "vel_y", "vel_z", "mass")}, scheme,
                    "extended", eps=0.02)
    fresh.setGravitationalConstant(1.5)
    for _ in range(2):
        ps.update(1.0 / 128)
        fresh.update(1.0 / 128)
    assert np.array_equal(ps.getExtendedState()[0], fresh.getExtendedState()[0])
    # a switch of the scheme or of the mode loses the residuals
    ps.setHermiteStatePrecision("fp32")
    s = ps.getState()
    assert np.array_equal(ps.getExtendedState()[0], np.stack([s.pos_x, s.pos_y, s.pos_z], 1).astype(np.float64))


# ---- the facade's program ----------------------------------------------------------------------------------------------
def test_facade_hermite_ext_program(nb, ctx):
    exe = os.path.join(ROOT, "n-body_amd", "lib", "hermite_ext_tests")
    assert os.path.exists(exe), "build with __graft_entry__.build()"
    env = dict(os.environ)
    env["LD_LIBRARY_PATH"] = os.path.dirname(exe) + os.pathsep + env.get("LD_LIBRARY_PATH", "")
    r = subprocess.run([exe], cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    print(r.stdout)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    got = dict(re.findall(r"^hermite_ext (\S+) (\S+)$", r.stdout, re.M))
    # the same two macro steps through the Python host: the same bits in hi and lo
    n = 1000
    hst = nb.ParticleData()
    nb.ParticleDataManager.allocateHost(hst, n)
    nb.ParticleInitializer.initUniform(hst, nb.UniformDistParams((-1, -1, -1), (1, 1, 1), 0.5, 1.5), 7)
    X = np.stack([hst.pos_x, hst.pos_y, hst.pos_z], 1).astype(np.float64) * 0.05 + np.array([64.0, -32.0, 16.0])
    V = np.stack([np.float32(0.1) * hst.pos_y, np.float32(-0.1) * hst.pos_x, np.zeros(n, np.float32)], 1).astype(np.float64)
    d = nb.ParticleData()
    nb.ParticleDataManager.allocateDevice(d, n)
    nb.ParticleDataManager.copyToDevice(d, hst)
    fc = _direct(nb, float(np.float32(1.7)), float(np.float32(0.01)))
    b = nb.BlockHermiteIntegrator()
    b.setParameters(0.02, 0.01, 6)
    b.setStatePrecision("extended")
    b.setExtendedState(d, X, V, fc)
    b.advance(d, fc, 1.0 / 64, 2)
    Xe, Ve = b.getExtendedState(d)
    fnv = 1469598103934665603
    st = _state(d)
    parts = [st[k] for k in F[:6]]  # the hi parts, then the residuals of pos and of vel as [N][3] arrays
    parts += [(Z - _col(st, name)).astype(np.float32) for Z, name in ((Xe, "pos"), (Ve, "vel"))]
    for part in parts:
        for byte in np.ascontiguousarray(part).tobytes():
            fnv = ((fnv ^ byte) * 1099511628211) & 0xFFFFFFFFFFFFFFFF
    assert got["fnv"] == f"{fnv:016x}"
    assert got["precision"] == "extended"

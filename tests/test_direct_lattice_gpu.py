"""Every form of the Direct N^2 kernels, pair by pair, on an exact integer lattice (direct_lattice_ref.py).

Bodies on distinct integer sites, small integer masses, G = 1, eps^2 = 2^40: every intermediate of every kernel is
2^-60 times an integer below 2^24, so the result does not depend on the order of the sums, on atomics or on the bodies
per lane, and equals the O(N) int64 formula BIT FOR BIT on every body.  One pair left out, counted twice or credited to
another body or slot moves a body by at least one whole unit, whatever N is -- where the 1e-5 oracle tests of
test_direct_gpu.py see a single pair only when it is large.

The one thing the argument takes from the hardware is v_rsq_f32(2^40) == 2^-20 exactly (the instruction is specified to
1 ulp).  PREFLIGHT OUTCOME, measured on an MI355X: EXACT -- the two-body case below gives 2^-60 (5, -3, 2) bit for bit
through every form of the one-sided kernel (scalar, packed and scalar-cache bodies at 1, 2, 4 targets per lane) and
through the symmetric one (test_preflight_two_bodies loops over them), so every comparison in this file is an equality (torch.equal on the device; a failure copies back and decodes body and partner).

The eps^2 < 1e-12 GUARD instantiations are not reached (the construction needs the large softening): test_edge_cases
keeps covering them."""
import numpy as np
import pytest
import torch

import direct_lattice_ref as L
from gpu_util import to_device

pytestmark = pytest.mark.gpu


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


# Every PACKED body array handed to the packed entry points (all of them are built by _bodies) is followed, in the same
# allocation, by one more row: a body of mass 5 inside the box that belongs to no set.  (The SoA arrays that to_device
# allocates and the points of the field calls carry none.)  A kernel that reads one row too many (j <= n for j < n) stays inside the allocation and
# pairs everybody with it: a whole-unit error like any other wrong pair, instead of whatever the next allocation holds
# (it decodes as "no single partner" with delta = m (canary - p_i), m = 5 or the common mass factor).
CANARY = np.array([[7, -5, 3, 5]], np.float32)


def _bodies(packed):
    return _dev(np.concatenate([packed, CANARY]))[:packed.shape[0]]


_CACHE = {}


def _case(n, assignment, masses, keep=False):
    """(lattice, packed bodies on the device, expected float4 rows on the device); keep: shared by the tests of a session"""
    key = (n, assignment, masses)
    if key in _CACHE:
        return _CACHE[key]
    lat = L.lattice(n, assignment, masses)
    case = (lat, _bodies(lat.packed), _dev(L.acc_rows(L.expect_all_pairs(lat))))
    if keep:
        _CACHE[key] = case
    return case


def _same(got, want, lat, ref_u, R, tag, src=None, scale=L.UNIT):
    """got == want on the device -- all bodies, all three components, column 3 zero; on a mismatch the first failing
    bodies are copied back and decoded (src: the partners are another set's bodies)"""
    if torch.equal(got, want):
        return
    g = got.cpu().numpy()
    col3 = "" if np.all(g[:, 3] == 0) else f"; column 3 is not zero on {int((g[:, 3] != 0).sum())} bodies"
    pytest.fail(f"{tag}{col3}\n" + L.describe(lat, L.units(g, scale), ref_u, R, src))


def test_preflight_two_bodies(nb, ctx):
    """v_rsq_f32(2^40) is exactly 2^-20: the whole tier stands on it (see the docstring of this file)"""
    p = _bodies(np.array([[0, 0, 0, 1], [5, -3, 2, 1]], np.float32))
    want = np.array([[5, -3, 2, 0], [-5, 3, -2, 0]], np.float64) * L.UNIT
    try:
        # the automatic choice, every form of the one-sided kernel, the symmetric kernel (slots: the default mode)
        for variant, tpl in ((-1, 0),) + L.ONE_SIDED_FORMS + ((3, 2), (3, 16)):
            ctx.tuning(variant, tpl, 0)
            a = nb.direct_forces_packed(ctx, p, p, L.G, L.EPS2).cpu().numpy()
            assert ctx.directInfo()["last_kernel"] == (2 if variant == 3 else 0)
            assert np.array_equal(a.astype(np.float64), want), (variant, tpl, (a.astype(np.float64) / L.UNIT).tolist())
    finally:
        ctx.tuning()


# ---- one-sided direct_kernel ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("masses", ["threes", "g0123"])
@pytest.mark.parametrize("variant,tpl", L.ONE_SIDED_FORMS)
def test_one_sided_all_pairs(nb, ctx, variant, tpl, masses):
    try:
        for n in L.ONE_SIDED_SIZES:
            for assignment in L.ASSIGNMENTS:
                lat, p, want = _case(n, assignment, masses, keep=True)
                for splits in L.ONE_SIDED_SPLITS:   # 64: more than there are tiles
                    ctx.tuning(variant, tpl, splits)
                    a = nb.direct_forces_packed(ctx, p, p, L.G, L.EPS2)
                    assert ctx.directInfo()["last_kernel"] == 0
                    _same(a, want, lat, L.expect_all_pairs(lat), tpl, f"one-sided variant {variant}, {tpl} targets per "
                          f"lane, {splits} splits, n = {n}, {assignment}")
    finally:
        ctx.tuning()


@pytest.mark.parametrize("assignment", L.ASSIGNMENTS)
def test_one_sided_targets_are_not_the_sources(nb, ctx, assignment):
    src, p, _ = _case(2049, assignment, "g0123", keep=True)
    ref = L.expect_all_pairs(src)
    # 333 points of the lattice: every third one on a body, the rest on free sites (even = whole coordinates)
    free = L.lattice(L.NSITES, assignment).p[2049:]
    pts = free[:333].copy()
    pts[::3] = src.p[5:5 + 111 * 17:17]
    u2, _ = L.expect_points(2 * pts, src)
    assert np.all(u2 % 2 == 0)
    t = _bodies(np.concatenate([pts, np.zeros((333, 1))], 1).astype(np.float32))
    want_pts = _dev(L.acc_rows(u2 // 2))
    points = L.Lattice(pts, np.zeros(333, np.int64))
    whole = L.Lattice(src.p, np.zeros(src.n, np.int64))
    # a target sub-range against all sources (the sharded form), and accumulate onto an integer prefill
    lo, hi = 700, 1400
    sub = _bodies(src.packed[lo:hi])
    want_sub = _dev(L.acc_rows(ref[lo:hi]))
    pre = np.random.default_rng(3).integers(-1000, 1001, (hi - lo, 3))
    want_acc = _dev(L.acc_rows(ref[lo:hi], prefill=pre))
    try:
        for variant, tpl in L.ONE_SIDED_FORMS:
            for splits in (0, 3):
                ctx.tuning(variant, tpl, splits)
                tag = f"variant {variant}, {tpl} targets per lane, {splits} splits"
                a = nb.direct_forces_packed(ctx, t, p, L.G, L.EPS2)
                assert ctx.directInfo()["last_kernel"] == 0
                _same(a, want_pts, points, u2 // 2, tpl, f"333 points against 2,049 bodies, {tag}", src)
                a = nb.direct_forces_packed(ctx, sub, p, L.G, L.EPS2)
                _same(a, want_sub, whole.cut(lo, hi), ref[lo:hi], tpl, f"targets [{lo}, {hi}) against all sources, {tag}", src)
                out = _dev(L.acc_rows(pre))
                nb.direct_forces_packed(ctx, sub, p, L.G, L.EPS2, out=out, accumulate=True)
                assert torch.equal(out, want_acc), f"accumulate onto a prefilled array, {tag}"
    finally:
        ctx.tuning()


# ---- symmetric kernel, all pairs --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("masses", L.MASSES)
@pytest.mark.parametrize("R", L.SYM_R)
def test_symmetric_all_pairs(nb, ctx, R, masses):
    """variant 3 (and 4 at 16 bodies per lane) x slots / atomics x splits, at the smallest sizes that reach every branch
    of the half ring; every result equals the formula, hence every other result, bit for bit"""
    try:
        for n in L.sym_sizes(R):
            for assignment in L.ASSIGNMENTS:
                lat, p, want = _case(n, assignment, masses)
                for mode, kernel in ((2, 2), (0, 1)):     # slot planes required / fp64 atomics
                    ctx.deterministic(mode)
                    for variant in ((3, 4) if R == 16 else (3,)):
                        for splits in L.SYM_SPLITS:
                            ctx.tuning(variant, R, splits)
                            a = nb.direct_forces_packed(ctx, p, p, L.G, L.EPS2)
                            info = ctx.directInfo(n, L.EPS2)
                            assert info["last_kernel"] == kernel == info["kernel"]
                            assert info["bodies_per_lane_equal"] == R and info["bodies_per_lane_general"] == R
                            _same(a, want, lat, L.expect_all_pairs(lat), R, f"symmetric variant {variant}, {R} bodies per "
                                  f"lane, {'slots' if mode else 'atomics'}, {splits} splits, n = {n}, {assignment}, {masses}")
    finally:
        ctx.deterministic(True)
        ctx.tuning()


@pytest.mark.parametrize("masses", ["ones", "g0123"])
def test_symmetric_long_rings(nb, ctx, masses):
    """the half ring with many partners: 40 superblocks (20 of them skip the partner at d = 20), 39, 40 with one body in
    the last one -- and the automatic choice of a plain call on all 20,480 sites (symmetric from 12,288 bodies on)"""
    try:
        for R, n in L.LONG_RINGS:
            for assignment in L.ASSIGNMENTS:
                lat, p, want = _case(n, assignment, masses)
                for mode, kernel in ((2, 2), (0, 1)):
                    ctx.deterministic(mode)
                    for splits in (0, 5):
                        ctx.tuning(3 if R else -1, R, splits)
                        a = nb.direct_forces_packed(ctx, p, p, L.G, L.EPS2)
                        info = ctx.directInfo(n, L.EPS2)
                        assert info["last_kernel"] == kernel == info["kernel"]
                        Rr = R or 6     # the automatic choice below 28,000 bodies: 6 per lane, 14 superblocks here
                        assert info["bodies_per_lane_equal"] == Rr and info["bodies_per_lane_general"] == Rr
                        _same(a, want, lat, L.expect_all_pairs(lat), Rr, f"symmetric, {Rr} bodies per lane, "
                              f"{'slots' if mode else 'atomics'}, {splits} splits, n = {n}, {assignment}, {masses}")
    finally:
        ctx.deterministic(True)
        ctx.tuning()


# ---- symmetric kernel, two disjoint sets --------------------------------------------------------------------------------------
@pytest.mark.parametrize("masses", L.RECT_MASSES)
@pytest.mark.parametrize("R", L.RECT_R)
def test_symmetric_two_sets(nb, ctx, R, masses):
    """the pair kernel against an independent reference: forces on A from B and the reactions on B, outputs prefilled
    with 7.0 and overwritten; once per shape accumulated onto an integer prefill.  equal3: the common mass factor m0 = 3,
    which the atomic form applies in the kernel and the slot form in the finalize pass"""
    try:
        for shape in L.rect_shapes(R):
            for assignment in L.ASSIGNMENTS:
                A, B = L.rect_sets(R, shape, assignment, masses)
                ua, ub = L.expect_two_sets(A, B)
                pa, pb = _bodies(A.packed), _bodies(B.packed)
                want_a, want_b = _dev(L.acc_rows(ua)), _dev(L.acc_rows(ub))
                for mode, kernel in ((2, 2), (0, 1)):
                    ctx.deterministic(mode)
                    for variant in ((-1, 4) if R == 16 else (-1,)):
                        for splits in L.RECT_SPLITS:
                            ctx.tuning(variant, R, splits)
                            acc_a = torch.full((A.n, 4), 7.0, device="cuda")
                            acc_b = torch.full((B.n, 4), 7.0, device="cuda")
                            nb.direct_forces_pair_packed(ctx, pa, pb, L.G, L.EPS2, acc_a, acc_b)
                            assert ctx.directInfo()["last_kernel"] == kernel
                            tag = (f"two sets {shape}, variant {variant}, {R} bodies per lane, {'slots' if mode else 'atomics'}, "
                                   f"{splits} splits, {assignment}, {masses}")
                            _same(acc_a, want_a, A, ua, R, tag + ": forces on A (partners in B)", B)
                            _same(acc_b, want_b, B, ub, R, tag + ": reactions on B (partners in A)", A)
                    # accumulate_a / accumulate_b onto an integer prefill
                    rng = np.random.default_rng(A.n)
                    fa, fb = rng.integers(-1000, 1001, (A.n, 3)), rng.integers(-1000, 1001, (B.n, 3))
                    acc_a, acc_b = _dev(L.acc_rows(fa)), _dev(L.acc_rows(fb))
                    nb.direct_forces_pair_packed(ctx, pa, pb, L.G, L.EPS2, acc_a, acc_b, accumulate_a=True, accumulate_b=True)
                    assert torch.equal(acc_a, _dev(L.acc_rows(ua, prefill=fa))), f"accumulate_a, two sets {shape}, R = {R}, mode {mode}"
                    assert torch.equal(acc_b, _dev(L.acc_rows(ub, prefill=fb))), f"accumulate_b, two sets {shape}, R = {R}, mode {mode}"
    finally:
        ctx.deterministic(True)
        ctx.tuning()


# ---- the SoA entry point and the fused Velocity-Verlet step ---------------------------------------------------------------------
def _soa(lat):
    z = np.zeros(lat.n, np.float32)
    return dict(pos_x=lat.p[:, 0].astype(np.float32), pos_y=lat.p[:, 1].astype(np.float32), pos_z=lat.p[:, 2].astype(np.float32),
                vel_x=z, vel_y=z, vel_z=z, mass=lat.m.astype(np.float32))


def _soa3(d, stem):
    return torch.stack([getattr(d, stem + "_x"), getattr(d, stem + "_y"), getattr(d, stem + "_z")], 1)


@pytest.mark.parametrize("assignment", L.ASSIGNMENTS)
def test_soa_forces_and_fused_kick(nb, ctx, assignment):
    """DirectForceCalculator.computeForces and three Integrator.integrate steps at n = 2 S + 1, 6 bodies per lane, symmetric
    kernel forced.  dt = 2^-4, zero initial velocities, and no body has a zero coordinate: the drift moves a body by
    a dt^2 / 2 < 1e-14, far below half an ulp of a coordinate of at least 1, so the positions stay ON the lattice, every
    evaluation returns the same integers and the k-th kick gives v = k dt a exactly (k u < 2^24)."""
    R, dt = 6, 2.0 ** -4
    n = 2 * 256 * R + 1
    lat = L.lattice(n, assignment, "g123", nonzero=True)
    ref = L.expect_all_pairs(lat)
    assert 3 * np.abs(ref).max() < 2 ** 24
    want = _dev(L.acc_rows(ref)[:, :3])
    fc = nb.DirectForceCalculator()
    fc.setGravitationalConstant(L.G)
    fc.setSofteningParameter(L.EPS)
    assert fc.softening_eps2_ == L.EPS2
    integ = nb.Integrator()
    d, _ = to_device(nb, _soa(lat))
    pos0 = _soa3(d, "pos").clone()
    try:
        ctx.tuning(3, R, 0)
        fc.computeForces(d)
        info = ctx.directInfo(n, L.EPS2)
        assert info["last_kernel"] == 2 and info["bodies_per_lane_equal"] == R and info["bodies_per_lane_general"] == R
        a = _soa3(d, "acc")
        assert torch.equal(a, want), "computeForces (SoA)\n" + L.describe(lat, L.units(a.cpu().numpy()), ref, R)
        for k in (1, 2, 3):
            integ.integrate(d, fc, dt)
            assert ctx.directInfo()["last_kernel"] == 2
            v = _soa3(d, "vel")
            if k == 1:    # the first kick: half_dt (a_old + a_new), both from the integer reference
                half = _dev((L.acc_rows(2 * ref, scale=L.UNIT * dt / 2))[:, :3])
                assert torch.equal(v, half), "first kick\n" + L.describe(lat, L.units(v.cpu().numpy(), L.UNIT * dt), ref, R)
            assert torch.equal(_soa3(d, "pos"), pos0), f"step {k}: a body left the lattice"
            assert torch.equal(_soa3(d, "acc"), want) and torch.equal(_soa3(d, "acc_old"), want), f"step {k}"
            assert torch.equal(v, _dev(L.acc_rows(k * ref, scale=L.UNIT * dt)[:, :3])), f"kick {k}"
    finally:
        ctx.tuning()


# ---- direct_field_kernel ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("assignment", L.ASSIGNMENTS)
@pytest.mark.parametrize("n_src", L.FIELD_SOURCES)
def test_field_at_points(nb, ctx, n_src, assignment):
    """computeField (the entry point of test_field_gpu.py): 300 points run 2 points per lane, 40,000 run 4 (one_sided_shape
    switches at 32,768); every third point sits on a body (d = 0 to the force, m_j to the potential), the others on the
    half-integer lattice (their u is a multiple of 1/2: exact all the same)"""
    src = L.lattice(n_src, assignment, "g0123")
    fc = nb.DirectForceCalculator()
    fc.setGravitationalConstant(L.G)
    fc.setSofteningParameter(L.EPS)
    d, _ = to_device(nb, _soa(src))
    for count in L.FIELD_POINTS:
        pts2 = L.field_points2(count, src)
        u2, msum = L.expect_points(pts2, src)
        want = L.acc_rows(u2, scale=L.UNIT / 2)
        want[:, 3] = np.float32(-L.G * L.PHI_UNIT * msum)
        assert float(want[0, 3]) == -L.PHI_UNIT * msum
        out = fc.computeField(d, _dev((pts2 / 2.0).astype(np.float32)))
        if not torch.equal(out, _dev(want)):
            o = out.cpu().numpy()
            phi_bad = np.nonzero(o[:, 3] != want[:, 3])[0]
            pytest.fail(f"{count} points against {n_src} bodies: potential differs at {phi_bad.size} points "
                        f"(first {phi_bad[:4].tolist()}: {(-o[phi_bad[:4], 3].astype(np.float64) / L.PHI_UNIT).tolist()} for {msum})\n"
                        + L.describe(L.Lattice(pts2, np.zeros(count, np.int64)), L.units(o, L.UNIT / 2), u2, 4 if count >= 32768 else 2,
                                     L.Lattice(2 * src.p, src.m)))

"""Restatement in numpy of the EXTENDED STATE PRECISION of the two Hermite integrators (csrc/hermite_common.h; the model
is written out in include/nbody_hip.h and DESIGN.md section 4.11).  It restates on top of tests/hermite_ref.py and
tests/hermite_block_ref.py, which it leaves as they are.

The state of body i is the double-single pair X = hi + lo, V = hi + lo: hi = fl32(X), lo = fl32(X - hi).  Predictor and
corrector are the fp64 expressions of hermite_ref.hermite_steps evaluated from hi + lo and rounded to hi + lo instead
of to fp32; a and j stay fp32.  The pair sweep sees {xp_hi, xp_lo, vp_hi} and forms
    d = (x_j,hi - x_i,hi) + (x_j,lo - x_i,lo)        in fp32, in that association,
    w = v_j,hi - v_i,hi                              in fp32.
Two evaluations are given: acc_jerk_ext, the ARITHMETIC MODEL of that sweep (fp32 pair arithmetic from d and w on, the
sums in fp64 -- what the figures of the issue were computed with), and hermite_ref.acc_jerk on hi + lo in fp64, the
reference the engine and the model are held against.
"""
import os

import numpy as np

import hermite_block_ref as hbr
import hermite_ref as hr

F32 = np.float32
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "hermite_ext_refs.npz")


def split(X):
    """fp64 -> (hi, lo), both fp32 values held in fp64 arrays: hi = fl32(X), lo = fl32(X - hi)"""
    X = np.asarray(X, np.float64)
    hi = X.astype(F32).astype(np.float64)
    lo = (X - hi).astype(F32).astype(np.float64)
    return hi, lo


def rnd2(X):
    """X rounded to the hi + lo representation (|X - rnd2(X)| <= 2^-49 |X|)"""
    hi, lo = split(X)
    return hi + lo


# A note on ties.  hi is the fp32 number nearest to the UNROUNDED fp64 value; lo = fl32(X - hi) can round up to exactly
# half an ulp of hi, and then hi + lo is an exact tie between hi and its neighbour: fl32(hi + lo) goes to the even one,
# which need not be hi.  Velocities sit near such ties often (v + (a0 + a1) h / 2 is a short dyadic number when h is a
# power of two, and the jerk term is tiny), so the hi parts are carried along explicitly (pos_hi, vel_hi below) and are
# never recovered by rounding hi + lo.  In the engine pos_* / vel_* are those hi parts.


def acc_jerk_ext(hi, lo, vel, m, G, eps, targets=None, use_lo=True, block=256):
    """The arithmetic model of the extended pair sweep: (a [T, 3], j [T, 3]) in fp64.  Positions hi + lo (fp32 each),
    velocities `vel` (their hi parts); every pair quantity in fp32 (numpy's fp32 operations, unfused: the engine's fused
    multiply-adds and its v_rsq_f32 differ from these in the last bit), the terms summed in fp64.  use_lo=False drops the
    residuals: the fp32 mode's d = fl(x_j) - fl(x_i)."""
    hi = np.asarray(hi, np.float64).astype(F32)
    lo = np.asarray(lo, np.float64).astype(F32)
    v = np.asarray(vel, np.float64).astype(F32)
    mm = np.asarray(m, F32)
    idx = np.arange(len(hi)) if targets is None else np.asarray(targets)
    e2 = F32(hr.eps2_of(eps))
    guard = e2 < 1e-12
    a = np.zeros((len(idx), 3))
    j = np.zeros((len(idx), 3))
    for b in range(0, len(idx), block):
        t = idx[b:b + block]
        d = hi[None, :, :] - hi[t, None, :]
        if use_lo:
            d = d + (lo[None, :, :] - lo[t, None, :])
        w = v[None, :, :] - v[t, None, :]
        d2 = (d * d).sum(2, dtype=F32)
        dw = (d * w).sum(2, dtype=F32)
        with np.errstate(divide="ignore", invalid="ignore"):
            inv = F32(1.0) / np.sqrt(d2 + e2)
            if guard:
                inv = np.where(d2 > 0, inv, F32(0.0)).astype(F32)
            inv2 = inv * inv
            f = (mm[None, :] * inv) * inv2
            q = (dw * inv2) * F32(-3.0)
        ta = f[:, :, None] * d
        tj = f[:, :, None] * (q[:, :, None] * d + w)
        assert ta.dtype == F32 and tj.dtype == F32
        a[b:b + block] = G * ta.astype(np.float64).sum(1)
        j[b:b + block] = G * tj.astype(np.float64).sum(1)
    return a, j


def model_evaluate(m, G, eps, use_lo=True):
    """evaluate(xp, vp) for hermite_steps_ext: the arithmetic model on the split predicted state"""
    def ev(xp, vp):
        h, l = split(xp)
        return acc_jerk_ext(h, l, vp, m, G, eps, use_lo=use_lo)
    return ev


def hermite_steps_ext(pos, vel, m, G, eps, dt, steps, evaluate=None, acc=None, jerk=None):
    """hermite_ref.hermite_steps with the extended state: pos, vel fp64 (rounded to hi + lo on entry), a and j fp32, the
    predicted velocity the sweep sees fp32 (its hi part), the predicted position hi + lo.  evaluate(xp, vp) -> (a, j, ...)
    with xp = hi + lo in fp64 and vp fp32 values; default: the arithmetic model.  acc / jerk given: the run is seeded with
    them instead of priming (the GPU tests pass the engine's own).  -> dict(pos, vel, pos_hi, vel_hi, acc, acc_old, jerk,
    largest): pos and vel in fp64 (hi + lo), pos_hi and vel_hi their hi parts (what pos_* / vel_* hold); largest [N, 3]
    the largest term magnitude of the last corrector expression of pos."""
    if evaluate is None:
        evaluate = model_evaluate(m, G, eps)
    h = float(F32(dt))
    r32 = lambda z: np.asarray(z).astype(F32).astype(np.float64)  # noqa: E731
    (x_hi, x_lo), (v_hi, v_lo) = split(pos), split(vel)
    x, v = x_hi + x_lo, v_hi + v_lo
    if acc is None:
        a, j = evaluate(x, r32(v))[:2]
        a, j = r32(a), r32(j)
    else:
        a, j = np.asarray(acc, np.float64).copy(), np.asarray(jerk, np.float64).copy()
    a_old = np.zeros_like(a)
    largest = np.abs(x)
    for _ in range(steps):
        xp = rnd2(x + v * h + a * (0.5 * h * h) + j * (h * h * h / 6.0))
        vp = r32(v + a * h + j * (0.5 * h * h))
        a1, j1 = evaluate(xp, vp)[:2]
        a1, j1 = r32(a1), r32(j1)
        v_hi, v_lo = split(v + (a + a1) * (0.5 * h) + (j - j1) * (h * h / 12.0))
        v1 = v_hi + v_lo
        largest = np.maximum(np.abs(x), np.maximum(np.abs((v + v1) * (0.5 * h)), np.abs((a - a1) * (h * h / 12.0))))
        x_hi, x_lo = split(x + (v + v1) * (0.5 * h) + (a - a1) * (h * h / 12.0))
        x = x_hi + x_lo
        v, a_old, a, j = v1, a, a1, j1
    return dict(pos=x, vel=v, pos_hi=x_hi, vel_hi=v_hi, acc=a, acc_old=a_old, jerk=j, largest=largest)


class BlockHermiteExt(hbr.BlockHermite):
    """hermite_block_ref.BlockHermite with the extended state: x and v are held to hi + lo, a and j fp32; every body is
    predicted from hi + lo over its own h_i (position to hi + lo, velocity to fp32); the level rules are the parent's.
    x_hi, v_hi: the hi parts (what pos_* / vel_* hold).  evaluate(xp, vp, targets) as there; default: the arithmetic
    model."""

    def __init__(self, pos, vel, m, G, eps, dt_max, evaluate=None, **kw):
        mm = np.asarray(m)
        if evaluate is None:
            def evaluate(xp, vp, t):
                hi, lo = split(xp)
                return acc_jerk_ext(hi, lo, vp, mm, G, eps, targets=t)
        sweep = evaluate

        def evaluate(xp, vp, t):  # the sweep sees the hi part of a velocity, at priming too
            return sweep(xp, np.asarray(vp).astype(F32).astype(np.float64), t)
        # state_dtype float64: the parent keeps x and v as given (here: rounded to hi + lo); _rnd, which it applies to a
        # and j, is fp32 below
        super().__init__(rnd2(pos), rnd2(vel), m, G, eps, dt_max, state_dtype=np.float64, evaluate=evaluate, **kw)
        self.x_hi, self.v_hi = split(pos)[0], split(vel)[0]

    def _rnd(self, z):
        return np.asarray(z).astype(F32).astype(np.float64)

    def predicted(self, t):
        h = ((t - self.tick).astype(np.float64) * self.dt_max / 2.0 ** self.L)[:, None]
        xp = rnd2(self.x + self.v * h + self.a * (0.5 * h * h) + self.j * (h * h * h / 6.0))
        vp = self._rnd(self.v + self.a * h + self.j * (0.5 * h * h))
        return xp, vp

    def correct(self, A, t, a1, j1):
        # the parent's corrector rounds with _rnd: correct in hi + lo here, then let the parent do the bookkeeping with
        # these values in place
        h = (self.dt_max / 2.0 ** self.level[A])[:, None]
        x, v, a, j = self.x[A], self.v[A], self.a[A], self.j[A]
        v_hi, v_lo = split(v + (a + a1) * (0.5 * h) + (j - j1) * (h * h / 12.0))
        v1 = v_hi + v_lo
        x_hi, x_lo = split(x + (v + v1) * (0.5 * h) + (a - a1) * (h * h / 12.0))
        super().correct(A, t, a1, j1)
        self.x[A], self.v[A] = x_hi + x_lo, v1
        self.x_hi[A], self.v_hi[A] = x_hi, v_hi


def block_steps_ext(pos, vel, m, G, eps, dt_max, macro_steps, **kw):
    return BlockHermiteExt(pos, vel, m, G, eps, dt_max, **kw).macro(macro_steps).result()


# ---- the displaced-cluster geometries of the evaluation checks ---------------------------------------------------------
GEOMETRIES = {"centred": (1.0, (0.0, 0.0, 0.0)), "scale0.05_at_64": (0.05, (64.0, -32.0, 16.0)),
              "scale0.01_at_1000": (0.01, (1000.0, 0.0, 0.0))}


def displaced_cluster(pos, vel, m, scale, centre):
    """A cluster (fp32 arrays, total mass M) shrunk by `scale` about the origin and moved to `centre`, in fp64: positions
    scale * pos + centre (NOT fp32-representable), velocities scaled by scale^-1/2 (the virial ratio is kept)."""
    X = np.asarray(pos, np.float64) * scale + np.asarray(centre, np.float64)
    V = np.asarray(vel, np.float64) / np.sqrt(scale)
    return X, V, np.asarray(m, F32)


# ---- the accuracy cases -----------------------------------------------------------------------
CENTRE = np.array([20.0, 10.0, 0.0])
BINARY = dict(e=0.9, eps=1e-4, T=2.0 * np.pi, steps=25600, ref_steps=102400)
BLOCK = dict(eps=hbr.BINARY["eps"], T=hbr.BINARY["T"], macro=hbr.BINARY["macro"], L=hbr.BINARY["L"],
             ref_steps=hbr.BINARY["ref_steps"], etas=(0.02, 0.005))


def binary_state(displaced):
    """hermite_ref.binary(e = 0.9) in fp64, its centre of mass at the origin or at CENTRE"""
    pos, vel, m = hr.binary(e=BINARY["e"])
    return pos.astype(np.float64) + (CENTRE if displaced else 0.0), vel.astype(np.float64), m


def block_state():
    """hermite_block_ref.binary_case() (the e = 0.9 binary and the light body) moved to CENTRE, in fp64"""
    pos, vel, m = hbr.binary_case()
    return pos.astype(np.float64) + CENTRE, vel.astype(np.float64), m


def compute_references():
    """the fp64 end states the accuracy checks are measured against (what tests/golden/hermite_ext_refs.npz holds)"""
    out = {}
    c = BINARY
    for name, displaced in (("binary_centred_ref", False), ("binary_displaced_ref", True)):
        pos, vel, m = binary_state(displaced)
        out[name] = hr.hermite_steps(pos, vel, m, 1.0, c["eps"], c["T"] / c["ref_steps"], c["ref_steps"], np.float64)["pos"]
    pos, vel, m = block_state()
    c = BLOCK
    out["block_displaced_ref"] = hr.hermite_steps(pos, vel, m, 1.0, c["eps"], c["T"] / c["ref_steps"], c["ref_steps"],
                                                  np.float64)["pos"]
    return out


def references():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}

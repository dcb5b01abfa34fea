"""fp64 restatements for the Direct force-and-jerk kernel and the fourth-order Hermite integrator (csrc/hermite.hip).
numpy only; the GPU tests compare the engine against these, the CPU tests pin them to closed forms.

With d = r_j - r_i, w = v_j - v_i, h = |d|^2 + eps^2 (eps^2 the fp32 product the engine forms):
    a_i = G sum_j m_j d h^-3/2          j_i = G sum_j m_j [ w - 3 (d.w)/h d ] h^-3/2
The self pair has d = w = 0 and adds nothing.  A coincident pair of two distinct bodies adds nothing to a and
m_j w eps^-3 to j (the derivative of the softened kernel) -- except under the engine's guard convention, eps^2 < 1e-12,
where a pair with |d|^2 = 0 adds nothing to either sum.
"""
import numpy as np

U = 2.0 ** -24  # fp32 unit round-off


def eps2_of(eps):
    """eps^2 as the engine forms it: the fp32 product"""
    return float(np.float32(eps) * np.float32(eps))


def acc_jerk(pos, vel, m, G, eps, targets=None, block=256):
    """(a [T, 3], j [T, 3], S_a [T], S_j [T]) in fp64 from the given (fp32 or fp64) bodies, for the bodies `targets`
    (indices; default all).  S_a = G sum m |d| h^-3/2 and S_j = G sum m (|w| + 3 |d.w| |d| / h) h^-3/2 are the sums of
    the term magnitudes: they scale the error of an fp32 summation."""
    pos = np.asarray(pos, np.float64)
    vel = np.asarray(vel, np.float64)
    m = np.asarray(m, np.float64)
    idx = np.arange(len(pos)) if targets is None else np.asarray(targets)
    e2 = eps2_of(eps)
    guard = e2 < 1e-12
    a = np.zeros((len(idx), 3))
    j = np.zeros((len(idx), 3))
    sa = np.zeros(len(idx))
    sj = np.zeros(len(idx))
    for b in range(0, len(idx), block):
        t = idx[b:b + block]
        d = pos[None, :, :] - pos[t, None, :]
        w = vel[None, :, :] - vel[t, None, :]
        d2 = (d * d).sum(2)
        h = d2 + e2
        with np.errstate(divide="ignore", invalid="ignore"):
            f = m[None, :] * h ** -1.5
            if guard:
                f = np.where(d2 > 0.0, f, 0.0)
                h = np.where(d2 > 0.0, h, 1.0)
        dw = (d * w).sum(2)
        q = -3.0 * dw / h
        a[b:b + block] = G * (f[:, :, None] * d).sum(1)
        j[b:b + block] = G * (f[:, :, None] * (w + q[:, :, None] * d)).sum(1)
        nd = np.sqrt(d2)
        sa[b:b + block] = G * (f * nd).sum(1)
        sj[b:b + block] = G * (f * (np.sqrt((w * w).sum(2)) + 3.0 * np.abs(dw) * nd / h)).sum(1)
    return a, j, sa, sj


def hermite_steps(pos, vel, m, G, eps, dt, steps, state_dtype=np.float32, evaluate=None):
    """`steps` PEC Hermite steps (Makino & Aarseth 1992 as Hut & Makino write them) of size dt:
        xp = x + v dt + a dt^2/2 + j dt^3/6        vp = v + a dt + j dt^2/2
        (a1, j1) = acc_jerk(xp, vp)
        v1 = v + (a + a1) dt/2 + (j - j1) dt^2/12  x1 = x + (v + v1) dt/2 + (a - a1) dt^2/12
    state_dtype float32 is the engine's arithmetic model: x, v, a, j (and the predicted state the sums are evaluated
    at) are fp32, every sum and every predictor / corrector expression is formed in fp64 and rounded once; float64:
    everything in fp64.  dt is taken as the fp32 number the engine is given.  evaluate(x, v) -> (a, j, ...) replaces
    acc_jerk (the GPU tests pass the same restatement running in fp64 on the device).
    -> dict(pos, vel, acc, acc_old, jerk)."""
    if evaluate is None:
        evaluate = lambda x, v: acc_jerk(x, v, m, G, eps)  # noqa: E731
    T = state_dtype
    h = float(np.float32(dt))
    x = np.asarray(pos, T).astype(np.float64)
    v = np.asarray(vel, T).astype(np.float64)
    rnd = lambda z: z.astype(T).astype(np.float64)  # noqa: E731
    a, j = evaluate(x, v)[:2]
    a, j = rnd(a), rnd(j)
    a_old = np.zeros_like(a)
    for _ in range(steps):
        xp = rnd(x + v * h + a * (0.5 * h * h) + j * (h * h * h / 6.0))
        vp = rnd(v + a * h + j * (0.5 * h * h))
        a1, j1 = evaluate(xp, vp)[:2]
        a1, j1 = rnd(a1), rnd(j1)
        v1 = rnd(v + (a + a1) * (0.5 * h) + (j - j1) * (h * h / 12.0))
        x = rnd(x + (v + v1) * (0.5 * h) + (a - a1) * (h * h / 12.0))
        v, a_old, a, j = v1, a, a1, j1
    return dict(pos=x, vel=v, acc=a, acc_old=a_old, jerk=j)


def vv_steps(pos, vel, m, G, eps, dt, steps, state_dtype=np.float64, evaluate=None):
    """Velocity Verlet (the reference's integrator): x += v dt + a dt^2/2 ; a1 = a(x) ; v += (a + a1) dt/2, the state
    rounded to state_dtype after every update, the sums in fp64.  -> dict(pos, vel, acc)."""
    if evaluate is None:
        evaluate = lambda x, v: acc_jerk(x, v, m, G, eps)  # noqa: E731
    T = state_dtype
    h = float(np.float32(dt))
    x = np.asarray(pos, T).astype(np.float64)
    v = np.asarray(vel, T).astype(np.float64)
    rnd = lambda z: z.astype(T).astype(np.float64)  # noqa: E731
    a = rnd(evaluate(x, v)[0])
    for _ in range(steps):
        x = rnd(x + v * h + a * (0.5 * h * h))
        a1 = rnd(evaluate(x, v)[0])
        v = rnd(v + (a + a1) * (0.5 * h))
        a = a1
    return dict(pos=x, vel=v, acc=a)


def suggest_dt(a, j, eta=0.02):
    """eta min_i |a_i| / |j_i| over the bodies with |j_i| > 0 (+inf when there is none)"""
    na = np.linalg.norm(np.asarray(a, np.float64), axis=1)
    nj = np.linalg.norm(np.asarray(j, np.float64), axis=1)
    ok = nj > 0
    return float(eta * (na[ok] / nj[ok]).min()) if ok.any() else float("inf")


def energy(pos, vel, m, G, eps):
    """(KE, PE) in fp64, PE = -G sum_{i<j} m_i m_j / sqrt(r^2 + eps^2)"""
    pos = np.asarray(pos, np.float64)
    vel = np.asarray(vel, np.float64)
    m = np.asarray(m, np.float64)
    ke = 0.5 * (m * (vel * vel).sum(1)).sum()
    d = pos[None, :, :] - pos[:, None, :]
    r = np.sqrt((d * d).sum(2) + eps2_of(eps))
    iu = np.triu_indices(len(pos), 1)
    pe = -G * (m[:, None] * m[None, :] / r)[iu].sum()
    return ke, pe


def binary(e=0.5, a=1.0, M=1.0):
    """An equal-mass binary of total mass M, semi-major axis a and eccentricity e in the x-y plane at apocentre, centre
    of mass at rest at the origin (G = 1): -> (pos [2, 3], vel [2, 3], m [2]) in fp32.  Period 2 pi sqrt(a^3 / M)."""
    r = a * (1.0 + e)
    v = np.sqrt(M * (2.0 / r - 1.0 / a))
    pos = np.array([[-0.5 * r, 0.0, 0.0], [0.5 * r, 0.0, 0.0]], np.float32)
    vel = np.array([[0.0, -0.5 * v, 0.0], [0.0, 0.5 * v, 0.0]], np.float32)
    return pos, vel, np.array([0.5 * M, 0.5 * M], np.float32)

"""fp64 restatement of the ensemble diagnostics (nbody_hip_system_diag, include/nbody_hip.h) and
the systems tests/test_system_diag_*.py and tools/system_diag_time.py share.  numpy only.

reference(X, V, m, G, eps) evaluates one system from its fp64 state (the output of get_state_f64): the sums of
tests/hermite_ref.energy and a few lines for the rest, in row blocks so that 4,096 bodies do not need the n x n x 3 array
at once.  Every sum is formed from its fp64 terms in extended precision (np.longdouble), so the reference's own summation
error is far below the bound the tests assert; next to every sum stands sum |t_k|, which that bound is made of.  The
winner of each minimum comes with its runner-up, so that a test can assert the gap that makes an index comparison
meaningful.
"""
import math

import numpy as np

import hermite_ref as hr

U53 = 2.0 ** -53
THREADS = 256          # csrc/system_diag.hip: kDiagThreads
# the 15 sizes of the value test: no partner; one pair; odd rows; both sides of a wave, of the 256 workers, of two rows
# per worker, of the 512-body tile; a third tile holding one body; the largest system (8 tiles)
SIZES = (1, 2, 3, 5, 63, 64, 65, 255, 256, 257, 511, 512, 513, 1025, 4096)


def chain_pairs(n):
    """L(n) of the pair sum: a thread adds at most q = ceil(ceil(n / 2) (n - 1) / 256) terms, the wave reduction 6 more
    additions, the four waves 3"""
    return -(-(((n + 1) // 2) * (n - 1)) // THREADS) + 9


def chain_bodies(n):
    """L(n) of the per-body sums: ceil(n / 256) terms per thread, then the same reduction"""
    return -(-n // THREADS) + 9


def sum_bound(chain, abs_sum):
    """(L + 32) 2^-53 sum |t_k|"""
    return (chain + 32) * U53 * abs_sum


def _ld_sum(a):
    return np.sum(np.asarray(a, np.longdouble))


def reference(X, V, m, G, eps, block=256):
    """-> dict: the fields of the struct in fp64 (sums rounded once from extended precision), `abs` the sums of |t_k|
    (per component for the vectors), `min_gap` / `bind_gap` the relative distance of the runner-up from the winner
    (inf when there is none), `bind_cancel` = (T + U) / |E_b| of the winner."""
    X = np.asarray(X, np.float64)
    V = np.asarray(V, np.float64)
    m = np.asarray(m, np.float64)
    n = len(m)
    eps2 = hr.eps2_of(eps)
    out, ab = {}, {}
    out["mass"] = float(_ld_sum(m))
    mx, mv = m[:, None] * X, m[:, None] * V
    cr = np.cross(X, V)
    # (a cross product cancels inside the term: its rounding is bounded by the products it is made of)
    cr_abs = np.stack([np.abs(X[:, 1] * V[:, 2]) + np.abs(X[:, 2] * V[:, 1]), np.abs(X[:, 2] * V[:, 0]) + np.abs(X[:, 0] * V[:, 2]),
                       np.abs(X[:, 0] * V[:, 1]) + np.abs(X[:, 1] * V[:, 0])], 1)
    sm = np.array([float(_ld_sum(mx[:, c])) for c in range(3)])
    out["com"] = sm / out["mass"] if out["mass"] != 0 else np.zeros(3)
    out["momentum"] = np.array([float(_ld_sum(mv[:, c])) for c in range(3)])
    out["ang_mom"] = np.array([float(_ld_sum(m * cr[:, c])) for c in range(3)])
    ke_t = 0.5 * m * (V * V).sum(1)
    out["kinetic"] = float(_ld_sum(ke_t))
    ab["mx"] = np.abs(mx).sum(0)
    ab["momentum"] = np.abs(mv).sum(0)
    ab["ang_mom"] = (np.abs(m)[:, None] * cr_abs).sum(0)
    ab["kinetic"] = float(np.abs(ke_t).sum())
    pe = np.longdouble(0)
    pe_abs = 0.0
    seps, binds = [], []   # candidates (value, i, j): the two smallest of every block
    for i0 in range(0, n, block):
        i1 = min(i0 + block, n)
        d = X[None, :, :] - X[i0:i1, None, :]
        w = V[None, :, :] - V[i0:i1, None, :]
        r2 = (d * d).sum(2)
        w2 = (w * w).sum(2)
        ii, jj = np.nonzero(np.arange(n)[None, :] > np.arange(i0, i1)[:, None])
        r2, w2 = r2[ii, jj], w2[ii, jj]
        ii = ii + i0
        if ii.size == 0:
            continue
        mm = m[ii] * m[jj]
        h = r2 + eps2
        ok = h != 0
        t = G * mm[ok] / np.sqrt(h[ok])
        pe -= _ld_sum(t)
        pe_abs += float(np.abs(t).sum())
        r = np.sqrt(r2)
        for k in np.lexsort((jj, ii, r))[:2]:
            seps.append((r[k], int(ii[k]), int(jj[k])))
        ms = m[ii] + m[jj]
        can = (r > 0) & (ms > 0)
        if can.any():
            ic, jc = ii[can], jj[can]
            eb = 0.5 * (mm[can] / ms[can]) * w2[can] - G * mm[can] / r[can]
            for k in np.lexsort((jc, ic, eb))[:2]:
                binds.append((eb[k], int(ic[k]), int(jc[k])))
    out["potential"] = float(pe)
    ab["potential"] = pe_abs
    seps.sort()
    binds.sort()
    out["min_sep"], out["min_i"], out["min_j"] = (seps[0] if seps else (math.inf, -1, -1))
    out["min_gap"] = (seps[1][0] - seps[0][0]) / seps[0][0] if len(seps) > 1 and seps[0][0] > 0 else math.inf
    out.update(bind_energy=0.0, bind_a=0.0, bind_e=0.0, bind_i=-1, bind_j=-1, bind_gap=math.inf, bind_cancel=0.0)
    if binds and binds[0][0] < 0:
        _, i, j = binds[0]
        out["bind_i"], out["bind_j"] = i, j
        if len(binds) > 1:
            out["bind_gap"] = (binds[1][0] - binds[0][0]) / abs(binds[0][0])
        # the winner's elements in extended precision, rounded once
        ld = np.longdouble
        d, w = X[j].astype(ld) - X[i].astype(ld), V[j].astype(ld) - V[i].astype(ld)
        mi, mj, g = ld(m[i]), ld(m[j]), ld(G)
        r = np.sqrt((d * d).sum())
        mu = mi * mj / (mi + mj)
        kin, pot = ld(0.5) * mu * (w * w).sum(), g * mi * mj / r
        eb = kin - pot
        hv = np.cross(d, w)
        q = 1 + 2 * (eb / mu) * (hv * hv).sum() / (g * (mi + mj)) ** 2
        out["bind_energy"] = float(eb)
        out["bind_a"] = float(-g * mi * mj / (2 * eb))
        out["bind_e"] = float(np.sqrt(max(q, ld(0))))
        out["bind_cancel"] = float((kin + pot) / abs(eb))
    out["n"] = n
    out["abs"] = ab
    return out


# ---- the systems ---------------------------------------------------------------------------------------------------------
def plummer64(nb, n, seed):
    """a Plummer sphere of n bodies with general masses, as fp64 arrays (pos [n, 3], vel [n, 3], m fp32)"""
    ic = nb.ic.plummer(n, seed=seed)
    m = (ic["mass"] * np.random.default_rng(5 + seed).uniform(0.5, 2.0, n)).astype(np.float32)
    pos = np.stack([ic["pos_x"], ic["pos_y"], ic["pos_z"]], 1).astype(np.float64)
    vel = np.stack([ic["vel_x"], ic["vel_y"], ic["vel_z"]], 1).astype(np.float64)
    return pos, vel, m


def triple64(e, seed):
    """hermite_ref.binary(e) at apocentre and a light perturber at a few semi-major axes, as fp64 arrays"""
    pos, vel, m = hr.binary(e=e)
    rng = np.random.default_rng(seed)
    u = rng.normal(size=3)
    u /= np.linalg.norm(u)
    p3 = 4.0 * u
    v3 = 0.3 * rng.normal(size=3)
    return (np.concatenate([pos.astype(np.float64), p3[None, :]]), np.concatenate([vel.astype(np.float64), v3[None, :]]),
            np.concatenate([m, np.array([0.05], np.float32)]))


CENTRE = np.array([64.0, -32.0, 16.0])
SCALE = 0.01


def value_systems(nb, shifted, seed=11):
    """The ensemble of the value test: SIZES, the 3-body system an e = 0.5 binary with a perturber, and a second triple with
    e = 0.9 after it -- 16 systems, offsets no multiple of 4, 64 or 256.  -> list of (pos, vel, m) in fp64; shifted: positions
    of scale SCALE centred at CENTRE (not representable in fp32: the residuals matter), velocities scaled to match."""
    out = []
    for n in SIZES:
        if n == 3:
            out.append(triple64(0.5, seed))
            out.append(triple64(0.9, seed + 1))
        else:
            out.append(plummer64(nb, n, seed + n))
    if not shifted:
        return out
    return [(CENTRE + SCALE * p, v / math.sqrt(SCALE) * (1.0 + 2.0 ** -30), m) for p, v, m in out]


def small_systems(nb, seed=3):
    """the ensemble of the independence, graph and facade tests: 1, 2, 3, 65 and 257 bodies around the origin"""
    out = []
    for n in (1, 2, 3, 65, 257):
        out.append(triple64(0.9, seed) if n == 3 else plummer64(nb, n, seed + n))
    return out


def concat64(systems):
    """-> (pos [N, 3], vel [N, 3], m [N], offsets)"""
    off = np.concatenate([[0], np.cumsum([len(s[2]) for s in systems])]).astype(np.uint64)
    return (np.concatenate([s[0] for s in systems]), np.concatenate([s[1] for s in systems]),
            np.concatenate([s[2] for s in systems]).astype(np.float32), off)


def ic32(pos, vel, m):
    """the ic dict of the fp32 roundings"""
    p, v = np.asarray(pos, np.float32), np.asarray(vel, np.float32)
    return dict(pos_x=p[:, 0].copy(), pos_y=p[:, 1].copy(), pos_z=p[:, 2].copy(), vel_x=v[:, 0].copy(), vel_y=v[:, 1].copy(),
                vel_z=v[:, 2].copy(), mass=np.asarray(m, np.float32).copy())

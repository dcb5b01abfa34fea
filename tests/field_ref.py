"""fp64 restatement of the field at arbitrary points (nbody_hip_{direct,tree,grid}_field) for the tests.

A point is never a body: nothing is skipped by index.  A body coincident with the point adds zero force and
-G m / eps to phi; with eps^2 < 1e-12 (the kernels' guard convention) it adds nothing to either.

  direct_field   a = G sum m d (d^2 + eps^2)^-3/2, phi = -G sum m (d^2 + eps^2)^-1/2 over all bodies, d = r_j - x;
                 also S = G sum m |d| (d^2 + eps^2)^-3/2, the sum of the force terms' magnitudes (the yardstick of the
                 fp32 bounds), and G sum m (d^2 + eps^2)^-1/2 = |phi|
  tree_field     the walk of quadrupole_ref.Restatement from positions instead of bodies: opening decisions in fp32
                 exactly as the kernel takes them, leaves body by body without a self-skip, accepted nodes in fp64
  hash_cells     the grid's clamped cell coordinates of points, in fp32 as cell_coord forms them
  hash_field     truncated force and shifted truncated potential over the 27-cell window of each point's cell; the pair
                 decision on the unsoftened fp32 r^2 (one product, two fused multiply-adds) < fl(rc * rc)
  hash_field_all the same sum over ALL bodies (what the window gives for cutoff <= cell)
"""
import numpy as np

from potential_ref import fp32_dist2
from quadrupole_ref import node_eval


def _e2(eps):
    return float(np.float32(eps) * np.float32(eps))


def direct_field(points, pos, m, G, eps, chunk=512):
    x = np.asarray(points, np.float32)[:, :3]
    pos32 = np.asarray(pos, np.float32)
    m = np.asarray(m, np.float64)
    e2 = _e2(eps)
    guard = e2 < 1e-12
    acc, phi, S = np.zeros((len(x), 3)), np.zeros(len(x)), np.zeros(len(x))
    for a in range(0, len(x), chunk):
        d = pos32[None, :, :].astype(np.float64) - x[a:a + chunk, None, :].astype(np.float64)
        r2 = (d * d).sum(-1)
        ok = (r2 > 0) if guard else np.ones_like(r2, bool)
        with np.errstate(divide="ignore"):
            inv = np.where(ok, 1.0 / np.sqrt(np.where(ok, r2 + e2, 1.0)), 0.0)
        f = m[None, :] * inv ** 3
        acc[a:a + chunk] = G * (f[:, :, None] * d).sum(1)
        phi[a:a + chunk] = -G * (m[None, :] * inv).sum(1)
        S[a:a + chunk] = G * (f * np.sqrt(r2)).sum(1)
    return acc, phi, S


def tree_field(rest, points, theta, G, eps, order, batch=2048):
    """(acc (k, 3), phi (k,), S (k,)) at `points` over the exported tree of `rest` (quadrupole_ref.Restatement); S = G x
    the sum of the magnitudes of the monopole-sized terms (m |d| h^-3/2 per leaf body and accepted node)"""
    x32 = np.asarray(points, np.float32)[:, :3]
    k = len(x32)
    theta2 = np.float32(np.float32(theta) * np.float32(theta))
    eps2 = np.float32(np.float32(eps) * np.float32(eps))
    guard = float(eps2) < 1e-12
    acc, phi, S = np.zeros((k, 3)), np.zeros(k), np.zeros(k)
    for b0 in range(0, k, batch):
        ti = np.arange(b0, min(b0 + batch, k))
        nd = np.zeros(len(ti), np.int64)
        while ti.size:
            leaf = rest.leaf[nd]
            li, ln = ti[leaf], nd[leaf]
            if li.size:
                lens = rest.last[ln] - rest.first[ln]
                rep_t = np.repeat(li, lens)
                starts = np.cumsum(lens) - lens
                q = np.arange(lens.sum()) - np.repeat(starts, lens) + np.repeat(rest.first[ln], lens)
                body = rest.order[q]
                d32 = (rest.pos32[body] - x32[rep_t]).astype(np.float32)
                r2 = fp32_dist2(d32[:, 0], d32[:, 1], d32[:, 2]).astype(np.float64)
                ok = (r2 > 0) if guard else np.ones(len(r2), bool)
                d = d32.astype(np.float64)
                h = r2 + float(eps2)
                with np.errstate(divide="ignore"):
                    inv = np.where(ok, 1.0 / np.sqrt(np.where(ok, h, 1.0)), 0.0)
                f = rest.m[body] * inv ** 3
                for a in range(3):
                    acc[:, a] += np.bincount(rep_t, f * d[:, a], minlength=k)
                phi += np.bincount(rep_t, rest.m[body] * inv, minlength=k)
                S += np.bincount(rep_t, f * np.sqrt(r2), minlength=k)
            ti, nd = ti[~leaf], nd[~leaf]
            if not ti.size:
                break
            d32 = (rest.com32[nd] - x32[ti]).astype(np.float32)
            d2 = fp32_dist2(d32[:, 0], d32[:, 1], d32[:, 2])
            dist2 = (d2 + eps2).astype(np.float32)
            far = rest.size2[nd] < (theta2 * dist2).astype(np.float32)
            ai, an = ti[far], nd[far]
            if ai.size:
                d = rest.c[an] - x32[ai].astype(np.float64)
                h = (d * d).sum(1) + float(eps2)
                a_n, p_n = node_eval(d, h, rest.M[an], rest.S[an], order)
                for a in range(3):
                    acc[:, a] += np.bincount(ai, a_n[:, a], minlength=k)
                phi += np.bincount(ai, p_n, minlength=k)
                S += np.bincount(ai, rest.M[an] * np.sqrt((d * d).sum(1)) * h ** -1.5, minlength=k)
            oi, on = ti[~far], nd[~far]
            ch = rest.children[on]
            valid = ch >= 0
            ti = np.repeat(oi, valid.sum(1))
            nd = ch[valid]
    return G * acc, -G * phi, G * S


def hash_cells(points, bmin, cell, dims):
    """cell id of every point: min(max(int(floorf(fl(fl(p - lo) / cell))), 0), dim - 1) per axis, x fastest"""
    x = np.asarray(points, np.float32)[:, :3]
    lo = np.asarray(bmin, np.float32)
    dims = np.asarray(dims, np.int64)
    with np.errstate(invalid="ignore", over="ignore"):
        q = np.floor(((x - lo[None, :]).astype(np.float32) / np.float32(cell)).astype(np.float32))
    q = np.where(np.isnan(q), 0.0, q)
    c = np.clip(q, 0, (dims - 1)[None, :].astype(np.float64)).astype(np.int64)
    return c[:, 0] + c[:, 1] * dims[0] + c[:, 2] * dims[0] * dims[1]


def _hash_terms(x32, cand_pos32, cand_m, G, eps, cutoff):
    """(acc, phi, kappa-scale S, phi scale) of ONE point from candidate bodies"""
    e2 = _e2(eps)
    rc2 = np.float32(np.float32(cutoff) * np.float32(cutoff))
    shift = 1.0 / np.sqrt(float(rc2) + e2)
    d32 = (cand_pos32 - x32[None, :]).astype(np.float32)
    r2 = fp32_dist2(d32[:, 0], d32[:, 1], d32[:, 2])
    ok = r2 < rc2
    if e2 < 1e-12:
        ok &= r2 > 0
    d, r2, mm = d32[ok].astype(np.float64), r2[ok].astype(np.float64), cand_m[ok]
    inv = 1.0 / np.sqrt(r2 + e2)
    f = mm * inv ** 3
    return (G * (f[:, None] * d).sum(0), -G * (mm * (inv - shift)).sum(), G * (f * np.sqrt(r2)).sum(),
            G * (mm * inv).sum())


def hash_field_all(points, pos, m, G, eps, cutoff):
    """the truncated sum over all bodies: (acc (k, 3), phi (k,), S (k,), phi scale (k,))"""
    x = np.asarray(points, np.float32)[:, :3]
    pos32, m = np.asarray(pos, np.float32), np.asarray(m, np.float64)
    out = [_hash_terms(x[i], pos32, m, G, eps, cutoff) for i in range(len(x))]
    return (np.array([o[0] for o in out]).reshape(-1, 3), np.array([o[1] for o in out]), np.array([o[2] for o in out]),
            np.array([o[3] for o in out]))


def hash_field(points, point_cells, pos, m, G, eps, cutoff, cell_of, dims):
    """the 27-cell window of each point's cell (point_cells: hash_cells, or the grid's own ids for points that are
    bodies); cell_of: the grid's cell id of every body"""
    x = np.asarray(points, np.float32)[:, :3]
    pos32, m = np.asarray(pos, np.float32), np.asarray(m, np.float64)
    gx, gy, gz = (int(v) for v in dims)
    c = np.asarray(cell_of, np.int64)
    order = np.argsort(c, kind="stable")
    cs = c[order]
    pc = np.asarray(point_cells, np.int64)
    cx, cy, cz = pc % gx, (pc // gx) % gy, pc // (gx * gy)
    out = []
    for i in range(len(x)):
        cand = [np.zeros(0, np.int64)]
        for dz in (-1, 0, 1):
            for dy in (-1, 0, 1):
                z, y = cz[i] + dz, cy[i] + dy
                if not (0 <= z < gz and 0 <= y < gy):
                    continue
                x0, x1 = max(cx[i] - 1, 0), min(cx[i] + 1, gx - 1)
                b = (z * gy + y) * gx
                lo, hi = np.searchsorted(cs, b + x0), np.searchsorted(cs, b + x1 + 1)
                cand.append(order[lo:hi])
        j = np.concatenate(cand)
        out.append(_hash_terms(x[i], pos32[j], m[j], G, eps, cutoff))
    return (np.array([o[0] for o in out]).reshape(-1, 3), np.array([o[1] for o in out]), np.array([o[2] for o in out]),
            np.array([o[3] for o in out]))

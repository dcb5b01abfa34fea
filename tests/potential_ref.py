"""fp64 restatement of the per-body potentials (nbody_hip_{direct,tree,grid}_potential) for the tests.

  direct_phi  phi_i = -G sum_{j != i} m_j / sqrt(r_ij^2 + eps^2)
  hash_phi    phi_i = -G sum_j m_j (1 / sqrt(r^2 + eps^2) - 1 / sqrt(rc^2 + eps^2)) over the pair set of the hash force:
              bodies of the 27 neighbouring cells (cell ids as the grid assigned them) with the unsoftened fp32 r^2
              (one product, two fused multiply-adds, as the kernels form it) below rc^2 = fl(rc * rc); with
              `guard` (eps^2 < 1e-12) coincident pairs are left out too.
Also returns the scale G sum_j m_j / sqrt(r^2 + eps^2) over the same pairs, the bound's yardstick (the shift cancels
terms near rc, so a relative bound on phi itself means nothing there).
"""
import numpy as np


def direct_phi(pos, m, G, eps, chunk=1024):
    pos = np.asarray(pos, np.float64)
    m = np.asarray(m, np.float64)
    n = len(m)
    e2 = float(np.float32(eps) * np.float32(eps))
    out = np.empty(n)
    for a in range(0, n, chunk):
        d = pos[None, :, :] - pos[a:a + chunk, None, :]
        r2 = (d * d).sum(-1) + e2
        with np.errstate(divide="ignore"):
            inv = np.where(r2 > 0, 1.0 / np.sqrt(np.where(r2 > 0, r2, 1.0)), 0.0)
        idx = np.arange(a, min(a + chunk, n))
        inv[idx - a, idx] = 0.0
        out[a:a + chunk] = -G * (inv * m[None, :]).sum(1)
    return out


def fp32_dist2(dx, dy, dz):
    """fma(dz, dz, fma(dy, dy, dx * dx)) in fp32 (each fma rounded once: exact in fp64, then rounded)."""
    dx, dy, dz = (np.asarray(v, np.float32) for v in (dx, dy, dz))
    t = (dx * dx).astype(np.float32)
    t = (dy.astype(np.float64) * dy + t).astype(np.float32)
    return (dz.astype(np.float64) * dz + t).astype(np.float32)


def shifted_term(r2, rc, eps):
    """the shifted pair term 1 / sqrt(r^2 + eps^2) - 1 / sqrt(rc^2 + eps^2) (fp64)"""
    e2 = float(np.float32(eps) * np.float32(eps))
    rc2 = float(np.float32(rc) * np.float32(rc))
    return 1.0 / np.sqrt(np.asarray(r2, np.float64) + e2) - 1.0 / np.sqrt(rc2 + e2)


def hash_phi(pos, m, G, eps, cutoff, cell_of, dims, idx=None):
    """phi (and the bound's scale) of the bodies `idx` (default: all), cell_of = the grid's cell id of every body."""
    pos32 = np.asarray(pos, np.float32)
    m = np.asarray(m, np.float64)
    n = len(m)
    gx, gy, gz = (int(v) for v in dims)
    c = np.asarray(cell_of, np.int64)
    cx, cy, cz = c % gx, (c // gx) % gy, c // (gx * gy)
    e2 = float(np.float32(eps) * np.float32(eps))
    rc2 = np.float32(np.float32(cutoff) * np.float32(cutoff))
    guard = e2 < 1e-12
    shift = 1.0 / np.sqrt(float(rc2) + e2)
    order = np.argsort(c, kind="stable")
    cs = c[order]
    idx = np.arange(n) if idx is None else np.asarray(idx)
    phi, scale = np.zeros(len(idx)), np.zeros(len(idx))
    for k, i in enumerate(idx):
        cand = []
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
        j = j[j != i]
        d = pos32[j] - pos32[i]
        r2 = fp32_dist2(d[:, 0], d[:, 1], d[:, 2])
        ok = r2 < rc2
        if guard:
            ok &= r2 > 0
        j, r2 = j[ok], r2[ok].astype(np.float64)
        inv = 1.0 / np.sqrt(r2 + e2)
        phi[k] = -G * (m[j] * (inv - shift)).sum()
        scale[k] = G * (m[j] * inv).sum()
    return phi, scale

"""CPU restatement of the k nearest neighbours, the local density and the density centre (include/nbody_hip_neighbours.h)
for the tests.  No GPU, no package import.

  topk            brute force O(n^2): per body the k smallest keys (bits(fp32_dist2) << 32 | index) over the other bodies
                  (skipped by position, a NaN never taken), optionally restricted to the 27-cell window through given cell
                  ids (the grid's own); -1 / +inf in unused slots
  status_of       the status rule (3 coincident k-th, 0 exact, 1 window-limited, 2 fewer than k)
  density_of      Casertano-Hut in fp64 in the stated order
  ordered_sum     a sum of n fp64 terms in the model's order (n <= 32 in turn; chunks of 1,024, 256 strided sums, the
                  32 .. 1 folds)
  density_centre  the two passes on top of it -> a record of DTYPE
"""
import numpy as np

from potential_ref import fp32_dist2

SPHERE = 4.1887902047863905  #NBODY_HIP_SPHERE_4PI_3: the fp64 nearest to 4 pi / 3
EMPTY = np.uint64(0xFFFFFFFFFFFFFFFF)
S, C, T = 32, 1024, 256  # kCentreSmall, kCentreChunk, kCentreThreads (test_neighbours_cpu.py reads the header and compares)

DTYPE = np.dtype([("centre", "<f8", (3,)), ("core_radius", "<f8"), ("rho_sum", "<f8"), ("rho2_sum", "<f8"),
                  ("n", "<i4"), ("status", "<i4"), ("reserved", "<i4", (2,))])
assert DTYPE.itemsize == 64


def cell_xyz(cell_of, dims):
    gx, gy, _ = (int(v) for v in dims)
    c = np.asarray(cell_of, np.int64)
    return np.stack([c % gx, (c // gx) % gy, c // (gx * gy)], 1)


def topk(pos, k, cell_of=None, dims=None, rows=None, block=256):
    """-> (index [r, k] int32, dist2 [r, k] float32) for the bodies `rows` (default: all)"""
    pos = np.ascontiguousarray(pos, np.float32).reshape(-1, 3)
    n = len(pos)
    rows = np.arange(n) if rows is None else np.asarray(rows, np.int64)
    xyz = None if cell_of is None else cell_xyz(cell_of, dims)
    index = np.full((len(rows), k), -1, np.int32)
    dist2 = np.full((len(rows), k), np.inf, np.float32)
    ids = np.arange(n, dtype=np.uint64)
    for b0 in range(0, len(rows), block):
        r = rows[b0:b0 + block]
        d = pos[None, :, :] - pos[r, None, :]
        d2 = fp32_dist2(d[..., 0], d[..., 1], d[..., 2])
        keys = (d2.view(np.uint32).astype(np.uint64) << np.uint64(32)) | ids[None, :]
        drop = np.isnan(d2) | (ids[None, :] == r[:, None].astype(np.uint64))
        if xyz is not None:
            drop |= (np.abs(xyz[None, :, :] - xyz[r, None, :]) > 1).any(2)
        keys[drop] = EMPTY
        kk = min(k, n)
        part = np.sort(keys, axis=1)[:, :kk]
        have = part != EMPTY
        index[b0:b0 + block, :kk] = np.where(have, (part & np.uint64(0xFFFFFFFF)).astype(np.int64), -1)
        bits = (part >> np.uint64(32)).astype(np.uint32)
        dist2[b0:b0 + block, :kk] = np.where(have, bits.view(np.float32), np.float32(np.inf))
    return index, dist2


def whole_grid(dims):
    return max(int(v) for v in dims) <= 2


def status_of(index, dist2, cell, dims):
    k = index.shape[1]
    found = index[:, k - 1] >= 0
    d2k = dist2[:, k - 1]
    cell2 = np.float32(np.float32(cell) * np.float32(cell))
    exact = (d2k < cell2) | whole_grid(dims)
    return np.where(~found, 2, np.where(d2k == 0, 3, np.where(exact, 0, 1))).astype(np.int32)


def density_of(index, dist2, status, mass):
    k = index.shape[1]
    m = np.asarray(mass, np.float32).astype(np.float64)
    msum = np.zeros(len(index), np.float64)
    for s in range(k - 1):
        msum = msum + np.where(index[:, s] >= 0, m[np.maximum(index[:, s], 0)], 0.0)
    with np.errstate(all="ignore"):
        r = np.sqrt(dist2[:, k - 1].astype(np.float64))
        rho = msum / (SPHERE * ((r * r) * r))
    return np.where((status == 2) | (status == 3), 0.0, rho)


def search(pos, mass, k, cell, cell_of, dims):
    """the whole call on one build -> (index, dist2, rho, status)"""
    index, dist2 = topk(pos, k, cell_of, dims)
    status = status_of(index, dist2, cell, dims)
    return index, dist2, density_of(index, dist2, status, mass), status


def _fold64(s):
    """s [..., 64] -> [...]: s_l += s_(l + off) for l < off, off = 32 .. 1"""
    s = s.copy()
    off = 32
    while off:
        s[..., :off] = s[..., :off] + s[..., off:2 * off]
        off //= 2
    return s[..., 0]


def ordered_sum(t):
    """the sum of the fp64 terms t [n] (position order) in the model's order"""
    t = np.asarray(t, np.float64)
    n = len(t)
    if n <= S:
        total = np.float64(0.0)
        for v in t:
            total = total + v
        return float(total)
    chunks = -(-n // C)
    pad = np.zeros(chunks * C, np.float64)  # (+0 for the positions a chunk does not have: s + 0 == s for the sums here)
    pad[:n] = t
    q = pad.reshape(chunks, C // T, T)      # position 256 j + t of a chunk
    s = np.zeros((chunks, T), np.float64)
    for j in range(C // T):
        s = s + q[:, j, :]
    runs = _fold64(s.reshape(chunks, T // 64, 64))
    chunk = runs[:, 0]
    for w in range(1, T // 64):
        chunk = chunk + runs[:, w]
    c = np.zeros(64, np.float64)
    for first in range(0, chunks, 64):
        part = chunk[first:first + 64]
        c[:len(part)] = c[:len(part)] + part
    return float(_fold64(c))


def density_centre(pos, rho, members=None):
    pos = np.ascontiguousarray(pos, np.float32).reshape(-1, 3)
    rho = np.asarray(rho, np.float64)
    out = np.zeros(1, DTYPE)[0]
    if members is None:
        members = np.arange(len(pos))
    members = np.asarray(members, np.int64)
    if ((members < 0) | (members >= len(pos))).any():
        out["status"] = 1
        return out
    out["n"] = len(members)
    w = rho[members]
    x = pos[members].astype(np.float64)
    s1 = ordered_sum(w)
    if s1 == 0.0:
        return out
    centre = np.array([ordered_sum(w * x[:, a]) / s1 for a in range(3)])
    d = x - centre[None, :]
    r2 = ((d[:, 0] * d[:, 0]) + (d[:, 1] * d[:, 1])) + (d[:, 2] * d[:, 2])
    w2 = w * w
    s2 = ordered_sum(w2)
    big_r = ordered_sum(w2 * r2)
    out["centre"], out["rho_sum"], out["rho2_sum"] = centre, s1, s2
    out["core_radius"] = 0.0 if s2 == 0.0 else np.sqrt(np.float64(big_r) / np.float64(s2))
    return out


def seeded_set(n):
    """the general data of csrc/neighbours_check.cpp (seeded(n, false)): rho [n] float64, pos [n, 3] float32"""
    p = np.arange(n, dtype=np.uint64)
    a = p * np.uint64(2654435761) + np.uint64(12345)
    b = p * np.uint64(40503) + np.uint64(977)
    f = np.float32
    rho = (1 + (a % np.uint64(1000003)).astype(np.int64)).astype(np.float64) / 4099.0
    m = np.uint64(100003)
    x = ((b % m).astype(np.int64) - 50000).astype(f) / f(1021.0)
    y = (((b // np.uint64(7)) % m).astype(np.int64) - 50000).astype(f) / f(2039.0) + f(3.0)
    z = (((b // np.uint64(13)) % m).astype(np.int64) - 50000).astype(f) / f(4093.0) - f(2.0)
    return rho, np.stack([x, y, z], 1).astype(f)

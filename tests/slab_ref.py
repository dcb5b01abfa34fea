"""ONE plain restatement of the bookkeeping kernels of the z-slab decomposition (csrc/slab.hip, the box / layer kernels of
csrc/spatial_hash.hip, the packed drift / kick of csrc/integrator.hip) in numpy and Python integers: no device, no
library.  The fp32 arithmetic is spelt out operation by operation with np.float32 (the library is built without
fast-math: `/` on the device is correctly rounded); the two fused multiply-adds of the kernels (the layer centre of
slab_owner_cuts, drift1 / kick1 of common.h) are rounded ONCE, from the exact rational value (fma32).

Used by tests/test_slab_cpu.py (the restatement against the host entry point and a brute force), tests/test_slab_gpu.py
(the kernels against it, bit for bit) and the CPU stand-in of tests/test_sharded_cpu.py."""
import math
from fractions import Fraction

import numpy as np

F = np.float32
PAD = F(0.001)
GRID_TOO_LARGE = 0x40000000


# ---- fp32 from exact values -------------------------------------------------------------------------------------------
def round_f32(q):
    """the Fraction q rounded to the nearest fp32, ties to even (denormals and overflow to infinity included); q != 0"""
    neg, m = q < 0, abs(q)
    e = m.numerator.bit_length() - m.denominator.bit_length()      # 2^(e-1) < m < 2^(e+1)
    if m < Fraction(2) ** e:
        e -= 1                                                     # now 2^e <= m < 2^(e+1)
    ulp = max(e, -126) - 23
    scaled = m / Fraction(2) ** ulp
    n = scaled.numerator // scaled.denominator
    rem = scaled - n
    if rem > Fraction(1, 2) or (rem == Fraction(1, 2) and n & 1):
        n += 1
    v = math.ldexp(n, ulp) if n * Fraction(2) ** ulp < Fraction(2) ** 128 else math.inf   # n <= 2^24: exact in a double
    return F(-v if neg else v)


def fma32(a, b, c):
    """fmaf(a, b, c) of finite fp32 values: a b + c exactly, rounded once"""
    a, b, c = F(a), F(b), F(c)
    prod = Fraction(float(a)) * Fraction(float(b))
    q = prod + Fraction(float(c))
    if q == 0:   # the sign of an exact zero: that of the fp32 sum when both terms are zeros, + when they cancel
        return a * b + c if prod == 0 else F(0.0)
    return round_f32(q)


def fma32_array(a, b, c, exact_only=False):
    """fma32 element by element.  The exact helper is slow, so it is kept for the elements that need it: the product of
    two fp32 values is exact in a double, and the sum rounded to a double and then to fp32 differs from the sum rounded
    once ONLY where the double landed exactly midway between two fp32 values (there the bits it lost decide; every fp32
    value and every midpoint is a double, and rounding is monotone) -- those, exact zeros (their sign) and overflows go
    through fma32.  exact_only: all of them do (tests/test_slab_cpu.py holds the two paths to each other)."""
    a, b, c = np.broadcast_arrays(np.asarray(a, F), np.asarray(b, F), np.asarray(c, F))
    with np.errstate(all="ignore"):
        s = a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)
        out = s.astype(F)
        r = out.astype(np.float64)
        below, above = (np.nextafter(out, F(s_)).astype(np.float64) for s_ in (-np.inf, np.inf))
        doubt = (s == (r + below) / 2) | (s == (r + above) / 2) | (s == 0) | ~np.isfinite(out)
    if exact_only:
        doubt = np.ones(a.shape, bool)
    for k in zip(*np.nonzero(doubt)):
        out[k] = fma32(a[k], b[k], c[k])
    return out


# ---- the global grid and a body's layer -------------------------------------------------------------------------------
def axis_cells(lo, hi, cell):
    """slab_axis_cells: ceil((hi - lo) / cell) + 1, or the too-large verdict"""
    with np.errstate(all="ignore"):
        cells = np.ceil((F(hi) - F(lo)) / F(cell))
    return int(cells) + 1 if F(0.0) <= cells < F(1.0e9) else GRID_TOO_LARGE


def geometry(gbox, cell):
    """-> (lo[3] fp32, [gx, gy, gz]) of the grid derived from the unpadded box {min x,y,z, max x,y,z}"""
    lo = [F(gbox[a]) - PAD for a in range(3)]
    hi = [F(gbox[3 + a]) + PAD for a in range(3)]
    return lo, [axis_cells(lo[a], hi[a], cell) for a in range(3)]


def layer(z, lo_z, cell, gz):
    """slab_layer / cell_coord: clip(floor((z - lo_z) / cell), 0, gz - 1), clipped before the conversion to int"""
    c = np.floor((np.asarray(z, F) - F(lo_z)) / F(cell))
    return np.clip(c.astype(np.float64), 0.0, float(gz - 1)).astype(np.int64)


# ---- owners -------------------------------------------------------------------------------------------------------------
def owner_equal(layer_, gz, W):
    """equal layer counts: rank r owns [r gz / W, (r+1) gz / W)"""
    return ((layer_ + 1) * W - 1) // gz


def layer_centre(layer_, lo_z, cell):
    """the ONE fma of slab_owner_cuts: (layer + 1/2) cell + lo_z, rounded once"""
    return fma32(F(int(layer_)) + F(0.5), cell, lo_z)


def owner_cuts(layer_, lo_z, cell, cuts):
    """the number of cuts at or below the layer's centre"""
    zc = layer_centre(layer_, lo_z, cell)
    return sum(1 for c in cuts if F(c) <= zc)


def owner_table(gz, lo_z, cell, W, cuts=None):
    """owner of every layer of the grid"""
    if cuts is None:
        return np.array([owner_equal(z, gz, W) for z in range(gz)], np.int64)
    assert len(cuts) == W - 1
    return np.array([owner_cuts(z, lo_z, cell, cuts) for z in range(gz)], np.int64)


def up(x):
    return np.nextafter(F(x), F(np.inf))


def down(x):
    return np.nextafter(F(x), F(-np.inf))


def crafted_cuts(lo_z, cell, gz, W, rng):
    """name -> W - 1 ascending cuts around the centres of `gz` layers (the CPU and the GPU tests run the same sets)"""
    k = W - 1
    if k == 0:
        return {"none": np.zeros(0, F)}
    layers = np.sort(rng.choice(gz, size=k, replace=k > gz))
    centres = np.array([layer_centre(z, lo_z, cell) for z in layers], F)
    assert np.all(np.diff(centres) >= 0)
    top = layer_centre(gz - 1, lo_z, cell)
    sets = {"at_centre": centres,                                   # that layer goes to the upper rank
            "ulp_below": np.array([down(c) for c in centres], F),   # also the upper rank
            "ulp_above": np.array([up(c) for c in centres], F),     # the lower rank
            "all_below": np.full(k, down(F(lo_z)), F),              # everything to rank W - 1
            "all_above": np.full(k, up(top), F),                    # everything to rank 0
            "random": np.sort(rng.uniform(float(lo_z), float(top), k).astype(F))}
    if k >= 2:
        eq = centres.copy()
        eq[1] = eq[0]                                               # two equal cuts: rank 1 owns no layer
        sets["two_equal"] = np.sort(eq)
    return sets


def balanced_cuts(hist, lo_z, cell, W, n):
    """the balancing rule of the sharded host (csrc/sharded_hash.hip): the k-th cut is the lower edge of the first layer
    at which the running count reaches k n / W, or its upper edge when that leaves the smaller error"""
    gz, run, z, cuts = len(hist), 0, 0, []
    for k in range(1, W):
        want = int(float(n) * k / W)
        while z < gz and run + int(hist[z]) <= want:
            run += int(hist[z])
            z += 1
        b = z + 1 if z < gz and (want - run) * 2 > int(hist[z]) else z
        cuts.append(F(lo_z) + F(b) * F(cell))
    return np.array(cuts, F)


# ---- the partition pass -------------------------------------------------------------------------------------------------
def partition(posm, vel, acc, gid, gbox, cell, W, rank, hist_cap, cuts=None):
    """nbody_hip_slab_partition[_cuts] -> dict of
       holes [L]     the leavers' input positions, ascending
       rows  [L,16]  grouped by new owner ascending, input order within a group; gid (or the input position) in word 12
                     and the layer in word 13 as int bits, zeros in words 7, 11, 14, 15
       send  [W]     row `rank` of the send matrix
       hist  [min(gz, hist_cap)]  bodies per layer -- also when gz > hist_cap
       info  [gx, gy, gz, gz > hist_cap]
       layer [n], dest [n]        every body's layer and new owner"""
    posm = np.asarray(posm, F).reshape(-1, 4)
    n = posm.shape[0]
    lo, dims = geometry(gbox, cell)
    gz = dims[2]
    z = layer(posm[:, 2], lo[2], cell, gz)
    if cuts is None:
        dest = owner_equal(z, gz, W)
    else:
        assert len(cuts) == W - 1
        uniq, inv = np.unique(z, return_inverse=True)
        dest = np.array([owner_cuts(int(u), lo[2], cell, cuts) for u in uniq], np.int64)[inv.reshape(-1)]
    holes = np.flatnonzero(dest != rank)
    order = holes[np.argsort(dest[holes], kind="stable")]
    rows = np.zeros((order.size, 16), F)
    if order.size:
        rows[:, 0:4] = posm[order]
        rows[:, 4:7] = np.asarray(vel, F)[order, :3]
        rows[:, 8:11] = np.asarray(acc, F)[order, :3]
        ids = order if gid is None else np.asarray(gid)[order]
        rows[:, 12] = ids.astype(np.int32).view(F)
        rows[:, 13] = z[order].astype(np.int32).view(F)
    nh = min(gz, hist_cap)
    return dict(holes=holes.astype(np.int32), rows=rows, send=np.bincount(dest, minlength=W).astype(np.int32),
                hist=np.bincount(z[z < nh], minlength=nh).astype(np.int32),
                info=np.array([dims[0], dims[1], gz, int(gz > hist_cap)], np.int32), layer=z, dest=dest)


# ---- the fill pass ------------------------------------------------------------------------------------------------------
def fill(posm, vel, acc, gid, n_old, holes, arrivals):
    """nbody_hip_slab_fill, IN PLACE on arrays with room for max(n_old, n_new) bodies (gid may be None) -> n_new.
    Arrival t goes to holes[t], or to n_old + (t - L) once the holes are used up; when A < L the non-hole bodies of the
    old tail [n_new, n_old), ascending, go into holes[A:], ascending.  Nothing else is written.  The pass only moves
    words: posm / vel / acc [., 4] and arrivals [A, 16] may be fp32 or, all of them, their bit patterns as 4-byte ints."""
    holes = np.asarray(holes, np.int64)
    arrivals = np.asarray(arrivals).reshape(-1, 16)
    assert arrivals.dtype == posm.dtype == vel.dtype == acc.dtype and arrivals.dtype.itemsize == 4
    A, L = arrivals.shape[0], holes.size
    n_new = n_old - L + A
    slots = np.concatenate([holes[:min(A, L)], np.arange(n_old, n_old + max(A - L, 0), dtype=np.int64)])
    posm[slots] = arrivals[:, 0:4]
    vel[slots] = arrivals[:, 4:8]
    acc[slots] = arrivals[:, 8:12]
    if gid is not None:
        gid[slots] = np.ascontiguousarray(arrivals[:, 12]).view(np.int32)
    if A < L:
        is_hole = np.zeros(n_old, bool)
        is_hole[holes] = True
        tail = n_new + np.flatnonzero(~is_hole[n_new:n_old])
        to = holes[A:A + tail.size]
        for arr in (posm, vel, acc) + (() if gid is None else (gid,)):
            arr[to] = arr[tail]
    return n_new


# ---- the packed drift and kick --------------------------------------------------------------------------------------------
def drift(p, v, a, dt):
    """drift1 (common.h): p + fma(a, 0.5f dt dt, v dt), the fma rounded once; arrays of fp32 coordinates"""
    dt = F(dt)
    h = F(0.5) * dt * dt
    return np.asarray(p, F) + fma32_array(a, h, np.asarray(v, F) * dt)


def kick(v, a_old, a_new, dt):
    """kick1 (common.h): fma(a_old + a_new, 0.5f dt, v)"""
    return fma32_array(np.asarray(a_old, F) + np.asarray(a_new, F), F(0.5) * F(dt), v)

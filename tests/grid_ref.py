"""What tests/test_grid_cpu.py and tests/test_grid_gpu.py share: crafted grids given as key histograms, and the references of
everything the spatial-hash force kernels read -- the start array, an exported layer, the work list of cell_units_kernel --
derived from ONE thing the suite already trusts: np.searchsorted on the sorted cell ids.  All integer data, all exact.

A crafted grid has the explicit bounds lo = 0, hi = (g - 1) cell per axis, which grid_axis_cells turns into exactly g cells,
and a body of cell (i, j, k) sits at ((i + f) cell, (j + f) cell, (k + f) cell) with f = 0.5 (or anything in [0.1, 0.9]):
its key is i + j gx + k gx gy.  So a case is a histogram: how many bodies each cell holds.  Nothing here imports torch."""
import numpy as np

import sort_ref as sr

F = np.float32
GAP_INLINE = 64        # kGapInline: a run of this many cells or more goes to cell_gap_kernel's list
COARSE = 64            # kLbCoarse
HEAVY = 48             # kHeavyCell: cells above it put their units at the front of the list
CROWDED = 64           # the most crowded cell is reported when above it
UNIT_CELLS = 8         # kUnitCells: consecutive cells per thread of cell_units_kernel
UNIT_BLOCK = 2048      # cells per workgroup of cell_units_kernel
SPLIT_CNT = 6          # NBH_HASH_SPLIT_CNT's default
INT_MAX = 0x7fffffff
UNITS, BODIES, PAIRS = 0, 1, 2
TOP = np.uint32(0x80000000)


# ---- crafted grids ------------------------------------------------------------------------------------------------------
def bounds_of(dims, cell=1.0):
    return (0.0, 0.0, 0.0) + tuple(float((g - 1) * cell) for g in dims)


class Crafted:
    """bodies of a key histogram `hist` (bodies per cell, length gx gy gz) on the grid `dims`, in a shuffled order.
    jitter: positions anywhere in the middle 80 % of their cell (or in the given range of it) instead of its centre
    (force cases)."""

    def __init__(self, dims, hist, seed=0, cell=1.0, jitter=False):
        dims = tuple(int(g) for g in dims)
        hist = np.asarray(hist, np.int64)
        self.dims, self.cell, self.total = dims, cell, dims[0] * dims[1] * dims[2]
        assert hist.size == self.total and hist.min() >= 0 and hist.sum() > 0
        rng = np.random.default_rng(seed)
        self.keys = rng.permutation(np.repeat(np.arange(self.total), hist)).astype(np.int32)   # intended keys, input order
        self.n = self.keys.size
        gx, gy = dims[0], dims[1]
        ijk = np.stack([self.keys % gx, (self.keys // gx) % gy, self.keys // (gx * gy)], 1).astype(np.float64)
        frac = rng.uniform(*((0.1, 0.9) if jitter is True else jitter), ijk.shape) if jitter else 0.5
        p = ((ijk + frac) * cell).astype(F)
        self.ic = sr.bodies(p[:, 0], p[:, 1], p[:, 2])
        self.bounds = bounds_of(dims, cell)
        self.hist = hist
        self.posm = sr.posm_of(self.ic)
        self.order = sr.stable_order(self.keys)
        self.sorted_keys = self.keys[self.order]
        self.sorted_posm = self.posm[self.order]

    def oracle_keys(self, oracle):
        """(dims, keys) as the oracle states them for these bodies and bounds: must equal what was intended"""
        lo, dims = sr.grid_geometry(oracle, self.ic, self.cell, self.bounds)
        return tuple(dims), sr.grid_keys(oracle, self.ic, self.cell, lo, dims)


# ---- the start array ----------------------------------------------------------------------------------------------------
def covered(dims, slab=None):
    """(base, count) of the cells [base, base + count] the start array covers, as grid_build_packed clips a slab
    (z_first, z_count); None: an empty slab.  slab None or z_count <= 0: the whole grid."""
    layer, gz = dims[0] * dims[1], dims[2]
    if slab is None or slab[1] <= 0:
        return 0, layer * gz
    z0, z1 = max(slab[0], 0), min(slab[0] + slab[1], gz)
    return (z0 * layer, (z1 - z0) * layer) if z1 > z0 else None


def has_array(n, cov):
    return cov is not None and 0 < cov[1] <= 16 * n + 4096


def builder(n, cov, lb_env=None):
    """which kernels make the start array: None (no array), "two-level", "position" (cell_mark + cell_gap) or "cell"
    (NBH_HASH_LB=cell)"""
    if not has_array(n, cov):
        return None
    if cov[1] > 2 * n:
        return "two-level"
    return "cell" if lb_env == "cell" else "position"


def start_array(sorted_keys, cov):
    base, count = cov
    return np.searchsorted(sorted_keys, np.arange(base, base + count + 1), "left").astype(np.int32)


def long_runs(sorted_keys, cov):
    """number of runs cell_mark_kernel hands to the gap list: owned cell ranges of GAP_INLINE cells or more"""
    base, count = cov
    k = np.concatenate([[base - 1], sorted_keys.astype(np.int64), [base + count]])
    lo, hi = np.maximum(k[:-1] + 1, base), np.minimum(k[1:], base + count)
    return int(((k[1:] != k[:-1]) & (hi - lo >= GAP_INLINE)).sum())


# ---- an exported layer ---------------------------------------------------------------------------------------------------
def layer_export(lb, cov, dims, z, sorted_posm):
    """(bodies [m, 4] float32, lb_out [layer + 1] int32) of nbody_hip_grid_export_layer; None: the layer is not covered"""
    layer = dims[0] * dims[1]
    k0 = z * layer - cov[0]
    if z < 0 or z >= dims[2] or k0 < 0 or k0 + layer > cov[1]:
        return None
    first, last = int(lb[k0]), int(lb[k0 + layer])
    return sorted_posm[first:last], (lb[k0:k0 + layer + 1] - first).astype(np.int32)


# ---- the work list --------------------------------------------------------------------------------------------------------
def unit_rows(units):
    """rows {cell, chunk} in a canonical order (the order inside a group is unspecified)"""
    units = np.asarray(units, np.int64).reshape(-1, 2)
    return units[np.lexsort((units[:, 1], units[:, 0]))].astype(np.int32)


def unit_list(lb, cov, cell_first, cell_end, chunk, min_cnt=1, mode=UNITS):
    """the list of the cells [cell_first, cell_end): dict heavy / other (canonical rows), counts [4], light (sorted uint32)"""
    assert cov[0] <= cell_first < cell_end <= cov[0] + cov[1]
    k = np.arange(cell_first, cell_end + 1) - cov[0]
    lo = lb[k].astype(np.int64)
    cnt = np.diff(lo)
    nus = np.where(cnt >= min_cnt, (cnt + chunk - 1) // chunk, 0)
    cells = np.repeat(np.arange(cnt.size), nus)
    q = np.arange(nus.sum()) - np.repeat(np.cumsum(nus) - nus, nus)
    rows = np.stack([cells, q], 1)
    heavy = np.repeat(cnt > HEAVY, nus)
    light = np.empty(0, np.uint32)
    if mode != UNITS:
        lc = np.where(cnt < min_cnt, cnt, 0)
        if mode == BODIES:
            pos = np.repeat(lo[:-1], lc) + (np.arange(lc.sum()) - np.repeat(np.cumsum(lc) - lc, lc))
            light = pos.astype(np.uint32)
        else:
            items = (lc + 1) // 2
            j = np.arange(items.sum()) - np.repeat(np.cumsum(items) - items, items)
            pos = (np.repeat(lo[:-1], items) + 2 * j).astype(np.uint32)
            odd_last = 2 * j + 1 >= np.repeat(lc, items)
            light = np.where(odd_last, pos | TOP, pos).astype(np.uint32)
    mx = int(cnt.max())
    counts = np.array([heavy.sum(), mx if mx > CROWDED else 0, (~heavy).sum(), light.size], np.int32)
    return {"heavy": unit_rows(rows[heavy]), "other": unit_rows(rows[~heavy]), "counts": counts, "light": np.sort(light)}


# ---- the 1-D patterns of the start-array cases (histograms over (G, 1, 1)) -----------------------------------------------
RUNS = (0, 1, 62, 63, 64, 65, 127, 128, 129)
ONE_CELL_N = (1, 255, 256, 257)
FULL_G = (1, 63, 64, 65, 255, 256, 257, 4097)


def hist_runs(edge, m):
    """(a) `edge` empty cells, then occupied cells (m bodies each) separated by runs of every length of RUNS, then `edge`
    empty cells"""
    h = [0] * edge + [m]
    for r in RUNS:
        h += [0] * r + [m]
    return np.array(h + [0] * edge)


def hist_one_cell(G, where, n):
    """(b) n bodies in the first, last or middle cell of G"""
    h = np.zeros(G, np.int64)
    h[{"first": 0, "last": G - 1, "middle": G // 2}[where]] = n
    return h


def hist_every(G, step, m):
    """(c) m bodies in every step-th cell and in the last one (step 1: no empty cell)"""
    h = np.zeros(G, np.int64)
    h[::step] = m
    h[G - 1] = m
    return h


def hist_random(G, share, seed, unit=False):
    """(d) `share` of the cells occupied, by 1 to 300 bodies (unit: by one)"""
    rng = np.random.default_rng(seed)
    occ = rng.permutation(G)[:max(1, int(round(G * share)))]
    h = np.zeros(G, np.int64)
    h[occ] = 1 if unit else rng.integers(1, 301, occ.size)
    return h


def line_cases():
    """name -> (histogram, the builder it is written for without / with NBH_HASH_LB=cell)"""
    cases = {}
    for e in RUNS:
        cases[f"runs edge {e} x64"] = (hist_runs(e, 64), "position")
        cases[f"runs edge {e} x1"] = (hist_runs(e, 1), "two-level")
    for n in ONE_CELL_N:
        for where in ("first", "last", "middle"):
            cases[f"one cell {where} n {n} dense"] = (hist_one_cell(2 * n, where, n), "position")
            cases[f"one cell {where} n {n} sparse"] = (hist_one_cell(2 * n + 90, where, n), "two-level")
    for G in FULL_G:
        cases[f"full {G} x3"] = (hist_every(G, 1, 3), "position")
        cases[f"full {G} x1"] = (hist_every(G, 1, 1), "position")
        if G >= 63:   # (no empty cell and more than two cells per body exclude each other: the coarse level's sizes with
            cases[f"third {G} x1"] = (hist_every(G, 3, 1), "two-level")   # every third cell and the last one occupied)
    for share, G in ((0.9, 600), (0.3, 1500), (0.02, 5000)):
        cases[f"random {share} x300"] = (hist_random(G, share, G), "position")
        cases[f"random {share} x1"] = (hist_random(G, share, G, unit=True), "position" if share > 0.5 else "two-level")
    # (e) both thresholds, on the side where an array exists
    h = np.zeros(1000, np.int64)
    h[::2] = 1
    cases["2n"] = (h, "position")                                        # 500 bodies, 1,000 cells
    h = np.zeros(1001, np.int64)
    h[:1000:2] = 1
    cases["2n + 1"] = (h, "two-level")                                   # 500 bodies, 1001 cells
    h = np.zeros(16 * 100 + 4096, np.int64)
    h[:200:2] = 1
    cases["16n + 4096"] = (h, "two-level")                               # 100 bodies, 5,696 cells: the last grid with an array
    return cases


def hist_many_runs():
    """(f) 3,016 occupied cells of 33 bodies, 65 empty cells between them: 3,015 runs for the gap list, more than the 2,048
    waves of cell_gap_kernel; 99,528 bodies, 199,000 cells (at most two per body)"""
    h = np.zeros(199000, np.int64)
    h[0:66 * 3016:66] = 33
    return h


def hist_no_array():
    """(e) one cell more than 16 n + 4096: no start array.  100 bodies, two in every third cell of the first 150 (with
    NO_ARRAY_JITTER they are closer than a cutoff of one cell: every body has a force)"""
    h = np.zeros(16 * 100 + 4096 + 1, np.int64)
    h[:150:3] = 2
    return h


NO_ARRAY_JITTER = (0.3, 0.7)


# ---- slabs ----------------------------------------------------------------------------------------------------------------
SLAB_GRIDS = ((5, 3, 9), (8, 4, 6))     # layers of 15 cells (no multiple of four) and of 32


def slabs_of(gz):
    return ((0, 0), (0, 1), (2, 3), (gz - 1, 1), (gz - 2, 5), (-1, 3), (gz, 2))


def hist_slab(dims, slab, outside, seed):
    """0 to 9 bodies per cell (a third of the cells empty) in the layers of the slab; outside: in the layers below and above
    it as well"""
    rng = np.random.default_rng(seed)
    total, layer = dims[0] * dims[1] * dims[2], dims[0] * dims[1]
    h = np.where(rng.random(total) < 0.33, 0, rng.integers(1, 10, total))
    cov = covered(dims, slab)
    if not outside:
        assert cov is not None
        inside = np.zeros(total, bool)
        inside[cov[0]:cov[0] + cov[1]] = True
        h = np.where(inside, h, 0)
        h[cov[0] + layer // 2] = max(h[cov[0] + layer // 2], 1)
    return h


# ---- the unit-list cases ----------------------------------------------------------------------------------------------------
UNIT_SETTINGS = ((64, 1, UNITS), (128, 1, UNITS), (256, 1, UNITS), (128, SPLIT_CNT, BODIES), (128, INT_MAX, PAIRS))
UNIT_LINES = (2047, 2048, 2049, 4097)


def unit_populations(chunk, min_cnt):
    m = min(min_cnt, 40)   # (INT_MAX: every cell is light; a stand-in pair around a small number keeps the list short)
    return sorted({0, 1, m - 1, m, 48, 49, 63, 64, 65, chunk - 1, chunk, chunk + 1, 2 * chunk + 1, 300})


def hist_units(total, chunk, min_cnt, seed):
    """the populations of unit_populations scattered over `total` cells: every fifth cell holds one of them in turn (the
    first and the last cell always), the rest a few bodies or none"""
    rng = np.random.default_rng(seed)
    pops = unit_populations(chunk, min_cnt)
    h = np.where(rng.random(total) < 0.5, 0, rng.integers(1, 4, total))
    at = np.unique(np.concatenate([np.arange(0, total, 5), [total - 1]]))
    h[at] = np.array(pops)[(np.arange(at.size) + seed) % len(pops)]
    return h


# ---- thin grids (forces at the rim) -------------------------------------------------------------------------------------------
RIM_GRIDS = ((1, 1, 1), (2, 1, 1), (1, 2, 3), (3, 3, 3), (70, 1, 1), (1, 1, 70), (2, 70, 2))
RIM_N = 2000


def rim_bodies(dims, cell=1.0, n=RIM_N):
    """n bodies uniform in the box [0, g cell) per axis of the crafted grid `dims`, masses in [0.5, 1.5]; -> (ic, bounds)"""
    rng = np.random.default_rng(1000 + 100 * dims[0] + 10 * dims[1] + dims[2])
    p = (rng.random((n, 3)) * np.array(dims) * cell).astype(F)
    p = np.minimum(p, np.nextafter((np.array(dims) * cell).astype(F), F(0)))
    ic = sr.bodies(p[:, 0], p[:, 1], p[:, 2])
    ic["mass"] = rng.uniform(0.5, 1.5, n).astype(F)
    return ic, bounds_of(dims, cell)

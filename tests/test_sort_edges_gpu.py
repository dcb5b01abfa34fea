"""The two radix sorts of our own (the Onesweep driver of csrc/onesweep.h, the hand-written sort of csrc/radix_sort.h) at the
shapes where a radix sort goes wrong, on the PRODUCT path: the digit counts come from the key kernels
(assign_cells_kernel / morton_kernel through DigitHistogram::flush, eight replicas folded by the scan kernels), not from
the sorts' own histogram kernels, which is all BodySort::self_test exercises.

One reference: np.argsort(key, kind="stable") of the keys the oracle states (cell ids of oracle_assign_cells on the
grid's geometry; oracle_bh_keys >> (63 - 3 max_depth) on the root cube of oracle_bh_root).  Every comparison is integer
or bitwise equality: the permutation, the cell ranges, the float4 payload.  A rank off by one, a look-back sum one tile
short or a lost tie order all give a NEARLY sorted permutation that the force tolerances would not notice.

NBH_OWN_SORT_FROM=0 and NBH_SORT are read when a grid / tree is created, so they are set in-process (monkeypatch) before
the constructor.  effective_sort falls back to the public sort silently, hence every case first asserts the verdict of
the self-test through nbody_hip_sort_info.  Every case also builds the same input on a second object made under
NBH_SORT=public: a failure on both sides points at the key restatement, a failure on one side at the sort.
(tests/test_sort_gpu.py compares the three sorts once, at 300,000 bodies, in child processes.)"""
import ctypes as C

import numpy as np
import pytest

import sort_ref as sr
from gpu_util import acc_of, to_device

pytestmark = pytest.mark.gpu

N_EDGE = 24581                       # three tiles of 8,192 and five keys: the last tile is nearly empty
SIZES = [1, 2, 63, 64, 65, 511, 512, 513, 8191, 8192, 8193, 16384, 24577, 100003]
IMPLS = ["own", "driver"]
CLUMP = 9000                         # more than one tile of 8,192 in one cell / one deepest leaf

_memo = {}


def memo(key, make):
    """inputs and their references are computed once and shared by the cases (own / driver, both sides) that need them"""
    if key not in _memo:
        _memo[key] = make()
    return _memo[key]


def same(got, want, what):
    if got.shape == want.shape and np.array_equal(got, want):
        return
    assert got.shape == want.shape, f"{what}: shape {got.shape} against {want.shape}"
    diff = got != want
    bad = np.flatnonzero(diff if diff.ndim == 1 else diff.any(axis=1))
    k = int(bad[0])
    pytest.fail(f"{what}: {bad.size} of {want.shape[0]} entries differ, first at {k}: got {got[k]}, want {want[k]}")


# ---- which sort ---------------------------------------------------------------------------------------------------------
def select(nb, monkeypatch, which):
    """the environment of the objects created next"""
    if which == "driver" and sr.sort_info(nb)[0] == 0:
        pytest.skip("the Onesweep driver is compiled out (another rocPRIM than the one it was written against)")
    monkeypatch.setenv("NBH_OWN_SORT_FROM", "0")
    monkeypatch.setenv("NBH_SORT", which)


def assert_selected(nb, which):
    """after the object exists (its creation ran the self-tests): the sort asked for is in use, not its fallback.
    effective_sort has one more silent fallback that no verdict shows and the C ABI cannot read: the hand-written sort
    also gives way to the public one when the object's mapped error word has no device address (a failed host
    allocation or mapping).  An `own` case would then run rocPRIM and pass; nothing here can tell."""
    compiled, driver_ok, own_ok, _ = sr.sort_info(nb)
    if which == "own":
        assert own_ok == 1, f"the hand-written sort failed its self-test ({own_ok}): the public sort would run"
    elif which == "driver":
        assert compiled == 1 and driver_ok == 1, f"the Onesweep driver failed its self-test ({driver_ok})"


# ---- cases --------------------------------------------------------------------------------------------------------------
class GridCase:
    """bodies + the geometry, keys, permutation, cell ranges and payload the oracle and np.argsort expect of their grid"""

    def __init__(self, oracle, ic, cell=1.0, bounds=None, ranges=True):
        self.ic, self.cell, self.bounds, self.n = ic, cell, bounds, ic["pos_x"].size
        self.lo, self.dims = sr.grid_geometry(oracle, ic, cell, bounds)
        self.total = self.dims[0] * self.dims[1] * self.dims[2]
        self.bits = sr.bits_for(self.total)
        self.keys = sr.grid_keys(oracle, ic, cell, self.lo, self.dims)
        self.order = sr.stable_order(self.keys)
        self.posm = sr.posm_of(ic)
        self.sorted_words = self.posm[self.order].view(np.uint32)
        self.ranges = None
        if ranges:
            sk, cells = self.keys[self.order], np.arange(self.total)
            left, right = np.searchsorted(sk, cells, "left"), np.searchsorted(sk, cells, "right")
            full = right > left
            self.ranges = (np.where(full, left, 0).astype(np.int32), np.where(full, right, 0).astype(np.int32))


class TreeCase:
    def __init__(self, oracle, ic, depth):
        self.ic, self.depth, self.n = ic, depth, ic["pos_x"].size
        self.keys = sr.tree_keys(oracle, ic, depth)
        self.order = sr.stable_order(self.keys)


def build_grid(nb, grid, case):
    """-> what must stay alive until the build has been read back"""
    if case.bounds is None:
        d, _ = to_device(nb, case.ic)
        grid.build(d)
        return d
    import torch
    posm = torch.from_numpy(case.posm).cuda()
    bounds = (C.c_float * 6)(*case.bounds)
    nb._lib.check(nb._lib.load().nbody_hip_grid_build_packed(grid._h, posm.data_ptr(), case.n, bounds))
    return posm


def check_grid(nb, grid, case, tag):
    dims, total, lo, _ = grid._info()
    assert list(dims) == list(case.dims) and total == case.total, f"{tag}: grid {dims} against the oracle's {case.dims}"
    assert sr.bits_for(grid.getTotalCells()) == case.bits, f"{tag}: {grid.getTotalCells()} cells"
    assert [np.float32(v) for v in lo] == [np.float32(v) for v in case.lo], f"{tag}: origin {lo} against {case.lo}"
    cs, ce, pc, si = sr.grid_cell_data(nb, grid, case.n, case.total if case.ranges else None)
    same(pc, case.keys, f"{tag}: particle_cells against the oracle's cell ids")
    same(si, case.order, f"{tag}: sorted_indices against the stable argsort")
    if case.ranges:
        same(cs, case.ranges[0], f"{tag}: cell_start against searchsorted(left)")
        same(ce, case.ranges[1], f"{tag}: cell_end against searchsorted(right)")
    same(sr.grid_sorted_bodies(nb, grid, case.n), case.sorted_words, f"{tag}: sorted float4 bodies against posm[order]")


def run_grid(nb, monkeypatch, which, cases, env=()):
    """builds `cases` one after the other on ONE grid made under NBH_SORT=which, then on one made under NBH_SORT=public"""
    for k, v in env:
        monkeypatch.setenv(k, v)
    nmax = max(c.n for c in cases)
    for side in (which, "public"):
        select(nb, monkeypatch, side)
        grid = nb.SpatialHashGrid(nmax, cases[0].cell)
        assert_selected(nb, side)
        for k, case in enumerate(cases):
            keep = build_grid(nb, grid, case)
            check_grid(nb, grid, case, f"NBH_SORT={side}, build {k}, N={case.n}, {case.bits} key bits")
            del keep
        grid.close()


def run_tree(nb, monkeypatch, which, cases):
    """as run_grid.  The tree's own keys cannot be read back, so only the permutation is compared: where morton_kernel
    and the oracle's keys disagree, BOTH sides fail (the public one too); a failure of `which` alone is the sort's."""
    nmax, depth = max(c.n for c in cases), cases[0].depth
    assert depth >= 11   # (wide keys: the trees up to depth 10 sort 30-bit keys with the public sort alone)
    for side in (which, "public"):
        select(nb, monkeypatch, side)
        tree = nb.BarnesHutTree(nmax)
        tree.setParams(depth, 1)
        assert_selected(nb, side)
        for k, case in enumerate(cases):
            d, _ = to_device(nb, case.ic)
            tree.build(d)
            same(sr.tree_order(nb, tree, case.n), case.order,
                 f"NBH_SORT={side}, build {k}, N={case.n}, depth {depth} ({3 * depth} key bits): sorted_indices_ against "
                 "the stable argsort")
        tree.close()


# ---- body sets ----------------------------------------------------------------------------------------------------------
def uniform(nb, n, half, seed):
    ic = nb.ic.uniform_box(n, seed=seed, lo=-half, hi=half)
    return sr.bodies(ic["pos_x"], ic["pos_y"], ic["pos_z"])


def plummer(nb, n, seed):
    ic = nb.ic.plummer(n, seed=seed)
    return sr.bodies(ic["pos_x"], ic["pos_y"], ic["pos_z"])


WIDE = 54.25                                             # bodies in +-54.25: 110^3 cells of size 1 = 21 key bits
WIDE_BOUNDS = (-54.251, -54.251, -54.251, 54.251, 54.251, 54.251)   # the same grid as explicit (padded) bounds
DISTRIBUTIONS = ["one_position", "two_corners", "clump", "line", "ascending", "descending"]


def distribution(nb, name, key_of):
    """N_EDGE bodies inside +-54; key_of(ic) -> their sort keys (for the two orderings of the uniform set)"""
    n, rng = N_EDGE, np.random.default_rng(77)
    if name == "one_position":
        return sr.bodies(np.full(n, 3.3), np.full(n, -7.1), np.full(n, 20.9))
    if name == "two_corners":
        c = np.where(np.arange(n) % 2 == 0, -54.0, 54.0)
        return sr.bodies(c, c, c)
    if name == "clump":   # CLUMP bodies at one position (one cell, one leaf of the deepest level) scattered through the list
        p = rng.uniform(-54.0, 54.0, (n, 3))
        p[rng.permutation(n)[:CLUMP]] = (10.4, 10.5, 10.6)
        return sr.bodies(p[:, 0], p[:, 1], p[:, 2])
    if name == "line":
        return sr.bodies(rng.uniform(-54.0, 54.0, n), np.full(n, 0.5), np.full(n, 0.5))
    ic = uniform(nb, n, 54.0, seed=78)
    order = sr.stable_order(key_of(ic))
    assert np.unique(key_of(ic)).size > n // 2
    return sr.take(ic, order if name == "ascending" else order[::-1])


# ---- sizes --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", IMPLS)
@pytest.mark.parametrize("n", SIZES)
def test_sizes_grid(nb, oracle, ctx, monkeypatch, which, n):
    """uniform box, 17^3 cells = 13 key bits (two places, the last 3 bits wide) from 63 bodies on; below one tile, one
    tile exactly, one key more, a last tile of one key (24,577) and 13 tiles (100,003: the look-back walks over
    PARTIAL words)"""
    case = memo(("grid size", n), lambda: GridCase(oracle, uniform(nb, n, 8.0, seed=100 + n)))
    if n >= 511:
        assert case.bits == 13
    run_grid(nb, monkeypatch, which, [case])


@pytest.mark.parametrize("which", IMPLS)
@pytest.mark.parametrize("n", SIZES)
def test_sizes_tree(nb, oracle, ctx, monkeypatch, which, n):
    """Plummer sphere at depth 20: bits 3..63, six full places"""
    case = memo(("tree size", n), lambda: TreeCase(oracle, plummer(nb, n, seed=200 + n), 20))
    run_tree(nb, monkeypatch, which, [case])


# ---- key widths ---------------------------------------------------------------------------------------------------------
# bits -> half width of the uniform box: ceil(extent + 0.002) + 1 cells of size 1 per axis = 10, 11, 100, 110, 450
GRID_WIDTHS = {1: None, 10: 4.25, 11: 4.75, 20: 49.25, 21: WIDE, 27: 224.25}


@pytest.mark.parametrize("which", IMPLS)
@pytest.mark.parametrize("bits", sorted(GRID_WIDTHS))
def test_key_widths_grid(nb, oracle, ctx, monkeypatch, which, bits):
    """one place of 1 bit, one full place, two places with a last one of 1 bit, two full, three with 1 bit, three with 7.
    A build from the bodies alone never has fewer than 2 cells per axis, so the grid of ONE cell is built with explicit
    bounds that are a point (nbody_hip_grid_build_packed): every body is clamped into cell 0.  The 27-bit grid (9.1e7
    cells, under the limit of 1e8) is read back without its per-cell arrays."""
    def make():
        if bits == 1:
            return GridCase(oracle, uniform(nb, N_EDGE, 4.25, seed=301), bounds=(0.0,) * 6)
        return GridCase(oracle, uniform(nb, N_EDGE, GRID_WIDTHS[bits], seed=300 + bits), ranges=bits != 27)
    case = memo(("grid width", bits), make)
    want = {1: 1, 10: 10 ** 3, 11: 11 ** 3, 20: 100 ** 3, 21: 110 ** 3, 27: 450 ** 3}[bits]
    assert case.total == want and case.bits == bits   # (check_grid holds the grid's own getTotalCells() to the same)
    run_grid(nb, monkeypatch, which, [case])


@pytest.mark.parametrize("which", IMPLS)
@pytest.mark.parametrize("depth", [11, 14, 17, 20, 21])
def test_key_widths_tree(nb, oracle, ctx, monkeypatch, which, depth):
    """33, 42, 51, 60 and 63 sorted bits from bit 30, 21, 12, 3 and 0: 4, 5, 6, 6 and 7 places (both ping-pong parities), the
    last one 3, 2, 1, 10 and 3 bits wide"""
    ic = memo(("tree width bodies",), lambda: plummer(nb, N_EDGE, seed=400))
    case = memo(("tree width", depth), lambda: TreeCase(oracle, ic, depth))
    assert int(case.keys.max()) < 1 << (3 * depth)
    run_tree(nb, monkeypatch, which, [case])


# ---- key distributions --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", IMPLS)
@pytest.mark.parametrize("name", DISTRIBUTIONS)
def test_key_distributions_grid(nb, oracle, ctx, monkeypatch, which, name):
    """the 21-bit grid (110^3 cells, explicit bounds so that it does not depend on where the bodies are): all keys equal
    (every tile puts 8,192 keys into one bin, every wave counter reaches 512), two keys, one cell of more than a tile,
    a line, input in order and in reverse order"""
    def keys(ic):
        lo, dims = sr.grid_geometry(oracle, ic, 1.0, WIDE_BOUNDS)
        return sr.grid_keys(oracle, ic, 1.0, lo, dims)
    case = memo(("grid distribution", name), lambda: GridCase(oracle, distribution(nb, name, keys), bounds=WIDE_BOUNDS))
    assert case.total == 110 ** 3 and case.bits == 21
    counts = np.bincount(case.keys)
    if name == "one_position":
        assert np.unique(case.keys).size == 1
    if name == "two_corners":
        assert np.unique(case.keys).size == 2
    if name == "clump":
        assert counts.max() > 8192
    if name == "ascending":
        assert np.all(np.diff(case.keys) >= 0)
    if name == "descending":
        assert np.all(np.diff(case.keys) <= 0)
    run_grid(nb, monkeypatch, which, [case])


@pytest.mark.parametrize("which", IMPLS)
@pytest.mark.parametrize("name", DISTRIBUTIONS)
def test_key_distributions_tree(nb, oracle, ctx, monkeypatch, which, name):
    """the same body sets under a tree of depth 21 (all 63 bits, seven places)"""
    case = memo(("tree distribution", name),
                lambda: TreeCase(oracle, distribution(nb, name, lambda ic: sr.tree_keys(oracle, ic, 21)), 21))
    uniq, counts = np.unique(case.keys, return_counts=True)
    if name == "one_position":
        assert uniq.size == 1
    if name == "two_corners":
        assert uniq.size == 2
    if name == "clump":
        assert counts.max() > 8192
    if name == "ascending":
        assert np.all(case.keys[1:] >= case.keys[:-1])
    if name == "descending":
        assert np.all(case.keys[1:] <= case.keys[:-1])
    run_tree(nb, monkeypatch, which, [case])


# ---- rebuilds on one object -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", IMPLS)
def test_rebuilds_grid(nb, oracle, ctx, monkeypatch, which):
    """100,003 -> 1 -> 8,193 -> 100,003 bodies on one grid of capacity 100,003, the key width going 15 -> 1 -> 21 -> 15.
    The digit counts are zeroed by grid_info_kernel (builds from the bodies), grid_info_set_kernel (the one-cell grid of the
    second build: explicit bounds) and hist_zero_kernel (builds 3 and 4 launch their key pass ahead of the grid record on
    the width of the build before, which is wrong both times)."""
    def make():
        base = uniform(nb, 100003, 14.25, seed=500)                    # 30^3 cells
        return [GridCase(oracle, base),
                GridCase(oracle, sr.take(base, np.arange(1)), bounds=(0.0,) * 6),
                GridCase(oracle, sr.scaled(sr.take(base, np.arange(8193)), WIDE / 14.25)),
                GridCase(oracle, base)]
    cases = memo(("grid rebuilds",), make)
    assert [c.n for c in cases] == [100003, 1, 8193, 100003]
    assert [c.bits for c in cases] == [15, 1, 21, 15]
    run_grid(nb, monkeypatch, which, cases)


@pytest.mark.parametrize("which", IMPLS)
def test_rebuilds_tree(nb, oracle, ctx, monkeypatch, which):
    """the same body counts on one tree of depth 20, which alternates two histogram buffers between its builds"""
    def make():
        base = plummer(nb, 100003, seed=501)
        return [TreeCase(oracle, base if n == 100003 else sr.take(base, np.arange(n)), 20) for n in (100003, 1, 8193, 100003)]
    run_tree(nb, monkeypatch, which, memo(("tree rebuilds",), make))


# ---- the key pass launched ahead of the grid record, with the hand-written sort -------------------------------------------
@pytest.mark.parametrize("mode", ["0", "1", "2"])
def test_speculated_key_pass_with_the_hand_written_sort(nb, oracle, ctx, monkeypatch, mode):
    """small / small / large / large / small (8^3 cells = 9 key bits, one place; 60^3 = 18 bits, two places): with
    NBH_HASH_SPECULATE=1 the guess is right, wrong (grown), right, wrong (shrunk); with 2 wrong at every build; 0: no guess.
    Every build against argsort."""
    def make():
        small = GridCase(oracle, uniform(nb, N_EDGE, 3.25, seed=600))
        large = GridCase(oracle, sr.scaled(small.ic, 9.0))
        return [small, small, large, large, small]
    cases = memo(("grid speculation",), make)
    assert [c.bits for c in cases] == [9, 9, 18, 18, 9]
    run_grid(nb, monkeypatch, "own", cases, env=(("NBH_HASH_SPECULATE", mode),))


# ---- the payload reaches the forces ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", IMPLS)
def test_forces_after_the_sort_grid(nb, oracle, ctx, monkeypatch, which):
    """15-bit grid, cutoff = cell = 1: the accelerations of a build sorted by `which` are those of the public sort's, bit
    for bit"""
    case = memo(("grid forces",), lambda: GridCase(oracle, uniform(nb, N_EDGE, 14.25, seed=700)))
    assert case.bits == 15
    acc = {}
    for side in (which, "public"):
        select(nb, monkeypatch, side)
        grid = nb.SpatialHashGrid(case.n, 1.0)
        assert_selected(nb, side)
        d, _ = to_device(nb, case.ic)
        grid.build(d)
        grid.computeForces(d, 1.0, 1.0, 0.05)
        acc[side] = acc_of(d).view(np.uint32).copy()
        check_grid(nb, grid, case, f"NBH_SORT={side}")
        grid.close()
    assert np.all(np.isfinite(acc["public"].view(np.float32))) and np.any(acc["public"])
    same(acc[which], acc["public"], f"accelerations after NBH_SORT={which} against NBH_SORT=public")


@pytest.mark.parametrize("which", IMPLS)
def test_forces_after_the_sort_tree(nb, oracle, ctx, monkeypatch, which):
    """depth-20 tree, theta = 0.5"""
    case = memo(("tree forces",), lambda: TreeCase(oracle, plummer(nb, N_EDGE, seed=701), 20))
    acc = {}
    for side in (which, "public"):
        select(nb, monkeypatch, side)
        tree = nb.BarnesHutTree(case.n)
        tree.setParams(20, 1)
        assert_selected(nb, side)
        d, _ = to_device(nb, case.ic)
        tree.build(d)
        tree.computeForces(d, 0.5, 1.0, 0.05)
        acc[side] = acc_of(d).view(np.uint32).copy()
        same(sr.tree_order(nb, tree, case.n), case.order, f"NBH_SORT={side}: sorted_indices_ against the stable argsort")
        tree.close()
    assert np.all(np.isfinite(acc["public"].view(np.float32))) and np.any(acc["public"])
    same(acc[which], acc["public"], f"accelerations after NBH_SORT={which} against NBH_SORT=public")

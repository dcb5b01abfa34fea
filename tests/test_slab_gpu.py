"""The bookkeeping kernels of the z-slab decomposition at their edge shapes, against tests/slab_ref.py, bit for bit:
nbody_hip_slab_partition / _partition_cuts / _fill (csrc/slab.hip), nbody_hip_bbox_packed / _drift_bbox_packed /
_cell_z_packed (csrc/spatial_hash.hip), nbody_hip_drift_packed / _kick_packed (csrc/integrator.hip).  A defect in these
loses, duplicates or misplaces a body; the force-parity tests above them only notice when that body is among those compared.

Every call goes through the C ABI with ctypes (HipBackend.slab_partition cannot pass cuts, a NULL gid or a separate
histogram).  Every output buffer is prefilled: rows, holes and the body arrays with a sentinel that must survive past what
the call writes, the send matrix, the histogram and info with garbage that must be zeroed or overwritten (with guard words
behind them that must survive).  Every comparison is == on integers or bit patterns; a failure names the first entry.

The shape of the partition pass: <= 256 blocks, block b works on [b chunk, (b+1) chunk) in rounds of 256 bodies, chunk a
multiple of 256.  Up to 65,536 bodies every block has one round; 65,537 is the first two-round shape (chunk 512, the
blocks from 129 on are empty), 131,073 the first three-round one (chunk 768: round 2 reuses round 0's wave_cnt buffer),
200,000 has four (chunk 1024, the last block partial with a partial second round)."""
import ctypes as C

import numpy as np
import pytest
import torch

import slab_ref as ref

pytestmark = pytest.mark.gpu

F = np.float32
FSENT = 0x7FC5A5A5       # rows and body arrays before a call: the bits of a NaN that no kernel here produces
ISENT = -0x5A5A5A5B      # holes and ids before a call
GARBAGE = 0x3C3C3C3C     # send matrix, histogram and info before a call
GUARD = 16               # words behind every buffer that must keep what they held
HIST_CAP = 4096
BOX = (0.0, 0.0, 0.0, 8.0, 8.0, 40.0)        # cell 1: 42 layers
SIZES = [0, 1, 63, 64, 65, 255, 256, 257, 1000, 65535, 65536, 65537, 131073, 200000]
WORLDS = [(1, 0), (2, 0), (2, 1), (3, 1), (8, 0), (8, 7), (32, 13), (64, 63)]
TWO_WORLDS = [(3, 1), (8, 7)]
POP_SIZES = [1000, 131073]
ERR_VALIDATION = -1

_memo = {}


def memo(key, make):
    """inputs and their references are computed once and shared by the cases that need them"""
    if key not in _memo:
        _memo[key] = make()
    return _memo[key]


def same(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    if got.shape == want.shape and np.array_equal(got, want):
        return
    assert got.shape == want.shape, f"{what}: shape {got.shape} against {want.shape}"
    diff = got != want
    bad = np.flatnonzero(diff if diff.ndim == 1 else diff.reshape(diff.shape[0], -1).any(axis=1))
    k = int(bad[0])
    pytest.fail(f"{what}: {bad.size} of {want.shape[0]} entries differ, first at {k}: got {got[k]}, want {want[k]}")


def all_equal(got, value, what):
    got = np.asarray(got)
    same(got, np.full(got.shape, value, got.dtype), what)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def bits(a):
    """the words of an fp32 / int32 array (or of a device tensor) as uint32"""
    if isinstance(a, torch.Tensor):
        a = a.cpu().numpy()
    return np.ascontiguousarray(a).view(np.uint32)


def prefilled(shape, value):
    return torch.full(shape, value, dtype=torch.int32, device="cuda")


def ptr(t):
    return None if t is None or t.numel() == 0 else t.data_ptr()


def launch_shape(n):
    """(blocks, chunk) of the partition pass, restated from nbody_hip_slab_partition_cuts"""
    nblocks = min(max((n + 255) // 256, 1), 256)
    chunk = max(((n + nblocks - 1) // nblocks + 255) // 256 * 256, 256)
    return nblocks, chunk


def test_the_sizes_are_where_the_shape_of_the_partition_changes():
    assert [launch_shape(n) for n in (0, 1, 256, 257, 65535, 65536)] == [(1, 256), (1, 256), (1, 256), (2, 256), (256, 256),
                                                                        (256, 256)]
    assert launch_shape(65537) == (256, 512) and (65537 + 511) // 512 == 129      # blocks 129.. have nothing
    assert launch_shape(131072) == (256, 512) and launch_shape(131073) == (256, 768)
    assert launch_shape(200000) == (256, 1024) and 200000 % 1024 == 320           # 196 blocks; the last: 256 + 64 bodies


# ---- populations ---------------------------------------------------------------------------------------------------------
class Pop:
    """the bodies of one rank (ids a permutation, so that an id is not a position) and the GLOBAL box"""

    def __init__(self, z, gbox, seed, xy=8.0):
        rng = np.random.default_rng(seed)
        self.n = n = int(np.asarray(z).size)
        self.posm = np.empty((n, 4), F)
        self.posm[:, 0:2] = rng.uniform(0.0, xy, (n, 2))
        self.posm[:, 2] = z
        self.posm[:, 3] = rng.uniform(0.5, 1.5, n)
        self.vel = rng.normal(size=(n, 4)).astype(F)      # (the w lanes are not zero: the rows must not carry them)
        self.acc = rng.normal(size=(n, 4)).astype(F)
        self.gid = (rng.permutation(n) * 3 + 1).astype(np.int32)
        self.gbox = np.array(gbox, F)
        self._dev = None

    def device(self):
        if self._dev is None:
            self._dev = {k: dev(getattr(self, k)) for k in ("posm", "vel", "acc", "gid", "gbox")}
        return self._dev


def grid_of(gbox, cell):
    lo, dims = ref.geometry(gbox, cell)
    return lo[2], dims[2]


def layer_z(layers, lo_z, cell):
    """a z well inside each of `layers`: its centre"""
    uniq, inv = np.unique(layers, return_inverse=True)
    return np.array([ref.layer_centre(int(k), lo_z, cell) for k in uniq], F)[inv.reshape(-1)]


def uniform_pop(n):
    return memo(("uniform", n), lambda: Pop(np.random.default_rng(10 + n).uniform(0.0, 40.0, n).astype(F), BOX, 20 + n))


def gauss_pop(n):
    def make():
        z = np.clip(20.0 + 6.0 * np.random.default_rng(30 + n).normal(size=n), 0.0, 40.0).astype(F)
        return Pop(z, BOX, 40 + n)
    return memo(("gauss", n), make)


def shaped_pop(name, n, W, rank):
    """the populations of the issue on the 42-layer box (equal layer counts)"""
    def make():
        rng = np.random.default_rng(1000 * n + 10 * W + rank + sum(map(ord, name)))
        lo_z, gz = grid_of(BOX, 1.0)
        owner = ref.owner_table(gz, lo_z, 1.0, W)
        mine, others = np.flatnonzero(owner == rank), np.flatnonzero(owner != rank)
        inside = rng.uniform(float(mine[0]) + 0.01, float(mine[-1]) + 0.99, n).astype(F) + lo_z
        if name == "inside":
            z = inside
        elif name == "outside":
            z = rng.uniform(0.0, 40.0, n).astype(F)
            stay = owner[ref.layer(z, lo_z, 1.0, gz)] == rank
            z[stay] = layer_z(rng.choice(others, int(stay.sum())), lo_z, 1.0)
        elif name == "one_owner":
            z = inside
            go = rng.random(n) < 0.3
            go[n // 2] = True
            z[go] = layer_z(np.full(int(go.sum()), np.flatnonzero(owner == (rank + 1) % W)[0]), lo_z, 1.0)
        else:
            k = {"leaver_first": 0, "leaver_last": n - 1}.get(name)
            k = int(name.split("_")[1]) if k is None else k
            z = inside
            z[k] = layer_z(rng.choice(others, 1), lo_z, 1.0)[0]
        return Pop(z, BOX, 50 + n)
    return memo((name, n, W, rank), make)


# ---- the partition pass against the restatement ---------------------------------------------------------------------------
def run_partition(nb, ctx, pop, cell, W, rank, hist_cap=HIST_CAP, cuts=None, ids=True, adjacent=True, tag=""):
    """one call, every output compared with ref.partition -> (the reference, the rows and holes read back)"""
    lib, d, n = nb._lib.load(), pop.device(), pop.n
    cap = max(n, 1)
    rows, holes = prefilled((cap, 16), FSENT), prefilled((cap,), ISENT)
    if adjacent:     # matrix and histogram in one block, as the sharded hosts hold them: one fill
        stats = prefilled((W * W + hist_cap + GUARD,), GARBAGE)
        sm_ptr, hist_ptr = stats.data_ptr(), stats.data_ptr() + 4 * W * W
    else:            # two allocations: two fills
        sm, hist = prefilled((W * W + GUARD,), GARBAGE), prefilled((hist_cap + GUARD,), GARBAGE)
        sm_ptr, hist_ptr = sm.data_ptr(), hist.data_ptr()
    info = prefilled((4 + GUARD,), GARBAGE)
    args = [ctx.handle, ptr(d["posm"]), ptr(d["vel"]), ptr(d["acc"]), ptr(d["gid"]) if ids else None, n,
            d["gbox"].data_ptr(), float(cell), W, rank, hist_cap, rows.data_ptr(), holes.data_ptr(), sm_ptr, hist_ptr,
            info.data_ptr()]
    if cuts is None:
        nb._lib.check(lib.nbody_hip_slab_partition(*args))
    else:
        cbuf = (C.c_float * max(len(cuts), 1))(*[float(c) for c in cuts])
        nb._lib.check(lib.nbody_hip_slab_partition_cuts(*args, cbuf))
    rows, holes, info = rows.cpu().numpy(), holes.cpu().numpy(), info.cpu().numpy()
    if adjacent:
        stats = stats.cpu().numpy()
        sm, hist = stats[:W * W], stats[W * W:W * W + hist_cap]
        guards = [("behind the histogram", stats[W * W + hist_cap:])]
    else:
        sm, hist = sm.cpu().numpy(), hist.cpu().numpy()
        guards = [("behind the send matrix", sm[W * W:]), ("behind the histogram", hist[hist_cap:])]
        sm, hist = sm[:W * W], hist[:hist_cap]
    key = ("partition", id(pop), float(cell), W, rank, hist_cap, None if cuts is None else bytes(np.asarray(cuts, F)), ids)
    want = memo(key, lambda: ref.partition(pop.posm, pop.vel, pop.acc, pop.gid if ids else None, pop.gbox, cell, W, rank,
                                           hist_cap, cuts))
    tag = f"{tag} n={n} W={W} rank={rank} cell={float(cell):.3f} hist_cap={hist_cap}"
    L, nh = want["holes"].size, want["hist"].size
    same(info[:4], want["info"], f"{tag}: info")
    all_equal(info[4:], GARBAGE, f"{tag}: the words behind info")
    for what, g in guards:
        all_equal(g, GARBAGE, f"{tag}: the words {what}")
    want_sm = np.zeros((W, W), np.int32)
    want_sm[rank] = want["send"]
    same(sm.reshape(W, W), want_sm, f"{tag}: send matrix (rows)")
    same(hist[:nh], want["hist"], f"{tag}: layer histogram")
    all_equal(hist[nh:], 0, f"{tag}: the histogram from layer {nh} on")
    same(holes[:L], want["holes"], f"{tag}: holes against the leavers' positions")
    all_equal(holes[L:], ISENT, f"{tag}: holes past the {L} leavers")
    same(bits(rows[:L]), bits(want["rows"]), f"{tag}: rows (of 16 words)")
    all_equal(rows[L:], FSENT, f"{tag}: rows past the {L} leavers")
    return want, rows[:L], holes[:L]


def test_partition_of_nothing(nb, ctx):
    """n = 0 with NULL body arrays and W > 1: an all-zero row and histogram, info from the box"""
    for W, rank in WORLDS[1:]:
        pop = memo(("empty",), lambda: Pop(np.zeros(0, F), BOX, 1))
        want, _, _ = run_partition(nb, ctx, pop, 1.0, W, rank)
        assert want["info"].tolist() == [10, 10, 42, 0] and not want["send"].any() and not want["hist"].any()


@pytest.mark.parametrize("W,rank", TWO_WORLDS)
@pytest.mark.parametrize("n", SIZES[1:])
def test_partition_sizes(nb, ctx, n, W, rank):
    want, _, _ = run_partition(nb, ctx, uniform_pop(n), 1.0, W, rank)
    assert want["info"].tolist() == [10, 10, 42, 0]
    if n >= 1000:
        assert 0 < want["holes"].size < n


@pytest.mark.parametrize("W,rank", WORLDS)
@pytest.mark.parametrize("n", POP_SIZES)
def test_partition_worlds(nb, ctx, n, W, rank):
    """W = 64 is what csrc/slab.hip accepts (NBODY_HIP_MAX_RANKS, the sharded systems' limit, is 32)"""
    want, _, _ = run_partition(nb, ctx, uniform_pop(n), 1.0, W, rank)
    assert (want["holes"].size == 0) == (W == 1)
    if W == 64:   # every layer its own owner, 22 ranks own nothing (the bodies reach layer 39 or 40 of the 42)
        assert np.count_nonzero(want["send"]) == np.unique(want["layer"]).size >= 40


@pytest.mark.parametrize("W,rank", TWO_WORLDS)
@pytest.mark.parametrize("name", ["inside", "outside", "one_owner", "leaver_first", "leaver_last", "leaver_255", "leaver_256",
                                  "leaver_511", "leaver_512"])
@pytest.mark.parametrize("n", POP_SIZES)
def test_partition_populations(nb, ctx, n, name, W, rank):
    """nobody leaves (nothing written), everybody leaves, all leavers to one owner, ONE leaver at the ends and at the seams
    of the rounds of 256"""
    want, _, _ = run_partition(nb, ctx, shaped_pop(name, n, W, rank), 1.0, W, rank, tag=name)
    L = want["holes"].size
    if name == "inside":
        assert L == 0
    elif name == "outside":
        assert L == n and want["send"][rank] == 0
    elif name == "one_owner":
        assert 0 < L < n and np.count_nonzero(want["send"]) == 2
    else:
        assert L == 1


@pytest.mark.parametrize("n", POP_SIZES)
def test_partition_all_64_owners_in_every_wave(nb, ctx, n):
    """W = 64, body i bound for owner i % 64 (129 layers, so that every rank owns some)"""
    box = (0.0, 0.0, 0.0, 8.0, 8.0, 127.5)

    def make():
        lo_z, gz = grid_of(box, 1.0)
        assert gz == 129
        owner = ref.owner_table(gz, lo_z, 1.0, 64)
        first = np.array([np.flatnonzero(owner == r)[0] for r in range(64)])
        return Pop(layer_z(first[np.arange(n) % 64], lo_z, 1.0), box, 60 + n)
    pop = memo(("mod64", n), make)
    want, _, _ = run_partition(nb, ctx, pop, 1.0, 64, 63)
    same(want["dest"], np.arange(n) % 64, "the population itself")


@pytest.mark.parametrize("rank", [0, 3, 7])
@pytest.mark.parametrize("n", POP_SIZES)
def test_partition_fewer_layers_than_ranks(nb, ctx, n, rank):
    """gz = 2 with W = 8: the layers belong to ranks 3 and 7, six ranks own nothing.  (A grid of two layers has its whole
    box in layer 0 -- the second one is the spare layer every grid has -- so half of these bodies lie ABOVE the box given
    to the pass, where only the clamp puts them into layer 1.)"""
    box = (0.0, 0.0, 0.0, 8.0, 8.0, 0.9)
    pop = memo(("gz2", n), lambda: Pop(np.random.default_rng(70 + n).uniform(0.0, 2.0, n).astype(F), box, 71 + n))
    want, _, _ = run_partition(nb, ctx, pop, 1.0, 8, rank)
    assert want["info"][2] == 2 and np.flatnonzero(want["send"]).tolist() == [3, 7]


@pytest.mark.parametrize("W,rank", TWO_WORLDS)
@pytest.mark.parametrize("n", POP_SIZES)
def test_partition_without_ids_and_with_a_separate_histogram(nb, ctx, n, W, rank):
    run_partition(nb, ctx, uniform_pop(n), 1.0, W, rank, ids=False, tag="gid NULL")
    run_partition(nb, ctx, uniform_pop(n), 1.0, W, rank, adjacent=False, tag="two allocations")
    run_partition(nb, ctx, uniform_pop(n), 1.0, W, rank, ids=False, adjacent=False, tag="gid NULL, two allocations")


# ---- bodies on the layer boundaries; the slab's layer and the grid's layer are one function ------------------------------
def boundary_pop(cell):
    def make():
        lo_z, gz = grid_of(BOX, cell)
        edge = np.array([F(lo_z) + F(k) * F(cell) for k in range(gz + 1)], F)
        hi_z = F(BOX[5]) + ref.PAD
        far = np.array([lo_z - F(5), lo_z - F(1e6), ref.down(lo_z), hi_z + F(5), hi_z + F(1e6), ref.up(hi_z),
                        F(lo_z) + F(gz) * F(cell) + F(3)], F)
        z = np.concatenate([edge, np.nextafter(edge, F(-np.inf)), np.nextafter(edge, F(np.inf)), far])
        return Pop(np.random.default_rng(80).permutation(z), BOX, 81)
    return memo(("boundary", float(cell)), make)


def device_layers(nb, ctx, pop, lo_z, cell, gz):
    cz = prefilled((pop.n + GUARD,), ISENT)
    nb._lib.check(nb._lib.load().nbody_hip_cell_z_packed(ctx.handle, pop.device()["posm"].data_ptr(), pop.n, float(lo_z),
                                                         float(cell), gz, cz.data_ptr()))
    cz = cz.cpu().numpy()
    all_equal(cz[pop.n:], ISENT, "nbody_hip_cell_z_packed: the words behind its output")
    return cz[:pop.n]


@pytest.mark.parametrize("W,rank", TWO_WORLDS)
@pytest.mark.parametrize("cell", [F(1.0), F(0.7)], ids=["cell1", "cell0.7"])
def test_partition_on_the_layer_boundaries(nb, ctx, cell, W, rank):
    """z = fp32(lo_z + k cell) for every k, its neighbours on both sides, and z outside the box (clamped to layers 0 and
    gz - 1).  The layers of the rows and the histogram are also those of nbody_hip_cell_z_packed."""
    pop = boundary_pop(cell)
    lo_z, gz = grid_of(BOX, cell)
    assert gz == (42 if cell == F(1.0) else 59)
    want, rows, holes = run_partition(nb, ctx, pop, cell, W, rank, tag="boundaries")
    z = pop.posm[:, 2]
    below, above = z < lo_z, z >= F(lo_z) + F(gz) * F(cell)
    assert below.sum() >= 4 and above.sum() >= 4       # (what ref.layer says of them is the C expression's clamp)
    assert np.all(want["layer"][below] == 0) and np.all(want["layer"][above] == gz - 1)
    assert np.all(np.bincount(want["layer"], minlength=gz) >= 1)
    cz = device_layers(nb, ctx, pop, lo_z, cell, gz)
    same(cz, want["layer"].astype(np.int32), "nbody_hip_cell_z_packed against ref.layer")
    at = np.empty(int(pop.gid.max()) + 1, np.int64)
    at[pop.gid] = np.arange(pop.n)                     # id -> input position
    same(rows[:, 13], cz[at[rows[:, 12]]], "the layers in the rows against nbody_hip_cell_z_packed")
    same(want["hist"], np.bincount(cz, minlength=gz).astype(np.int32), "the histogram against nbody_hip_cell_z_packed")


@pytest.mark.parametrize("n", SIZES[1:])
def test_cell_z_sizes(nb, ctx, n):
    pop = uniform_pop(n)
    lo_z, gz = grid_of(BOX, 1.0)
    same(device_layers(nb, ctx, pop, lo_z, 1.0, gz), ref.layer(pop.posm[:, 2], lo_z, 1.0, gz).astype(np.int32),
         f"nbody_hip_cell_z_packed, n={n}")


# ---- grids taller than the LDS histogram -----------------------------------------------------------------------------------
@pytest.mark.parametrize("W,rank", TWO_WORLDS)
@pytest.mark.parametrize("hist_cap", [8192, 4096])
def test_partition_tall_grids(nb, ctx, hist_cap, W, rank):
    """a column of 5,000 layers (2 x 2 cells wide: nothing allocates cells here).  hist_cap 8192: the layers from 4,096 on
    are counted with global atomics; hist_cap 4096: the verdict info[3] = 1, and the histogram of the first 4,096 layers,
    the rows and the holes are still right"""
    box = (0.0, 0.0, 0.0, 1e-4, 1e-4, 4998.5)
    pop = memo(("tall",), lambda: Pop(np.random.default_rng(90).uniform(0.0, 4998.5, 20000).astype(F), box, 91, xy=1e-4))
    want, _, _ = run_partition(nb, ctx, pop, 1.0, W, rank, hist_cap=hist_cap, tag="tall")
    assert want["info"].tolist() == [2, 2, 5000, int(hist_cap == 4096)]
    assert want["hist"].size == min(5000, hist_cap) and want["hist"][4000:].sum() > 0
    run_partition(nb, ctx, pop, 1.0, W, rank, hist_cap=hist_cap, adjacent=False, tag="tall, two allocations")


# ---- cuts ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("W,rank", TWO_WORLDS)
@pytest.mark.parametrize("n", SIZES)
def test_partition_cuts_sizes(nb, ctx, n, W, rank):
    """cuts from the population's own layer histogram by the balancing rule of the sharded host"""
    pop = gauss_pop(n)
    lo_z, gz = grid_of(BOX, 1.0)
    hist = np.bincount(ref.layer(pop.posm[:, 2], lo_z, 1.0, gz), minlength=gz)
    cuts = ref.balanced_cuts(hist, lo_z, 1.0, W, n)
    assert cuts.size == W - 1 and np.all(np.diff(cuts) >= 0)
    want, _, _ = run_partition(nb, ctx, pop, 1.0, W, rank, cuts=cuts, tag="balanced cuts")
    if n >= 65535:
        assert want["send"].min() > 0.5 * n / W       # (the cuts do balance: equal layer counts leave the end ranks 5 %)


def host_owner(nb, layer, lo_z, cell, W, cuts):
    buf = (C.c_float * max(len(cuts), 1))(*[float(c) for c in cuts])
    return nb._lib.load().nbody_hip_slab_layer_owner(int(layer), float(lo_z), float(cell), W, buf)


@pytest.mark.parametrize("cell", [F(1.0), F(0.7)], ids=["cell1", "cell0.7"])
@pytest.mark.parametrize("W", [2, 5, 32, 64])
def test_partition_crafted_cuts(nb, ctx, W, cell):
    """one body per layer; cuts exactly at layer centres, one ulp either side, two equal ones, all below, all above.
    Each body's owner ON THE DEVICE -- recovered from the holes, the grouping of the rows and the send row -- is the one
    the host entry point and the restatement name."""
    lo_z, gz = grid_of(BOX, cell)
    rank = W // 2
    z = np.array([ref.layer_centre(k, lo_z, cell) for k in range(gz)], F)
    assert ref.layer(z, lo_z, cell, gz).tolist() == list(range(gz))
    pop = memo(("per layer", float(cell)), lambda: Pop(z, BOX, 95))
    for name, cuts in ref.crafted_cuts(lo_z, cell, gz, W, np.random.default_rng(100 + W)).items():
        want, rows, holes = run_partition(nb, ctx, pop, cell, W, rank, cuts=cuts, ids=False, tag=f"cuts {name}")
        owner = np.full(gz, rank, np.int64)
        off = 0
        for q in range(W):
            if q != rank:
                cnt = int(want["send"][q])          # (run_partition has held the device's send row to this)
                owner[rows[off:off + cnt, 12]] = q  # ids = input positions = layers
                off += cnt
        assert off == holes.size
        same(np.flatnonzero(owner != rank), holes, f"cuts {name}: holes against the rows' ids")
        same(owner, np.array([host_owner(nb, k, lo_z, cell, W, cuts) for k in range(gz)]),
             f"cuts {name}, W={W}: the device's owners against nbody_hip_slab_layer_owner")
        same(owner, ref.owner_table(gz, lo_z, cell, W, cuts), f"cuts {name}, W={W}: the device's owners against ref.owner_cuts")
        if name == "two_equal":
            assert 1 not in owner
        if name in ("all_below", "all_above"):
            assert set(owner.tolist()) == {W - 1 if name == "all_below" else 0}


def test_partition_rejects_descending_cuts(nb, ctx):
    """the validation error, and nothing written"""
    pop, W = uniform_pop(1000), 3
    d = pop.device()
    rows, holes = prefilled((pop.n, 16), FSENT), prefilled((pop.n,), ISENT)
    stats, info = prefilled((W * W + HIST_CAP,), GARBAGE), prefilled((4,), GARBAGE)
    rc = nb._lib.load().nbody_hip_slab_partition_cuts(
        ctx.handle, d["posm"].data_ptr(), d["vel"].data_ptr(), d["acc"].data_ptr(), d["gid"].data_ptr(), pop.n,
        d["gbox"].data_ptr(), 1.0, W, 1, HIST_CAP, rows.data_ptr(), holes.data_ptr(), stats.data_ptr(),
        stats.data_ptr() + 4 * W * W, info.data_ptr(), (C.c_float * 2)(25.0, 15.0))
    assert rc == ERR_VALIDATION and b"ascend" in nb._lib.load().nbody_hip_last_error()
    torch.cuda.synchronize()
    all_equal(rows.cpu().numpy(), FSENT, "rows after the rejected call")
    all_equal(holes.cpu().numpy(), ISENT, "holes after the rejected call")
    all_equal(stats.cpu().numpy(), GARBAGE, "matrix and histogram after the rejected call")
    all_equal(info.cpu().numpy(), GARBAGE, "info after the rejected call")


# ---- the fill pass ---------------------------------------------------------------------------------------------------------
FILL_CASES = ["empties", "append", "equal", "one_fewer", "more", "tail_holes", "front_holes", "interleaved", "hole_below_end",
              "hole_at_end", "hole_both", "no_ids"]


def fill_case(name, M, rng):
    """-> (n_old, holes ascending, A) with max(A, L) = M (hole_both: M + 1)"""
    pick = lambda n, k, without=(): np.sort(rng.choice(np.setdiff1d(np.arange(n), without), k, replace=False))  # noqa: E731
    if name == "empties":                       # the rank loses every body and gets none
        return M, np.arange(M), 0
    if name == "append":                        # no holes (holes == NULL): arrivals behind the old end
        return M + 37, np.zeros(0, np.int64), M
    if name == "equal":
        return 2 * M + 13, pick(2 * M + 13, M), M
    if name == "one_fewer":                     # ONE slot to close
        return 2 * M + 13, pick(2 * M + 13, M), M - 1
    if name == "more":                          # the holes used up, the rest appended
        return 2 * M + 13, pick(2 * M + 13, M // 2), M
    if name == "tail_holes":                    # every hole left open lies in the tail: nothing moves
        return 3 * M, np.arange(2 * M, 3 * M), M // 3
    if name == "front_holes":                   # every body of the tail moves
        return 3 * M, np.arange(M), M // 3
    if name in ("interleaved", "no_ids"):
        return 2 * M + 5, np.arange(0, 2 * M, 2), M // 2
    L = M + 1 if name == "hole_both" else M     # a hole in the last slot below the new end / the first slot behind it
    n_old, A = 3 * M + 3, M // 2
    n_new = n_old - L + A
    forced = {"hole_below_end": [n_new - 1], "hole_at_end": [n_new], "hole_both": [n_new - 1, n_new]}[name]
    return n_old, np.sort(np.concatenate([pick(n_old, L - len(forced), without=[n_new - 1, n_new]), forced])), A


@pytest.mark.parametrize("name", FILL_CASES)
@pytest.mark.parametrize("M", [1, 255, 256, 257, 70000])
def test_fill(nb, ctx, M, name):
    """the slot layout of ref.fill, bit for bit over the whole arrays: [0, n_new), what the pass leaves behind in
    [n_new, n_old), and the sentinel past n_old + max(A - L, 0)"""
    rng = np.random.default_rng(1000 * M + FILL_CASES.index(name))
    n_old, holes, A = fill_case(name, M, rng)
    L = holes.size
    n_new = n_old - L + A
    assert max(A, L) == (M + 1 if name == "hole_both" else M) and np.all(np.diff(holes) > 0) and n_new >= 0
    if name == "tail_holes":
        assert np.all(holes[A:] >= n_new)
    if name == "front_holes":
        assert holes[-1] < n_new
    cap = max(n_old, n_new) + GUARD
    words = lambda rows, width: rng.integers(0, 2 ** 32, (rows, width), dtype=np.uint32).view(np.int32)  # noqa: E731
    state = []
    for _ in range(3):
        a = np.full((cap, 4), FSENT, np.int32)
        a[:n_old] = words(n_old, 4)
        state.append(a)
    gid = np.full(cap, ISENT, np.int32)
    gid[:n_old] = rng.permutation(n_old)
    arrivals = words(A, 16)
    use_ids = name != "no_ids"
    d = [dev(a) for a in state] + [dev(gid) if use_ids else None]
    d_holes, d_arr = dev(holes.astype(np.int32)), dev(arrivals)
    nb._lib.check(nb._lib.load().nbody_hip_slab_fill(ctx.handle, ptr(d_arr), A, ptr(d_holes), L, n_old, d[0].data_ptr(),
                                                     d[1].data_ptr(), d[2].data_ptr(), ptr(d[3])))
    got = [t.cpu().numpy() for t in d[:3]] + [d[3].cpu().numpy() if use_ids else None]
    assert ref.fill(state[0], state[1], state[2], gid if use_ids else None, n_old, holes, arrivals) == n_new
    tag = f"fill {name}: n_old={n_old} L={L} A={A} n_new={n_new}"
    for k, what in enumerate(("posm", "vel", "acc")):
        same(got[k][:n_new], state[k][:n_new], f"{tag}: {what} in [0, n_new)")
        same(got[k][n_new:], state[k][n_new:], f"{tag}: {what} behind n_new (left-overs and the sentinel)")
        all_equal(got[k][max(n_old, n_new):], FSENT, f"{tag}: {what} past the last slot the pass may write")
    if use_ids:
        same(got[3], gid, f"{tag}: ids")
        all_equal(got[3][max(n_old, n_new):], ISENT, f"{tag}: ids past the last slot the pass may write")


# ---- the conservation law of the decomposition, on the device kernels only ----------------------------------------------------
def device_box(nb, ctx, posm_dev, n):
    out = prefilled((6 + GUARD,), GARBAGE)
    nb._lib.check(nb._lib.load().nbody_hip_bbox_packed(ctx.handle, posm_dev.data_ptr(), n, out.data_ptr()))
    out = out.cpu().numpy()
    all_equal(out[6:], GARBAGE, "nbody_hip_bbox_packed: the words behind its output")
    return out[:6].view(F)


@pytest.mark.parametrize("W", [2, 3, 8])
def test_round_trip(nb, ctx, W):
    """W virtual ranks on the one context, 60,000 bodies, four rounds of move -> box -> partition -> exchange -> fill; cuts
    from the second round on; the third round moves most bodies.  The rows are exchanged on the host exactly as the sharded
    host orders them: the sender's groups by owner, the receiver's arrivals by source rank."""
    lib, n, cell = nb._lib.load(), 60000, F(1.0)
    rng = np.random.default_rng(200 + W)
    words = lambda a: np.ascontiguousarray(a).view(np.int32)  # noqa: E731
    P = np.empty((n, 4), F)
    P[:, :3] = rng.uniform((0, 0, 0), (8, 8, 40), (n, 3))
    P[:, 3] = rng.uniform(0.5, 1.5, n)
    V, Acc = rng.normal(size=(n, 4)).astype(F), rng.normal(size=(n, 4)).astype(F)
    start = rng.permutation(n)                                  # the first distribution is arbitrary: most bodies move at once
    ranks = [dict(gid=np.sort(part).astype(np.int32)) for part in np.array_split(start, W)]
    cuts, prev = None, None
    for rnd in range(4):
        # about 10 % change owner: a step of mean length 0.8 sigma crosses one of W - 1 boundaries in a box of 40
        P[:, 2] = rng.uniform(0.0, 40.0, n) if rnd == 2 else np.clip(P[:, 2] + rng.normal(0.0, 5.0 / (W - 1), n), -3.0, 43.0)
        for r in ranks:                                        # the rank's arrays as they stand (the host moved z only)
            r["posm"], r["vel"], r["acc"] = P[r["gid"]].copy(), V[r["gid"]].copy(), Acc[r["gid"]].copy()
            r["n"] = r["gid"].size
            r["dev"] = {k: dev(r[k]) for k in ("posm", "vel", "acc", "gid")}
        boxes = [device_box(nb, ctx, r["dev"]["posm"], r["n"]) for r in ranks if r["n"]]
        gbox = np.concatenate([np.min([b[:3] for b in boxes], 0), np.max([b[3:] for b in boxes], 0)]).astype(F)
        same(bits(gbox), bits(np.concatenate([P[:, :3].min(0), P[:, :3].max(0)])), f"round {rnd}: the reduced box")
        lo, dims = ref.geometry(gbox, cell)
        gz = dims[2]
        if rnd >= 1:   # physical coordinates, from the previous evaluation's histogram on the previous evaluation's grid
            cuts = ref.balanced_cuts(prev[0], prev[1], cell, W, n)
        layers = ref.layer(P[:, 2], lo[2], cell, gz)
        table = ref.owner_table(gz, lo[2], cell, W, cuts)
        want_owner = table[layers]                              # the rank the reference names, by id
        gbox_dev = dev(gbox)
        M, hist = np.zeros((W, W), np.int64), np.zeros(HIST_CAP, np.int64)
        for k, r in enumerate(ranks):
            cap = max(r["n"], 1)
            r["rows"], r["holes"] = prefilled((cap, 16), FSENT), prefilled((cap,), ISENT)
            stats, info = prefilled((W * W + HIST_CAP,), GARBAGE), prefilled((4,), GARBAGE)
            d = r["dev"]
            nb._lib.check(lib.nbody_hip_slab_partition_cuts(
                ctx.handle, ptr(d["posm"]), ptr(d["vel"]), ptr(d["acc"]), ptr(d["gid"]), r["n"], gbox_dev.data_ptr(), 1.0,
                W, k, HIST_CAP, r["rows"].data_ptr(), r["holes"].data_ptr(), stats.data_ptr(), stats.data_ptr() + 4 * W * W,
                info.data_ptr(), None if cuts is None else (C.c_float * max(W - 1, 1))(*[float(c) for c in cuts])))
            stats = stats.cpu().numpy()
            assert info.cpu().numpy().tolist() == [dims[0], dims[1], gz, 0]
            same(stats[:W * W].reshape(W, W)[np.arange(W) != k], np.zeros((W - 1, W), np.int32), f"round {rnd}: foreign rows")
            M[k] = stats[k * W:(k + 1) * W]
            hist += stats[W * W:]
        same(hist[:gz], np.bincount(layers, minlength=gz), f"round {rnd}: the summed histogram against all layers")
        same(M.sum(1), np.array([r["n"] for r in ranks]), f"round {rnd}: row sums of the send matrix")
        moved = int(M.sum() - np.trace(M))
        assert moved > (n // 3 if rnd in (0, 2) else n // 50) and (rnd in (0, 2) or moved < n // 3), (rnd, moved)
        host_rows = [r["rows"].cpu().numpy() for r in ranks]
        for q, r in enumerate(ranks):
            got = []
            for p in range(W):                                  # arrivals by source rank ...
                if p != q:
                    soff = sum(int(M[p, k]) for k in range(q) if k != p)   # ... each the sender's group for q
                    got.append(host_rows[p][soff:soff + int(M[p, q])])
            got = np.concatenate(got) if got else np.zeros((0, 16), np.int32)
            A, L, n_old = got.shape[0], int(r["n"] - M[q, q]), r["n"]
            n_new = n_old - L + A
            cap = max(n_old, n_new) + GUARD
            buf = {}
            for name in ("posm", "vel", "acc"):
                buf[name] = np.full((cap, 4), FSENT, np.int32)
                buf[name][:n_old] = words(r[name])
            buf["gid"] = np.full(cap, ISENT, np.int32)
            buf["gid"][:n_old] = r["gid"]
            d = {name: dev(a) for name, a in buf.items()}
            d_got = dev(got)
            nb._lib.check(lib.nbody_hip_slab_fill(ctx.handle, ptr(d_got), A, ptr(r["holes"]), L, n_old, d["posm"].data_ptr(),
                                                  d["vel"].data_ptr(), d["acc"].data_ptr(), d["gid"].data_ptr()))
            r["new"] = {name: t.cpu().numpy() for name, t in d.items()}
            r["n_new"] = n_new
            for name in ("posm", "vel", "acc"):
                all_equal(r["new"][name][max(n_old, n_new):], FSENT, f"round {rnd}, rank {q}: {name} behind the fill")
        same(np.array([r["n_new"] for r in ranks]), M.sum(0), f"round {rnd}: bodies per rank against the column sums")
        ids = np.concatenate([r["new"]["gid"][:r["n_new"]] for r in ranks])
        same(np.sort(ids), np.arange(n, dtype=np.int32), f"round {rnd}: every id exactly once")
        for q, r in enumerate(ranks):
            g = r["new"]["gid"][:r["n_new"]]
            same(want_owner[g], np.full(g.size, q), f"round {rnd}, rank {q}: every body on the rank the reference names")
            for name, whole in (("posm", P), ("vel", V), ("acc", Acc)):
                want = words(whole[g])
                if name != "posm":
                    arrived = ~np.isin(g, r["gid"])             # (a row carries vx, vy, vz, 0: the w lane of an arrival is 0)
                    want[arrived, 3] = 0
                same(r["new"][name][:r["n_new"]], want, f"round {rnd}, rank {q}: {name} by id, bit for bit")
            r["gid"] = g.copy()
        prev = (np.bincount(layers, minlength=gz), lo[2])


# ---- box, drift, kick ---------------------------------------------------------------------------------------------------
BOX_SIZES = [1, 63, 64, 65, 256, 257, 65536, 65537, 200000]      # <= 256 blocks: 65,537 is the first strided size
BOX_POPS = ["normal", "negative", "signed_zeros", "denormal", "huge"]


def box_population(name, n):
    def make():
        rng = np.random.default_rng(300 + n + sum(map(ord, name)))
        if name == "normal":
            p = (rng.normal(size=(n, 3)) * 10).astype(F)
        elif name == "negative":
            p = -rng.uniform(1.0, 100.0, (n, 3)).astype(F)
        elif name == "signed_zeros":                              # both signs, and +0 and -0 among them
            p = (rng.normal(size=(n, 3)) * 5).astype(F)
            p[rng.random((n, 3)) < 0.25] = F(0.0)
            p[rng.random((n, 3)) < 0.25] = F(-0.0)
        elif name == "denormal":
            p = (rng.integers(1, 1 << 23, (n, 3)).astype(np.uint32) | (rng.integers(0, 2, (n, 3)).astype(np.uint32) << 31)).view(F)
        else:
            p = (rng.uniform(-1.0, 1.0, (n, 3)) * 3e38).astype(F)
        if n >= 2:   # the extremes of x and y: the first body and the last (the last lane of a partial wave); of z: the last
            #          lane of the last full wave and a body in the middle
            where = [(0, n - 1), (n - 1, 0), (n // 64 * 64 - 1, n // 2) if n >= 128 else (n - 1, 0)]
            for a, (i_lo, i_hi) in enumerate(where):
                lo_v, hi_v = np.nextafter(p[:, a].min(), F(-np.inf)), np.nextafter(p[:, a].max(), F(np.inf))
                if name == "huge":
                    lo_v, hi_v = F(-3e38), F(3e38)
                    p[:, a] = np.clip(p[:, a], F(-2.9e38), F(2.9e38))
                p[i_lo, a], p[i_hi, a] = lo_v, hi_v
        posm = np.empty((n, 4), F)
        posm[:, :3], posm[:, 3] = p, rng.uniform(-1e30, 1e30, n)     # (the mass lane must not enter the box)
        return posm
    return memo(("box", name, n), make)


@pytest.mark.parametrize("name", BOX_POPS)
@pytest.mark.parametrize("n", BOX_SIZES)
def test_bbox_packed(nb, ctx, n, name):
    posm = box_population(name, n)
    want = np.concatenate([posm[:, :3].min(0), posm[:, :3].max(0)])
    if name == "negative":
        assert np.all(want < 0)
    if name == "denormal":
        assert np.all(np.abs(want) < F(1.2e-38)) and np.all(want != 0)
    if name == "huge" and n >= 2:
        assert bits(want).tolist() == bits(np.array([-3e38] * 3 + [3e38] * 3, F)).tolist()
    assert not np.any(want == 0) or n == 1       # (which of +0 and -0 is the smaller is not pinned: no extreme is a zero)
    same(bits(device_box(nb, ctx, dev(posm), n)), bits(want), f"nbody_hip_bbox_packed [{name}], n={n}")


def motion(n_max=200000):
    """positions, velocities, accelerations shared by the drift and kick cases: a size takes the first n bodies"""
    def make():
        rng = np.random.default_rng(400)
        p = (rng.normal(size=(n_max, 4)) * 5).astype(F)
        return p, rng.normal(size=(n_max, 4)).astype(F), rng.normal(size=(n_max, 4)).astype(F)
    return memo(("motion",), make)


DT = F(0.01)
EMPTY_BOX = np.array([0xFFFFFFFF] * 3 + [0] * 3, np.uint32)


@pytest.mark.parametrize("n", BOX_SIZES)
def test_drift_bbox_packed(nb, ctx, n):
    lib = nb._lib.load()
    p, v, a = (x[:n] for x in motion())
    d_v, d_a = dev(v), dev(a)
    plain = dev(p)
    nb._lib.check(lib.nbody_hip_drift_packed(ctx.handle, plain.data_ptr(), d_v.data_ptr(), d_a.data_ptr(), n, float(DT)))
    plain = plain.cpu().numpy()
    want = memo(("drift",), lambda: ref.drift(motion()[0][:, :3], motion()[1][:, :3], motion()[2][:, :3], DT))
    same(bits(plain[:, :3]), bits(want[:n]), f"nbody_hip_drift_packed against ref.drift (every body), n={n}")
    same(bits(plain[:, 3]), bits(p[:, 3]), f"nbody_hip_drift_packed: the mass lane, n={n}")
    fused, enc, out = dev(p), dev(EMPTY_BOX.view(np.int32)), prefilled((6 + GUARD,), GARBAGE)
    nb._lib.check(lib.nbody_hip_drift_bbox_packed(ctx.handle, fused.data_ptr(), d_v.data_ptr(), d_a.data_ptr(), n, float(DT),
                                                  enc.data_ptr(), out.data_ptr()))
    fused, box = fused.cpu().numpy(), out.cpu().numpy()
    same(bits(fused), bits(plain), f"nbody_hip_drift_bbox_packed against nbody_hip_drift_packed (mass lane included), n={n}")
    same(bits(box[:6]), bits(np.concatenate([plain[:, :3].min(0), plain[:, :3].max(0)])), f"the box of the NEW positions, n={n}")
    all_equal(box[6:], GARBAGE, "the words behind the box")
    same(bits(enc), EMPTY_BOX, f"enc re-armed after the call, n={n}")
    # a second call on the same enc, on bodies strictly inside the first box (at rest): the smaller box, not the union
    inner = plain.copy()
    inner[:, :3] *= F(0.5)
    zero = torch.zeros((n, 4), dtype=torch.float32, device="cuda")
    again, out2 = dev(inner), prefilled((6,), GARBAGE)
    nb._lib.check(lib.nbody_hip_drift_bbox_packed(ctx.handle, again.data_ptr(), zero.data_ptr(), zero.data_ptr(), n, float(DT),
                                                  enc.data_ptr(), out2.data_ptr()))
    want2 = np.concatenate([inner[:, :3].min(0), inner[:, :3].max(0)])
    same(bits(out2), bits(want2), f"the box of the second call on the same enc, n={n}")
    assert np.all(np.abs(want2) < np.abs(box[:6].view(F))) and not np.any(want2 == 0)
    same(bits(enc), EMPTY_BOX, f"enc re-armed after the second call, n={n}")


@pytest.mark.parametrize("n", [1, 257, 65537])
def test_kick_packed(nb, ctx, n):
    v, a_old, a_new = (x[:n] for x in motion())
    d_v, d_old, d_new = dev(v), dev(a_old), dev(a_new)
    nb._lib.check(nb._lib.load().nbody_hip_kick_packed(ctx.handle, d_v.data_ptr(), d_old.data_ptr(), d_new.data_ptr(), n,
                                                       float(DT)))
    got = d_v.cpu().numpy()
    want = memo(("kick",), lambda: ref.kick(motion()[0][:, :3], motion()[1][:, :3], motion()[2][:, :3], DT))
    same(bits(got[:, :3]), bits(want[:n]), f"nbody_hip_kick_packed against ref.kick (every body), n={n}")
    same(bits(got[:, 3]), bits(v[:, 3]), f"nbody_hip_kick_packed: the w lane, n={n}")

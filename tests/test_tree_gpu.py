"""The Barnes-Hut tree build (csrc/barnes_hut.hip: tree_flags_kernel, level_scan_kernel, tree_span_kernel, both
tree_fill_kernel forms, the double-double prefix monopoles, the bottom-up monopole and quadrupole passes, mark_hole)
against tests/tree_ref.py, NODE BY NODE, at the shapes where each of its edges binds.  The force tolerances of the other
Barnes-Hut tests cannot see a build that is subtly wrong (it mostly yields a valid coarser or finer tree); here the
permutation, every node record, the level bases of both numberings and the monopoles / second moments are held to an
independent statement of which nodes must exist.  DESIGN.md ("Testing the tree build") says which case is there for
which edge.  Trees cut by limitNodes are out of scope: the reference does not model the cut."""
import functools

import numpy as np
import pytest

import sort_ref as sr
import tree_ref as tr
from gpu_util import acc_of, packed, rel_err, to_device

pytestmark = pytest.mark.gpu
F = np.float32
TOL = 1e-5          # test_theta_zero_equals_direct / test_pair_walk_equals_plain_walk: per-body relative error
PREFIX_MAX = 1572864
PAIR_FROM = 98304


# ---- body sets -----------------------------------------------------------------------------------------------------------
def with_masses(ic, seed=1):
    ic = dict(ic)
    ic["mass"] = np.random.default_rng(seed).uniform(0.5, 2.0, ic["pos_x"].size).astype(F)
    return ic


def from_points(p, seed=1):
    p = np.asarray(p, np.float64).reshape(-1, 3)
    ic = {"pos_x": np.ascontiguousarray(p[:, 0], F), "pos_y": np.ascontiguousarray(p[:, 1], F),
          "pos_z": np.ascontiguousarray(p[:, 2], F)}
    for k in ("vel_x", "vel_y", "vel_z"):
        ic[k] = np.zeros(len(p), F)
    return with_masses(ic, seed)


@functools.lru_cache(maxsize=None)
def cube(n=70000, seed=3):
    """bodies uniform in [-1, 1]^3 with unequal masses; cube_first(n) = its first n"""
    return from_points(np.random.default_rng(seed).uniform(-1.0, 1.0, (n, 3)), seed)


def cube_first(n):
    return sr.take(cube(), np.arange(n))


def populated(counts, depth, seed=2):
    """counts[c] bodies in cell c (Morton index: level-1 octant in the top three bits, x = bit 2, y = bit 1, z = bit 0 of
    each octant) of the 2^depth lattice over [-1, 1]^3, jittered inside the middle 80 % of the cell; two of the bodies
    sit at the corners (-1, -1, -1) and (1, 1, 1) and pin the root cube (cells 0 and 8^depth - 1 must be occupied)"""
    rng = np.random.default_rng(seed)
    side = 1 << depth
    pts = []
    for c, k in enumerate(counts):
        q = [0, 0, 0]
        for lvl in range(depth):
            o = (c >> (3 * (depth - 1 - lvl))) & 7
            for a in range(3):
                q[a] = 2 * q[a] + ((o >> (2 - a)) & 1)
        u = rng.uniform(0.1, 0.9, (k, 3))
        pts.append((np.asarray(q) + u) / side * 2.0 - 1.0)
    assert counts[0] > 0 and counts[-1] > 0 and len(counts) == 8 ** depth
    pts[0][0] = (-1.0, -1.0, -1.0)
    pts[-1][-1] = (1.0, 1.0, 1.0)
    p = np.concatenate(pts)
    return from_points(p[rng.permutation(len(p))], seed)


def lattice(side, extra=()):
    g = (np.arange(side) + 0.5) / side * 2.0 - 1.0
    x, y, z = (v.ravel() for v in np.meshgrid(g, g, g, indexing="ij"))
    pts = np.stack([x, y, z], 1)
    if len(extra):
        pts = np.concatenate([pts, np.asarray(extra, np.float64).reshape(-1, 3)])
    return from_points(pts)


_refs = {}


def reference(oracle, key, ic, max_depth, leaf_max):
    """one RefTree per (body set, shape), shared by the tests that build it (never modified)"""
    k = (key, max_depth, leaf_max)
    if k not in _refs:
        _refs[k] = tr.RefTree(oracle, ic, max_depth, leaf_max)
    return _refs[k]


# ---- one build against the reference -------------------------------------------------------------------------------------
def make_tree(nb, capacity, max_depth=20, leaf_max=1, aligned=False, order=1):
    tree = nb.BarnesHutTree(capacity)
    if (max_depth, leaf_max) != (20, 1):
        tree.setParams(max_depth, leaf_max)
    if order != 1:
        tree.setMultipoleOrder(order)
    tree.walkForm(2 if aligned else 0)   # BEFORE the build: below 98,304 bodies the even-aligned ids exist only on request
    return tree


def check_build(nb, tree, ref, aligned, tag, order=1):
    """everything this file asserts of one build; returns the exported nodes"""
    n = ref.n
    sr_order = sr.tree_order(nb, tree, n)
    assert np.array_equal(sr_order, ref.order), \
        f"{tag}: the device permutation differs from the stable argsort at {np.flatnonzero(sr_order != ref.order)[:8]}"
    # which numbering ran -- first, so that a silent fall back to the other form fails here
    ran_aligned, id_base = tree.idLayout()
    assert id_base[1] == (2 if aligned else 1) and ran_aligned == aligned, \
        f"{tag}: built with {'aligned' if ran_aligned else 'plain'} ids (level_base[1] = {id_base[1]})"
    assert id_base == ref.level_base(aligned), f"{tag}: id bases {id_base} against {ref.level_base(aligned)}"
    st = tree.stats()
    assert st["level_base"] == ref.level_base_plain, f"{tag}: level_base {st['level_base']} against {ref.level_base_plain}"
    assert st["node_count"] == ref.node_count
    nodes = tree.copyNodesToHost()
    assert np.array_equal(tree.sorted_indices_, ref.order)
    tr.check_nodes(ref, nodes, bottom_up=n > PREFIX_MAX, tag=tag)
    if order == 2:
        tr.check_moments(ref, tree.copyMomentsToHost(), tag=tag)
    return nodes


def build_and_check(nb, oracle, key, ic, max_depth=20, leaf_max=1, aligned=False, order=1, tree=None):
    ref = reference(oracle, key, ic, max_depth, leaf_max)
    d, _ = to_device(nb, ic)
    own = tree is None
    if own:
        tree = make_tree(nb, ref.n, max_depth, leaf_max, aligned, order)
    tree.build(d)
    tag = f"{key}: n = {ref.n}, depth {max_depth}, leaf_max {leaf_max}, {'aligned' if aligned else 'plain'} ids, order {order}"
    nodes = check_build(nb, tree, ref, aligned, tag, order)
    if own:
        tree.close()
    return ref, nodes


# ---- a. sizes ------------------------------------------------------------------------------------------------------------
# word boundaries of the rank tables (64), workgroups of the flag / fill kernels (256), of the prefix sums (1024), the
# chunks of level_scan_kernel (G words over 16 waves, rounded up to 64: 65,536 bodies = 1,025 words = two chunks), the
# marker one past the last body (position n: a word of its own when 64 | n) and the flags kernel's n + 1 positions
SIZES = [1, 2, 3, 8, 9, 63, 64, 65, 127, 128, 255, 256, 257, 1023, 1024, 1025, 2048, 4095, 4096, 4097, 65535, 65536, 65537]


@pytest.mark.parametrize("aligned", [False, True], ids=["plain", "aligned"])
@pytest.mark.parametrize("n", SIZES)
def test_sizes_on_a_tree_of_exactly_n(nb, oracle, ctx, n, aligned):
    build_and_check(nb, oracle, ("cube", n), cube_first(n), aligned=aligned)


@pytest.mark.parametrize("aligned", [False, True], ids=["plain", "aligned"])
def test_sizes_on_one_reused_tree(nb, oracle, ctx, aligned):
    """the tables are laid out for each build's own n inside arrays sized for 70,000: descending, then ascending"""
    tree = make_tree(nb, 70000, aligned=aligned)
    for n in SIZES[::-1] + SIZES[1:]:
        build_and_check(nb, oracle, ("cube", n), cube_first(n), aligned=aligned, tree=tree)
    tree.close()


# ---- b. depth and key width ----------------------------------------------------------------------------------------------
# the bottom-up quadrupole passes put levels 0..4 into one workgroup (both sides of 4); 32-bit keys up to depth 10,
# 63-bit keys above, of which only the top 3 max_depth bits are sorted
@pytest.mark.parametrize("order,aligned", [(1, False), (1, True), (2, False)], ids=["order1-plain", "order1-aligned", "order2"])
@pytest.mark.parametrize("max_depth", [1, 2, 3, 4, 5, 6, 10, 11, 20, 21])
def test_depths(nb, oracle, ctx, max_depth, order, aligned):
    build_and_check(nb, oracle, ("cube", 5000), cube_first(5000), max_depth=max_depth, aligned=aligned, order=order)


# ---- c. leaf_max ---------------------------------------------------------------------------------------------------------
# side_extent is capped by i, by n - 1 - i and by leaf_max: all three bind when n is leaf_max - 1, leaf_max, leaf_max + 1
@pytest.mark.parametrize("aligned", [False, True], ids=["plain", "aligned"])
@pytest.mark.parametrize("leaf_max,n", [(lm, n) for lm in (1, 2, 3, 8, 64, 1024) for n in (lm - 1, lm, lm + 1, 3000) if n >= 1])
def test_leaf_max(nb, oracle, ctx, leaf_max, n, aligned):
    ic = cube_first(n)
    ref, nodes = build_and_check(nb, oracle, ("cube", n), ic, leaf_max=leaf_max, aligned=aligned)
    if n <= leaf_max:   # the root is the only node and a leaf
        assert len(nodes) == 1 and nodes[0]["is_leaf"] and nodes[0]["particle_count"] == n
    if n <= leaf_max and not aligned:   # ... and its walk is the direct sum (test_theta_zero_equals_direct's criterion)
        d, _ = to_device(nb, ic)
        tree = make_tree(nb, n, 20, leaf_max)
        tree.build(d)
        tree.computeForces(d, 0.5, 1.0, 0.01)
        a = acc_of(d)
        direct = nb.DirectForceCalculator()
        direct.setGravitationalConstant(1.0)
        direct.setSofteningParameter(0.01)
        direct.computeForces(d)
        assert rel_err(a, acc_of(d)).max() < TOL
        tree.close()


# ---- d. controlled populations -------------------------------------------------------------------------------------------
# node ends at 64 k - 1, 64 k, 64 k + 1 and at n, n a multiple of 64 / 256 / 1024; leaves of 255, 256, 257, 320 and 500
# bodies: both sides of tree_span_kernel's four-word window (a node that starts at bit 0 of a word sees 256 positions)
# and its gallop, which starts at word g0 + 4
def spread(counts, cells, total):
    out = [0] * total
    for c, k in zip(cells, counts):
        out[c] = k
    return out


CELLS2 = [0, 1, 2, 3, 8, 9, 17, 18, 27, 36, 45, 54, 63]
HEAD2 = [63, 1, 1, 63, 1, 127, 255, 1, 256, 257, 320, 500]      # ends 63 64 65 128 129 256 511 512 768 1025 1345 1845
POPULATIONS = {
    "depth2-n2048": (2, spread(HEAD2 + [203], CELLS2, 64)),       # n = 2 x 1024
    "depth2-n2112": (2, spread(HEAD2 + [267], CELLS2, 64)),       # n = 33 x 64
    "depth2-n2304": (2, spread(HEAD2 + [459], CELLS2, 64)),       # n = 9 x 256
    "depth2-n2047": (2, spread(HEAD2 + [202], CELLS2, 64)),       # n = 64 k - 1
    "depth2-n2049": (2, spread(HEAD2 + [204], CELLS2, 64)),       # n = 64 k + 1
    "depth1-n2048": (1, [255, 256, 257, 320, 500, 1, 63, 396]),   # the same leaves directly under the root
    "depth1-n1024": (1, [256, 0, 320, 0, 191, 0, 0, 257]),        # empty octants between them
}


@pytest.mark.parametrize("aligned", [False, True], ids=["plain", "aligned"])
@pytest.mark.parametrize("name", sorted(POPULATIONS))
def test_controlled_populations(nb, oracle, ctx, name, aligned):
    depth, counts = POPULATIONS[name]
    ic = populated(counts, depth)
    ref, _ = build_and_check(nb, oracle, name, ic, max_depth=depth, aligned=aligned)
    # the generator did what it says: the deepest level's nodes hold exactly the chosen counts
    assert ref.count[ref.level == depth].tolist() == [k for k in counts if k]
    assert ref.n == sum(counts)


# ---- e. degenerate geometry ----------------------------------------------------------------------------------------------
def degenerate(name):
    rng = np.random.default_rng(17)
    if name in ("coincident300", "coincident1000"):     # one chain to max_depth and one big leaf
        return from_points(np.tile([[0.3, -0.2, 0.7]], (int(name[10:]), 1)))
    if name == "two-corner-clusters":                   # the smallest and the largest keys of the cube, nothing between
        return from_points(np.concatenate([np.tile([[-1.0, -1.0, -1.0]], (150, 1)), np.tile([[1.0, 1.0, 1.0]], (170, 1))]))
    if name == "line":                                  # along x: two of the three key bits of every level are constant
        p = np.zeros((700, 3))
        p[:, 0] = rng.uniform(-1.0, 1.0, 700)
        return from_points(p)
    if name == "close-pair":                            # 1e-6 apart in a cloud of 2000: a one-child chain of ~15 levels
        p = rng.uniform(-1.0, 1.0, (2000, 3))
        p[1] = p[0] + (1e-6, 0.0, 0.0)
        return from_points(p)
    if name == "corners":
        return from_points([[sx, sy, sz] for sx in (-1, 1) for sy in (-1, 1) for sz in (-1, 1)])
    if name == "lattice":
        return lattice(16)
    if name == "lattice-plus-one":
        return lattice(16, extra=[(0.078125, 0.078125, 0.078125)])
    raise KeyError(name)


@pytest.mark.parametrize("aligned", [False, True], ids=["plain", "aligned"])
@pytest.mark.parametrize("name", ["coincident300", "coincident1000", "two-corner-clusters", "line", "close-pair", "corners",
                                  "lattice", "lattice-plus-one"])
def test_degenerate_geometry(nb, oracle, ctx, name, aligned):
    ref, _ = build_and_check(nb, oracle, name, degenerate(name), aligned=aligned)
    if name.startswith("coincident"):
        assert ref.level_counts == [1] * 21 and ref.count[-1] == ref.n
    if name == "close-pair":
        assert sum(ref.odd_groups) >= 10   # a hole at (nearly) every level of the chain


# ---- f. massless bodies --------------------------------------------------------------------------------------------------
def massless(name):
    rng = np.random.default_rng(23)
    if name == "every-second":
        ic = cube_first(3000)
        ic["mass"] = ic["mass"].copy()
        ic["mass"][::2] = 0.0
        return ic
    p = rng.uniform(-1.0, 1.0, (1500, 3))
    ic = from_points(p)
    if name == "massless-deepest-leaf":      # two coincident massless bodies: a leaf of two at max_depth, mass 0
        ic["pos_x"][11], ic["pos_y"][11], ic["pos_z"][11] = ic["pos_x"][10], ic["pos_y"][10], ic["pos_z"][10]
        ic["mass"][10:12] = 0.0
    elif name == "massless-octant":          # an internal node of mass 0 with massless children below it
        ic["mass"][(p > -0.01).all(1)] = 0.0   # (the root's centre is within 1e-3 of 0: all of octant 7)
    return ic


@pytest.mark.parametrize("order,aligned", [(1, False), (1, True), (2, False)], ids=["order1-plain", "order1-aligned", "order2"])
@pytest.mark.parametrize("name", ["every-second", "massless-deepest-leaf", "massless-octant"])
def test_massless_bodies(nb, oracle, ctx, name, order, aligned):
    ref, nodes = build_and_check(nb, oracle, name, massless(name), aligned=aligned, order=order)
    zero = ref.total_mass == 0
    assert zero.any() and np.all(nodes["total_mass"][zero] == 0) and np.all(nodes["center_of_mass"][zero] == 0)
    if name == "massless-deepest-leaf":
        assert (zero & (ref.count == 2) & (ref.level == 20)).any()
    if name == "massless-octant":
        assert (zero & ~ref.is_leaf).any()


# ---- g. reuse ------------------------------------------------------------------------------------------------------------
def forces(tree, d, form=None):
    if form is not None:
        tree.walkForm(form)
    tree.computeForces(d, 0.5, 1.0, 0.01)
    return acc_of(d)


def test_reuse_one_tree_through_shapes_and_numberings(nb, oracle, ctx):
    """stale planes, holes and pair blocks of an earlier (larger, deeper, aligned) build must not show in a later one"""
    steps = [  # (key, bodies, set_params, walk form set before the build, aligned)
        (("cube", 65537), cube_first(65537), None, 2, True),
        ("coincident300", degenerate("coincident300"), None, None, True),
        (("cube", 4097), cube_first(4097), (10, 4), None, True),
        (("cube", 65536), cube_first(65536), (21, 1), None, True),
        (("cube", 1025), cube_first(1025), None, 1, False),
    ]
    tree = nb.BarnesHutTree(65537)
    params, form = (20, 1), 0
    for key, ic, set_params, set_form, aligned in steps:
        if set_params:
            tree.setParams(*set_params)
            params = set_params
        if set_form is not None:
            tree.walkForm(set_form)
            form = set_form
        ref = reference(oracle, key, ic, *params)
        tag = f"reused tree, {key}: depth {params[0]}, leaf_max {params[1]}, walk form {form}"
        d, _ = to_device(nb, ic)
        tree.build(d)
        nodes = check_build(nb, tree, ref, aligned, tag)
        layout, level_base = tree.idLayout(), tree.stats()["level_base"]
        a = forces(tree, d)
        fresh = nb.BarnesHutTree(ref.n)
        fresh.setParams(*params)
        fresh.walkForm(form)
        fresh.build(d)
        fresh_nodes = fresh.copyNodesToHost()
        assert nodes.tobytes() == fresh_nodes.tobytes(), f"{tag}: nodes differ from a fresh tree's"
        assert fresh.idLayout() == layout and fresh.stats()["level_base"] == level_base, tag
        assert np.array_equal(forces(fresh, d), a), f"{tag}: forces differ from a fresh tree's"
        fresh.close()
        if aligned:   # the pair walk (cost-ordered and in plain order) against the plain walk over the same tree
            plain = forces(tree, d, 1)
            for f in (2, 3):
                assert rel_err(forces(tree, d, f), plain).max() < TOL, f"{tag}: walk form {f}"
            tree.walkForm(form)
    tree.close()


# ---- h. path thresholds, at their own sizes ------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def plummer():
    import nbody_amd as nb
    n = PREFIX_MAX + 1
    ic = with_masses(nb.ic.plummer(n, seed=11), seed=11)
    # the last body (the one the two largest builds differ by) sits inside the others' bounding box: both builds share
    # their root cube, and with it every key of the bodies they share
    r2 = ic["pos_x"].astype(np.float64) ** 2 + ic["pos_y"].astype(np.float64) ** 2 + ic["pos_z"].astype(np.float64) ** 2
    inner = int(np.argmin(r2[: PAIR_FROM - 1]))
    for k in ic:
        ic[k] = ic[k].copy()
        ic[k][[inner, n - 1]] = ic[k][[n - 1, inner]]
    return ic


@pytest.mark.parametrize("n,order,aligned", [(PAIR_FROM - 1, 1, False), (PAIR_FROM, 1, True), (PAIR_FROM, 2, True)])
def test_automatic_switch_to_aligned_ids(nb, oracle, ctx, n, order, aligned):
    ic = sr.take(plummer(), np.arange(n))
    ref = reference(oracle, ("plummer", n), ic, 20, 1)
    d, _ = to_device(nb, ic)
    tree = nb.BarnesHutTree(n)      # walk form automatic: the numbering is the build's own choice
    if order == 2:
        tree.setMultipoleOrder(2)
    tree.build(d)
    check_build(nb, tree, ref, aligned, f"plummer n = {n}, order {order}, automatic numbering", order)
    tree.close()


_big = {}


@pytest.mark.parametrize("n", [PREFIX_MAX, PREFIX_MAX + 1])
def test_last_prefix_build_and_first_bottom_up_build(nb, oracle, ctx, n):
    ic = sr.take(plummer(), np.arange(n))
    ref = tr.RefTree(oracle, ic, 20, 1)     # (not kept in the shared cache: two of these are half a gigabyte)
    d, _ = to_device(nb, ic)
    tree = nb.BarnesHutTree(n)
    tree.build(d)
    nodes = check_build(nb, tree, ref, True, f"plummer n = {n} ({'bottom-up' if n > PREFIX_MAX else 'prefix'} monopoles)")
    tree.close()
    _big[n] = (ref, nodes)
    if len(_big) < 2:
        return
    # the two builds differ by one body: at every level, the nodes that lie wholly before it in the Morton order hold
    # the same bodies in both trees and must agree -- in the reference exactly, in the builds in every integer field
    # (child links relative to their level) and, between the two monopole paths, within the bounds each was held to
    (ra, na), (rb, nb_) = _big[PREFIX_MAX], _big[PREFIX_MAX + 1]
    _big.clear()
    assert ra.root_half == rb.root_half and ra.root_center == rb.root_center
    where = int(np.flatnonzero(rb.order == PREFIX_MAX)[0])      # the extra body's sorted position
    assert np.array_equal(ra.order[:where], rb.order[:where])
    shared = 0
    for L in range(21):
        a0, b0 = ra.level_base_plain[L], rb.level_base_plain[L]
        k = int(np.searchsorted(rb.last[b0:rb.level_base_plain[L + 1]], where, "right"))   # nodes with last <= where
        sa, sb = slice(a0, a0 + k), slice(b0, b0 + k)
        assert np.array_equal(ra.first[sa], rb.first[sb]) and np.array_equal(ra.last[sa], rb.last[sb]), f"level {L}"
        assert np.array_equal(ra.total_mass[sa], rb.total_mass[sb]) and np.array_equal(ra.center_of_mass[sa], rb.center_of_mass[sb])
        for name in ("particle_count", "is_leaf", "particle_index", "half_size", "center"):
            assert np.array_equal(na[name][sa], nb_[name][sb]), f"level {L}: {name}"
        ca, cb = na["children"][sa].astype(np.int64), nb_["children"][sb].astype(np.int64)
        assert np.array_equal(ca < 0, cb < 0), f"level {L}: child slots"
        assert np.array_equal(np.where(ca < 0, -1, ca - ra.level_base_plain[L + 1]),
                              np.where(cb < 0, -1, cb - rb.level_base_plain[L + 1])), f"level {L}: child links"
        shared += k
    print(f"{shared} nodes lie before the extra body (sorted position {where}) and agree between the two builds")
    assert shared > 0


# ---- entry points --------------------------------------------------------------------------------------------------------
def test_entry_points_build_the_same_tree(nb, oracle, ctx):
    n = 4097
    ic = cube_first(n)
    ref = reference(oracle, ("cube", n), ic, 20, 1)
    d, _ = to_device(nb, ic)
    tree = nb.BarnesHutTree(n)
    tree.build(d)
    want = check_build(nb, tree, ref, False, "build").tobytes()
    tree.driftBuild(d, 0.0)            # x += v 0 + a 0: the same bodies through the fused drift + pack pass
    assert check_build(nb, tree, ref, False, "driftBuild(dt = 0)").tobytes() == want
    posm = packed(ic)
    nb._lib.check(nb._lib.load().nbody_hip_tree_build_packed(tree._h, posm.data_ptr(), n))
    assert check_build(nb, tree, ref, False, "nbody_hip_tree_build_packed").tobytes() == want
    tree.close()

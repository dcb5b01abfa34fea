"""Density-peak (HOP) groups (nbody_hip_hop_groups, include/nbody_hip_hop.h) on a real GPU.  Every comparison is
np.array_equal on labels, peak, offsets, members, group_peak and the five counts against the numpy restatement of
tests/hop_ref.py.  The lists are handed in directly, so the shapes are chosen for the kernels' edges and not by geometry:
the block and wave edges of the body kernels, chains across blocks for the pointer jumping, unread slots, the bad index,
zero records, record counts around the tile edges of the sort and the fold, the hand cases of the CPU file, a random graph
that regroups in every way, the same input permuted, determinism, the refusals; then end to end on two Plummer spheres
through ParticleSystem.hopGroups for the three force methods and SpatialHashGrid.hopGroups."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import hop_ref as ref

pytestmark = pytest.mark.gpu


def _call(nb, ctx, index, rho, n_hop, n_merge, delta_outer, delta_saddle=None, delta_peak=None, min_members=1):
    """one hop_groups call -> (the outputs as numpy arrays keyed like the reference's, the HopCatalogue)"""
    idx = torch.from_numpy(np.ascontiguousarray(index, np.int32)).cuda()
    r = torch.from_numpy(np.ascontiguousarray(rho, np.float64)).cuda()
    cat = nb.hop_groups(ctx, idx, r, n_hop, n_merge, delta_outer, delta_saddle, delta_peak, min_members)
    return _host(cat), cat


def _host(cat):
    return dict(labels=cat.labels.cpu().numpy(), peak=cat.peak.cpu().numpy(), offsets=cat.offsets.cpu().numpy(),
                members=cat.members.cpu().numpy(), group_peak=cat.group_peak.cpu().numpy(),
                counts=np.array([cat.n_groups, cat.n_members, cat.n_peaks, cat.rounds, cat.status], np.int64))


def _same(got, want, what=""):
    for key in ref.OUTPUTS:
        g, w = np.asarray(got[key]), np.asarray(want[key])
        assert g.shape == w.shape and np.array_equal(g, w), (what, key, g[:12], w[:12])
        if key != "counts":
            assert g.dtype == np.int32, (what, key, g.dtype)


def _check(nb, ctx, what="", **args):
    want = ref.reference(**args)
    got, cat = _call(nb, ctx, **args)
    _same(got, want, what)
    return got, want, cat


# ---- 1. the edges of the body kernels --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("count", [1, 2, 255, 256, 257, 1025])
def test_counts_at_the_block_edges(nb, ctx, count):
    for gen, seed in ((ref.random_graph, 11), (ref.local_graph, 12)):
        index, rho = gen(count, 3, 5, seed + count)
        _, want, _ = _check(nb, ctx, (count, gen.__name__), index=index, rho=rho, n_hop=3, n_merge=2, delta_outer=2.0,
                            delta_saddle=3.0, delta_peak=4.0)
        assert want["counts"][2] >= 1


def test_line_graph_with_rising_density_is_one_chain_across_blocks(nb, ctx):
    n = 5000
    got, _, _ = _check(nb, ctx, "rising", index=ref.line_graph(n), rho=np.arange(n, dtype=np.float64) + 1.0, n_hop=2, n_merge=2,
                       delta_outer=0.0, delta_saddle=0.0, delta_peak=0.0)
    assert (got["peak"] == n - 1).all() and got["counts"].tolist() == [1, n, 1, 1, 0]
    # ... and falling: the chain runs the other way, against the order of the blocks
    got, _, _ = _check(nb, ctx, "falling", index=ref.line_graph(n), rho=np.arange(n, 0, -1).astype(np.float64), n_hop=2, n_merge=2,
                       delta_outer=0.0, delta_saddle=0.0, delta_peak=0.0)
    assert (got["peak"] == 0).all()


def test_line_graph_with_equal_density_ends_at_body_zero(nb, ctx):
    n = 5000
    got, _, _ = _check(nb, ctx, "flat", index=ref.line_graph(n), rho=np.full(n, 2.5), n_hop=2, n_merge=2, delta_outer=1.0,
                       delta_saddle=2.0, delta_peak=2.5)
    assert (got["peak"] == 0).all() and (got["labels"] == 0).all() and got["group_peak"].tolist() == [0]


@pytest.mark.parametrize("k,n_hop,n_merge", [(1, 1, 0), (1, 1, 1), (7, 3, 5), (7, 6, 2), (32, 5, 3), (32, 32, 32)])
def test_k_and_the_slots_that_are_read(nb, ctx, k, n_hop, n_merge):
    n = 700
    index, rho = ref.local_graph(n, k, 6, 40 + k)
    read = max(n_hop, n_merge)
    index[:, read:] = n + np.arange(k - read, dtype=np.int32)  # unread slots: indices at and past count
    got, want, _ = _check(nb, ctx, (k, n_hop, n_merge), index=index, rho=rho, n_hop=n_hop, n_merge=n_merge, delta_outer=2.0,
                          delta_saddle=3.0, delta_peak=5.0)
    assert want["counts"][4] == 0 and want["counts"][0] >= 1
    # the same graph with the unread slots empty: the same answer
    clean = index.copy()
    clean[:, read:] = -1
    _same(ref.reference(clean, rho, n_hop, n_merge, 2.0, 3.0, 5.0), want)


@pytest.mark.parametrize("slot,value", [(0, 700), (2, 700), (4, 2 ** 31 - 1), (1, 701)])
def test_a_bad_index_in_a_read_slot(nb, ctx, slot, value):
    n = 700
    index, rho = ref.local_graph(n, 7, 6, 47)
    index[:, 5:] = n  # (unread: n_hop = 3, n_merge = 5)
    index[n - 1 if slot else 0, slot] = value
    got, want, cat = _check(nb, ctx, (slot, value), index=index, rho=rho, n_hop=3, n_merge=5, delta_outer=2.0, delta_saddle=3.0,
                            delta_peak=5.0)
    assert got["counts"].tolist() == [0, 0, 0, 0, 1] and (got["labels"] == -1).all() and (got["peak"] == -1).all()
    assert got["offsets"].tolist() == [0] and cat.status == 1


def test_n_merge_zero_and_zero_records_with_many_peaks(nb, ctx):
    n = 3000
    index, rho = ref.random_graph(n, 4, 9, 5)
    got, want, _ = _check(nb, ctx, "n_merge 0", index=index, rho=rho, n_hop=1, n_merge=0, delta_outer=3.0, delta_saddle=4.0,
                          delta_peak=6.0)
    assert want["n_records"] == 0 and want["counts"][2] > 500 and want["rounds"] == 1 and want["dropped"].size > 10
    # nobody names anybody: every body its own peak, the viable ones singletons, the others dropped
    alone = np.full((n, 4), -1, np.int32)
    got, want, _ = _check(nb, ctx, "alone", index=alone, rho=rho, n_hop=4, n_merge=4, delta_outer=3.0, delta_saddle=4.0, delta_peak=6.0)
    assert want["n_records"] == 0 and got["counts"][2] == n and got["counts"][0] == (rho >= 6.0).sum()
    # min_members above every group: an empty catalogue of live, labelled bodies
    got, _, _ = _check(nb, ctx, "min_members", index=alone, rho=rho, n_hop=4, n_merge=4, delta_outer=3.0, delta_saddle=4.0,
                       delta_peak=6.0, min_members=2)
    assert got["counts"][:2].tolist() == [0, 0] and got["offsets"].tolist() == [0] and (got["labels"] >= 0).any()


def test_every_body_dead(nb, ctx):
    index, rho = ref.random_graph(1000, 4, 9, 6)
    got, _, _ = _check(nb, ctx, "dead", index=index, rho=rho, n_hop=4, n_merge=4, delta_outer=100.0, delta_saddle=100.0,
                       delta_peak=100.0)
    assert got["counts"][:2].tolist() == [0, 0] and got["offsets"].tolist() == [0] and (got["labels"] == -1).all()
    assert got["counts"][2] >= 1 and got["counts"][3] == 1 and (got["peak"] >= 0).all()
    rho[::3] = np.nan  # and NaN densities among them
    _check(nb, ctx, "dead and NaN", index=index, rho=rho, n_hop=4, n_merge=4, delta_outer=100.0, delta_saddle=100.0, delta_peak=100.0)


def _ring(n, listing, seed):
    """n bodies, each its own peak (slot 0, the only one the hop reads, is empty); the first `listing` bodies name their
    successor in slot 1: exactly 2 * listing directed records, and a chain of edges for the regrouping to walk"""
    index = np.full((n, 2), -1, np.int32)
    index[:listing, 1] = (np.arange(listing) + 1) % n
    rho = (1.0 + np.random.default_rng(seed).integers(0, 12, size=n)).astype(np.float64)
    return index, rho


@pytest.mark.parametrize("records", [2, 254, 256, 258, 1022, 1024, 1026, 2046, 2048, 2050, 3838, 3840, 3842, 4094, 4096, 4098,
                                     8190, 8192, 8194])
def test_record_counts_around_the_tile_edges(nb, ctx, records):
    """256 and 1,024 records, and the candidates for one tile of the 64-bit pair sort and of the segmented maximum (256
    threads times 8, 15, 16 or 32 items), each crossed by one boundary pair -- records come two at a time"""
    n = records // 2 + 3
    index, rho = _ring(n, records // 2, records)
    got, want, _ = _check(nb, ctx, records, index=index, rho=rho, n_hop=1, n_merge=2, delta_outer=1.0, delta_saddle=6.0,
                          delta_peak=9.0)  # (every body live: rho >= 1)
    assert want["n_records"] == records and want["counts"][2] == n


@pytest.mark.parametrize("name", sorted(ref.hand_cases()))
def test_hand_cases(nb, ctx, name):
    args, answers = ref.hand_cases()[name]
    got, want, _ = _check(nb, ctx, name, **args)
    for key in ("labels", "peak", "offsets", "members", "group_peak"):
        if key in answers:
            assert got[key].tolist() == list(answers[key]), (name, key)
    assert got["counts"][3] == answers["rounds"] and got["counts"][2] == answers["n_peaks"]


# ---- 2. a graph that regroups in every way ---------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _regroup():
    args = ref.regroup_case()
    return args, ref.reference(**args)


def test_random_graph_with_massive_ties(nb, ctx):
    args, want = _regroup()
    assert want["rounds"] >= 3 and want["dropped"].size >= 1 and want["unions"] >= 1  # (else the test would pass empty)
    assert np.unique(args["rho"]).size == 16 and args["index"].shape == (3000, 8)
    got, _ = _call(nb, ctx, **args)
    _same(got, want, "regroup")
    for min_members in (2, 5, 50):
        _check(nb, ctx, min_members, **dict(args, min_members=min_members))
    for gen in (ref.random_graph, ref.local_graph):
        for n_hop, n_merge, deltas in ((8, 4, (4.0, 9.0, 12.0)), (2, 2, (6.0, 12.0, 16.0)), (1, 1, (2.0, 10.0, 15.0)),
                                       (8, 8, (0.0, 0.0, 0.0)), (4, 8, (16.0, 16.0, 16.0))):
            index, rho = gen(3000, 8, 16, 21)
            _check(nb, ctx, (gen.__name__, n_hop, n_merge), index=index, rho=rho, n_hop=n_hop, n_merge=n_merge, delta_outer=deltas[0],
                   delta_saddle=deltas[1], delta_peak=deltas[2])


def test_the_same_input_permuted(nb, ctx):
    args, _ = _regroup()
    n = 3000
    perm = np.random.default_rng(8).permutation(n)  # body i becomes body perm[i]
    inv = np.argsort(perm)

    def permuted(index, rho):
        moved = np.where(index >= 0, perm[np.maximum(index, 0)], index).astype(np.int32)
        return moved[inv], rho[inv]

    # with ties the lower index wins, so the answer of the permuted input is its own: the model decides, not the input order
    index, rho = permuted(args["index"], args["rho"])
    _check(nb, ctx, "permuted, ties", **dict(args, index=index, rho=rho))
    # without ties in rho (and hence none among the saddles of different pairs, which are sums of two of the densities
    # drawn here) the model names bodies only through root = the lowest peak index: the partition and the peaks map through
    # the permutation, the labels through the lowest member peak
    distinct = np.random.default_rng(9).permutation(n).astype(np.float64) + 0.25 * np.random.default_rng(10).random(n)
    plain_args = dict(args, rho=distinct, delta_outer=0.3 * n, delta_saddle=0.8 * n, delta_peak=0.9 * n)
    a, want_a, _ = _check(nb, ctx, "distinct", **plain_args)
    index, rho = permuted(plain_args["index"], distinct)
    b, _, _ = _check(nb, ctx, "distinct, permuted", **dict(plain_args, index=index, rho=rho))
    assert want_a["rounds"] >= 2 and want_a["counts"][0] >= 2
    assert np.array_equal(perm[a["peak"]], b["peak"][perm])
    groups_a = {frozenset(perm[a["members"][lo:hi]].tolist()) for lo, hi in zip(a["offsets"][:-1], a["offsets"][1:])}
    groups_b = {frozenset(b["members"][lo:hi].tolist()) for lo, hi in zip(b["offsets"][:-1], b["offsets"][1:])}
    assert groups_a == groups_b
    assert set(perm[a["group_peak"]].tolist()) == set(b["group_peak"].tolist())
    assert np.array_equal(a["labels"] < 0, b["labels"][perm] < 0) and a["counts"].tolist() == b["counts"].tolist()


def test_twice_the_same_call_gives_identical_bytes(nb, ctx):
    args, _ = _regroup()
    first, _ = _call(nb, ctx, **args)
    again, _ = _call(nb, ctx, **args)
    for key in ref.OUTPUTS:
        assert first[key].tobytes() == again[key].tobytes(), key


# ---- 3. refusals ------------------------------------------------------------------------------------------------------------------
def _copy(nb, ctx, n_groups, n_members):
    off = torch.full((n_groups + 1,), -7, dtype=torch.int32, device="cuda")
    mem = torch.full((max(n_members, 1),), -7, dtype=torch.int32, device="cuda")
    gp = torch.full((max(n_groups, 1),), -7, dtype=torch.int32, device="cuda")
    nb._lib.check(ctx._lib.nbody_hip_hop_groups_copy(ctx.handle, off.data_ptr(), mem.data_ptr(), gp.data_ptr()))
    ctx.synchronize()
    return off.cpu().numpy(), mem.cpu().numpy()[:n_members], gp.cpu().numpy()[:n_groups]


def test_a_refused_call_leaves_the_earlier_catalogue_copyable(nb, ctx):
    args, want = _regroup()
    got, cat = _call(nb, ctx, **args)
    idx = torch.from_numpy(args["index"]).cuda()
    rho = torch.from_numpy(args["rho"]).cuda()
    lib, P = ctx._lib, nb._lib.HopParamsStruct
    counts = (C.c_longlong * 5)(*([-5] * 5))
    labels = torch.full((3000,), -9, dtype=torch.int32, device="cuda")
    ok = (4, 2, 1, 0, 6.0, 12.0, 16.0)

    def call(count=3000, k=8, index=idx.data_ptr(), dens=rho.data_ptr(), params=ok, out=counts, handle=ctx.handle):
        p = P(*params) if params is not None else None
        return lib.nbody_hip_hop_groups(handle, count, k, index, dens, C.byref(p) if p is not None else None, labels.data_ptr(),
                                        None, C.byref(out) if out is not None else None)

    V, S = nb._lib.ERR_VALIDATION, nb._lib.ERR_STATE
    nan, inf = float("nan"), float("inf")
    refusals = [(dict(handle=None), S), (dict(index=None), S), (dict(dens=None), S), (dict(params=None), S), (dict(out=None), S),
                (dict(count=0), V), (dict(count=2 ** 30 + 1), V), (dict(count=-1), V), (dict(k=0), V), (dict(k=33), V),
                (dict(params=(0, 2, 1, 0, 6.0, 12.0, 16.0)), V), (dict(params=(9, 2, 1, 0, 6.0, 12.0, 16.0)), V),
                (dict(params=(4, -1, 1, 0, 6.0, 12.0, 16.0)), V), (dict(params=(4, 9, 1, 0, 6.0, 12.0, 16.0)), V),
                (dict(params=(4, 2, 0, 0, 6.0, 12.0, 16.0)), V), (dict(params=(4, 2, 1, 1, 6.0, 12.0, 16.0)), V),
                (dict(params=(4, 2, 1, 0, -1.0, 12.0, 16.0)), V), (dict(params=(4, 2, 1, 0, 6.0, 5.0, 16.0)), V),
                (dict(params=(4, 2, 1, 0, 6.0, 12.0, 11.0)), V), (dict(params=(4, 2, 1, 0, nan, 12.0, 16.0)), V),
                (dict(params=(4, 2, 1, 0, 6.0, nan, 16.0)), V), (dict(params=(4, 2, 1, 0, 6.0, 12.0, inf)), V)]
    for kw, code in refusals:
        assert call(**kw) == code, kw
        assert lib.nbody_hip_last_error()
    assert list(counts) == [-5] * 5 and (labels == -9).all()  # a refused call touches nothing
    off, mem, gp = _copy(nb, ctx, cat.n_groups, cat.n_members)
    assert np.array_equal(off, want["offsets"]) and np.array_equal(mem, want["members"]) and np.array_equal(gp, want["group_peak"])
    with pytest.raises(nb.ValidationException):
        nb.hop_groups(ctx, idx, rho, 0, 2, 6.0)
    with pytest.raises(nb.ValidationException):
        nb.hop_groups(ctx, idx, rho[:-1].contiguous(), 4, 2, 6.0)
    with pytest.raises(nb.ValidationException):
        nb.hop_groups(ctx, idx.to(torch.int64), rho, 4, 2, 6.0)
    # each pointer of the copy may be null; a context that has not searched has nothing to copy
    assert lib.nbody_hip_hop_groups_copy(ctx.handle, None, None, None) == 0
    fresh = nb.Context(0)
    try:
        assert lib.nbody_hip_hop_groups_copy(fresh.handle, None, None, None) == S
    finally:
        fresh.close()
    # the default thresholds are HOP's
    d = nb.hop_groups(ctx, idx, rho, 4, 2, 4.0)
    assert (d.delta_outer, d.delta_saddle, d.delta_peak) == (4.0, 10.0, 12.0)
    _same(_host(d), ref.reference(args["index"], args["rho"], 4, 2, 4.0))


# ---- 4. end to end: two Plummer spheres --------------------------------------------------------------------------------------------
N_A, N_B, SHIFT = 2048, 1024, 6.0


@functools.lru_cache(maxsize=None)
def _spheres(nb):
    a = {k: np.asarray(v, np.float32).copy() for k, v in nb.ic.plummer(N_A, seed=3).items()}
    b = {k: np.asarray(v, np.float32).copy() for k, v in nb.ic.plummer(N_B, seed=4).items()}
    b["pos_x"] = (b["pos_x"] + np.float32(SHIFT)).astype(np.float32)  # 6 scale radii
    return {k: np.concatenate([a[k], b[k]]) for k in a}


def _end_to_end(nb, cat, d_particles, ctx):
    res = cat.neighbours
    assert res is not None and res.k == 16 and cat.k == 16 and cat.n_hop == 16 and cat.n_merge == 4 and cat.status == 0
    index, rho = res.index.cpu().numpy(), res.rho.cpu().numpy()
    assert cat.delta_outer == ref.lower_median(rho) and cat.delta_saddle == 2.5 * cat.delta_outer
    want = ref.reference(index, rho, 16, 4, cat.delta_outer)
    got = _host(cat)
    _same(got, want, "end to end")
    sizes = np.diff(got["offsets"])
    big = np.nonzero(sizes > 256)[0]
    assert len(big) == 2, sizes
    side = got["group_peak"][big] >= N_A
    assert side.tolist() in ([False, True], [True, False])  # the two densest peaks lie in different spheres
    props = cat.properties(d_particles, ctx=ctx)
    assert len(props) == cat.n_groups and (props["status"] == 0).all() and np.array_equal(props["n"], sizes)
    assert np.array_equal(props["label"], got["members"][got["offsets"][:-1]])  # (the first member, not the HOP label)
    centres = np.sort(props["com"][big, 0])
    assert abs(centres[0]) < 0.5 and abs(centres[1] - SHIFT) < 0.5
    radii = cat.lagrangianRadii(d_particles, props["com"].copy(), (0.25, 0.5, 0.9), ctx=ctx)
    assert radii.shape == (cat.n_groups, 3) and (np.diff(radii[big], axis=1) > 0).all() and (radii[big, 1] < 2.0).all()
    out, offsets = cat.systems(d_particles)
    assert out.count == cat.n_members and offsets.numel() == cat.n_groups + 1


@pytest.mark.parametrize("method", ["DIRECT_N2", "BARNES_HUT", "SPATIAL_HASH"])
def test_particle_system_finds_the_two_spheres(nb, ctx, method):
    ic = _spheres(nb)
    ps = nb.ParticleSystem()
    ps.initialize(nb.SimulationConfig(particle_count=N_A + N_B, force_method=getattr(nb.ForceMethod, method)), ic)
    acc = ps.d_particles_.acc_x.clone()
    cat = ps.hopGroups()
    assert isinstance(cat, nb.HopCatalogue) and isinstance(cat, nb.GroupCatalogue)
    assert (cat.neighbours.status.cpu().numpy() == 0).all()  # every body resolved
    _end_to_end(nb, cat, ps.d_particles_, ps.force_calculator_.ctx)
    assert torch.equal(ps.d_particles_.acc_x, acc)
    ps.update(ps.getTimeStep())  # the force calculator goes on as before


def test_grid_and_calculator_find_the_two_spheres(nb, ctx):
    ic = _spheres(nb)
    n = N_A + N_B
    d, h = nb.ParticleData(), nb.ParticleData()
    nb.ParticleDataManager.allocateDevice(d, n)
    nb.ParticleDataManager.allocateHost(h, n)
    for k, v in ic.items():
        getattr(h, k)[:] = v
    nb.ParticleDataManager.copyToDevice(d, h)
    grid = nb.SpatialHashGrid(n, 2.0, ctx)
    grid.build(d)
    cat = grid.hopGroups(16)
    assert (cat.neighbours.status.cpu().numpy() != 0).any()  # window-limited bodies: the lists are the windows'
    _end_to_end(nb, cat, d, ctx)
    calc = nb.SpatialHashCalculator(2.0, 4.0, ctx)
    other = calc.hopGroups(d, 16, n_merge=4)
    _same(_host(other), _host(cat), "calculator")
    grid.close()

"""Radial profiles (nbody_hip_groups_radial_profile, include/nbody_hip_radial.h) on a real GPU: an integer lattice on which
the radial order, every cut and every mass are exact and must EQUAL the numpy restatement of tests/radial_ref.py; an axis
lattice on which the whole shell array must; general data against the long double restatement within derived bounds and
the mass cuts within their slack; bitwise determinism and independence of a group's place; the validation on the device;
the host error codes; and that the pass disturbs neither the grid nor the catalogue."""
import ctypes as C

import numpy as np
import pytest
import torch

import group_props_ref as gp
import radial_ref as ref
from test_radial_profile_cpu import general_catalogues

pytestmark = pytest.mark.gpu

FIELDS7 = ref.POS + ref.VEL + ("mass",)
MODES = ("mass", "number", "radius")


def _device(nb, fields):
    n = fields["mass"].size
    d, h = nb.ParticleData(), nb.ParticleData()
    nb.ParticleDataManager.allocateDevice(d, n)
    nb.ParticleDataManager.allocateHost(h, n)
    for k in FIELDS7:
        getattr(h, k)[:] = fields[k]
    nb.ParticleDataManager.copyToDevice(d, h)
    return d


def _same_bytes(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def _differences(got, want):
    lines = []
    for k in want.dtype.names:
        bad = np.argwhere((got[k] != want[k]).reshape(want.shape + (-1,)).any(-1))
        if len(bad):
            at = tuple(int(i) for i in bad[0])
            lines.append(f"{k}: {len(bad)} rows, first {at}: got {got[k][at]}, want {want[k][at]}")
    return "\n".join(lines)


def _run(nb, ctx, data, cuts, mode, with_order=True, **kw):
    """-> (groups, shells, sorted_members, sorted_q) of one call on the catalogue `data`"""
    n_members = data["members"].size
    sm = torch.full((n_members,), 7, dtype=torch.int32, device="cuda") if with_order else None
    sq = torch.full((n_members,), 7.0, dtype=torch.float32, device="cuda") if with_order else None
    groups, shells = nb.groups_radial_profile(ctx, data["d"], kw.get("offsets", data["off_dev"]), kw.get("members", data["mem_dev"]),
                                              kw.get("centres", data["cen_dev"]), cuts, mode, kw.get("vels", data["vel_dev"]),
                                              sm, sq)
    return groups, shells, (sm.cpu().numpy() if with_order else None), (sq.cpu().numpy() if with_order else None)


def _catalogue(nb, fields, offsets, members, centres, vels, d=None):
    return dict(fields=fields, offsets=offsets, members=members, centres=centres, vels=vels,
                d=_device(nb, fields) if d is None else d, off_dev=torch.from_numpy(offsets).cuda(),
                mem_dev=torch.from_numpy(members).cuda(), cen_dev=torch.from_numpy(centres).cuda(),
                vel_dev=torch.from_numpy(vels).cuda())


# ---- 1. the two lattices ------------------------------------------------------------------------------------------------------
COUNT = 90000


@pytest.fixture(scope="module")
def lattice(nb):
    sizes = ref.lattice_sizes()
    L = _catalogue(nb, *ref.lattice(sizes, COUNT))
    L["sizes"] = np.asarray(sizes)
    L["want"] = {m: ref.reference(L["fields"], L["offsets"], L["members"], L["centres"], ref.LATTICE_CUTS[m], m, L["vels"])
                 for m in MODES}
    return L


def test_struct_and_sizes(nb):
    assert nb.RADIAL_GROUP_DTYPE == ref.GROUP_DTYPE and nb.RADIAL_SHELL_DTYPE == ref.SHELL_DTYPE
    assert C.sizeof(nb._lib.RadialGroupStruct) == 32 and C.sizeof(nb._lib.RadialShellStruct) == 64


@pytest.mark.parametrize("mode", MODES)
def test_integer_lattice_is_exact(nb, ctx, lattice, mode):
    L, sizes = lattice, lattice["sizes"]
    for s in ref.LADDER + [64 * ref.C + 3]:
        assert (sizes == s).any(), s
    big = int(np.nonzero(sizes == 64 * ref.C + 3)[0][0])
    assert (sizes[:big] <= 6).sum() > 1000 and (sizes[big + 1:] <= 6).sum() > 1000
    want = L["want"][mode]
    K, n = want["shells"]["enclosed_count"], want["groups"]["n"]
    assert (want["groups"]["status"] == 0).all() and np.array_equal(n, sizes)
    # the cuts are worth the test (the recipe: tests/test_radial_profile_cpu.py)
    q_big = want["sorted_q"][L["offsets"][big]:L["offsets"][big + 1]]
    assert q_big[ref.C - 1] == q_big[ref.C] and (want["shells"]["count"] == 0).any()
    if mode == "mass":
        assert (K[:, 0] == 1).any() and (K[:, -1] == n).all() and K[int(np.nonzero(sizes == 2 * ref.C)[0][0]), 2] == ref.C
    if mode == "radius":
        assert (K[:, 0] > 0).any() and (K[:, 0] == 0).any() and (K[:, -1] == n).all() and np.isinf(want["shells"]["radius"][:, -1]).all()
    groups, shells, sm, sq = _run(nb, ctx, L, ref.LATTICE_CUTS[mode], mode)
    assert np.array_equal(sm, want["sorted_members"]) and np.array_equal(sq, want["sorted_q"])
    assert _same_bytes(groups, want["groups"]), _differences(groups, want["groups"])
    for k in ("count", "enclosed_count", "mass", "enclosed_mass", "radius", "reserved"):
        assert shells[k].tobytes() == want["shells"][k].tobytes(), (k, _differences(shells, want["shells"]))
    # the velocity sums are inexact here (r is a root): within the derived bound of the model's own absolute sums
    w = ref.wide(want["state"], K, K.shape[1])
    for g in (big, int(np.nonzero(sizes == ref.C + 1)[0][0]), 0, 1, 2):
        cnt = shells[g]["count"].astype(np.float64)
        for i, k in enumerate(ref.SUMS):
            assert (np.abs(shells[g][k] - w[g]["sums"][:, i]) <= (cnt + ref.K_SUM) * ref.U * w[g]["abs"][:, i]).all(), (g, k)


def test_the_outputs_of_the_order_are_optional_and_the_catalogue_object_calls_the_same(nb, ctx, lattice):
    L = lattice
    want = L["want"]["mass"]
    groups, shells, _, _ = _run(nb, ctx, L, ref.LATTICE_CUTS["mass"], "mass", with_order=False)
    again, shells2, sm, _ = _run(nb, ctx, L, ref.LATTICE_CUTS["mass"], "mass")
    assert _same_bytes(groups, again) and _same_bytes(shells, shells2) and _same_bytes(groups, want["groups"])
    cat = nb.GroupCatalogue(torch.zeros(COUNT, dtype=torch.int32, device="cuda"), L["off_dev"], L["mem_dev"], 1.0, 1)
    g3, s3 = cat.radialProfile(L["d"], L["cen_dev"], ref.LATTICE_CUTS["mass"], "mass", L["vel_dev"], ctx=ctx)
    assert _same_bytes(g3, groups) and _same_bytes(s3, shells)
    radii = cat.lagrangianRadii(L["d"], L["centres"], ref.LATTICE_CUTS["mass"], ctx=ctx)  # (host centres: uploaded)
    assert radii.tobytes() == want["shells"]["radius"].tobytes()
    # host arrays for the catalogue too
    g4, s4 = nb.groups_radial_profile(ctx, L["d"], L["offsets"], L["members"], L["centres"], ref.LATTICE_CUTS["mass"], "mass",
                                      L["vels"])
    assert _same_bytes(g4, groups) and _same_bytes(s4, shells)
    # a shell handed to the group properties through the sorted list: its mass is the shell's
    big = int(np.argmax(L["sizes"]))
    o0 = int(L["offsets"][big])
    K = want["shells"]["enclosed_count"][big]
    shell_off = np.array([o0] + [o0 + int(k) for k in K], np.int32)
    props = nb.groups_properties(ctx, L["d"], shell_off, sm)
    assert (props["status"] == 0).all() and np.array_equal(props["mass"], want["shells"]["mass"][big])
    assert np.array_equal(props["n"], want["shells"]["count"][big])


@pytest.mark.parametrize("mode", MODES)
def test_axis_lattice_whole_structs_to_the_byte(nb, ctx, mode):
    A = _catalogue(nb, *ref.lattice(ref.axis_sizes(), 20000, axis=True, seed=2))
    sizes = np.diff(A["offsets"])
    for s in ref.LADDER:
        assert (sizes == s).any(), s
    want = ref.reference(A["fields"], A["offsets"], A["members"], A["centres"], ref.AXIS_CUTS[mode], mode, A["vels"])
    assert (want["groups"]["status"] == 0).all() and want["shells"]["m_vr2"].any() and want["shells"]["m_vt2"].any()
    groups, shells, sm, sq = _run(nb, ctx, A, ref.AXIS_CUTS[mode], mode)
    assert np.array_equal(sm, want["sorted_members"]) and np.array_equal(sq, want["sorted_q"])
    assert _same_bytes(groups, want["groups"]), _differences(groups, want["groups"])
    assert _same_bytes(shells, want["shells"]), _differences(shells, want["shells"])


# ---- 2. general data ----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def general(nb, ctx):
    fields, cats = general_catalogues(nb)
    d = _device(nb, fields)
    out = {}
    for name, c in cats.items():
        G = _catalogue(nb, fields, c["offsets"], c["members"], c["centres"], c["vels"], d)
        G["want"] = ref.reference(fields, c["offsets"], c["members"], c["centres"], ref.FRACTIONS, "mass", c["vels"])
        G["got"] = _run(nb, ctx, G, ref.FRACTIONS, "mass")
        out[name] = G
    return out


@pytest.mark.parametrize("name", ["fof", "partition"])
def test_general_data_within_derived_bounds(nb, ctx, general, name):
    G = general[name]
    want = G["want"]
    groups, shells, sm, sq = G["got"]
    n = want["groups"]["n"]
    if name == "fof":
        assert (n == 1).sum() > 100 and ((n > 1) & (n <= ref.S)).sum() > 100 and n.max() > 2 * ref.C
    else:
        for s in ref.LADDER:
            assert (n == s).any(), s
    assert n.max() <= ref.N_MAX and n.sum() == gp.N_PLUMMER + gp.N_BACKGROUND
    # the order depends on per-member arithmetic alone
    assert np.array_equal(sm, want["sorted_members"]) and np.array_equal(sq, want["sorted_q"])
    for k in ("n", "status", "reserved", "r_max"):
        assert np.array_equal(groups[k], want["groups"][k]), k
    K = shells["enclosed_count"]
    assert np.array_equal(shells["count"], np.diff(np.concatenate((np.zeros((len(K), 1), np.int32), K), 1), axis=1))
    assert not shells["reserved"].any() and (K >= 1).all() and (K <= n[:, None]).all() and (K[:, -1] == n).all()
    wide = ref.wide(want["state"], K, len(ref.FRACTIONS))  # the wide sums over the DEVICE's shells
    worst = {k: 0.0 for k in ref.SUMS + ("enclosed_mass", "mass_of_group")}
    ambiguous = different = 0
    for g, w in wide.items():
        sh = shells[g]
        q = want["state"][g]["q"]
        assert np.array_equal(sh["radius"], np.sqrt(q[K[g] - 1].astype(np.float64))), g
        cnt, Kg = sh["count"].astype(np.float64), K[g].astype(np.float64)
        b = (Kg + ref.K_SUM) * ref.U * w["enclosed"]
        err = np.abs(sh["enclosed_mass"] - w["enclosed"])
        worst["enclosed_mass"] = max(worst["enclosed_mass"], float((err / b).max()))
        assert (err <= b).all(), (g, "enclosed_mass")
        for i, k in enumerate(ref.SUMS):
            b = (cnt + ref.K_SUM) * ref.U * w["abs"][:, i]
            err = np.abs(sh[k] - w["sums"][:, i])
            worst[k] = max(worst[k], float((err / np.where(b > 0, b, 1.0)).max()))
            assert (err <= b).all(), (g, k)
        M = np.float64(w["cum"][-1])
        err = abs(groups["mass"][g] - M) / ((n[g] + ref.K_SUM) * ref.U * M)
        worst["mass_of_group"] = max(worst["mass_of_group"], float(err))
        assert err <= 1, (g, "mass")
        for c, f in enumerate(ref.FRACTIONS):
            ok, amb = ref.mass_cut_checks(w["cum"], int(n[g]), f, int(K[g, c]))
            assert ok, (g, c, int(K[g, c]), int(want["shells"]["enclosed_count"][g, c]))
            ambiguous += amb
        different += int((K[g] != want["shells"]["enclosed_count"][g]).sum())
    total = len(wide) * len(ref.FRACTIONS)
    for k, v in worst.items():
        print(f"{name} {k}: largest |device - reference| / bound = {v:.3g}")
    print(f"{name}: {ambiguous} ambiguous of {total} pairs; the device's K differs from the model's in {different}")
    assert ambiguous <= ref.AMBIGUITY_CAP * total


@pytest.mark.parametrize("name", ["fof", "partition"])
def test_general_data_is_the_model_to_the_bit(nb, ctx, general, name):
    """the header's claim: the order of every sum is a function of n alone, so the fp64 restatement in that order is
    what the device computes, inexact data included"""
    G = general[name]
    groups, shells, _, _ = G["got"]
    assert _same_bytes(groups, G["want"]["groups"]), _differences(groups, G["want"]["groups"])
    assert _same_bytes(shells, G["want"]["shells"]), _differences(shells, G["want"]["shells"])


# ---- 3. determinism and place -------------------------------------------------------------------------------------------------
def _rearranged(G, order):
    lists = [G["members"][G["offsets"][g]:G["offsets"][g + 1]] for g in order]
    off = np.concatenate(([0], np.cumsum([len(x) for x in lists]))).astype(np.int32)
    mem = (np.concatenate(lists) if lists else np.zeros(0, np.int32)).astype(np.int32)
    return dict(offsets=off, members=mem, centres=G["centres"][order].copy(), vels=G["vels"][order].copy())


def test_bitwise_determinism_and_placement(nb, ctx, general):
    G = general["partition"]
    groups, shells, sm, sq = G["got"]
    again = _run(nb, ctx, G, ref.FRACTIONS, "mass")
    assert _same_bytes(groups, again[0]) and _same_bytes(shells, again[1]) and np.array_equal(sm, again[2])
    n_groups = len(groups)
    big = int(np.argmax(groups["n"]))
    others = [g for g in range(n_groups) if g != big]
    for order in ([big], [big] + others, others + [big], others[:7] + [big] + others[7:]):
        order = np.asarray(order)
        R = _rearranged(G, order)
        g2, s2 = nb.groups_radial_profile(ctx, G["d"], R["offsets"], R["members"], R["centres"], ref.FRACTIONS, "mass", R["vels"])
        assert _same_bytes(g2, groups[order]), _differences(g2, groups[order])
        assert _same_bytes(s2, shells[order]), _differences(s2, shells[order])
    # the other groups' centres changed: the group's rows are the same bytes
    moved = G["centres"].copy()
    moved += 0.37
    moved[big] = G["centres"][big]
    g3, s3 = nb.groups_radial_profile(ctx, G["d"], G["off_dev"], G["mem_dev"], moved, ref.FRACTIONS, "mass", G["vels"])
    assert g3[big:big + 1].tobytes() == groups[big:big + 1].tobytes() and s3[big].tobytes() == shells[big].tobytes()
    assert s3[others[0]].tobytes() != shells[others[0]].tobytes()


# ---- 4. validation on the device ----------------------------------------------------------------------------------------------
def test_bad_catalogues_on_the_device(nb, ctx, lattice):
    L = lattice
    sizes = L["sizes"]
    pick = lambda s: int(np.nonzero(sizes == s)[0][0])  # noqa: E731
    keep = np.array([pick(3), pick(ref.S + 1), pick(2 * ref.C + 1), pick(5), pick(ref.C), pick(2)])
    R = _rearranged(L, keep)
    cuts = ref.LATTICE_CUTS["mass"]
    fields = L["fields"]

    def call(off, mem, cen, vel, d=L["d"]):
        sm = torch.full((len(mem),), 7, dtype=torch.int32, device="cuda")
        sq = torch.full((len(mem),), 7.0, dtype=torch.float32, device="cuda")
        g, s = nb.groups_radial_profile(ctx, d, off, mem, cen, cuts, "mass", vel, sm, sq)
        return dict(groups=g, shells=s, sorted_members=sm.cpu().numpy(), sorted_q=sq.cpu().numpy())

    def same(got, want):
        assert _same_bytes(got["groups"], want["groups"]), _differences(got["groups"], want["groups"])
        assert _same_bytes(got["shells"], want["shells"]), _differences(got["shells"], want["shells"])
        assert np.array_equal(got["sorted_members"], want["sorted_members"]) and np.array_equal(got["sorted_q"], want["sorted_q"])

    clean = call(R["offsets"], R["members"], R["centres"], R["vels"])
    same(clean, ref.reference(fields, R["offsets"], R["members"], R["centres"], cuts, "mass", R["vels"]))
    assert (clean["groups"]["status"] == 0).all()
    # 1. offsets out of order: every group of the call
    for at, value in ((2, int(R["offsets"][1]) - 1), (0, -1), (len(keep), len(R["members"]) + 1)):
        off = R["offsets"].copy()
        off[at] = value
        got = call(off, R["members"], R["centres"], R["vels"])
        same(got, ref.reference(fields, off, R["members"], R["centres"], cuts, "mass", R["vels"]))
        assert (got["groups"]["status"] == 1).all() and (got["sorted_members"] == -1).all() and not got["shells"]["count"].any()
    # 2. an empty group between the others, and positions of no group at both ends
    off = np.concatenate((R["offsets"][:3], R["offsets"][2:])).astype(np.int32) + 5
    mem = np.concatenate((np.full(5, 3, np.int32), R["members"], np.full(4, 9, np.int32)))
    cen, vel = np.insert(R["centres"], 2, 1.0, axis=0), np.insert(R["vels"], 2, 1.0, axis=0)
    got = call(off, mem, cen, vel)
    same(got, ref.reference(fields, off, mem, cen, cuts, "mass", vel))
    rows = [0, 1, 3, 4, 5, 6]
    assert got["groups"]["status"].tolist() == [0, 0, 1, 0, 0, 0, 0]
    assert _same_bytes(got["groups"][rows], clean["groups"]) and _same_bytes(got["shells"][rows], clean["shells"])
    assert (got["sorted_members"][:5] == -1).all() and (got["sorted_members"][-4:] == -1).all()
    # 3. a bad member index in a small and in a chunked group
    mem = R["members"].copy()
    mem[int(R["offsets"][0]) + 1] = COUNT
    mem[int(R["offsets"][2]) + 2 * ref.C] = -1
    got = call(R["offsets"], mem, R["centres"], R["vels"])
    same(got, ref.reference(fields, R["offsets"], mem, R["centres"], cuts, "mass", R["vels"]))
    assert got["groups"]["status"].tolist() == [1, 0, 1, 0, 0, 0]
    assert _same_bytes(got["groups"][[1, 3, 4, 5]], clean["groups"][[1, 3, 4, 5]])
    assert _same_bytes(got["shells"][[1, 3, 4, 5]], clean["shells"][[1, 3, 4, 5]])
    # 4. a NaN position in a small and in a chunked group: status 2; a bad index on top: status 1
    f = {k: a.copy() for k, a in fields.items()}
    f["pos_y"][R["members"][int(R["offsets"][3]) + 1]] = np.nan
    f["pos_z"][R["members"][int(R["offsets"][4]) + ref.C - 1]] = np.nan
    d_nan = _device(nb, f)
    got = call(R["offsets"], R["members"], R["centres"], R["vels"], d_nan)
    same(got, ref.reference(f, R["offsets"], R["members"], R["centres"], cuts, "mass", R["vels"]))
    assert got["groups"]["status"].tolist() == [0, 0, 0, 2, 2, 0]
    assert _same_bytes(got["shells"][[0, 1, 2, 5]], clean["shells"][[0, 1, 2, 5]])
    mem = R["members"].copy()
    mem[int(R["offsets"][4])] = COUNT + 5
    got = call(R["offsets"], mem, R["centres"], R["vels"], d_nan)
    assert got["groups"]["status"].tolist() == [0, 0, 0, 2, 1, 0]
    # 5. a far member: q overflows to +inf, the group is fine and its r_max infinite
    f = {k: a.copy() for k, a in fields.items()}
    f["pos_x"][R["members"][int(R["offsets"][1])]] = 3e19
    got = call(R["offsets"], R["members"], R["centres"], R["vels"], _device(nb, f))
    same(got, ref.reference(f, R["offsets"], R["members"], R["centres"], cuts, "mass", R["vels"]))
    assert got["groups"]["status"][1] == 0 and np.isinf(got["groups"]["r_max"][1])


# ---- 5. the host ---------------------------------------------------------------------------------------------------------------
def test_host_error_codes(nb, ctx, lattice):
    L = lattice
    lib, E = ctx._lib, nb._lib
    s = L["d"].struct()
    groups, shells = nb.radial_tensors(4, 3, "cuda")
    n_members = L["members"].size
    good = (C.c_double * 3)(0.25, 0.5, 1.0)

    def call(ctx_h=ctx.handle, d=C.byref(s), offsets=L["off_dev"].data_ptr(), members=L["mem_dev"].data_ptr(), n_groups=4,
             n_mem=n_members, centres=L["cen_dev"].data_ptr(), cuts=good, n_cuts=3, mode=0, g=groups.data_ptr(),
             sh=shells.data_ptr()):
        return lib.nbody_hip_groups_radial_profile(ctx_h, d, offsets, members, n_groups, n_mem, centres, None, cuts, n_cuts, mode,
                                                   g, sh, None, None)

    assert call() == 0
    for kw in (dict(ctx_h=None), dict(d=None), dict(offsets=None), dict(cuts=None), dict(centres=None), dict(g=None), dict(sh=None)):
        assert call(**kw) == E.ERR_STATE, kw
    null_arrays = nb._lib.ParticleDataStruct()
    null_arrays.count = COUNT
    assert call(d=C.byref(null_arrays)) == E.ERR_STATE
    for kw in (dict(n_groups=-1), dict(n_mem=-1), dict(n_mem=2 ** 31), dict(n_cuts=0), dict(n_cuts=17), dict(mode=3), dict(mode=-1),
               dict(cuts=(C.c_double * 3)(0.5, 0.25, 1.0)), dict(cuts=(C.c_double * 3)(0.5, 0.5, 1.0)),
               dict(cuts=(C.c_double * 3)(0.0, 0.5, 1.0)), dict(cuts=(C.c_double * 3)(0.5, 1.0, 1.5)),
               dict(cuts=(C.c_double * 3)(0.5, float("nan"), 1.0)), dict(cuts=(C.c_double * 3)(-1.0, 0.5, 1.0), mode=2),
               dict(cuts=(C.c_double * 3)(0.5, float("inf"), float("inf")), mode=2),
               dict(n_groups=2 ** 28, cuts=(C.c_double * 16)(*[(i + 1) / 16 for i in range(16)]), n_cuts=16)):
        assert call(**kw) == E.ERR_VALIDATION, kw
    assert call(cuts=(C.c_double * 3)(0.0, 0.5, float("inf")), mode=2) == 0
    for bad in (0, 2 ** 30 + 1):
        t = L["d"].struct()
        t.count = bad
        assert call(d=C.byref(t)) == E.ERR_VALIDATION, bad
    # the order of the checks is the group properties': a null array before a bad count, a bad count before the cuts
    assert call(offsets=None, n_groups=-1) == E.ERR_STATE and call(n_groups=-1, n_cuts=0) == E.ERR_VALIDATION
    ctx.synchronize()
    # n_groups == 0 succeeds and touches nothing, whatever the other pointers are
    canary = torch.full((64,), 7, dtype=torch.uint8, device="cuda")
    assert lib.nbody_hip_groups_radial_profile(ctx.handle, C.byref(s), L["off_dev"].data_ptr(), None, 0, 0, None, None, good, 3, 0,
                                               canary.data_ptr(), canary.data_ptr(), canary.data_ptr(), canary.data_ptr()) == 0
    ctx.synchronize()
    assert (canary == 7).all()
    g0, s0 = nb.groups_radial_profile(ctx, L["d"], np.zeros(1, np.int32), np.zeros(0, np.int32), np.zeros((0, 3)), [0.5, 1.0])
    assert g0.shape == (0,) and s0.shape == (0, 2) and g0.dtype == ref.GROUP_DTYPE
    # the grid's call: no catalogue, no answer
    grid = nb.SpatialHashGrid(COUNT, 64.0, ctx)
    assert lib.nbody_hip_grid_groups_radial_profile(grid._h, C.byref(s), L["cen_dev"].data_ptr(), None, good, 3, 0,
                                                    groups.data_ptr(), shells.data_ptr(), None, None) == E.ERR_STATE
    assert lib.nbody_hip_grid_groups_radial_profile(None, C.byref(s), L["cen_dev"].data_ptr(), None, good, 3, 0,
                                                    groups.data_ptr(), shells.data_ptr(), None, None) == E.ERR_STATE
    with pytest.raises(nb.StateException, match="no group catalogue"):
        grid.groupRadialProfile(L["d"], np.zeros((0, 3)), [0.5])
    # the wrapper's own checks
    with pytest.raises(nb.ValidationException, match="mode"):
        nb.groups_radial_profile(ctx, L["d"], L["off_dev"], L["mem_dev"], L["cen_dev"], [0.5], "volume")
    with pytest.raises(nb.ValidationException, match="centres"):
        nb.groups_radial_profile(ctx, L["d"], L["off_dev"], L["mem_dev"], np.zeros((3, 3)), [0.5])
    with pytest.raises(nb.ValidationException, match="ascending"):
        nb.groups_radial_profile(ctx, L["d"], L["off_dev"], L["mem_dev"], L["cen_dev"], [0.5, 0.25])
    with pytest.raises(nb.ValidationException, match="sorted_q"):
        nb.groups_radial_profile(ctx, L["d"], L["off_dev"], L["mem_dev"], L["cen_dev"], [0.5], sorted_q=torch.zeros(3, device="cuda"))


def test_all_bodies_as_one_group(nb, ctx, lattice):
    L = lattice
    centre, cuts = np.array([[1.0, -2.0, 3.0]]), [0.1, 0.5, 0.9, 1.0]
    off = np.array([0, COUNT], np.int32)
    sm = torch.empty(COUNT, dtype=torch.int32, device="cuda")
    sm2 = torch.empty(COUNT, dtype=torch.int32, device="cuda")
    g1, s1 = nb.groups_radial_profile(ctx, L["d"], off, None, centre, cuts, "number", sorted_members=sm)
    g2, s2 = nb.groups_radial_profile(ctx, L["d"], off, np.arange(COUNT, dtype=np.int32), centre, cuts, "number", sorted_members=sm2)
    assert _same_bytes(g1, g2) and _same_bytes(s1, s2) and torch.equal(sm, sm2)
    want = ref.reference(L["fields"], off, None, centre, cuts, "number")
    assert np.array_equal(sm.cpu().numpy(), want["sorted_members"]) and _same_bytes(g1, want["groups"])
    assert g1["n"][0] == COUNT and s1["enclosed_count"][0].tolist() == [9000, 45000, 81000, 90000]
    for k in ("count", "enclosed_count", "radius", "mass", "enclosed_mass"):
        assert s1[k].tobytes() == want["shells"][k].tobytes(), k


def test_recorded_into_a_step_graph(nb, ctx, lattice):
    L = lattice
    cuts = ref.LATTICE_CUTS["mass"]
    want_g, want_s, _, _ = _run(nb, ctx, L, cuts, "mass", with_order=False)  # (the workspace exists from here)
    groups, shells = nb.radial_tensors(len(want_g), len(cuts), "cuda")
    with ctx.capture() as cap:
        nb.groups_radial_profile_into(ctx, L["d"], L["off_dev"], L["mem_dev"], L["cen_dev"], cuts, groups, shells, "mass",
                                      L["vel_dev"])
    cap.graph.launch()
    ctx.synchronize()
    g, s = nb.radial_arrays(groups, shells, len(cuts))
    assert _same_bytes(g, want_g) and _same_bytes(s, want_s)


def test_the_grid_and_the_catalogue_are_left_alone(nb, ctx, general):
    G = general["fof"]
    d = G["d"]
    calc = nb.SpatialHashCalculator(cell_size=2 * gp.LINK, cutoff_radius=2 * gp.LINK, ctx=ctx)
    calc.setSofteningParameter(0.01)
    cat = calc.findGroups(d, gp.LINK, 1)
    grid = calc.getGrid()

    def forces():
        grid.computeForces(d, 0.4, 1.0, 0.01)
        ctx.synchronize()
        return np.stack([d.acc_x.cpu().numpy(), d.acc_y.cpu().numpy(), d.acc_z.cpu().numpy()])

    before = forces()
    off, mem = cat.offsets.cpu().numpy(), cat.members.cpu().numpy()
    assert np.array_equal(off, G["offsets"]) and np.array_equal(mem, G["members"])  # the device's catalogue is the CPU's
    state = [getattr(d, k).clone() for k in FIELDS7]
    groups, shells, _, _ = G["got"]
    by_cat = cat.radialProfile(d, G["cen_dev"], ref.FRACTIONS, "mass", G["vel_dev"], ctx=ctx)
    by_grid = grid.groupRadialProfile(d, G["cen_dev"], ref.FRACTIONS, "mass", G["vel_dev"])
    for got in (by_cat, by_grid):
        assert _same_bytes(got[0], groups) and _same_bytes(got[1], shells)
    for k, t in zip(FIELDS7, state):
        assert torch.equal(getattr(d, k), t), k
    assert np.array_equal(before.view(np.uint32), forces().view(np.uint32))
    again = grid.findGroups(gp.LINK, 1)
    assert torch.equal(again.offsets, cat.offsets) and torch.equal(again.members, cat.members) and torch.equal(again.labels, cat.labels)


@pytest.mark.parametrize("method", ["DIRECT_N2", "BARNES_HUT", "SPATIAL_HASH"])
def test_lagrangian_radii_of_a_plummer_sphere(nb, ctx, method):
    n = 4096
    a = nb.ic.plummer(n, seed=11)
    ic = {k: np.asarray(a[k], np.float32) for k in FIELDS7}
    ps = nb.ParticleSystem()
    ps.initialize(nb.SimulationConfig(particle_count=n, force_method=getattr(nb.ForceMethod, method)), ic)
    radii = ps.lagrangianRadii()
    assert radii.shape == (3,) and (np.diff(radii) > 0).all()
    # ic.plummer: scale length a = 1; the half-mass radius of a Plummer sphere is 1.305 a.  A sanity bound on a finite,
    # truncated sample about an estimated centre, not a precision claim.
    half = ps.lagrangianRadii(fractions=(0.5,))[0]
    print(f"{method}: r_half = {half:.4f}, analytic 1.305")
    assert half == radii[1] and abs(half - 1.305) <= 0.15 * 1.305
    cat = ps.findGroups(0.15, 1)
    groups, shells, props = ps.groupProfiles(cat, (0.5, 1.0), "mass", centre="com")
    assert (groups["status"] == 0).all() and np.array_equal(groups["n"], props["n"])
    big = int(np.argmax(groups["n"]))
    assert abs(groups["mass"][big] - props["mass"][big]) <= 1e-12 * props["mass"][big]
    assert abs(shells["radius"][big, 1] - props["r_max"][big]) <= 1e-6 * props["r_max"][big]  # q is a float
    g2, s2, p2 = ps.groupProfiles(cat, (0.5, 1.0), "mass", centre="potential")
    assert (g2["status"] == 0).all() and s2["radius"][big, 0] > 0

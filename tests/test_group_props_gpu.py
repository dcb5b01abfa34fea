"""Group properties (nbody_hip_groups_properties, include/nbody_hip_group_props.h) on a real GPU: an exact lattice on which
every quantity is exact in fp64 and the whole struct array must EQUAL the numpy restatement of tests/group_props_ref.py;
general data against that restatement within bounds derived from its own absolute sums; bitwise determinism and
independence of a group's place in the catalogue; the per-group validation on the device; the host error codes; and that
the pass disturbs neither the grid nor the next step."""
import ctypes as C

import numpy as np
import pytest
import torch

import group_props_ref as ref

pytestmark = pytest.mark.gpu

FIELDS7 = ref.POS + ref.VEL + ("mass",)


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
    """the fields and rows in which two struct arrays differ: what an assertion prints"""
    lines = []
    for k in want.dtype.names:
        bad = np.nonzero((got[k] != want[k]).reshape(len(want), -1).any(1))[0]
        if bad.size:
            g = int(bad[0])
            lines.append(f"{k}: {bad.size} rows, first {g} (n = {want['n'][g]}): got {got[k][g]}, want {want[k][g]}")
    return "\n".join(lines)


# ---- 1. the exact lattice -----------------------------------------------------------------------------------------------
COUNT = 90000


@pytest.fixture(scope="module")
def lattice(nb):
    sizes = ref.lattice_sizes()
    fields, offsets, members, phi = ref.lattice(sizes, COUNT)
    assert members[-1] == COUNT - 1 and offsets[-1] == members.size < COUNT  # body count - 1; bodies in no group
    d = _device(nb, fields)
    return dict(sizes=sizes, fields=fields, offsets=offsets, members=members, phi=phi, d=d,
                off_dev=torch.from_numpy(offsets).cuda(), mem_dev=torch.from_numpy(members).cuda(),
                phi_dev=torch.from_numpy(phi).cuda())


def test_struct_and_sizes(nb):
    assert nb.GROUP_PROPS_DTYPE == ref.DTYPE and C.sizeof(nb._lib.GroupPropsStruct) == 192
    for name, typ in nb._lib.GroupPropsStruct._fields_:
        assert getattr(nb._lib.GroupPropsStruct, name).offset == ref.DTYPE.fields[name][1], name


def test_lattice_is_exact(nb, ctx, lattice):
    L = lattice
    sizes = np.asarray(L["sizes"])
    for s in (1, 2, 3, ref.S - 1, ref.S, ref.S + 1, ref.C - 1, ref.C, ref.C + 1, 2 * ref.C, 2 * ref.C + 1, 64 * ref.C + 3):
        assert (sizes == s).any(), s
    big = int(np.nonzero(sizes == 64 * ref.C + 3)[0][0])
    assert (sizes[:big] <= 6).sum() > 1000 and (sizes[big + 1:] <= 6).sum() > 1000  # small groups before and after
    want, _ = ref.reference(L["fields"], L["offsets"], L["members"], L["phi"])
    assert (want["status"] == 0).all() and (want["n"] == sizes).all()
    # the recipe holds: X and V are the integer centres, ties exist in both extrema
    assert np.array_equal(want["com"], np.round(want["com"])) and np.array_equal(want["vel"], np.round(want["vel"]))
    got = nb.groups_properties(ctx, L["d"], L["off_dev"], L["mem_dev"], L["phi_dev"])
    assert got.dtype == ref.DTYPE
    assert np.array_equal(got, want), _differences(got, want)
    assert _same_bytes(got, want)  # (the reserved words and the sign of every zero too)
    # the catalogue object's own call is the same call
    cat = nb.GroupCatalogue(torch.zeros(COUNT, dtype=torch.int32, device="cuda"), L["off_dev"], L["mem_dev"], 1.0, 1)
    assert _same_bytes(cat.properties(L["d"], L["phi_dev"], ctx), want)


def test_lattice_without_phi_and_host_arrays(nb, ctx, lattice):
    L = lattice
    want, _ = ref.reference(L["fields"], L["offsets"], L["members"], None)
    assert (want["phi_min_body"] == -1).all() and not want["potential"].any() and not want["phi_min"].any()
    got = nb.groups_properties(ctx, L["d"], L["offsets"], L["members"])  # host arrays: uploaded by the call
    assert np.array_equal(got, want), _differences(got, want)
    assert _same_bytes(got, want)


def test_no_groups(nb, ctx, lattice):
    L = lattice
    out = nb.groups_properties(ctx, L["d"], np.zeros(1, np.int32), np.zeros(0, np.int32), L["phi_dev"])
    assert out.shape == (0,) and out.dtype == ref.DTYPE
    s = L["d"].struct()
    # the C call itself: n_groups = 0 succeeds and touches nothing, whatever the other pointers are
    canary = torch.full((192,), 7, dtype=torch.uint8, device="cuda")
    assert ctx._lib.nbody_hip_groups_properties(ctx.handle, C.byref(s), L["off_dev"].data_ptr(), None, 0, 0, None,
                                                canary.data_ptr()) == 0
    ctx.synchronize()
    assert (canary == 7).all()


# ---- 2. general data ----------------------------------------------------------------------------------------------------
N_PLUMMER, N_BACKGROUND = ref.N_PLUMMER, ref.N_BACKGROUND


@pytest.fixture(scope="module")
def general(nb, ctx):
    fields = ref.general_fields(nb.ic)
    n = fields["mass"].size
    d = _device(nb, fields)
    link = ref.LINK
    calc = nb.SpatialHashCalculator(cell_size=2 * link, cutoff_radius=2 * link, ctx=ctx)
    calc.setSofteningParameter(0.01)
    phi = torch.empty(n, dtype=torch.float32, device="cuda")
    calc.computePotential(d, phi)
    cat = calc.findGroups(d, link, 1)
    grid = calc.getGrid()
    by_grid = grid.groupProperties(d, phi)
    got = cat.properties(d, phi, ctx)
    return dict(fields=fields, d=d, phi=phi, cat=cat, got=got, by_grid=by_grid, grid=grid, calc=calc,
                offsets=cat.offsets.cpu().numpy(), members=cat.members.cpu().numpy(), phi_host=phi.cpu().numpy())


def test_general_data_within_derived_bounds(nb, ctx, general):
    Gd = general
    got = Gd["got"]
    want, aux = ref.reference(Gd["fields"], Gd["offsets"], Gd["members"], Gd["phi_host"], wide=True)
    sizes = want["n"]
    # the catalogue is worth the test: singletons, small groups, one-chunk groups and a group of several chunks
    assert (sizes == 1).sum() > 100 and ((sizes > 1) & (sizes <= ref.S)).sum() > 100
    assert sizes.max() > 2 * ref.C and sizes.sum() == N_PLUMMER + N_BACKGROUND
    bound = ref.bounds(want, aux)
    for k in ("n", "label", "status", "reserved", "phi_min", "phi_min_body"):
        # integers, and a minimum of the SAME floats with the same tie rule: no rounding is involved
        assert np.array_equal(got[k], want[k]), k
    worst = {}
    for k, b in bound.items():
        err = np.abs(got[k] - want[k])
        worst[k] = float((err / np.where(b > 0, b, 1.0)).max())
        print(f"{k}: largest |device - reference| / bound = {worst[k]:.3g} (largest error {err.max():.3g})")
        assert (err <= b).all(), (k, worst[k])
    # r_max_body: only where the reference's runner-up is further from the winner than both bounds together can move them
    decided = ref.r_max_decided(want, aux, bound)
    print(f"r_max_body decided in {decided.sum()} of {decided.size} groups")
    assert (~decided).sum() <= ref.R_MAX_UNDECIDED_CAP * decided.size  # the cap on the exclusion: at most 1 % of the groups
    assert np.array_equal(got["r_max_body"][decided], want["r_max_body"][decided])
    # whatever the gap, the device's body is a member of its group
    for g in np.nonzero(~decided)[0]:
        assert got["r_max_body"][g] in Gd["members"][Gd["offsets"][g]:Gd["offsets"][g + 1]]


# ---- 3. determinism and placement ---------------------------------------------------------------------------------------
def _rearranged(offsets, members, order):
    """the catalogue of the groups `order` (rows of the old one), in that order"""
    lists = [members[offsets[g]:offsets[g + 1]] for g in order]
    off = np.concatenate(([0], np.cumsum([len(x) for x in lists]))).astype(np.int32)
    return off, (np.concatenate(lists) if lists else np.zeros(0, np.int32)).astype(np.int32)


def test_bitwise_determinism_and_placement(nb, ctx, general):
    Gd = general
    got = Gd["got"]
    again = Gd["cat"].properties(Gd["d"], Gd["phi"], ctx)
    assert _same_bytes(got, again)
    assert _same_bytes(got, Gd["by_grid"])  # the grid's convenience call is the generic call
    G = len(got)
    order = np.arange(G)[::-1]
    off, mem = _rearranged(Gd["offsets"], Gd["members"], order)
    rev = nb.groups_properties(ctx, Gd["d"], off, mem, Gd["phi"])
    assert _same_bytes(rev, got[order]), _differences(rev, got[order])
    order = np.arange(0, G, 2)
    off, mem = _rearranged(Gd["offsets"], Gd["members"], order)
    half = nb.groups_properties(ctx, Gd["d"], off, mem, Gd["phi"])
    assert _same_bytes(half, got[order]), _differences(half, got[order])


# ---- 4. validation on the device, error codes on the host ---------------------------------------------------------------
def test_bad_groups_do_not_touch_their_neighbours(nb, ctx, lattice):
    L = lattice
    offsets, members = L["offsets"].astype(np.int64), L["members"]
    sizes = np.diff(offsets)
    pick = lambda s: int(np.nonzero(sizes == s)[0][0])  # noqa: E731
    keep = [pick(3), pick(ref.S + 1), pick(2 * ref.C + 1), pick(5), pick(ref.C), pick(2)]
    lists = [members[offsets[g]:offsets[g + 1]].copy() for g in keep]
    clean_off, clean_mem = _rearranged(offsets, members, keep)
    clean = nb.groups_properties(ctx, L["d"], clean_off, clean_mem, L["phi_dev"])
    assert (clean["status"] == 0).all()
    # the same groups with bad ones between them: a small and a chunked group with a member = count, a small and a
    # chunked one with a member = -1, an empty group, and a group whose offsets run backwards
    def spoiled(g, value, at):
        x = members[offsets[g]:offsets[g + 1]].copy()
        x[at] = value
        return x
    rows = [lists[0], spoiled(pick(4), COUNT, 2), lists[1], spoiled(pick(2 * ref.C), COUNT, 2 * ref.C - 1), lists[2],
            spoiled(pick(6), -1, 0), lists[3], spoiled(pick(ref.C + 1), -1, ref.C), lists[4], np.zeros(0, np.int32), lists[5]]
    good_rows = [0, 2, 4, 6, 8, 10]
    mem = np.concatenate(rows).astype(np.int32)
    off = np.concatenate(([0], np.cumsum([len(x) for x in rows]))).astype(np.int32)
    # ... and offsets[g] > offsets[g + 1]: row 11 steps back by seven members; row 12 is then the three members from
    # there on, a legal group that overlaps the one at row 8
    off = np.concatenate((off, [off[-1] - 7, off[-1] - 4])).astype(np.int32)
    got = nb.groups_properties(ctx, L["d"], off, mem, L["phi_dev"])
    want, _ = ref.reference(L["fields"], off, mem, L["phi"])
    bad_rows = [1, 3, 5, 7, 9, 11]
    assert (want["status"][bad_rows] == 1).all() and (want["status"][good_rows + [12]] == 0).all()
    zero = np.zeros(1, ref.DTYPE)
    zero["status"] = 1
    for r in bad_rows:
        assert got[r:r + 1].tobytes() == zero.tobytes(), r
    assert _same_bytes(got[good_rows], clean), _differences(got[good_rows], clean)
    assert np.array_equal(got, want), _differences(got, want)


def test_host_error_codes(nb, ctx, lattice):
    L = lattice
    lib, E = ctx._lib, nb._lib
    s = L["d"].struct()
    out = nb.group_props_tensor(4, "cuda")
    off, mem = L["off_dev"].data_ptr(), L["mem_dev"].data_ptr()
    n_members = L["members"].size

    def call(ctx_h=ctx.handle, d=C.byref(s), offsets=off, members=mem, n_groups=4, n_mem=n_members, o=out.data_ptr()):
        return lib.nbody_hip_groups_properties(ctx_h, d, offsets, members, n_groups, n_mem, None, o)

    assert call() == 0
    assert call(ctx_h=None) == E.ERR_STATE
    assert call(d=None) == E.ERR_STATE
    assert call(offsets=None) == E.ERR_STATE
    assert call(members=None) == E.ERR_STATE
    assert call(o=None) == E.ERR_STATE
    null_arrays = nb._lib.ParticleDataStruct()
    null_arrays.count = COUNT
    assert call(d=C.byref(null_arrays)) == E.ERR_STATE
    assert call(n_groups=-1) == E.ERR_VALIDATION
    assert call(n_mem=-1) == E.ERR_VALIDATION
    assert call(n_mem=2 ** 31) == E.ERR_VALIDATION
    for bad in (0, 2 ** 30 + 1):
        t = L["d"].struct()
        t.count = bad
        assert call(d=C.byref(t)) == E.ERR_VALIDATION, bad
    ctx.synchronize()
    if torch.cuda.device_count() > 1:
        other = nb.Context(1)
        assert lib.nbody_hip_groups_properties(other.handle, C.byref(s), off, mem, 4, n_members, None,
                                               out.data_ptr()) == E.ERR_VALIDATION
        other.close()
    # the grid's call: no catalogue, no answer
    grid = nb.SpatialHashGrid(COUNT, 64.0, ctx)
    assert lib.nbody_hip_grid_groups_properties(grid._h, C.byref(s), None, out.data_ptr()) == E.ERR_STATE
    assert lib.nbody_hip_grid_groups_properties(None, C.byref(s), None, out.data_ptr()) == E.ERR_STATE
    with pytest.raises(nb.StateException, match="no group catalogue"):
        grid.groupProperties(L["d"])
    with pytest.raises(nb.ValidationException, match="phi"):
        nb.groups_properties(ctx, L["d"], L["off_dev"], L["mem_dev"], torch.zeros(5, device="cuda"))
    with pytest.raises(nb.ValidationException, match="192"):
        nb.groups_properties_into(ctx, L["d"], L["off_dev"], L["mem_dev"], nb.group_props_tensor(3, "cuda"))


def test_recorded_into_a_step_graph(nb, ctx, lattice):
    L = lattice
    want = nb.groups_properties(ctx, L["d"], L["off_dev"], L["mem_dev"], L["phi_dev"])  # (the workspace exists from here)
    out = nb.group_props_tensor(len(want), "cuda")
    with ctx.capture() as cap:
        nb.groups_properties_into(ctx, L["d"], L["off_dev"], L["mem_dev"], out, L["phi_dev"])
    cap.graph.launch()
    ctx.synchronize()
    assert _same_bytes(nb.group_props_array(out), want)


# ---- 5. the pass disturbs nothing ---------------------------------------------------------------------------------------
def test_the_next_force_call_is_left_alone(nb, ctx, general):
    Gd = general
    d, grid = Gd["d"], Gd["grid"]

    def forces():
        grid.computeForces(d, 0.4, 1.0, 0.01)
        ctx.synchronize()
        return np.stack([d.acc_x.cpu().numpy(), d.acc_y.cpu().numpy(), d.acc_z.cpu().numpy()])

    grid.build(d)
    cat = grid.findGroups(0.2, 1)
    before = forces()
    state = [getattr(d, k).clone() for k in FIELDS7]
    props = cat.properties(d, Gd["phi"], ctx)
    by_grid = grid.groupProperties(d, Gd["phi"])
    assert _same_bytes(props, by_grid) and _same_bytes(props, Gd["got"])
    for k, t in zip(FIELDS7, state):
        assert torch.equal(getattr(d, k), t), k
    after = forces()
    assert np.array_equal(before.view(np.uint32), after.view(np.uint32))


@pytest.mark.parametrize("method", ["DIRECT_N2", "BARNES_HUT", "SPATIAL_HASH"])
def test_particle_system_update_is_left_alone(nb, ctx, method):
    n = 3000
    a = nb.ic.plummer(n, seed=11)
    ic = {k: np.asarray(a[k], np.float32) for k in FIELDS7}

    def system():
        ps = nb.ParticleSystem()
        ps.initialize(nb.SimulationConfig(particle_count=n, force_method=getattr(nb.ForceMethod, method)), ic)
        return ps

    def state(ps):
        d = ps.d_particles_
        return np.stack([getattr(d, k).cpu().numpy() for k in FIELDS7 + ("acc_x", "acc_y", "acc_z")]).view(np.uint32)

    plain, probed = system(), system()
    cat = probed.findGroups(0.15, 1)
    props = probed.groupProperties(cat, with_potential=True)
    bare = probed.groupProperties(cat)
    for ps in (plain, probed):
        ps.update(ps.getTimeStep())
    assert np.array_equal(state(plain), state(probed))
    # with_potential: phi is the method's own per-body potential, the rest is the same pass
    assert (props["status"] == 0).all() and props["n"].sum() == n
    for k in ("mass", "com", "vel", "ang_mom", "kinetic", "inertia", "r_max", "r_max_body", "n", "label"):
        assert np.array_equal(props[k], bare[k]), k
    assert (bare["phi_min_body"] == -1).all() and (props["phi_min_body"] >= 0).all()
    members, offsets = cat.members.cpu().numpy(), cat.offsets.cpu().numpy()
    big = int(np.argmax(props["n"]))
    assert props["phi_min_body"][big] in members[offsets[big]:offsets[big + 1]]
    assert props["phi_min"][big] < 0 and props["potential"][big] < 0
    # the potential-minimum centre of the Plummer sphere's main group lies near its centre of mass
    p = np.array([ic[k][props["phi_min_body"][big]] for k in ref.POS])
    assert np.linalg.norm(p - props["com"][big]) < 0.5 * props["r_max"][big]

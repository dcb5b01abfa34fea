"""The radial profiles without a GPU: the CPU checks of csrc/radial_plan.h (make radial_plan_check) and of the arithmetic
of csrc/radial_common.h (make radial_check), both under AddressSanitizer and UBSan; what the sources promise (no HIP in
the plan, no fused product, no floating-point atomic, no inline assembly in the kernels); the struct layouts; and the test
reference of tests/radial_ref.py itself: against a plain-Python loop, on bad catalogues, and the cap on ambiguous mass
cuts on the general data of the GPU test."""
import os
import re
import subprocess

import numpy as np

import group_props_ref as gp
import radial_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "n-body_amd", "csrc")


def code(name):
    return re.sub(r"//.*", "", open(os.path.join(CSRC, name)).read())


def _check_program(target, sources, flags=()):
    r = subprocess.run(["make", "-C", CSRC, target], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert target + ": ok" in r.stdout and "FAIL" not in r.stdout
    mk = open(os.path.join(CSRC, "Makefile")).read()
    rule = mk[mk.index("../lib/" + target + ":"):].split("\n\n")[0]
    assert "-fsanitize=address,undefined -fno-sanitize-recover=all" in rule and "$(CXX)" in rule
    for word in tuple(sources) + tuple(flags):
        assert word in rule, word
    assert target in re.search(r"^\.PHONY:(.*)$", mk, re.M).group(1)
    assert "../lib/" + target in mk[mk.index("\nclean:"):]
    assert re.search(r"^int main\(", code(target + ".cpp"), re.M)
    return mk


def test_plan_check_builds_and_passes():
    _check_program("radial_plan_check", ("radial_plan.h", "group_props_plan.h"))
    plan = code("radial_plan.h")
    for word in ("hip_runtime", "hipMalloc", "hipStream", "hipLaunch", "threadIdx", "__global__", "common.h", "nbody_hip", "<vector>"):
        assert word not in plan, word
    assert int(re.search(r"constexpr int kRadialMaxCuts = (\d+);", plan).group(1)) == ref.MAX_CUTS
    header = open(os.path.join(ROOT, "include", "nbody_hip_radial.h")).read()
    assert f"#define NBODY_HIP_RADIAL_MAX_CUTS {ref.MAX_CUTS}" in header
    for name, value in (("MASS", ref.MASS), ("NUMBER", ref.NUMBER), ("RADIUS", ref.RADIUS)):
        assert re.search(rf"#define NBODY_HIP_RADIAL_{name} {value}\b", header)
    # the model states the two sizes of the forms, and they are the group properties'
    assert f"n <= {ref.S}:" in header and f"n > {ref.S}:" in header and f"chunks of {ref.C:,} ranks" in header


def test_arithmetic_check_builds_and_passes():
    mk = _check_program("radial_check", ("radial_common.h",), ("-ffp-contract=off",))
    assert re.search(r"^radial_profile\.o: CXXFLAGS \+= -ffp-contract=off$", mk, re.M)
    assert "radial_profile.hip" in re.search(r"^SRCS\s*:=(.*)$", mk, re.M).group(1)
    kernels = code("radial_profile.hip")
    assert '#include "radial_common.h"' in kernels and '#include "radial_plan.h"' in kernels
    for word in ("asm", "atomicAdd(", "unsafeAtomicAdd", "__fma", "fma("):
        assert word not in kernels, word  # no inline assembly, no floating-point atomics, no fused products
    assert "kGroupSmall = " not in kernels and "kGroupChunk = " not in kernels
    common = code("radial_common.h")
    assert "fma" not in common and "hip_runtime" not in common


def test_struct_layouts_in_the_header(nb):
    header = open(os.path.join(ROOT, "include", "nbody_hip_radial.h")).read()
    for struct, dtype, twin, ctype in (("nbody_hip_radial_group", ref.GROUP_DTYPE, nb.RADIAL_GROUP_DTYPE, nb._lib.RadialGroupStruct),
                                       ("nbody_hip_radial_shell", ref.SHELL_DTYPE, nb.RADIAL_SHELL_DTYPE, nb._lib.RadialShellStruct)):
        body = header[header.index("typedef struct " + struct + " {"):header.index("} " + struct + ";")]
        names = re.findall(r"^\s+(?:double|int)\s+(\w+)", body, re.M)
        assert tuple(names) == dtype.names == twin.names and dtype == twin
        for name, _ in ctype._fields_:
            assert getattr(ctype, name).offset == dtype.fields[name][1], name
    assert nb.RADIAL_MODES == ref.MODES and nb.RADIAL_MAX_CUTS == ref.MAX_CUTS


def test_reference_against_a_plain_python_loop():
    """the lattices and the numpy restatement, n <= 9: every group against nested Python loops, exactly"""
    sizes = [1, 2, 3, 4, 5, 6, 7, 8, 9, 9, 2, 1]
    rng = np.random.default_rng(0)
    for seed in range(4):
        for axis in (False, True):
            fields, offsets, members, centres, vels = ref.lattice(sizes, 80, axis=axis, seed=seed)
            assert len(set(members.tolist())) == members.size == sum(sizes)
            if seed == 3:  # inexact data through the same two restatements
                for k in fields:
                    fields[k] = (fields[k] + rng.normal(0, 0.3, 80)).astype(np.float32)
            for mode, cuts in ref.LATTICE_CUTS.items():
                got = ref.reference(fields, offsets, members, centres, cuts, mode, vels)
                want = ref.plain_python(fields, offsets, members, centres, cuts, mode, vels)
                assert (got["groups"]["status"] == 0).all() and not got["groups"]["reserved"].any()
                for g, row in enumerate(want):
                    o0, o1 = offsets[g], offsets[g + 1]
                    assert got["sorted_members"][o0:o1].tolist() == row["order"], (seed, mode, g)
                    assert np.array_equal(got["sorted_q"][o0:o1], np.array(row["q"], np.float32))
                    assert got["groups"][g]["mass"] == row["E"][-1] and got["groups"][g]["n"] == sizes[g]
                    assert got["groups"][g]["r_max"] == np.sqrt(np.float64(row["q"][-1]))
                    sh = got["shells"][g]
                    assert sh["enclosed_count"].tolist() == row["K"]
                    assert sh["count"].tolist() == np.diff([0] + row["K"]).tolist()
                    assert np.array_equal(sh["radius"], np.array(row["radius"]))
                    assert np.array_equal(sh["enclosed_mass"], np.array([row["E"][K - 1] if K else 0.0 for K in row["K"]]))
                    for i, name in enumerate(ref.SUMS):
                        assert np.array_equal(sh[name], np.array([four[i] for four in row["sums"]])), (seed, mode, g, name)
                    assert not sh["reserved"].any()


def test_the_lattices_hold_their_recipe():
    fields, offsets, members, centres, vels = ref.lattice(ref.lattice_sizes(60, 60), 80000)
    sizes = np.diff(offsets)
    for s in ref.LADDER + [64 * ref.C + 3]:
        assert (sizes == s).any(), s
    assert all(np.abs(fields[k][members]).max() <= 512 for k in ref.POS)
    got = {mode: ref.reference(fields, offsets, members, centres, cuts, mode, vels) for mode, cuts in ref.LATTICE_CUTS.items()}
    mass, radius = got["mass"], got["radius"]
    K, n = mass["shells"]["enclosed_count"], mass["groups"]["n"]
    assert (mass["groups"]["status"] == 0).all() and np.array_equal(n, sizes)
    assert (K[:, 0] == 1).any() and (K[:, -1] == n).all() and (mass["shells"]["count"] == 0).any()
    g2c = int(np.nonzero(sizes == 2 * ref.C)[0][0])
    assert K[g2c, 2] == ref.C  # half the mass of the group of 2 C equal masses: a cut exactly at rank C
    assert np.array_equal(mass["shells"]["enclosed_mass"][:, -1], mass["groups"]["mass"])
    # many equal q, across rank C too; radius 0 holds only members on the centre, +inf everybody
    big = int(np.argmax(sizes))
    q = mass["sorted_q"][offsets[big]:offsets[big + 1]]
    assert np.unique(q).size < 200 and q[ref.C - 1] == q[ref.C] and (q.astype(np.float64) < 2 ** 24).all()
    Kr = radius["shells"]["enclosed_count"]
    assert (Kr[:, 0] > 0).any() and (Kr[:, 0] == 0).any() and (Kr[:, -1] == sizes).all()
    for g in np.nonzero(Kr[:, 0] > 0)[0][:20]:
        assert not mass["sorted_q"][offsets[g]:offsets[g] + Kr[g, 0]].any()
    # every sum is exact: the masses are multiples of 2^-4 below 2^24
    assert (mass["groups"]["mass"] * 16 == np.round(mass["groups"]["mass"] * 16)).all() and mass["groups"]["mass"].max() < 2 ** 24
    # the axis lattice: every term is an integer times a power of two
    fields, offsets, members, centres, vels = ref.lattice(ref.axis_sizes(40), 20000, axis=True, seed=2)
    ax = ref.reference(fields, offsets, members, centres, ref.AXIS_CUTS["number"], "number", vels)
    for name in ref.SUMS:
        assert (ax["shells"][name] * 16 == np.round(ax["shells"][name] * 16)).all(), name
    for g, st in ax["state"].items():
        assert (st["terms"] * 16 == np.round(st["terms"] * 16)).all()


def test_the_model_orders_are_sums():
    """the two written-out orders against plain sums on exact data, and against long double on inexact data"""
    rng = np.random.default_rng(3)
    for n in (1, 2, 31, 32, 33, 255, 256, 257, 1023, 1024, 1025, 2048, 2049, 5000, 64 * 1024 + 3):
        m = 2.0 ** rng.integers(-4, 4, n)
        assert np.array_equal(ref.enclosed_model(m), np.cumsum(m)), n
        assert ref.ordered_sum(m) == m.sum(), n
        x = rng.uniform(0.5, 1.5, n)
        wide = np.cumsum(x.astype(np.longdouble))
        E = ref.enclosed_model(x)
        assert (np.abs(E - wide) <= (np.arange(n) + ref.K_SUM) * ref.U * wide).all(), n
        assert abs(ref.ordered_sum(x) - wide[-1]) <= (n + ref.K_SUM) * ref.U * wide[-1], n


def test_reference_marks_bad_catalogues():
    fields, offsets, members, centres, vels = ref.lattice([3, 4, 5, 2], 30)
    cuts = [0.5, 1.0]
    clean = ref.reference(fields, offsets, members, centres, cuts, "mass", vels)
    assert (clean["groups"]["status"] == 0).all() and (clean["sorted_members"] >= 0).all()
    zero_rows = np.zeros(2, ref.SHELL_DTYPE).tobytes()

    def bad_group(got, g, status):
        want = np.zeros(1, ref.GROUP_DTYPE)
        want["status"] = status
        assert got["groups"][g:g + 1].tobytes() == want.tobytes() and got["shells"][g].tobytes() == zero_rows
        assert (got["sorted_members"][offsets[g]:offsets[g + 1]] == -1).all()
        assert not got["sorted_q"][offsets[g]:offsets[g + 1]].any()

    def untouched(got, rows, clean_rows=None):
        for g, h in zip(rows, clean_rows or rows):
            assert got["groups"][g:g + 1].tobytes() == clean["groups"][h:h + 1].tobytes()
            assert got["shells"][g].tobytes() == clean["shells"][h].tobytes()

    # offsets out of order anywhere: every group of the call
    for off in ([0, 3, 7, 12, 11], [0, 7, 3, 12, 14], [-1, 3, 7, 12, 14], [0, 3, 7, 12, 15]):
        got = ref.reference(fields, np.array(off, np.int32), members, centres, cuts, "mass", vels)
        assert (got["groups"]["status"] == 1).all() and not got["groups"]["n"].any()
        assert got["shells"].tobytes() == np.zeros((4, 2), ref.SHELL_DTYPE).tobytes() and (got["sorted_members"] == -1).all()
    # an empty group alone (the catalogue: groups 0, 1, an empty one, 2, 3)
    off5 = np.array([0, 3, 7, 7, 12, 14], np.int32)
    c5, v5 = np.insert(centres, 2, 0.0, axis=0), np.insert(vels, 2, 0.0, axis=0)
    got = ref.reference(fields, off5, members, c5, cuts, "mass", v5)
    assert got["groups"]["status"].tolist() == [0, 0, 1, 0, 0]
    untouched(got, [0, 1, 3, 4], [0, 1, 2, 3])
    # a bad member index alone
    for value in (30, -1):
        mem = members.copy()
        mem[4] = value
        got = ref.reference(fields, offsets, mem, centres, cuts, "mass", vels)
        assert got["groups"]["status"].tolist() == [0, 1, 0, 0]
        bad_group(got, 1, 1)
        untouched(got, [0, 2, 3])
    # a NaN position alone: status 2; with a bad index too, status 1 wins
    f = {k: a.copy() for k, a in fields.items()}
    f["pos_y"][members[8]] = np.nan
    got = ref.reference(f, offsets, members, centres, cuts, "mass", vels)
    assert got["groups"]["status"].tolist() == [0, 0, 2, 0]
    bad_group(got, 2, 2)
    untouched(got, [0, 1, 3])
    mem = members.copy()
    mem[9] = 99
    assert ref.reference(f, offsets, mem, centres, cuts, "mass", vels)["groups"]["status"].tolist() == [0, 0, 1, 0]
    # a far member: q overflows to +inf and sorts last
    f = {k: a.copy() for k, a in fields.items()}
    f["pos_x"][members[0]] = 3e19
    got = ref.reference(f, offsets, members, centres, cuts, "mass", vels)
    assert got["groups"]["status"][0] == 0 and np.isinf(got["groups"]["r_max"][0]) and got["sorted_members"][2] == members[0]
    # positions of no group stay -1
    got = ref.reference(fields, offsets[1:], members, centres[1:], cuts, "mass", vels[1:])
    assert (got["sorted_members"][:3] == -1).all() and (got["sorted_members"][3:] >= 0).all()
    untouched(got, [0, 1, 2], [1, 2, 3])
    # the cuts the host refuses
    assert ref.check_cuts([0.5, 0.5], ref.MASS) == 4 and ref.check_cuts([0.0], ref.MASS) == 3 and ref.check_cuts([0.0], ref.RADIUS) == 0
    assert ref.check_cuts([], ref.MASS) == 1 and ref.check_cuts([0.5], 7) == 2 and ref.check_cuts([float("nan")], ref.RADIUS) == 3


def general_catalogues(nb):
    """the two catalogues of the general-data test, on the CPU: friends-of-friends of the Plummer sphere in its
    background, and an arbitrary partition of the same bodies into the size ladder; centres and bulk velocities are the
    fp64 com and vel of the group properties' reference"""
    import groups_ref
    fields = gp.general_fields(nb.ic)
    pos = np.stack([fields[k] for k in ref.POS], 1)
    offsets, members = groups_ref.catalogue(groups_ref.fof_labels(pos, np.float32(gp.LINK)), 1)
    out = {}
    for name, (off, mem) in (("fof", (offsets, members)), ("partition", ref.partition(len(pos)))):
        props, _ = gp.reference(fields, off, mem)
        out[name] = dict(offsets=off, members=mem, centres=props["com"].copy(), vels=props["vel"].copy())
    return fields, out


def test_general_data_keeps_the_ambiguous_cuts_under_their_cap(nb):
    fields, cats = general_catalogues(nb)
    pairs = 0
    for name, cat in cats.items():
        got = ref.reference(fields, cat["offsets"], cat["members"], cat["centres"], ref.FRACTIONS, "mass", cat["vels"])
        n = got["groups"]["n"]
        assert (got["groups"]["status"] == 0).all() and n.max() <= ref.N_MAX
        if name == "fof":
            assert (n == 1).sum() > 100 and ((n > 1) & (n <= ref.S)).sum() > 100 and n.max() > 2 * ref.C
        else:
            for s in ref.LADDER:
                assert (n == s).any(), s
        wide = ref.wide(got["state"], got["shells"]["enclosed_count"], len(ref.FRACTIONS))
        ambiguous = 0
        for g, w in wide.items():
            for c, f in enumerate(ref.FRACTIONS):
                ok, amb = ref.mass_cut_checks(w["cum"], int(n[g]), f, int(got["shells"]["enclosed_count"][g, c]))
                assert ok, (name, g, c)  # the reference's own K passes its own test
                ambiguous += amb
        total = len(wide) * len(ref.FRACTIONS)
        pairs += total
        print(f"{name}: {ambiguous} ambiguous of {total} (group, cut) pairs")
        assert ambiguous <= ref.AMBIGUITY_CAP * total, (name, ambiguous, total)
        # the fp64 model lies within the derived bound of the wide restatement
        for g, w in wide.items():
            sh = got["shells"][g]
            cnt, K = sh["count"].astype(np.float64), sh["enclosed_count"].astype(np.float64)
            assert (np.abs(sh["enclosed_mass"] - w["enclosed"]) <= (K + ref.K_SUM) * ref.U * w["enclosed"]).all(), (name, g)
            for i, k in enumerate(ref.SUMS):
                assert (np.abs(sh[k] - w["sums"][:, i]) <= (cnt + ref.K_SUM) * ref.U * w["abs"][:, i]).all(), (name, g, k)
    print(f"{pairs} pairs in all")

"""The group properties without a GPU: the CPU check of csrc/group_props_plan.h (make group_props_plan_check: the chunks of
a group, the chunk bound the launches are sized from, the launch sizes, the workspace table -- under AddressSanitizer and
UBSan), the CPU check of the arithmetic of csrc/group_props_common.h in the summation order of the model (make
group_props_check: exact lattice, long double restatement, tie rules), and the test reference of
tests/group_props_ref.py itself: its lattice recipe and its numpy restatement against a plain-Python triple loop."""
import os
import re
import subprocess

import numpy as np

import group_props_ref as ref

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
    _check_program("group_props_plan_check", ("group_props_plan.h",))
    plan = code("group_props_plan.h")
    for word in ("hip_runtime", "hipMalloc", "hipStream", "hipLaunch", "threadIdx", "__global__", "common.h", "nbody_hip", "<vector>"):
        assert word not in plan, word
    # the sizes the tests mirror are the header's
    assert int(re.search(r"constexpr int kGroupSmall = (\d+);", plan).group(1)) == ref.S
    assert int(re.search(r"constexpr int kGroupChunk = (\d+);", plan).group(1)) == ref.C
    r = subprocess.run([os.path.join(ROOT, "n-body_amd", "lib", "group_props_plan_check"), "sizes"], capture_output=True, text=True)
    assert r.stdout.split()[:4] == ["S", str(ref.S), "C", str(ref.C)]
    # ... and the model in the public header states the same two numbers
    header = open(os.path.join(ROOT, "include", "nbody_hip_group_props.h")).read()
    assert f"n <= {ref.S}:" in header and f"n > {ref.S}:" in header and f"chunks of {ref.C:,} positions" in header


def test_arithmetic_check_builds_and_passes():
    mk = _check_program("group_props_check", ("group_props_common.h", "group_props_plan.h"), ("-ffp-contract=off",))
    # the kernels are built without contraction too, and take sizes and arithmetic from the two headers alone
    assert re.search(r"^group_props\.o: CXXFLAGS \+= -ffp-contract=off$", mk, re.M)
    kernels = code("group_props.hip")
    assert '#include "group_props_common.h"' in kernels and '#include "group_props_plan.h"' in kernels
    for word in ("asm", "atomicAdd(", "unsafeAtomicAdd", "__fma", "fma("):
        assert word not in kernels, word  # no inline assembly, no floating-point atomics, no fused products
    assert kernels.count("atomicOr(") == 1 and "kGroupSmall = " not in kernels and "kGroupChunk = " not in kernels
    common = code("group_props_common.h")
    assert "fma" not in common and "hip_runtime" not in common


def test_struct_layout_in_the_header():
    header = open(os.path.join(ROOT, "include", "nbody_hip_group_props.h")).read()
    body = header[header.index("typedef struct nbody_hip_group_props {"):header.index("} nbody_hip_group_props;")]
    names = re.findall(r"^\s+(?:double|int)\s+(\w+)", body, re.M)
    assert tuple(names) == ref.DTYPE.names


def test_reference_against_a_plain_python_loop():
    """the lattice recipe and the numpy restatement, n <= 9: every group against three nested Python loops, exactly"""
    sizes = [1, 2, 3, 4, 5, 6, 7, 8, 9, 9, 2, 1]
    for seed in range(5):
        fields, offsets, members, phi = ref.lattice(sizes, 80, seed=seed)
        assert members[-1] == 79 and len(set(members.tolist())) == members.size == sum(sizes)
        for use_phi in (phi, None):
            got, _ = ref.reference(fields, offsets, members, use_phi)
            want = ref.plain_python(fields, offsets, members, use_phi)
            for g, row in enumerate(want):
                for k, v in row.items():
                    assert np.array_equal(np.asarray(v, dtype=got[k].dtype), got[k][g]), (seed, g, k, v, got[k][g])
            assert not got["reserved"].any()
        # the recipe: the centre of mass is the integer centre exactly, mirrored pairs tie in r_max, phi ties exist
        got, _ = ref.reference(fields, offsets, members, phi)
        assert np.array_equal(got["com"], np.round(got["com"])) and np.array_equal(got["vel"], np.round(got["vel"]))
        assert (np.abs(got["com"]) <= 512).all() and (np.abs(got["vel"]) <= 16).all()
        for g in range(len(sizes)):
            mem = members[offsets[g]:offsets[g + 1]]
            if len(mem) >= 2:  # the winner of a tie is the lower index of a mirrored pair (or of several)
                x = np.stack([fields[k][mem].astype(np.float64) for k in ref.POS], 1) - got["com"][g]
                r2 = (x * x).sum(1)
                tied = mem[r2 == r2.max()]
                assert len(tied) >= 2 and got["r_max_body"][g] == tied.min()
    # ties in phi: some small group has its minimum more than once
    fields, offsets, members, phi = ref.lattice(ref.lattice_sizes(50, 50), 80000)
    got, _ = ref.reference(fields, offsets, members, phi)
    ties = 0
    for g in np.nonzero(got["n"] <= 6)[0]:
        mem = members[offsets[g]:offsets[g + 1]]
        hit = mem[phi[mem] == got["phi_min"][g]]
        assert got["phi_min_body"][g] == hit.min()
        ties += len(hit) > 1
    assert ties >= 5
    # every term of the big group is far below 2^53 halves: the sums are exact in any order
    big = int(np.argmax(got["n"]))
    assert got["n"][big] == 64 * ref.C + 3 and np.abs(got["inertia"][big]).max() < 2.0 ** 40
    assert (got["inertia"] * 2 == np.round(got["inertia"] * 2)).all() and (got["potential"] * 32 == np.round(got["potential"] * 32)).all()


def test_reference_marks_bad_groups():
    fields, offsets, members, phi = ref.lattice([3, 4, 5], 30)
    members = members.copy()
    members[4] = 30  # = count, in group 1
    off = np.array([0, 3, 7, 7, 12, 9], np.int32)  # group 2 empty, group 4 runs backwards
    got, _ = ref.reference(fields, off, members, phi)
    assert got["status"].tolist() == [0, 1, 1, 0, 1] and got["n"].tolist() == [3, 0, 0, 5, 0]
    zero = np.zeros(1, ref.DTYPE)
    zero["status"] = 1
    for g in (1, 2, 4):
        assert got[g:g + 1].tobytes() == zero.tobytes()
    members[4] = -1
    assert ref.reference(fields, off, members, phi)[0]["status"].tolist() == [0, 1, 1, 0, 1]


def test_general_data_keeps_the_r_max_exclusion_under_its_cap(nb):
    """the reference alone, on the data of the GPU test with friends-of-friends restated on the CPU: the groups in which
    r_max_body cannot be asserted (runner-up within twice the bound) stay under 1 %"""
    import groups_ref
    fields = ref.general_fields(nb.ic)
    pos = np.stack([fields[k] for k in ref.POS], 1)
    labels = groups_ref.fof_labels(pos, np.float32(ref.LINK))
    offsets, members = groups_ref.catalogue(labels, 1)
    phi = -np.random.default_rng(1).uniform(0.1, 1.0, len(pos)).astype(np.float32)
    want, aux = ref.reference(fields, offsets, members, phi, wide=True)
    bound = ref.bounds(want, aux)
    decided = ref.r_max_decided(want, aux, bound)
    assert (~decided).sum() <= ref.R_MAX_UNDECIDED_CAP * decided.size, ((~decided).sum(), decided.size)
    n = want["n"]
    assert (n == 1).sum() > 100 and ((n > 1) & (n <= ref.S)).sum() > 100 and n.max() > 2 * ref.C and n.max() <= ref.N_MAX
    # the bounds are bounds: the fp64 restatement (another order, fp64 sums) lies within them of the wide one
    narrow, _ = ref.reference(fields, offsets, members, phi)
    for k, b in bound.items():
        assert (np.abs(narrow[k] - want[k]) <= b).all(), k

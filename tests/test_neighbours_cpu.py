"""The k nearest neighbours, the local density and the density centre without a GPU: the restatement of
tests/neighbours_ref.py against scipy's kd-tree and against plain loops, and the CPU check of the shared arithmetic
csrc/neighbours_common.h (make neighbours_check: the insertion against a sort, the K choice, the argument rule, the status
rule at its edge, the density-centre order -- under AddressSanitizer and UBSan, run as a program)."""
import os
import re
import subprocess

import numpy as np
from scipy.spatial import cKDTree

import neighbours_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "n-body_amd", "csrc")
U = 2.0 ** -24


def code(name):
    return re.sub(r"//.*", "", open(os.path.join(CSRC, name)).read())


def test_restatement_against_a_kd_tree():
    """2,000 uniform bodies, no cell restriction: the same neighbour sets as cKDTree.query on the widened coordinates, and
    every fp32 d2 within 5 u of the fp64 one (three differences, their squares and the two additions of the chain)"""
    pos = np.random.default_rng(21).random((2000, 3)).astype(np.float32)
    tree = cKDTree(pos.astype(np.float64))
    for k in (1, 6, 32):
        index, dist2 = ref.topk(pos, k)
        dist, nn = tree.query(pos.astype(np.float64), k + 1)
        assert (nn[:, 0] == np.arange(2000)).all()  # distinct bodies: each is its own nearest
        assert np.array_equal(np.sort(index, 1), np.sort(nn[:, 1:], 1))
        d = pos[index].astype(np.float64) - pos[:, None, :].astype(np.float64)
        exact = (d * d).sum(2)
        assert (np.abs(dist2.astype(np.float64) - exact) <= 5 * U * exact).all()
        assert (np.diff(dist2, axis=1) >= 0).all() and (index >= 0).all()
        status = ref.status_of(index, dist2, 10.0, (1, 1, 1))
        assert (status == 0).all()


def test_restatement_in_small_cases():
    # ties go to the lowest index; a coincident body is a neighbour; the body itself is skipped by position
    pos = np.array([[0, 0, 0], [1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, 0, 0], [np.nan, 0, 0]], np.float32)
    index, dist2 = ref.topk(pos, 4)
    assert index[0].tolist() == [4, 1, 2, 3] and dist2[0].tolist() == [0.0, 1.0, 1.0, 1.0]
    assert index[4].tolist() == [0, 1, 2, 3]
    assert index[5].tolist() == [-1] * 4 and np.isinf(dist2[5]).all()  # every d2 of the NaN body is a NaN
    assert 5 not in index
    index, dist2 = ref.topk(pos[:3], 4)
    assert index[0].tolist() == [1, 2, -1, -1] and dist2[0].tolist()[:2] == [1.0, 1.0] and np.isinf(dist2[0, 2:]).all()
    # the status rule at the edge, and the whole-grid exemption
    one = np.float32(1.0)
    idx = np.zeros((4, 1), np.int32)
    d2 = np.array([[np.nextafter(one, np.float32(0))], [one], [np.nextafter(one, np.float32(2))], [0.0]], np.float32)
    assert ref.status_of(idx, d2, 1.0, (3, 1, 1)).tolist() == [0, 1, 1, 3]
    assert ref.status_of(idx, d2, 1.0, (2, 2, 2)).tolist() == [0, 0, 0, 3]
    assert ref.status_of(np.full((1, 1), -1, np.int32), np.full((1, 1), np.inf, np.float32), 1.0, (2, 2, 2)).tolist() == [2]
    # the density: a known answer (k = 3: the two nearer masses over the sphere of the third) and k = 1
    index = np.array([[1, 2, 3]], np.int32)
    dist2 = np.array([[1.0, 2.0, 4.0]], np.float32)
    mass = np.array([9.0, 2.0, 3.0, 5.0], np.float32)
    rho = ref.density_of(index, dist2, np.array([0]), mass)
    assert rho[0] == 5.0 / (ref.SPHERE * 8.0)
    assert ref.density_of(index[:, :1], dist2[:, :1], np.array([0]), mass)[0] == 0.0
    assert ref.density_of(index, dist2, np.array([3]), mass)[0] == 0.0 and ref.density_of(index, dist2, np.array([2]), mass)[0] == 0.0
    assert ref.SPHERE == 4.0 * np.pi / 3.0
    # the cell restriction: bodies two cells apart are no candidates
    pos = np.array([[0.5, 0.5, 0.5], [1.5, 0.5, 0.5], [2.5, 0.5, 0.5]], np.float32)
    index, _ = ref.topk(pos, 2, np.array([0, 1, 2]), (3, 1, 1))
    assert index.tolist() == [[1, -1], [0, 2], [1, -1]]


def test_ordered_sum_against_plain_loops():
    rng = np.random.default_rng(22)
    for n in (0, 1, 2, 31, 32):
        t = rng.normal(size=n)
        total = 0.0
        for v in t:
            total = total + float(v)
        assert ref.ordered_sum(t) == total
    for n in (33, 64, 255, 256, 257, 1023, 1024, 1025, 2500, 65 * 1024 + 7):
        t = rng.normal(size=n) * 10.0 ** rng.integers(-3, 4, n)
        chunks = []
        for base in range(0, n, 1024):
            s = [0.0] * 256
            for j in range(4):
                for lane in range(256):
                    p = base + 256 * j + lane
                    if p < min(base + 1024, n):
                        s[lane] = s[lane] + float(t[p])
            for w in range(4):
                off = 32
                while off:
                    for lane in range(off):
                        s[64 * w + lane] = s[64 * w + lane] + s[64 * w + lane + off]
                    off //= 2
            chunks.append(((s[0] + s[64]) + s[128]) + s[192])
        c = [0.0] * 64
        for i, v in enumerate(chunks):
            c[i % 64] = c[i % 64] + v
        off = 32
        while off:
            for lane in range(off):
                c[lane] = c[lane] + c[lane + off]
            off //= 2
        assert ref.ordered_sum(t) == c[0], n
    # integers: exact in any order
    t = rng.integers(-1000, 1000, 70000).astype(np.float64)
    assert ref.ordered_sum(t) == t.sum()


def test_check_program_builds_and_passes():
    r = subprocess.run(["make", "-C", CSRC, "neighbours_check"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "neighbours_check: ok" in r.stdout and "FAIL" not in r.stdout
    mk = open(os.path.join(CSRC, "Makefile")).read()
    rule = mk[mk.index("../lib/neighbours_check:"):].split("\n\n")[0]
    assert "-fsanitize=address,undefined -fno-sanitize-recover=all" in rule and "$(CXX)" in rule
    for word in ("neighbours_common.h", "-ffp-contract=off"):
        assert word in rule, word
    assert "neighbours_check" in re.search(r"^\.PHONY:(.*)$", mk, re.M).group(1)
    assert "../lib/neighbours_check" in mk[mk.index("\nclean:"):]
    assert re.search(r"^int main\(", code("neighbours_check.cpp"), re.M)
    # the density centre is built without contraction, the shared header is free of HIP, and the kernels take their
    # arithmetic from it: no atomics on floats, no LDS, no cross-lane step, no inline assembly in the search
    assert re.search(r"^density_centre\.o: CXXFLAGS \+= -ffp-contract=off$", mk, re.M)
    common = code("neighbours_common.h")
    for word in ("hip_runtime", "fma", "__shfl", "atomic"):
        assert word not in common, word
    search = code("grid_neighbours.inc")
    assert '#include "neighbours_common.h"' in search
    for word in ("asm", "atomic", "__shared__", "__shfl", "__syncthreads", "__ballot"):
        assert word not in search, word
    centre = code("density_centre.hip")
    for word in ("asm", "atomicAdd(", "unsafeAtomicAdd", "fma"):
        assert word not in centre, word
    assert centre.count("atomicOr(") == 1


def test_density_centre_restatement_against_the_shared_header():
    """the numpy restatement and the C++ header, run on the CPU in the model's order over the same seeded sets: bitwise"""
    exe = os.path.join(ROOT, "n-body_amd", "lib", "neighbours_check")
    if not os.path.exists(exe):
        subprocess.run(["make", "-C", CSRC, "../lib/neighbours_check"], check=True, capture_output=True, timeout=600)
    r = subprocess.run([exe, "cases"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = r.stdout.splitlines()
    assert lines[0].split() == ["sizes", "S", str(ref.S), "C", str(ref.C), "T", str(ref.T)]
    header = open(os.path.join(ROOT, "include", "nbody_hip_neighbours.h")).read()
    assert f"n <= {ref.S}:" in header and f"n > {ref.S}:" in header and f"chunks of {ref.C:,} positions" in header
    assert f"#define NBODY_HIP_SPHERE_4PI_3 {ref.SPHERE!r}" in header
    seen = []
    for line in lines[1:]:
        w = line.split()
        assert w[0] == "centre"
        n = int(w[1])
        want = [float.fromhex(v) for v in w[2:]]
        rho, pos = ref.seeded_set(n)
        got = ref.density_centre(pos, rho)
        assert [*got["centre"], got["core_radius"], got["rho_sum"], got["rho2_sum"]] == want, n
        assert got["n"] == n and got["status"] == 0
        seen.append(n)
    assert {1, 32, 33, 1024, 1025, 65537} <= set(seen)
    # members: a bad index, the empty weight
    rho, pos = ref.seeded_set(50)
    assert ref.density_centre(pos, rho, [0, 50])["status"] == 1 and ref.density_centre(pos, rho, [-1])["status"] == 1
    z = ref.density_centre(pos, np.zeros(50), np.arange(40))
    assert z["n"] == 40 and z["status"] == 0 and not z["centre"].any() and z["core_radius"] == 0 and z["rho_sum"] == 0
    sub = ref.density_centre(pos, rho, np.arange(10, 20))
    whole = ref.density_centre(pos[10:20], rho[10:20])
    assert sub == whole


def test_struct_layout_in_the_header():
    header = open(os.path.join(ROOT, "include", "nbody_hip_neighbours.h")).read()
    body = header[header.index("typedef struct nbody_hip_density_centre_t {"):header.index("} nbody_hip_density_centre_t;")]
    names = re.findall(r"^\s+(?:double|int)\s+(\w+)", body, re.M)
    assert tuple(names) == ref.DTYPE.names

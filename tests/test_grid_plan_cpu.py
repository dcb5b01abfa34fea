"""The host decisions of the spatial hash without a GPU: the CPU check of csrc/grid_plan.h (make grid_plan_check: the force
plan against a restatement of the three if-chains and of launch_cell_forces it replaces, the start-array plan against the
block of the build it replaces, the grid record, key bits and size functions against their former expressions, the array
replacement over the grid's tables under a failing allocator -- under AddressSanitizer and UBSan), and that
spatial_hash.hip takes those decisions from that one header."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "n-body_amd", "csrc")


def code(name):
    return re.sub(r"//.*", "", open(os.path.join(CSRC, name)).read())


def test_grid_plan_check_builds_and_passes():
    r = subprocess.run(["make", "-C", CSRC, "grid_plan_check"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "grid_plan_check: ok" in r.stdout and "FAIL" not in r.stdout
    mk = open(os.path.join(CSRC, "Makefile")).read()
    rule = mk[mk.index("../lib/grid_plan_check:"):].split("\n\n")[0]
    assert "-fsanitize=address,undefined -fno-sanitize-recover=all" in rule and "$(CXX)" in rule
    assert "grid_plan.h" in rule and "device_arrays.h" in rule
    prerequisites = re.search(r"^%\.o:(.*)$", mk, re.M).group(1)
    assert "grid_plan.h" in prerequisites and "device_arrays.h" in prerequisites
    assert "grid_plan_check" in re.search(r"^\.PHONY:(.*)$", mk, re.M).group(1)
    assert "../lib/grid_plan_check" in mk[mk.index("\nclean:"):]
    check = code("grid_plan_check.cpp")
    assert re.search(r"^int main\(\)", check, re.M) and '#include "grid_plan.h"' in check


def test_the_header_is_plain_cxx():
    for name in ("grid_plan.h", "device_arrays.h"):
        plan = code(name)
        for word in ("hip_runtime", "hipMalloc", "hipFree", "hipStream", "hipLaunch", "threadIdx", "__global__", "__device__",
                     "common.h", "body_sort.h", "nbody_hip", "<vector>"):
            # (__host__ __device__ appears once, in the macro that is empty for a plain C++ compiler)
            found = plan.count(word) - (1 if name == "grid_plan.h" and word == "__device__" else 0)
            assert found == 0, (name, word)
    plan = code("grid_plan.h")
    assert "#define NBH_GRID_HD __host__ __device__" in plan and "#if defined(__HIPCC__)" in plan
    for fn in ("grid_axis_cells(", "grid_cells_times(", "bits_for(", "key_bits(", "speculated_bits(", "grid_from_bounds(",
               "grid_too_large(", "grid_sizes(", "start_array_capacity(", "unit_list_capacity(", "point_capacity(",
               "start_array_plan(", "force_plan(", "force_auto_tuning(", "unit_list_per_xcd(", "unit_list_bound(", "layer_cells("):
        assert len(re.findall(r"inline \w[\w ]*\b" + re.escape(fn), plan)) == 1, fn
    arrays = code("device_arrays.h")
    assert len(re.findall(r"inline \w[\w ]*\breplace_arrays\(", arrays)) == 1


def test_spatial_hash_takes_every_rule_from_the_header():
    plan = code("grid_plan.h")
    sh = code("spatial_hash.hip")
    assert '#include "grid_plan.h"' in sh and "static_assert(kGridBlock == kBlock" in sh
    for struct in ("struct GridInfo", "struct ForcePlan", "struct StartArrayPlan"):
        assert struct not in sh and struct in plan, struct
    # (HashParams and cut_const_ok stay in spatial_hash.hip: tests/hash_pair_ref.py reads their limits there)
    assert "struct HashParams" in sh and "struct HashParams" not in plan
    for const in ("kBodyBelow", "kSplitFrom", "kFilterFrom", "kFilterFromInside", "kSplitCnt", "kCellsPerWave", "kCellWPB",
                  "kMaxWv", "kUnitCells", "kGapInline", "kLbCoarse"):
        assert len(re.findall(r"constexpr \w+ " + const + r"\b", plan)) == 1, const
        assert not re.findall(r"constexpr \w+ " + const + r"\b", sh), const
    host = sh.split("using namespace nbh;")[1]
    # the automatic choice, the limits and the density rule are written in the header alone
    for word in ("kBodyBelow", "kSplitFrom", "kFilterFrom", "kFilterFromInside", "kCellsPerWave", "kMaxWv", "kGapInline", "kLbCoarse",
                 "0x7fffffff", "16LL *", "100000000", "65535", "prebuilt"):
        assert word not in host, word
    assert "prebuilt" not in sh
    for word in ("0x7fffffff", "16LL *", "65535u"):
        assert word in plan, word
    assert len(re.findall(r"\b100000000LL", plan)) == 1
    # one plan per force call, on the common path of the three entries; one plan per start array
    assert host.count("force_plan(") == 1 and host.count("start_array_plan(") == 1
    common = host[host.index("static int grid_forces("):host.index("static int grid_forces_common(")]
    assert "force_plan(" in common
    assert host.count("grid_forces(ForceEntry::") == 3
    for entry in ("ForceEntry::Whole", "ForceEntry::TwoGrids", "ForceEntry::Layer"):
        assert host.count(entry) == 1, entry
    # everything that judges the grid as built reads built_cell: cell_size is what the NEXT build takes
    uses = re.findall(r"(\w+)->cell_size", host)
    assert uses and set(uses) == {"g"}
    for fn in ("grid_forces", "nbody_hip_grid_forces_pair_packed", "nbody_hip_grid_forces_layer_packed", "nbody_hip_grid_field",
               "nbody_hip_grid_potential"):
        body = host[host.index(fn + "("):]
        body = body[:body.index("\n}\n")]
        assert "cell_size" not in body, fn
    # allocations: one hipMalloc and one hipFree besides the pinned ones, behind replace_arrays
    assert host.count("hipMalloc(") == 1 and host.count("hipFree(") == 1
    assert host.count("hipHostMalloc(") == 1 and host.count("getenv(") == 5
    env = host[host.index("static void grid_read_env("):]
    assert env[:env.index("\n}\n")].count("getenv(") == 5
    # the staged build
    for stage in ("static int build_box(", "static hipError_t build_keys(", "static int build_wait_record(",
                  "static int build_start_array("):
        assert host.count(stage) == 1, stage
    assert "launch_cell_forces(const ForcePlan& p, const ForceCall& c)" in host

"""The host decisions of the Barnes-Hut tree without a GPU: the CPU check of csrc/tree_plan.h (make tree_plan_check: the
walk plan against a restatement of the if-chain it replaces, the size table and build layout against the arrays they
index, the array replacement under a failing allocator, the node decode on a hand-made tree -- under AddressSanitizer and
UBSan), and that barnes_hut.hip takes those decisions from that one header."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "n-body_amd", "csrc")


def test_tree_plan_check_builds_and_passes():
    r = subprocess.run(["make", "-C", CSRC, "tree_plan_check"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "tree_plan_check: ok" in r.stdout and "FAIL" not in r.stdout
    mk = open(os.path.join(CSRC, "Makefile")).read()
    rule = mk[mk.index("../lib/tree_plan_check:"):]
    assert "-fsanitize=address,undefined -fno-sanitize-recover=all" in rule.split("\n\n")[0]
    assert "$(CXX)" in rule.split("\n\n")[0]
    assert "tree_plan.h" in re.search(r"^%\.o:(.*)$", mk, re.M).group(1)
    assert "device_arrays.h" in re.search(r"^%\.o:(.*)$", mk, re.M).group(1) and "device_arrays.h" in rule.split("\n\n")[0]
    assert "tree_plan_check" in re.search(r"^\.PHONY:(.*)$", mk, re.M).group(1)
    assert "../lib/tree_plan_check" in mk[mk.index("\nclean:"):]


def test_the_header_is_plain_cxx_and_barnes_hut_uses_it():
    code = lambda name: re.sub(r"//.*", "", open(os.path.join(CSRC, name)).read())  # noqa: E731
    plan = code("tree_plan.h")
    for word in ("hip_runtime", "hipMalloc", "hipFree", "hipStream", "hipLaunch", "threadIdx", "__global__", "__device__",
                 "common.h", "body_sort.h", "nbody_hip", "<vector>"):
        assert word not in plan, word
    for fn in ("tree_sizes(", "tree_node_bound(", "tree_id_bound(", "tree_params_fit(", "build_layout(", "walk_plan(",
               "walk_guard(", "walk_scheduled(", "compact_ids(", "decode_nodes("):
        assert len(re.findall(r"inline \w[\w ]*\b" + re.escape(fn), plan)) == 1, fn
    # the array replacement is shared with the spatial hash: one definition, in the header both plan headers include
    arrays = code("device_arrays.h")
    assert '#include "device_arrays.h"' in plan
    for fn in ("replace_arrays(", "release_arrays(", "array_slot("):
        assert len(re.findall(r"inline \w[\w ]*\b" + re.escape(fn), arrays)) == 1, fn
        assert not re.findall(r"inline \w[\w ]*\b" + re.escape(fn), plan), fn
    for word in ("hip_runtime", "hipMalloc", "hipFree", "__device__", "common.h", "<vector>"):
        assert word not in arrays, word
    bh = code("barnes_hut.hip")
    assert '#include "tree_plan.h"' in bh
    # one definition of every rule: the launch macros are gone, the schedule size is written in the header alone, and
    # the guard rule, the bounds and the structures the decode reads are not defined a second time
    assert "NBH_BH_LAUNCH" not in bh and "NBH_BH_QLAUNCH" not in bh
    cap = re.compile(r"waves\s*/\s*8\s*\+\s*waves\s*/\s*32\s*\+\s*8")
    assert len(cap.findall(plan)) == 1 and not cap.findall(bh)
    assert "1e-12f" not in bh and len(re.findall(r"1e-12f", plan)) == 1
    assert "tree_params_fit(" in bh and "/ (size_t)(leaf_max + 1)" not in bh
    for struct in ("struct TreeRoot", "NodeRec {", "struct RefOctreeNode"):
        assert struct not in bh and struct in plan, struct
    # the walk, the potential and the field take their plan / guard from the header; every host copy goes through the
    # header's compaction
    host = bh.split("using namespace nbh;")[1]
    assert host.count("walk_plan(") == 1 and host.count("walk_guard(") == 2
    assert host.count("walk_scheduled(") == 1 and host.count("build_layout(") == 1
    assert host.count("compact_ids(") == 2 and host.count("decode_nodes(") == 1
    assert "hipMalloc(" in host and host.count("hipMalloc(") == 1 and host.count("hipFree(") == 1
    check = code("tree_plan_check.cpp")
    assert re.search(r"^int main\(\)", check, re.M) and '#include "tree_plan.h"' in check

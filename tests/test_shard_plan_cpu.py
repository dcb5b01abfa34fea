"""The host arithmetic of the sharded Direct system without a GPU: the CPU check of csrc/shard_plan.h (make
shard_plan_check: shard bounds, pair schedule and the plan of the reaction exchange -- every cross-shard body pair once,
the written-out restatements, matched slots, RCCL's message order, the block table's room -- under AddressSanitizer and
UBSan), and that sharded.hip takes all of it from that one header."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "n-body_amd", "csrc")


def test_shard_plan_check_builds_and_passes():
    r = subprocess.run(["make", "-C", CSRC, "shard_plan_check"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "shard_plan_check: ok" in r.stdout and "FAIL" not in r.stdout
    mk = open(os.path.join(CSRC, "Makefile")).read()
    rule = mk[mk.index("../lib/shard_plan_check:"):]
    assert "-fsanitize=address,undefined -fno-sanitize-recover=all" in rule.split("\n\n")[0]
    assert "$(CXX)" in rule.split("\n\n")[0]
    assert "shard_plan.h" in re.search(r"^%\.o:(.*)$", mk, re.M).group(1)
    assert "shard_plan_check" in re.search(r"^\.PHONY:(.*)$", mk, re.M).group(1)
    assert "../lib/shard_plan_check" in mk[mk.index("\nclean:"):]


def test_the_header_is_plain_cxx_and_sharded_hip_uses_it():
    code = lambda name: re.sub(r"//.*", "", open(os.path.join(CSRC, name)).read())  # noqa: E731
    plan = code("shard_plan.h")
    for word in ("hip_runtime", "hipMalloc", "hipStream", "threadIdx", "__global__", "comm.h", "common.h", "nbody_hip"):
        assert word not in plan, word
    assert set(re.findall(r"#include\s+(\S+)", plan)) == {"<cstddef>", "<vector>"}
    fns = ("shard_bounds(", "pair_schedule(", "sharded_direct_plan(", "in_ranges(")
    for fn in fns:
        assert len(re.findall(r"inline \w[\w ]*\b" + re.escape(fn), plan)) == 1, fn
    # one definition of every rule: sharded.hip includes the header, defines none of it again and calls each
    text = code("sharded.hip")
    assert '#include "shard_plan.h"' in text
    for fn in fns:
        assert not re.search(r"^[ \t]*(?:static |inline )*[\w:]+[\w:<>*& ]*\s+" + re.escape(fn) + r"[^;{]*\{", text, re.M), fn
        assert re.search(r"\b" + re.escape(fn), text), fn
    # the two exported functions are argument checks plus a call: the schedule's arithmetic is gone from the file
    for gone in (r"world / 2", r"\(world - 1\) / 2", r"\bS / 2", r"\(size_t\)world - 1"):
        assert not re.search(gone, text), gone
    # no search for the receiving block on the per-step path: the schedule is asked for once per call of the ABI function
    assert text.count("pair_schedule(") == 2 and "nbody_hip_pair_schedule(s->W" not in text
    check = code("shard_plan_check.cpp")
    assert re.search(r"^int main\(\)", check, re.M) and '#include "shard_plan.h"' in check

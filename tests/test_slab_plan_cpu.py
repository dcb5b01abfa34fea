"""The host arithmetic of the sharded spatial hash's exchange without a GPU: the CPU check of csrc/slab_plan.h (make
plan_check: layer owners, slab map, balanced cuts, adoption rule and the exchange plan against written-out restatements,
under AddressSanitizer and UBSan), and that the device code and the host take the owner functions from that one header."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "n-body_amd", "csrc")


def test_plan_check_builds_and_passes():
    r = subprocess.run(["make", "-C", CSRC, "plan_check"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "slab_plan_check: ok" in r.stdout and "FAIL" not in r.stdout
    mk = open(os.path.join(CSRC, "Makefile")).read()
    rule = mk[mk.index("../lib/slab_plan_check:"):]
    assert "-fsanitize=address,undefined -fno-sanitize-recover=all" in rule.split("\n\n")[0]
    assert "$(CXX)" in rule.split("\n\n")[0]
    assert "slab_plan.h" in re.search(r"^%\.o:(.*)$", mk, re.M).group(1)
    assert "plan_check" in re.search(r"^\.PHONY:(.*)$", mk, re.M).group(1)
    assert "../lib/slab_plan_check" in mk[mk.index("\nclean:"):]


def test_the_header_is_plain_cxx_and_both_sides_use_it():
    code = lambda name: re.sub(r"//.*", "", open(os.path.join(CSRC, name)).read())  # noqa: E731
    plan = code("slab_plan.h")
    for word in ("hip_runtime", "hipMalloc", "hipStream", "threadIdx", "__global__", "comm.h", "common.h", "nbody_hip"):
        assert word not in plan, word
    for fn in ("grid_from_box(", "slab_owner(", "slab_owner_cuts(", "slab_map(", "balanced_cuts(", "adopt_cuts(", "exchange_plan("):
        assert len(re.findall(r"inline \w[\w ]*\b" + re.escape(fn), plan)) == 1, fn
    # one definition of every rule: the device code and the host include the header and define none of it again
    for name in ("slab.hip", "sharded_hash.hip"):
        text = code(name)
        assert '#include "slab_plan.h"' in text, name
        for fn in ("slab_owner(", "slab_owner_cuts(", "grid_from_box(", "balanced_cuts(", "layer_owner_equal"):
            assert not re.search(r"\b(?:int|void)\s+" + re.escape(fn), text), (name, fn)
    assert "layer_owner_equal" not in code("sharded_hash.hip")
    check = code("slab_plan_check.cpp")
    assert re.search(r"^int main\(\)", check, re.M) and '#include "slab_plan.h"' in check

"""The host decisions of the ensemble integrator without a GPU: the CPU check of csrc/hermite_batch_plan.h (make
batch_plan_check: the advance plan against a restatement of the three-branch choice it replaces, the recording rule against
the ran_eagerly lines of the four configuration calls over every short sequence of calls, the shared argument checks against
the loops they replace, code and message -- under AddressSanitizer and UBSan), and that hermite_batch.hip takes those
decisions from that one header, keeps one table of the features' device memory and one text of the priming kernels."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "n-body_amd", "csrc")


def code(name):
    return re.sub(r"//.*", "", open(os.path.join(CSRC, name)).read())


def test_batch_plan_check_builds_and_passes():
    r = subprocess.run(["make", "-C", CSRC, "batch_plan_check"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "hermite_batch_plan_check: ok" in r.stdout and "FAIL" not in r.stdout
    mk = open(os.path.join(CSRC, "Makefile")).read()
    rule = mk[mk.index("../lib/hermite_batch_plan_check:"):].split("\n\n")[0]
    assert "-fsanitize=address,undefined -fno-sanitize-recover=all" in rule and "$(CXX)" in rule
    assert "hermite_batch_plan.h" in rule
    assert re.search(r"^batch_plan_check: \.\./lib/hermite_batch_plan_check$", mk, re.M)
    prerequisites = re.search(r"^hermite_batch\.o:(.*)$", mk, re.M).group(1)
    for name in ("hermite_batch_plan.h", "hermite_batch_prime_sweep.inc", "hermite_batch_prime_finalize.inc",
                 "hermite_batch_resident_body.inc", "hermite_batch_layout.h"):
        assert name in prerequisites, name
    assert "batch_plan_check" in re.search(r"^\.PHONY:(.*)$", mk, re.M).group(1)
    assert "../lib/hermite_batch_plan_check" in mk[mk.index("\nclean:"):]
    check = code("hermite_batch_plan_check.cpp")
    assert re.search(r"^int main\(\)", check, re.M) and '#include "hermite_batch_plan.h"' in check
    # it restates the code the plan replaces: the three branches and the recording lines, not calls into the header
    restated = check[check.index("static Launch restated_advance("):check.index("static Launch planned_advance(")]
    assert "if (h->hier_on)" in restated and "else if (h->out_on)" in restated and "batch_advance_plan" not in restated
    restated = check[check.index("static void restated_set("):check.index("static void planned_set(")]
    assert restated.count("h->ran_eagerly = false;") == 6 and restated.count("h->mrg_ran_eagerly = false;") == 2
    assert "turn(" not in restated


def test_the_header_is_plain_cxx():
    plan = code("hermite_batch_plan.h")
    for word in ("hip", "threadIdx", "__global__", "__device__", "common.h", "<vector>", "NBH_FAIL"):
        assert word not in plan, word
    for fn in ("batch_advance_plan(", "batch_unknown_flags(", "batch_bad_system_radii(", "batch_bad_body_radii("):
        assert len(re.findall(r"inline \w[\w ]*\b" + re.escape(fn), plan)) == 1, fn
    assert "struct BatchFeatures" in plan and "void reset()" in plan and "void turn(BatchFeature f, bool to)" in plan


def test_hermite_batch_takes_every_decision_from_the_header():
    plan = code("hermite_batch_plan.h")
    hb = code("hermite_batch.hip")
    assert '#include "hermite_batch_plan.h"' in hb
    for struct in ("struct BatchFeatures", "struct BatchAdvancePlan"):
        assert struct not in hb and struct in plan, struct
    host = hb.split("using namespace nbh;")[1]
    # the handle holds one feature record and one array of allocations: none of the former fields is left
    for word in ("ev_on", "out_on", "hier_on", "mrg_on", "ev_flags", "out_flags", "hier_flags", "hier_kappa", "ev_mem", "out_mem",
                 "hier_mem", "mrg_mem", "snap_mem", "h->ran_eagerly", "h->mrg_ran_eagerly"):
        assert word not in host, word
    assert host.count("BatchFeatures feat;") == 1 and host.count("void* feat_mem[kBatchStores]") == 1
    # one plan per advance and one dispatch; the recording words are written by turn, by the priming and by an eager run
    advance = host[host.index('extern "C" int nbody_hip_hermite_batch_advance('):]
    advance = advance[:advance.index("\n}\n")]
    assert host.count("batch_advance_plan(") == 1 and advance.count("batch_advance_plan(") == 1
    assert advance.count("with_flags(") == 1 and advance.count("hipLaunchKernelGGL(") == 3 and "switch (plan.form)" in advance
    assert not re.search(r"\bif \(h->", advance[advance.index("batch_advance_plan("):])
    assert host.count("ran_eagerly = false") == 2 and host.count("ran_eagerly = true") == 2
    # every on-bit is written by turn: once for the off path and once for the on path of the three calls that upload, once
    # for the mergers; a new layout resets
    assert host.count(".turn(") == 3 and host.count("feat.reset()") == 1 and not re.search(r"\.on\[\w+\] = ", host)
    for fn in ("static int batch_feature_off(", "static int batch_feature_set("):
        assert host.count(fn) == 1, fn
    assert host.count("return batch_feature_off(h, ") == 3 and host.count("return batch_feature_set(h, ") == 3
    # one table, one reserve, one clear; one hipMalloc for all the features and one hipFree loop
    assert host.count("static const BatchFeatureStore kBatchStore[kBatchStores]") == 1
    for fn in ("static int batch_feature_reserve(", "static int batch_features_clear(", "static int batch_check_primed_arrays(",
               "static int batch_check_systems(", "static int batch_readout_begin(", "static int batch_set_begin("):
        assert host.count(fn) == 1, fn
    assert host.count("hipMalloc(") == 3  # the handle's state, the rows, a feature
    for kernel in ("batch_events_clear_kernel", "batch_outcomes_clear_kernel", "batch_hierarchy_clear_kernel",
                   "batch_mergers_clear_kernel"):
        assert host.count(kernel) == 1, kernel
    prime = host[host.index('extern "C" int nbody_hip_hermite_batch_prime('):]
    prime = prime[:prime.index("\n}\n")]
    # the priming's order: the mergers' clear before the pack, the other clears behind the finalize
    order = [prime.index(w) for w in ("held & mergers", "batch_pack_kernel", "batch_prime_sweep_kernel",
                                      "batch_prime_finalize_kernel", "held & ~mergers", "handle_primed_for(")]
    assert order == sorted(order) and "batch_features_held(h)" in prime
    # every message of the shared checks is written once, in the header or in a helper
    for text in ("the particle count or the arrays differ from the primed ones", "got room for %zu records",
                 "the ensemble has no layout: call set_layout first"):
        assert hb.count(text) == (3 if text.startswith("the ensemble has no layout") else 1), text  # (prime, diagnostics, set)
    for text in ("unknown %s flag bits 0x%x (known: %s)", "the %s radius of system %zu must be non-negative and finite, got %g",
                 "the radius of body %zu (body %zu of system %zu) must be non-negative and finite, got %g"):
        assert plan.count(text) == 1 and "flag bits" not in host and "must be non-negative and finite, got %g\"" not in host.replace(
            'kappa must be non-negative and finite, got %g"', ""), text
    # the "none" records of the events and the outcomes are written once, for the device and the host
    for fn in ("event_record_none(", "outcome_record_none("):
        assert len(re.findall(r"__host__ __device__ inline void " + re.escape(fn), hb)) == 1 and host.count(fn) >= 1, fn
    assert "memset(&none" not in host


def test_the_priming_kernels_share_their_text():
    hb = code("hermite_batch.hip")
    assert hb.count('#include "hermite_batch_prime_sweep.inc"') == 2 and hb.count('#include "hermite_batch_prime_finalize.inc"') == 2
    assert hb.count("jerk_tile<") == 0 and hb.count("block_prime_level(") == 0
    sweep, fin = code("hermite_batch_prime_sweep.inc"), code("hermite_batch_prime_finalize.inc")
    assert sweep.count("jerk_tile<R, GUARD, EXT>(") == 1 and sweep.count("__syncthreads()") == 1 and "return" not in sweep
    assert fin.count("block_prime_level(") == 1 and "return" not in fin
    for name in ("batch_prime_sweep_kernel", "batch_reprime_sweep_kernel"):
        body = hb[hb.index("void " + name + "("):]
        body = body[:body.index("\n}\n")]
        assert "template" not in body and body.count("#include") == 1 and "__launch_bounds__" not in body, name
    # the two uniform exits of the pass stand before the shared text, and the header of each text says why it is text
    body = hb[hb.index("void batch_reprime_sweep_kernel("):]
    body = body[:body.index("#include")]
    assert body.count("return;") == 2 and "mark[s]" in body
    for name in ("hermite_batch_prime_sweep.inc", "hermite_batch_prime_finalize.inc"):
        head = open(os.path.join(CSRC, name)).read()
        assert "The including kernel provides" in head and "text and not a function" in head and "disasm_diff" in head, name
    fin_kernel = hb[hb.index("void batch_prime_finalize_kernel("):]
    assert "const float& dt = dt_max[s];" in fin_kernel[:fin_kernel.index("\n}\n")]

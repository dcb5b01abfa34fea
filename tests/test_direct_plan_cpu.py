"""Shape and budget arithmetic of the Direct N^2 path (nbody_hip_direct_info with a NULL context: plain host code
in n-body_amd/csrc/direct_plan.h, no device needed) -- which kernel a call takes, with how many bodies per lane,
and what the deterministic form's slot planes cost (12 bytes per reaction slot, 24 per I-side slot, per body).  Then the
header itself: its CPU check (make direct_plan_check: every function against a restatement of the code it replaced, under
AddressSanitizer and UBSan), that it is plain C++, and that the family's files take their decisions from it."""
import ctypes as C
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "n-body_amd", "csrc")
FAMILY = ("direct.hip", "direct_sym.hip", "energy.hip", "hermite.hip", "hermite_block.hip", "hermite_batch.hip", "api.hip",
          "sharded.hip")
PLAN_FUNCTIONS = ("direct_guard(", "direct_pairs_ok(", "one_sided_shape(", "one_sided_plan(", "potential_splits(",
                  "symmetric_pays(", "sym_R(", "sym_residency(", "sym_split(", "sym_shape(", "pair_shape(",
                  "slot_budget_allows(", "direct_plan(", "pair_plan(", "narrow_sizes(", "block_takes_narrow(",
                  "block_takes_resident(", "block_schedule_check(")


def code(name):
    return re.sub(r"//.*", "", open(os.path.join(CSRC, name)).read())


def info(nb, n, eps2=1e-6):
    from nbody_amd._lib import DirectInfoStruct, check, load
    s = DirectInfoStruct()
    check(load().nbody_hip_direct_info(None, n, eps2, C.byref(s)))
    return s


def test_kernel_choice_by_size(nb):
    assert info(nb, 4096).kernel == 0 and info(nb, 12287).kernel == 0       # one-sided kernel below 12,288 bodies
    assert info(nb, 12288).kernel == 2                                       # symmetric kernel, slot planes
    assert info(nb, 1 << 20, eps2=0.0).kernel == 0                           # tiny softening: guarded one-sided kernel
    assert [info(nb, n).bodies_per_lane_equal for n in (12288, 27999, 28000, 99999, 100000, 199999, 200000, 1 << 20)] \
        == [6, 6, 8, 8, 12, 12, 16, 16]
    # general masses run with the same bodies per lane as equal masses (round 2: 12 where those take 16 -- the slot
    # kernel spilled; the single loop body of round 3 fits 246 registers)
    assert info(nb, 1 << 20).bodies_per_lane_general == 16 and info(nb, 150000).bodies_per_lane_general == 12


@pytest.mark.parametrize("n", [12288, 65536, 131072, 262144, 1 << 20, 1 << 21])
def test_slot_plane_bytes(nb, n):
    s = info(nb, n)
    assert s.kernel == 2 and s.deterministic_mode == 1 and s.last_kernel == -1 and s.workspace_bytes_held == 0

    def need(R):
        S = 256 * R
        NB = -(-n // S)
        D, plane = NB // 2, NB * S
        total = (D + 1) * (S // 64)
        splits = max(1, -(-256 * 16 // NB))
        per = max(4, -(-total // splits))
        if per > S // 64:
            per = -(-per // (S // 64)) * (S // 64)
        splits = -(-total // per)
        react = (D * 3 * plane * 4 + 255) // 256 * 256
        return D, splits, react + splits * 3 * plane * 8
    D, splits, b_eq = need(s.bodies_per_lane_equal)
    assert (s.reaction_slots, s.iside_slots) == (D, splits)
    assert s.workspace_bytes_needed == max(b_eq, need(s.bodies_per_lane_general)[2]) == s.slot_bytes_wanted


def test_headline_size_costs_under_2_gb_and_budget_switches_to_atomics(nb):
    s = info(nb, 1 << 20)
    # 128 reaction slots x 12 B + 15 I-side slots x 24 B per body = 1.9 GB for both instantiations
    # (round 2: 24 B per slot and a 12-bodies-per-lane general-mass shape with 183 slots: 4.6 GB reserved)
    assert s.reaction_slots == 128 and 1.85e9 < (128 * 12 + s.iside_slots * 24) * (1 << 20) < 2.0e9
    assert 1.85e9 < s.workspace_bytes_needed < 2.0e9
    big = info(nb, 1 << 22)
    assert big.kernel == 1 and big.slot_bytes_wanted > (24 << 30)            # beyond the 24 GiB budget: atomics ...
    assert big.workspace_bytes_needed == 3 * 8 * 4194304                     # ... 24 bytes per body
    with pytest.raises(Exception):
        info(nb, (1 << 30) + 1)


def test_direct_plan_check_builds_and_passes():
    r = subprocess.run(["make", "-C", CSRC, "direct_plan_check"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "direct_plan_check: ok" in r.stdout and "FAIL" not in r.stdout
    mk = open(os.path.join(CSRC, "Makefile")).read()
    rule = mk[mk.index("../lib/direct_plan_check:"):].split("\n\n")[0]
    assert "-fsanitize=address,undefined -fno-sanitize-recover=all" in rule and "$(CXX)" in rule
    assert "direct_plan.h" in rule
    assert re.search(r"^direct_plan_check: \.\./lib/direct_plan_check$", mk, re.M)
    assert "direct_plan.h" in re.search(r"^%\.o: %\.hip(.*)$", mk, re.M).group(1)
    assert "direct_plan_check" in re.search(r"^\.PHONY:(.*)$", mk, re.M).group(1)
    assert "../lib/direct_plan_check" in mk[mk.index("\nclean:"):]
    check = code("direct_plan_check.cpp")
    assert re.search(r"^int main\(\)", check, re.M) and '#include "direct_plan.h"' in check
    # it restates the code the header replaces, copied, not calls into the header
    restated = check[check.index("namespace restated {"):check.index("using namespace nbh;")]
    for fn in PLAN_FUNCTIONS + ("align256(", "plan_ceil("):
        assert not re.search(r"(?<![\w:])" + re.escape(fn), restated), fn
    assert "nbh::" not in restated and "1e-12f" in restated and "kNumCU * 8" in restated
    for fn in ("r_choose_shape(", "r_jerk_shape(", "r_potential_energy(", "r_energies_packed(", "r_direct_potential(",
               "r_sym_shape(", "r_pair_shape(", "r_direct_plan(", "r_det_budget_allows(", "r_variant(", "r_all_pairs_fallback(",
               "r_pair_call(", "r_narrow_step(", "r_narrow_resident(", "r_block_takes_narrow(", "r_block_form(",
               "r_schedule_bad("):
        assert len(re.findall(r"static [\w:]+ " + re.escape(fn), restated)) == 1, fn
        assert check[check.index("using namespace nbh;"):].count("restated::" + fn) >= 1, fn


def test_the_header_is_plain_cxx():
    plan = code("direct_plan.h")
    for word in ("hip", "__global__", "__device__", "common.h", "NBH_FAIL"):
        assert word not in plan, word
    for fn in PLAN_FUNCTIONS:
        assert len(re.findall(r"^(?:inline|constexpr) \w[\w ]*\b" + re.escape(fn), plan, re.M)) == 1, fn
    for struct in ("DirectTuning", "OneSidedShape", "OneSidedPlan", "PotentialSplits", "SymShape", "PairShape", "DirectPlan",
                   "PairPlan", "NarrowSizes", "ScheduleFault"):
        assert plan.count("struct " + struct + " {") == 1, struct
    assert plan.count("void demote_to_atomics()") == 2
    common = code("common.h")
    assert '#include "direct_plan.h"' in common and "nbh::DirectTuning tune;" in common
    for word in ("struct SymShape", "struct DirectPlan", "sym_shape(", "symmetric_pays(", "tune_variant", "tune_tpl", "tune_splits",
                 "det_budget"):
        assert word not in common, word


def test_the_family_takes_its_decisions_from_the_header():
    text = {f: code(f) for f in FAMILY}
    for f in ("direct.hip", "direct_sym.hip", "hermite.hip", "hermite_block.hip", "hermite_batch.hip", "api.hip", "sharded.hip"):
        assert "1e-12f" not in text[f], f
    for f in sorted(os.listdir(CSRC)):
        if f.endswith((".hip", ".h", ".inc")):
            for word in ("choose_shape(", "jerk_shape(", "NBH_DISPATCH", "NBH_PAIR_LAUNCH", "JerkShape"):
                assert word not in open(os.path.join(CSRC, f)).read(), (f, word)
    assert "kNumCU * 8" not in text["energy.hip"] and text["energy.hip"].count("potential_splits(") == 3
    assert text["direct_sym.hip"].count("hipMemGetInfo") == 1
    # the residency of the 16-bodies-per-lane kernels is one function; the number is written in the header alone
    assert "kSymRL16" not in text["direct_sym.hip"] and "kPairRL16" not in text["direct_sym.hip"]
    assert text["direct_sym.hip"].count("tune.variant") == 1
    info = text["api.hip"][text["api.hip"].index('extern "C" int nbody_hip_direct_info('):]
    info = info[:info.index("\n}\n")]
    assert "symmetric =" not in info and info.count("device_direct_plan(") == 1 and "direct_guard" not in info
    assert "direct_pairs_ok" not in info and "out->kernel = p.kernel();" in info
    # the force call executes the plan the info call reports
    packed = text["direct.hip"][text["direct.hip"].index("int direct_packed("):]
    packed = packed[:packed.index("\n}\n")]
    assert packed.count("device_direct_plan(") == 1 and "symmetric_pays" not in packed and "tune." not in packed.replace(
        "one_sided_plan(ctx->tune,", "")
    assert text["direct_sym.hip"].count("demote_to_atomics()") == 2 and text["direct_sym.hip"].count("kLargeWorkspace") == 1
    assert text["api.hip"].count("kLargeWorkspace") == 1 and "<< 20" not in text["api.hip"] + text["direct_sym.hip"]
    # each of the two schedule-fault messages appears once
    assert text["hermite_block.hip"].count("block-step schedule out of range") == 1
    assert text["hermite_batch.hip"].count("block-step schedule out of range") == 1
    block = text["hermite_block.hip"]
    assert block.count("block_schedule_fail(") == 3 and block.count("narrow_sizes(") == 2 and "kNarrowS - 1" not in block
    assert block.count("block_takes_narrow(") == 1 and block.count("block_takes_resident(") == 1

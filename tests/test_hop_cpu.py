"""The density-peak (HOP) groups without a GPU: the CPU check of csrc/hop_common.h and csrc/hop_plan.h (make hop_check,
under AddressSanitizer and UBSan); what the sources promise (no HIP in the two headers, no fused product, no
floating-point atomic, no inline assembly, one union-find and one catalogue shared with the friends-of-friends search);
the header's sentences; and the test reference of tests/hop_ref.py itself: against an independent plain-Python loop
written from the header's sentences (peaks followed one hop at a time, step 1 through
scipy.sparse.csgraph.connected_components), and against answers written out by hand for graphs of at most 12 bodies."""
import ctypes as C
import math
import os
import re
import subprocess

import numpy as np
import pytest
from scipy.sparse import coo_matrix
from scipy.sparse.csgraph import connected_components

import hop_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "n-body_amd", "csrc")
HEADER = os.path.join(ROOT, "include", "nbody_hip_hop.h")


def code(name):
    return re.sub(r"//.*", "", open(os.path.join(CSRC, name)).read())


def test_check_program_builds_and_passes():
    target = "hop_check"
    r = subprocess.run(["make", "-C", CSRC, target], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert target + ": ok" in r.stdout and "FAIL" not in r.stdout
    mk = open(os.path.join(CSRC, "Makefile")).read()
    rule = mk[mk.index("../lib/" + target + ":"):].split("\n\n")[0]
    assert "-fsanitize=address,undefined -fno-sanitize-recover=all" in rule and "$(CXX)" in rule
    for word in ("hop_common.h", "hop_plan.h", "-ffp-contract=off"):
        assert word in rule, word
    assert target in re.search(r"^\.PHONY:(.*)$", mk, re.M).group(1)
    assert "../lib/" + target in mk[mk.index("\nclean:"):]
    assert re.search(r"^int main\(", code(target + ".cpp"), re.M)
    assert re.search(r"^hop_groups\.o: CXXFLAGS \+= -ffp-contract=off$", mk, re.M)
    assert "hop_groups.hip" in re.search(r"^SRCS\s*:=(.*)$", mk, re.M).group(1)


def test_what_the_sources_promise():
    for name in ("hop_common.h", "hop_plan.h"):
        text = code(name)
        for word in ("hip_runtime", "hipMalloc", "hipStream", "hipLaunch", "threadIdx", "__global__", '"common.h"', "nbody_hip", "<vector>",
                     "fma"):
            assert word not in text, (name, word)
    kernels = code("hop_groups.hip")
    for word in ('#include "hop_common.h"', '#include "hop_plan.h"', '#include "nbody_hip_hop.h"', '#include "grid_groups.inc"',
                 "#define NBH_GROUPS_SHARED_PART_ONLY"):
        assert word in kernels, word
    for word in ("asm", "unsafeAtomicAdd", "atomicAdd(float", "atomicAdd(double", "__fma", "fma(", "atomicExch"):
        assert word not in kernels, word
    # every atomic of the file works on an integer word
    for m in re.finditer(r"atomic(Add|Max|Min|Or)\(([^,]+),", kernels):
        assert any(w in m.group(2) for w in ("word", "words", "best_rho", "best_peak", "root")), m.group(0)
    # one union-find and one catalogue: hop_groups.hip includes the shared part of the friends-of-friends search, which ends
    # where the rest of that file begins, and defines none of it again
    groups = code("grid_groups.inc")
    shared = groups[groups.index("#ifndef NBH_GROUPS_SHARED_PART\n"):groups.index("#endif  ")]
    assert groups.index("#ifndef NBH_GROUPS_SHARED_PART_ONLY") > groups.index(shared) + len(shared) - 1
    assert groups.rstrip().endswith("#endif")
    for fn in ("group_find(int* parent", "group_unite(int* parent", "void group_size_add(", "void group_heads_kernel",
               "void group_offsets_kernel"):
        assert fn in shared and groups.count(fn) == 1 and fn not in kernels, fn
    for word in ("hipMalloc", "nbody_hip_grid", "CellLookup", "GroupSort", "#include"):
        assert word not in shared, word  # the shared part needs common.h alone
    # the 64-bit sort is the one the radial profiles use, and no third sort is written here
    assert "rocprim::radix_sort_pairs" in kernels and "rocprim::radix_sort_pairs" in code("radial_profile.hip")
    assert "HopSort::run(SortImpl::Public" in kernels


def test_header_states_the_model(nb):
    text = " ".join(open(HEADER).read().replace("\n * ", " ").split())
    for sentence in ("better(j, b) := rho[j] > rho[b] || (rho[j] == rho[b] && j < b), compared in fp64",
                     "A NaN density is never better and is never beaten",
                     "live(i) := rho[i] >= delta_outer (false for a NaN)",
                     "b(i, j) = (rho[i] + rho[j]) * 0.5 in fp64, two roundings, nothing fused",
                     "viable(P) := live(P) && rho[P] >= delta_peak",
                     "the root of a component is its lowest peak index",
                     "ties to the lowest Q",
                     "label[i] = root[peak[i]] if i is live and its peak is anchored, else -1",
                     "counts_host[5] = {n_groups, n_members, n_peaks, rounds, status}",
                     "THE CALL BLOCKS", "It cannot be recorded into a step graph",
                     "A refused call touches nothing, an earlier catalogue included",
                     "not that program's greedy sweep"):
        assert sentence in text, sentence
    assert f"#define NBODY_HIP_HOP_MAX_K {ref.MAX_K}" in open(HEADER).read() and nb.HOP_MAX_K == ref.MAX_K
    body = open(HEADER).read()
    body = body[body.index("typedef struct {"):body.index("} nbody_hip_hop_params_t;")]
    names = re.findall(r"\b(n_hop|n_merge|min_members|reserved|delta_outer|delta_saddle|delta_peak)\b", body)
    assert [n for n, _ in nb._lib.HopParamsStruct._fields_] == list(dict.fromkeys(names))
    assert C.sizeof(nb._lib.HopParamsStruct) == 40 and nb._lib.HopParamsStruct.delta_outer.offset == 16
    assert "nbody_hip_hop_groups" in nb._lib.PROTOTYPES and "nbody_hip_hop_groups_copy" in nb._lib.PROTOTYPES
    assert issubclass(nb.HopCatalogue, nb.GroupCatalogue)
    for owner in (nb.SpatialHashGrid, nb.SpatialHashCalculator, nb.ParticleSystem):
        assert callable(owner.hopGroups)


# ---- an independent restatement: plain Python, one sentence of the header at a time ----------------------------------------------
def plain(index, rho, n_hop, n_merge, delta_outer, delta_saddle=None, delta_peak=None, min_members=1):
    index = [[int(v) for v in row] for row in np.asarray(index)]
    rho = [float(v) for v in np.asarray(rho, np.float64)]
    n = len(rho)
    d_outer, d_saddle, d_peak = ref.defaults(delta_outer, delta_saddle, delta_peak)
    for row in index:
        for s in range(max(n_hop, n_merge)):
            if row[s] >= n:
                return dict(labels=[-1] * n, peak=[-1] * n, offsets=[0], members=[], group_peak=[], counts=[0, 0, 0, 0, 1])

    def better(j, b):
        return rho[j] > rho[b] or (rho[j] == rho[b] and j < b)

    nxt = []
    for i in range(n):
        b = i
        for s in range(n_hop):
            j = index[i][s]
            if j >= 0 and better(j, b):
                b = j
        nxt.append(b)
    peak = []
    for i in range(n):
        p = i
        while nxt[p] != p:  # one hop at a time
            p = nxt[p]
        peak.append(p)
    live = [rho[i] >= d_outer for i in range(n)]
    S = {}
    for i in range(n):
        if not live[i]:
            continue
        for s in range(n_merge):
            j = index[i][s]
            if j >= 0 and live[j] and peak[i] != peak[j]:
                b = (rho[i] + rho[j]) * 0.5
                key = (min(peak[i], peak[j]), max(peak[i], peak[j]))
                if key not in S or b > S[key]:
                    S[key] = b
    peaks = [i for i in range(n) if peak[i] == i]
    viable = [P for P in peaks if live[P] and rho[P] >= d_peak]
    root, anchored_in = {}, {}
    if viable:
        at = {P: t for t, P in enumerate(viable)}
        links = [(at[P], at[Q]) for (P, Q), s in S.items() if P in at and Q in at and s >= d_saddle]
        rows_ = [a for a, _ in links]
        cols_ = [b for _, b in links]
        graph = coo_matrix((np.ones(len(links)), (rows_, cols_)), shape=(len(viable), len(viable)))
        _, comp = connected_components(graph, directed=False)
        lowest = {}
        for t, P in enumerate(viable):
            lowest[comp[t]] = min(lowest.get(comp[t], P), P)
        for t, P in enumerate(viable):
            root[P] = lowest[comp[t]]
            anchored_in[P] = 0
    edges_of = {}
    for (P, Q), s in S.items():
        edges_of.setdefault(P, []).append((Q, s))
        edges_of.setdefault(Q, []).append((P, s))
    rounds = 0
    while True:
        rounds += 1
        newly = {}
        for P in peaks:
            if not live[P] or P in anchored_in:
                continue
            best = None
            for Q, s in edges_of.get(P, []):
                if Q in anchored_in and anchored_in[Q] < rounds:
                    if best is None or s > best[1] or (s == best[1] and Q < best[0]):
                        best = (Q, s)
            if best is not None:
                newly[P] = root[best[0]]
        if not newly:
            break
        for P, r in newly.items():
            root[P] = r
            anchored_in[P] = rounds
    labels = [root[peak[i]] if live[i] and peak[i] in anchored_in else -1 for i in range(n)]
    groups = {}
    for i in range(n):
        if labels[i] >= 0:
            groups.setdefault(labels[i], []).append(i)
    kept = sorted(lab for lab, m in groups.items() if len(m) >= min_members)
    offsets, members, group_peak = [0], [], []
    for lab in kept:
        members += groups[lab]
        offsets.append(len(members))
        best = None
        for P in anchored_in:
            if root[P] == lab and (best is None or better(P, best)):
                best = P
        group_peak.append(best)
    return dict(labels=labels, peak=peak, offsets=offsets, members=members, group_peak=group_peak,
                counts=[len(kept), len(members), len(peaks), rounds, 0],
                dropped=[P for P in peaks if live[P] and P not in anchored_in], edges=sorted(S), saddles=[S[e] for e in sorted(S)])


def _same(got, want, what=""):
    for key in ref.OUTPUTS:
        assert np.array_equal(np.asarray(got[key]).reshape(-1), np.asarray(want[key]).reshape(-1)), (what, key)


def _hand(name):
    return ref.hand_cases()[name]


@pytest.mark.parametrize("name", sorted(ref.hand_cases()))
def test_hand_cases(name):
    args, want = _hand(name)
    assert len(args["rho"]) <= 12
    for impl in (ref.reference, plain):
        got = impl(**args)
        for key, value in want.items():
            have = got["counts"][2] if key == "n_peaks" else got["counts"][3] if key == "rounds" else got[key]
            assert np.array_equal(np.asarray(have).reshape(-1), np.asarray(value).reshape(-1)), (impl.__name__, name, key, have, value)
        assert got["counts"][4] == 0 and got["counts"][0] == len(want["offsets"]) - 1 and got["counts"][1] == len(want["members"])


def test_hand_cases_cover_what_they_must():
    cases = ref.hand_cases()
    assert {"tie", "nan", "minus_one", "n_hop_below_k", "saddle_at", "saddle_below", "dropped_pair", "chain_of_three",
            "asymmetric", "attach_choice"} <= set(cases)
    tie = cases["tie"][0]
    assert tie["rho"][1] == tie["rho"][2]
    assert math.isnan(cases["nan"][0]["rho"][2])
    assert (cases["minus_one"][0]["index"][:, 0] == -1).all()
    assert cases["n_hop_below_k"][0]["n_hop"] < cases["n_hop_below_k"][0]["index"].shape[1]
    at, below = cases["saddle_at"], cases["saddle_below"]
    assert at[1]["saddles"] == [at[0]["delta_saddle"]] and below[1]["saddles"] == [np.nextafter(below[0]["delta_saddle"], 0.0)]
    assert at[1]["labels"] == [0, 0, 0, 0] and below[1]["labels"] == [0, 0, 3, 3]
    assert cases["dropped_pair"][1]["dropped"] == [0, 3]
    assert cases["chain_of_three"][1]["rounds"] == 4
    asym = cases["asymmetric"][0]["index"]
    assert 1 in asym[0] and 0 not in asym[1]


@pytest.mark.parametrize("seed", range(6))
def test_reference_against_the_plain_loop(seed):
    rng = np.random.default_rng(100 + seed)
    for trial in range(40):
        n = int(rng.integers(1, 60))
        k = int(rng.integers(1, 7))
        gen = ref.random_graph if trial % 2 else ref.local_graph
        index, rho = gen(n, k, int(rng.integers(1, 6)), int(rng.integers(1 << 30)))
        if trial % 5 == 0:
            rho[rng.integers(0, n)] = np.nan
        if trial % 7 == 0:
            rho[rng.integers(0, n)] = np.inf
        n_hop = int(rng.integers(1, k + 1))
        n_merge = int(rng.integers(0, k + 1))
        d = np.sort(rng.integers(0, 7, size=3)).astype(float)
        args = dict(index=index, rho=rho, n_hop=n_hop, n_merge=n_merge, delta_outer=d[0], delta_saddle=d[1], delta_peak=d[2],
                    min_members=int(rng.integers(1, 4)))
        got, want = ref.reference(**args), plain(**args)
        _same(got, want, (seed, trial))
        assert sorted(got["dropped"].tolist()) == sorted(want["dropped"])
        assert [tuple(e) for e in got["edges"].tolist()] == want["edges"] and got["saddles"].tolist() == want["saddles"]
        assert got["n_records"] % 2 == 0 and got["n_records"] >= 2 * len(want["edges"])


def test_reference_on_the_graphs_of_the_gpu_test():
    """the random graph of 3,000 bodies of tests/test_hop_gpu.py really regroups: rounds, a dropped peak, a union"""
    args = ref.regroup_case()
    got = ref.reference(**args)
    assert got["rounds"] >= 3 and got["dropped"].size >= 1 and got["unions"] >= 1
    assert np.unique(args["rho"]).size == 16 and args["index"].shape == (3000, 8)
    _same(got, plain(**args))
    bad = dict(args, index=args["index"].copy())
    bad["index"][1234, 1] = 3000
    for impl in (ref.reference, plain):
        out = impl(**bad)
        assert list(out["counts"]) == [0, 0, 0, 0, 1] and (np.asarray(out["labels"]) == -1).all() and (np.asarray(out["peak"]) == -1).all()
    # ... and the same index in a slot the call does not read changes nothing
    unread = dict(args, index=args["index"].copy())
    unread["index"][:, args["n_hop"]:] = 3000 + 7
    assert max(args["n_hop"], args["n_merge"]) == args["n_hop"] < 8
    _same(ref.reference(**unread), got)


def test_line_graphs():
    n = 500
    up = ref.reference(ref.line_graph(n), np.arange(n, dtype=np.float64) + 1.0, 2, 2, 0.0, 0.0, 0.0)
    assert (up["peak"] == n - 1).all() and (up["labels"] == n - 1).all() and up["counts"].tolist() == [1, n, 1, 1, 0]
    flat = ref.reference(ref.line_graph(n), np.ones(n), 2, 2, 0.0, 0.0, 0.0)
    assert (flat["peak"] == 0).all() and flat["group_peak"].tolist() == [0]

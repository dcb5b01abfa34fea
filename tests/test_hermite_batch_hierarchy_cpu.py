"""The ensemble hierarchies (nbody_hip_batch_hierarchy_set / _get / _snapshot, EnsembleHierarchy, hierarchy_string), the
parts that need no GPU: the prototypes against the new header, both record layouts through ctypes, numpy and the header,
the Python-side validation, hierarchy_string on hand-made tables, the restatement's known answers and its own bound
against exact rational arithmetic for every case of the GPU tests (at the initial states and at the states the engine
reached, recorded under tests/golden/), the host check of the shared arithmetic under the sanitizers (make
hierarchy_check), and the null-handle answers."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import hermite_batch_hierarchy_ref as href
import hermite_batch_outcomes_ref as oref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "n-body_amd", "csrc")
CTYPES = {"nbody_hip_hermite_batch*": C.c_void_p, "const float*": C.c_void_p, "nbody_hip_batch_hierarchy_t*": C.c_void_p,
          "nbody_hip_batch_node_t*": C.c_void_p, "nbody_particle_data*": C.c_void_p, "int": C.c_int, "float": C.c_float,
          "size_t": C.c_size_t}
REC_OFFSETS = dict(resolved=0, top_count=4, macro=8, node_count=16, largest=20, min_sep=24, min_p=32, min_q=36, reserved=40)
NODE_OFFSETS = dict(left=0, right=4, parent=8, bodies=12, mass=16, a=24, e=32, r=40, energy=48, reserved=56)
NONE = href.NONE


def test_prototypes_are_bound_and_declared(nb):
    model = open(os.path.join(ROOT, "include", "nbody_hip.h")).read()
    header = open(os.path.join(ROOT, "include", "nbody_hip_hierarchy.h")).read()
    lib = nb._lib.load()
    for sym in ("nbody_hip_batch_hierarchy_set", "nbody_hip_batch_hierarchy_get", "nbody_hip_batch_hierarchy_snapshot"):
        m = re.search(r"NBODY_HIP_API\s+int\s+" + sym + r"\s*\(([^)]*)\)", header)
        assert m, sym
        args = [re.sub(r"\s*\w+$", "", " ".join(a.split())) for a in m.group(1).split(",")]
        res, argtypes = nb._lib.PROTOTYPES[sym]
        assert res is C.c_int and argtypes == [CTYPES[a] for a in args], (sym, args)
        assert getattr(lib, sym).argtypes == argtypes and getattr(lib, sym).restype is C.c_int
        assert not sym.startswith("nbody_hip_hermite_")  # (that set of names is pinned by test_hermite_handles_cpu.py)
    assert model.index("ensemble OUTCOMES") < model.index("ensemble HIERARCHIES") < model.index("ensemble DIAGNOSTICS")
    assert re.search(r"^#define NBODY_HIP_BATCH_HIERARCHY_STOP_ON_RESOLVED 1\s*$", model, re.M)
    assert re.search(r"^#define NBODY_HIP_BATCH_HIERARCHY_MAX 64\s*$", model, re.M)
    assert (nb._lib.BATCH_HIERARCHY_STOP_ON_RESOLVED, nb.BATCH_HIERARCHY_STOP_ON_RESOLVED, nb.BATCH_STOPPED_RESOLVED,
            nb.BATCH_HIERARCHY_MAX) == (1, 1, 4, 64)
    assert nb.BatchHierarchyStruct is nb._lib.BatchHierarchyStruct and nb.BatchNodeStruct is nb._lib.BatchNodeStruct
    assert nb.EnsembleHierarchy is nb.api.EnsembleHierarchy and nb.hierarchy_string is nb.api.hierarchy_string
    assert len(re.findall(r"^#define NBODY_HIP_ABI_VERSION 1\s*$", model, re.M)) == 1
    for word in ("contact (1) wins over escape (3), which wins over resolved (4), which wins over the budget (2)",
                 "a = (G M) / (-2.0 eps)", "ties to the smallest p, then the smallest q", "never overwritten until the next priming",
                 "r > kappa (apo_p + apo_q)", "prime clears the records, the tables and the stop words", "Left out.",
                 "contact (1) wins over escape (3), which wins over the budget"):  # (the last: the OUTCOMES wording stays)
        assert word in " ".join(model.replace(" * ", " ").split()), word


def _declared(model, name):
    body = re.search(r"typedef struct " + name + r" \{(.*?)\} " + name + ";", model, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    out = []
    for decl in body.split(";"):
        decl = " ".join(decl.split())
        if decl:
            ctype = re.match(r"(unsigned int|unsigned long long|double)\b", decl).group(1)
            out += [(n.strip(), ctype) for n in decl[len(ctype):].split(",")]
    return out


def test_record_layouts(nb):
    model = open(os.path.join(ROOT, "include", "nbody_hip.h")).read()
    want = {"unsigned int": C.c_uint, "unsigned long long": C.c_ulonglong, "double": C.c_double}
    for name, S, dt, offsets in (("nbody_hip_batch_hierarchy_t", nb._lib.BatchHierarchyStruct, nb.BATCH_HIERARCHY_DTYPE, REC_OFFSETS),
                                 ("nbody_hip_batch_node_t", nb._lib.BatchNodeStruct, nb.BATCH_NODE_DTYPE, NODE_OFFSETS)):
        declared = [(n, want[t]) for n, t in _declared(model, name)]
        declared = [("reserved", C.c_double * 3) if n == "reserved[3]" else (n, t) for n, t in declared]
        assert [n for n, _ in declared] == [n for n, _ in S._fields_], name
        assert all(a is b or (C.sizeof(a), a._type_) == (C.sizeof(b), b._type_) for (_, a), (_, b) in zip(declared, S._fields_)), name
        assert C.sizeof(S) == 64 and C.alignment(S) == 8
        assert {n: getattr(S, n).offset for n, _ in S._fields_} == offsets
        assert dt.itemsize == 64 and {n: dt.fields[n][1] for n in dt.names} == offsets
        assert [dt.fields[n][0].itemsize for n in dt.names] == [C.sizeof(t) for _, t in S._fields_]
    # the kernel file and the facade assert the same layouts at compile time
    for f in (os.path.join(CSRC, "hermite_batch.hip"), os.path.join(ROOT, "n-body_amd", "facade", "src", "facade_device.cpp")):
        text = " ".join(open(f).read().split())
        assert re.search(r"static_assert\(sizeof\((nbody_hip_batch_hierarchy_t|BatchHierarchy)\) == 64", text), f
        assert re.search(r"static_assert\(sizeof\((nbody_hip_batch_node_t|BatchNode)\) == 64", text), f


def test_python_side_validation(nb):
    e = nb.BlockHermiteEnsemble()
    h = nb.EnsembleHierarchy(e)
    with pytest.raises(nb.ValidationException, match="needs a BlockHermiteEnsemble"):
        nb.EnsembleHierarchy(object())
    with pytest.raises(nb.StateException, match="no layout"):
        h.set(1.0)
    for call in (h.records, h.nodes, lambda: h.snapshot(None), lambda: h.describe(0)):
        with pytest.raises(nb.StateException, match="not primed"):
            call()
    e.setLayout([0, 3, 8, 73])
    for bad, what in ((np.ones(2), "one per system"), (np.ones((3, 1)), "one per system"), (np.ones(4), "one per system"),
                      (np.array(["a"] * 3), "real numbers"), (np.ones(3, complex), "real numbers"),
                      (np.ones(3, bool), "real numbers")):
        with pytest.raises(nb.ValidationException, match=what):
            h.set(bad)
    for value in (-1e-6, float("nan"), float("inf"), -float("inf")):
        with pytest.raises(nb.ValidationException, match="separation radius of system 1 must be non-negative and finite"):
            h.set([1.0, value, 0.0])
        with pytest.raises(nb.ValidationException, match="separation radius of system 0"):
            h.set(value)
        with pytest.raises(nb.ValidationException, match="isolation factor must be non-negative and finite"):
            h.set([1.0, 1.0, 0.0], isolation=value)
    with pytest.raises(nb.ValidationException, match="system 2 has 65 bodies: a hierarchy is examined in systems of at most 64"):
        h.set(1.0)
    for nothing in (None, 0.0, [0, 0, 0]):
        with pytest.raises(nb.ValidationException, match="stop_on_resolved needs a separation radius > 0"):
            h.set(nothing, stop_on_resolved=True)
    assert e._hierarchy is None and e._h is None  # nothing was kept of a refused call, and none reached the library
    h.set([2.0, 0.5, 0], isolation=3, stop_on_resolved=True)  # kept for the handle the priming makes
    r, kappa, flags = e._hierarchy
    assert r.dtype == np.float32 and r.tolist() == [2.0, 0.5, 0.0] and kappa == 3.0 and flags == 1
    h.set(None)
    assert e._hierarchy is None
    e.setLayout([0, 4, 9])
    h.set(3)  # a scalar: every system; integers are real numbers
    assert e._hierarchy[0].tolist() == [3.0, 3.0] and e._hierarchy[1:] == (0.0, 0)
    e.setLayout([0, 4])  # a new layout drops the configuration
    assert e._hierarchy is None
    h.set(1.5)

    def refuse():
        raise nb.ValidationException("refused")
    e._h, e._layout_sent, e._send_hierarchy = object(), True, refuse
    try:
        with pytest.raises(nb.ValidationException, match="refused"):
            h.set(2.5, stop_on_resolved=True)
        assert e._hierarchy[0].tolist() == [1.5] and e._hierarchy[2] == 0
    finally:
        e._h, e._layout_sent = None, False
        del e._send_hierarchy
    assert sorted(n for n in dir(nb.EnsembleHierarchy) if not n.startswith("_")) == ["describe", "nodes", "records", "set", "snapshot"]
    assert sorted(n for n in dir(nb.EnsembleOutcomes) if not n.startswith("_")) == ["records", "set"]


def _tab(n, composites, slots=None):
    t = np.zeros(slots or 2 * n, np.dtype([("left", "<u4"), ("right", "<u4"), ("parent", "<u4"), ("bodies", "<u4")]))
    t["left"][:n] = t["right"][:n] = t["parent"][:n] = NONE
    for k, (a, b) in enumerate(composites):
        t["left"][n + k], t["right"][n + k], t["parent"][n + k] = a, b, NONE
        t["parent"][a] = t["parent"][b] = n + k
    return t


def test_hierarchy_string(nb):
    hs = nb.hierarchy_string
    assert hs(_tab(3, []), 3) == "0 1 2"                      # an ionisation
    assert hs(_tab(3, [(0, 1)]), 3) == "[0 1] 2"
    assert hs(_tab(3, [(0, 2)]), 3) == "[0 2] 1"              # an exchange
    assert hs(_tab(3, [(1, 2)]), 3) == "0 [1 2]"
    assert hs(_tab(3, [(1, 2), (0, 3)]), 3) == "[0 [1 2]]"
    assert hs(_tab(3, [(0, 1), (2, 3)]), 3) == "[[0 1] 2]"    # the child that holds the lowest body comes first
    assert hs(_tab(4, [(2, 3), (0, 1)]), 4) == "[0 1] [2 3]"  # the top nodes by their lowest body, not by their ids
    assert hs(_tab(4, [(1, 3), (0, 4), (2, 5)]), 4) == "[[0 [1 3]] 2]"
    assert hs(_tab(5, [(3, 4), (1, 5)]), 5) == "0 [1 [3 4]] 2"
    assert hs(_tab(2, [], slots=4), 2) == "0 1" and hs(_tab(1, [], slots=2), 1) == "0"
    a, b = _tab(4, [(0, 1), (2, 3)]), _tab(4, [(2, 3), (0, 1)])
    assert hs(a, 4) == hs(b, 4)                               # the same outcome whatever the order the pairs were made in
    full = np.zeros(6, nb.BATCH_NODE_DTYPE)
    for k in ("left", "right", "parent"):
        full[k] = _tab(3, [(0, 2)])[k]
    assert hs(full, 3) == "[0 2] 1"
    bad = _tab(3, [(0, 1)])
    bad["left"][3] = 3
    with pytest.raises(nb.ValidationException, match="not a node table"):
        hs(bad, 3)
    with pytest.raises(nb.ValidationException, match="at least 3 rows"):
        hs(_tab(1, []), 3)


# ---- the restatement ----------------------------------------------------------------------------------------------------------
def _rows(rows):
    a = np.asarray(rows, np.float64)
    return a[:, 0:3], a[:, 3:6], a[:, 6]


def test_known_answers_of_the_restatement():
    """the circular binary of two masses 2 at distance 1 (G = 1): w = 2, eps = -2, a = 1, h = 2, e = 0, all exact"""
    X, V, m = _rows(href.BIN + [[100, 0, 0, 5, 0, 0, 1]])
    ev = href.evaluate(X, V, m, 1.0, 10.0, 5.0)
    c = ev.nodes[3]
    assert href.forest(ev) == "[0 1] 2" and (c.left, c.right, c.parent, c.bodies) == (0, 1, NONE, 2)
    assert (c.m, c.a, c.e, c.r, c.energy) == (4.0, 1.0, 0.0, 1.0, -2.0)
    assert (ev.resolved, ev.top_count, ev.node_count, ev.largest, ev.min_sep, ev.min_p, ev.min_q) == (1, 2, 4, 2, 100.0, 2, 3)
    assert href.evaluate(X, V, m, 1.0, 100.0, 0.0).resolved == 0   # r = r_sep: the comparison is strict
    assert href.evaluate(X, V, m, 1.0, 10.0, 100.0).resolved == 0  # r = kappa apo likewise
    assert href.evaluate(X, V, m, 1.0, 10.0, 99.0).resolved == 1
    # a general bound pair: a = 1, e = 0.9 (G M = 1) at the eccentric anomalies E: the elements come back at every phase
    for E in np.linspace(0.05, 2 * np.pi - 0.05, 23):
        rr = 1 - 0.9 * np.cos(E)
        x, y = np.cos(E) - 0.9, np.sqrt(1 - 0.81) * np.sin(E)
        vx, vy = -np.sin(E) / rr, np.sqrt(1 - 0.81) * np.cos(E) / rr
        X, V, m = _rows([[0.5 * x, 0.5 * y, 0, 0.5 * vx, 0.5 * vy, 0, 0.5], [-0.5 * x, -0.5 * y, 0, -0.5 * vx, -0.5 * vy, 0, 0.5]])
        ev = href.evaluate(X, V, m, 1.0, 1.0, 0.0)
        c = ev.nodes[2]
        assert ev.top_count == 1 and abs(c.a - 1) < 1e-13 and abs(c.e - 0.9) < 1e-13 and abs(c.energy + 0.5) < 1e-13 and abs(c.r - rr) < 1e-14
    for name, c in href.snapshot_cases().items():
        X, V, m = href.state_of(c["ic"])
        ev = href.evaluate(X, V, m, 1.0, c["r_sep"], c["kappa"])
        assert (ev.top_count, ev.node_count, ev.resolved) == (c["K"], c["nodes"], c["resolved"]), name
        assert c["forest"] is None or href.forest(ev) == c["forest"], name
    ev = href.evaluate(*href.state_of(href.snapshot_cases()["mirrored 2+2"]["ic"]), 1.0, 5, 2)
    assert ev.nodes[4].a == ev.nodes[5].a and (ev.nodes[4].left, ev.nodes[4].right, ev.nodes[5].left, ev.nodes[5].right) == (0, 1, 2, 3)
    ev = href.evaluate(*href.state_of(href.snapshot_cases()["cold chain of 64"]["ic"]), 1.0, 1, 0)
    assert all(b.e == 1.0 for b in ev.nodes[64:]) and [b.bodies for b in ev.nodes[64:]] == list(range(2, 65))
    # NaN input: never a candidate, never resolved, never the smallest separation
    X, V, m = _rows([[np.nan, 0, 0, 0, 0, 0, 1], [1, 0, 0, 0, 0, 0, 1]])
    ev = href.evaluate(X, V, m, 1.0, 0.5, 0.0)
    assert (ev.top_count, ev.resolved, ev.min_sep, ev.min_p) == (2, 0, None, NONE)


def _against_exact(tag, X, V, m, G, r_sep, kappa):
    ev, bd, ex = href.evaluate(X, V, m, G, r_sep, kappa), href.bounded(X, V, m, G, r_sep, kappa), href.exact(X, V, m, G, r_sep, kappa)
    ok, why = href.clear(bd)
    assert ok, (tag, why)
    assert href.forest(ev) == href.forest(bd) == href.forest(ex), tag
    assert [(b.left, b.right, b.parent, b.bodies) for b in ev.nodes] == [(b.left, b.right, b.parent, b.bodies) for b in ex.nodes], tag
    assert (ev.resolved, ev.top, ev.largest, ev.min_p, ev.min_q) == (ex.resolved, ex.top, ex.largest, ex.min_p, ex.min_q), tag
    vals, _ = href.node_values(ev, href.FLOAT)
    same, tol = href.node_values(bd, href.BOUNDED)
    want, _ = href.node_values(ex, href.EXACT)
    assert np.array_equal(vals, same), tag  # (the bounded run carries the restatement's own values)
    assert (np.abs(vals - want) <= tol).all(), (tag, np.argwhere(np.abs(vals - want) > tol)[:3])
    if ev.min_sep is not None:
        assert abs(float(ev.min_sep) - float(ex.min_sep)) <= bd.min_sep.e, tag
    with np.errstate(divide="ignore", invalid="ignore"):
        return float(np.nanmax(np.where(tol > 0, np.abs(vals - want) / tol, 0.0)))


def test_the_restatement_is_within_its_bound_of_exact_arithmetic():
    """every snapshot case of the GPU tests at its state: restatement within its own bound of exact arithmetic, the same
    forest, every decision clear"""
    for name, c in href.snapshot_cases().items():
        worst = _against_exact(name, *href.state_of(c["ic"]), 1.0, c["r_sep"], c["kappa"])
        print(f"{name}: |restatement - exact| / bound at most {worst:.3f}", flush=True)
    for name, ic in (("fly-by", oref.flyby_ic()), ("2+2", href.two_plus_two_ic())):
        _against_exact(name, *href.state_of(ic), 1.0, 2.0, 2.0)


def test_the_restatement_on_the_states_the_engine_reached():
    """the same on the recorded states (tests/golden/hermite_batch_hierarchy_states.npz: X and V after every macro step of
    the walk and of the eight fly-bys, which the GPU tests assert the engine still reaches bit for bit): at every boundary
    up to the first resolved one the restatement lies within its bound of exact arithmetic and every decision is clear"""
    w = href.WALK
    Xs, Vs, m = href.recorded("walk")
    assert Xs.shape == Vs.shape == (w["macros"], 7, 3) and Xs.dtype == np.float64 and m.dtype == np.float32
    firsts = []
    for (a, b), r_sep, want in (((0, 3), w["r_sep"][0], "[0 1] 2"), ((3, 7), w["r_sep"][1], "[0 1] [2 3]")):
        for k in range(w["macros"]):
            _against_exact(("walk", a, k + 1), Xs[k, a:b], Vs[k, a:b], m[a:b], 1.0, r_sep, w["kappa"])
            ev = href.evaluate(Xs[k, a:b], Vs[k, a:b], m[a:b], 1.0, r_sep, w["kappa"])
            if ev.resolved:
                assert href.forest(ev) == want
                firsts.append(k + 1)
                break
    assert firsts == [5, 8]
    Xs, Vs, m = href.recorded("fly")
    assert Xs.shape == (href.FLY["macros"], 24, 3)
    firsts = []
    for s, r_sep in enumerate(href.FLY_RSEP):
        a, b = 3 * s, 3 * s + 3
        first = 0
        for k in range(href.FLY["macros"] if r_sep > 0 else 0):
            _against_exact(("fly-by", s, k + 1), Xs[k, a:b], Vs[k, a:b], m[a:b], 1.0, r_sep, href.FLY["kappa"])
            if href.evaluate(Xs[k, a:b], Vs[k, a:b], m[a:b], 1.0, r_sep, href.FLY["kappa"]).resolved:
                first = k + 1
                break
        firsts.append(first)
    assert firsts == [2, 3, 4, 5, 7, 8, 0, 0]


def test_clear_refuses_a_marginal_decision():
    """the condition has teeth: a piece a few ulps beyond the radius, an energy that nearly cancels, and two candidates
    whose a differ in the last bits are not clear"""
    X, V, m = _rows(href.BIN + [[100, 0, 0, 5, 0, 0, 1]])
    assert href.clear(href.bounded(X, V, m, 1.0, 10.0, 5.0))[0]
    Xc = X.copy()
    Xc[2, 0] = 100 * (1 + 3e-12)
    ok, why = href.clear(href.bounded(Xc, V, m, 1.0, 100.0, 0.0))
    assert not ok and "criterion 0" in why
    Vc = V.copy()
    Vc[2, 0] = np.sqrt(2 * 5.0 / 100.0) * (1 + 1e-12)  # the single on a parabola but for 1e-12
    ok, why = href.clear(href.bounded(X, Vc, m, 1.0, 10.0, 0.0))
    assert not ok and "eps < 0" in why
    s = 1 + 1e-13  # two binaries whose a differ by 1e-13
    X, V, m = _rows([[-10.5, 0, 0, -3, -1, 0, 2], [-9.5, 0, 0, -3, 1, 0, 2], [9.5, 0, 0, 3, -s, 0, 2], [10.5, 0, 0, 3, s, 0, 2]])
    ok, why = href.clear(href.bounded(X, V, m, 1.0, 5.0, 2.0))
    assert not ok and "smallest a" in why


# ---- the shared arithmetic under the sanitizers ---------------------------------------------------------------------------------
def test_hierarchy_check_builds_and_passes():
    r = subprocess.run(["make", "-C", CSRC, "hierarchy_check"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "hierarchy_check: ok" in r.stdout and "FAIL" not in r.stdout
    mk = open(os.path.join(CSRC, "Makefile")).read()
    rule = mk[mk.index("../lib/hermite_batch_hierarchy_check:"):]
    assert "-fsanitize=address,undefined -fno-sanitize-recover=all" in rule.split("\n\n")[0]
    assert re.search(r"^hierarchy_check: \.\./lib/hermite_batch_hierarchy_check$", mk, re.M)
    assert "hierarchy_check" in mk[mk.index(".PHONY"):] and "../lib/hermite_batch_hierarchy_check" in mk[mk.index("clean:"):]
    src = open(os.path.join(CSRC, "hermite_batch_hierarchy_check.cpp")).read()
    assert re.search(r"^int main\(\)", src, re.M) and '#include "hermite_batch_hierarchy_common.h"' in src and "long double" in src
    common = re.sub(r"//.*", "", open(os.path.join(CSRC, "hermite_batch_hierarchy_common.h")).read())
    for word in ("hip/", "__global__", "__shfl", "threadIdx", "float4", "__shared__"):  # plain C++: kernel and check share it
        assert word not in common, word
    assert common.count("NBH_NO_CONTRACT") >= 5 and "hierarchy_model(" in common
    kernel = open(os.path.join(CSRC, "hermite_batch.hip")).read()
    for word in ('#include "hermite_batch_hierarchy_common.h"', "hier_pair(", "hier_composite(", "hier_ecc(", "hier_pair_resolved(",
                 "hier_key_less(", "batch_hierarchy_test<EXT>", "batch_hierarchy_snapshot_kernel"):
        assert word in kernel, word
    test_fn = kernel[kernel.index("batch_hierarchy_test(const ResidentSystem"):kernel.index("// The snapshot (nbody_hip_batch_hierarchy_snapshot)")]
    assert "atomic" not in test_fn and "while" not in test_fn
    inc = open(os.path.join(CSRC, "hermite_batch_resident_body.inc")).read()
    assert inc.count("if constexpr (HIERARCHY)") >= 4
    assert len(re.findall(r"HIERARCHY = false", kernel)) == 2 and len(re.findall(r"HIERARCHY = true", kernel)) == 1


# ---- the null-handle answers ------------------------------------------------------------------------------------------------------
def test_null_handle_answers(nb):
    lib = nb._lib.load()
    rec = (nb.BatchHierarchyStruct * 2)()
    nodes = (nb.BatchNodeStruct * 12)()
    radii = (C.c_float * 2)(1.0, 1.0)
    for rc in (lib.nbody_hip_batch_hierarchy_set(None, None, 0.0, 0),
               lib.nbody_hip_batch_hierarchy_set(None, C.cast(radii, C.c_void_p), 1.0, 1),
               lib.nbody_hip_batch_hierarchy_get(None, C.cast(rec, C.c_void_p), 2, C.cast(nodes, C.c_void_p), 12),
               lib.nbody_hip_batch_hierarchy_get(None, C.cast(rec, C.c_void_p), 2, None, 0),
               lib.nbody_hip_batch_hierarchy_snapshot(None, None, C.cast(rec, C.c_void_p), 2, C.cast(nodes, C.c_void_p), 12)):
        assert rc == nb._lib.ERR_STATE
        assert lib.nbody_hip_last_error().startswith(b"null block-step Hermite ensemble")

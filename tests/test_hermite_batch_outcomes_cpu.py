"""The ensemble outcomes (nbody_hip_batch_outcomes_set / _get, EnsembleOutcomes), the parts that need no GPU: the
prototypes against the new header, the record's layout through ctypes, numpy and the header, the Python-side validation,
the restatement's known answers and its own error against exact rational arithmetic for every case of the GPU tests (at
the initial states and at the states the engine reached, recorded under tests/golden/), the
host check of the shared arithmetic under the sanitizers (make outcomes_check), and the null-handle answers."""
import ctypes as C
import math
import os
import re
import subprocess

import numpy as np
import pytest

import hermite_batch_outcomes_ref as oref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "n-body_amd", "csrc")
CTYPES = {"nbody_hip_hermite_batch*": C.c_void_p, "const float*": C.c_void_p, "nbody_hip_batch_outcome_t*": C.c_void_p,
          "int": C.c_int, "size_t": C.c_size_t}
OFFSETS = dict(escaped=0, escaper=4, macro=8, r=16, vr=24, energy=32, rest_mass=40, reserved=48, reserved2=56)


def test_prototypes_are_bound_and_declared(nb):
    model = open(os.path.join(ROOT, "include", "nbody_hip.h")).read()
    header = open(os.path.join(ROOT, "include", "nbody_hip_outcomes.h")).read()
    lib = nb._lib.load()
    for sym in ("nbody_hip_batch_outcomes_set", "nbody_hip_batch_outcomes_get"):
        m = re.search(r"NBODY_HIP_API\s+int\s+" + sym + r"\s*\(([^)]*)\)", header)
        assert m, sym
        args = [re.sub(r"\s*\w+$", "", " ".join(a.split())) for a in m.group(1).split(",")]
        res, argtypes = nb._lib.PROTOTYPES[sym]
        assert res is C.c_int and argtypes == [CTYPES[a] for a in args], (sym, args)
        assert getattr(lib, sym).argtypes == argtypes and getattr(lib, sym).restype is C.c_int
        assert not sym.startswith("nbody_hip_hermite_")  # (that set of names is pinned by test_hermite_handles_cpu.py)
    assert model.index("ensemble OUTCOMES") > model.index("ensemble EVENTS")
    assert model.index("ensemble OUTCOMES") < model.index("ensemble DIAGNOSTICS")
    assert re.search(r"^#define NBODY_HIP_BATCH_OUTCOMES_STOP_ON_ESCAPE 1\s*$", model, re.M)
    assert (nb._lib.BATCH_OUTCOMES_STOP_ON_ESCAPE, nb.BATCH_OUTCOMES_STOP_ON_ESCAPE, nb.BATCH_STOPPED_ESCAPE) == (1, 1, 3)
    assert nb.BatchOutcomeStruct is nb._lib.BatchOutcomeStruct and nb.EnsembleOutcomes is nb.api.EnsembleOutcomes
    assert len(re.findall(r"^#define NBODY_HIP_ABI_VERSION 1\s*$", model, re.M)) == 1
    for word in ("off = 32, 16, 8, 4, 2, 1", "eight waves", "never overwritten until the next priming", "Limitation.",
                 "contact (1) wins over escape (3), which wins over the budget", "A massless body can escape",
                 "prime clears all records"):
        assert word in " ".join(model.split()), word


def test_record_layout(nb):
    model = open(os.path.join(ROOT, "include", "nbody_hip.h")).read()
    body = re.search(r"typedef struct nbody_hip_batch_outcome_t \{(.*?)\} nbody_hip_batch_outcome_t;", model, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    declared = []
    for decl in body.split(";"):
        decl = " ".join(decl.split())
        if decl:
            ctype = re.match(r"(unsigned int|unsigned long long|double)\b", decl).group(1)
            declared += [(n.strip(), ctype) for n in decl[len(ctype):].split(",")]
    want = {"unsigned int": C.c_uint, "unsigned long long": C.c_ulonglong, "double": C.c_double}
    S = nb._lib.BatchOutcomeStruct
    assert [(n, want[t]) for n, t in declared] == list(S._fields_)
    assert [n for n, _ in declared][:7] == ["escaped", "escaper", "macro", "r", "vr", "energy", "rest_mass"]
    assert C.sizeof(S) == 64 and C.alignment(S) == 8
    assert {n: getattr(S, n).offset for n, _ in S._fields_} == OFFSETS
    dt = nb.BATCH_OUTCOME_DTYPE
    assert dt.itemsize == 64 and {n: dt.fields[n][1] for n in dt.names} == OFFSETS
    assert [dt.fields[n][0].itemsize for n in dt.names] == [C.sizeof(t) for _, t in S._fields_]
    # the kernel file and the facade assert the same layout at compile time
    for f in (os.path.join(CSRC, "hermite_batch.hip"), os.path.join(ROOT, "n-body_amd", "facade", "src", "facade_device.cpp")):
        text = " ".join(open(f).read().split())
        assert re.search(r"static_assert\(sizeof\((nbody_hip_batch_outcome_t|BatchOutcome)\) == 64", text), f


def test_python_side_validation(nb):
    e = nb.BlockHermiteEnsemble()
    o = nb.EnsembleOutcomes(e)
    with pytest.raises(nb.ValidationException, match="needs a BlockHermiteEnsemble"):
        nb.EnsembleOutcomes(object())
    with pytest.raises(nb.StateException, match="no layout"):
        o.set(1.0)
    with pytest.raises(nb.StateException, match="not primed"):
        o.records()
    e.setLayout([0, 3, 8, 9])
    for bad, what in ((np.ones(2), "one per system"), (np.ones((3, 1)), "one per system"), (np.ones(4), "one per system"),
                      (np.array(["a"] * 3), "real numbers"), (np.ones(3, complex), "real numbers"),
                      (np.ones(3, bool), "real numbers")):
        with pytest.raises(nb.ValidationException, match=what):
            o.set(bad)
    for value in (-1e-6, float("nan"), float("inf"), -float("inf")):
        with pytest.raises(nb.ValidationException, match="escape radius of system 1 must be non-negative and finite"):
            o.set([1.0, value, 0.0])
        with pytest.raises(nb.ValidationException, match="escape radius of system 0"):
            o.set(value)
    for nothing in (None, 0.0, [0, 0, 0]):
        with pytest.raises(nb.ValidationException, match="stop_on_escape needs an escape radius > 0"):
            o.set(nothing, stop_on_escape=True)
    assert e._outcomes is None and e._h is None  # nothing was kept of a refused call, and none reached the library
    o.set([2.0, 0, 0.5], stop_on_escape=True)   # kept for the handle the priming makes
    r, flags = e._outcomes
    assert r.dtype == np.float32 and r.tolist() == [2.0, 0.0, 0.5] and flags == 1
    o.set(3)                                     # a scalar: every system; integers are real numbers
    assert e._outcomes[0].tolist() == [3.0, 3.0, 3.0] and e._outcomes[1] == 0
    o.set(None)
    assert e._outcomes is None
    o.set(1.5)
    e.setLayout([0, 4])                          # a new layout drops the configuration
    assert e._outcomes is None
    # a send that fails leaves the configuration the handle has, not the one it never got
    o.set(1.5)

    def refuse():
        raise nb.ValidationException("refused")
    e._h, e._layout_sent, e._send_outcomes = object(), True, refuse
    try:
        with pytest.raises(nb.ValidationException, match="refused"):
            o.set(2.5, stop_on_escape=True)
        assert e._outcomes[0].tolist() == [1.5] and e._outcomes[1] == 0
    finally:
        e._h, e._layout_sent = None, False
        del e._send_outcomes
    # the ensemble's own public surface is unchanged: the companion holds the two methods
    assert sorted(n for n in dir(nb.EnsembleOutcomes) if not n.startswith("_")) == ["records", "set"]


# ---- the restatement's known answers ------------------------------------------------------------------------------------
def _rows(rows):
    a = np.asarray(rows, np.float64)
    return a[:, 0:3], a[:, 3:6], a[:, 6]


def test_known_answers_of_the_restatement():
    # two equal bodies receding radially: r = 4, |w| = 1, G M = 1: e = 1/2 - 1/4 = v_inf^2 / 2 exactly
    X, V, m = _rows([[2, 0, 0, 0.5, 0, 0, 0.5], [-2, 0, 0, -0.5, 0, 0, 0.5]])
    b = oref.evaluate(X, V, m, 1.0, 3.0)
    assert (b.count, b.lowest) == (2, 0)
    assert b.r.tolist() == [4.0, 4.0] and b.vr.tolist() == [1.0, 1.0] and b.e.tolist() == [0.25, 0.25] and b.rest.tolist() == [0.5, 0.5]
    assert oref.evaluate(X, V, m, 1.0, 4.0).count == 0          # r == r_esc: the comparison is strict
    assert oref.evaluate(X, V, m, 1.0, 0.0).count == 0          # r_esc = 0: no test
    # a general hyperbola: v_inf = 0.3 seen at r = 10, 0.7 rad off the radius: e = v_inf^2 / 2 analytically
    vinf, r = 0.3, 10.0
    w = math.sqrt(vinf * vinf + 2.0 / r)
    c, s = math.cos(0.7), math.sin(0.7)
    X, V, m = _rows([[0.25 * r, 0, 0, 0.25 * w * c, 0.25 * w * s, 0, 0.75], [-0.75 * r, 0, 0, -0.75 * w * c, -0.75 * w * s, 0, 0.25]])
    b = oref.evaluate(X, V, m, 1.0, 5.0)
    assert (b.count, b.lowest) == (2, 0)
    assert np.allclose(b.e, 0.5 * vinf * vinf, rtol=0, atol=1e-15) and np.allclose(b.r, r, rtol=0, atol=1e-14)
    assert np.allclose(b.vr, w * c, rtol=0, atol=1e-15) and b.rest.tolist() == [0.25, 0.75]
    # the bound e = 0.9 pair (a = 1, G M = 1) with r_esc = 1.5 inside the apocentre 1.9: at every phase of the orbit
    # e = -1/2, so no body ever escapes -- also where r > r_esc and the pair is moving outward
    for E in np.linspace(0.05, 2 * math.pi - 0.05, 41):   # the eccentric anomaly
        rr = 1 - 0.9 * math.cos(E)
        x, y = math.cos(E) - 0.9, math.sqrt(1 - 0.81) * math.sin(E)
        vx, vy = -math.sin(E) / rr, math.sqrt(1 - 0.81) * math.cos(E) / rr
        X, V, m = _rows([[0.5 * x, 0.5 * y, 0, 0.5 * vx, 0.5 * vy, 0, 0.5], [-0.5 * x, -0.5 * y, 0, -0.5 * vx, -0.5 * vy, 0, 0.5]])
        b = oref.evaluate(X, V, m, 1.0, 1.5)
        assert b.count == 0 and np.allclose(b.e, -0.5, rtol=0, atol=1e-13) and np.allclose(b.r, rr, rtol=0, atol=1e-14)
        if rr > 1.5 and E < math.pi:
            assert (b.dw > 0).all()   # beyond the radius and receding: only the energy holds it back
    # an unbound body beyond r_esc that approaches
    X, V, m = _rows([[2, 0, 0, -0.5, 0, 0, 0.5], [-2, 0, 0, 0.5, 0, 0, 0.5]])
    b = oref.evaluate(X, V, m, 1.0, 3.0)
    assert b.count == 0 and b.e.tolist() == [0.25, 0.25] and b.vr.tolist() == [-1.0, -1.0]
    # M_r = 0 for the body that holds the whole mass; the massless one escapes
    X, V, m = _rows([[0, 0, 0, 0, 0, 0, 1.0], [4, 0, 0, 1, 0, 0, 0.0]])
    b = oref.evaluate(X, V, m, 1.0, 3.0)
    assert (b.count, b.lowest) == (1, 1) and b.rest.tolist() == [0.0, 1.0]
    assert (b.r[0], b.vr[0], b.e[0]) == (0.0, 0.0, 0.0) and (b.r[1], b.vr[1], b.e[1]) == (4.0, 1.0, 0.25)
    assert oref.evaluate(X, V, np.zeros(2), 1.0, 3.0).count == 0     # nobody has mass
    # NaN input: every comparison is false
    Xn = X.copy()
    Xn[0, 1] = np.nan
    assert oref.evaluate(Xn, V, m, 1.0, 3.0).count == 0
    assert oref.evaluate(X, V, m, np.nan, 3.0).count == 0
    # n = 1
    b = oref.evaluate([[5.0, 0, 0]], [[3.0, 0, 0]], [1.0], 1.0, 1.0)
    assert (b.count, b.lowest) == (0, oref.NONE)


def test_the_sum_order_of_the_restatement():
    """model_sum against the three stages written out as loops, at sizes on both sides of every edge of the order"""
    rng = np.random.default_rng(3)
    for n in (1, 2, 63, 64, 65, 511, 512, 513, 1025, 4096):
        t = rng.normal(size=n) * 10.0 ** rng.integers(-6, 6, n)
        lanes = [0.0] * 512
        for i in range(n):
            lanes[i % 512] = lanes[i % 512] + float(t[i])
        for w in range(8):
            off = 32
            while off:
                for lane in range(off):
                    lanes[64 * w + lane] = lanes[64 * w + lane] + lanes[64 * w + lane + off]
                off //= 2
        total = lanes[0]
        for w in range(1, 8):
            total = total + lanes[64 * w]
        assert float(oref.model_sum(t)) == total, n
    assert [oref.sum_ops(n) for n in (1, 512, 513, 4096)] == [14, 14, 15, 21]


def _check_against_exact(tag, X, V, m, G, r_esc):
    b, bd = oref.evaluate(X, V, m, G, r_esc), oref.bounds(X, V, m, G)
    n = len(m)
    pick = range(n) if n <= 64 else sorted(set(np.flatnonzero(b.escapes).tolist() + list(range(0, n, 97)) + [n - 1]))
    ex = oref.exact(X, V, m, G, pick)
    worst = [0.0, 0.0, 0.0]
    for i, (r, vr, e, rest, dw) in ex.items():
        if rest <= 0.0:
            assert not b.escapes[i] and b.rest[i] == 0.0
            continue
        for k, (got, want, tol) in enumerate(((b.r[i], r, bd.dr[i]), (b.vr[i], vr, bd.dvr[i]), (b.e[i], e, bd.de[i]))):
            assert abs(got - want) <= tol, (tag, i, k, got, want, tol)
            worst[k] = max(worst[k], abs(got - want) / tol if tol else 0.0)
        assert abs(b.dw[i] - dw) <= bd.ddw[i] and abs(b.rest[i] - rest) <= bd.dM[i], (tag, i)
        if b.escapes[i]:
            assert bd.rel[i] < oref.REL_MAX, (tag, i, bd.rel[i])  # (what the bound's second-order factor rests on)
    assert oref.clear(b, bd, r_esc).all(), (tag, np.flatnonzero(~oref.clear(b, bd, r_esc))[:5])
    print(f"{tag}: n {n}, kappa {bd.kappa[0]:.3g} {bd.kappa[1]:.3g} {bd.kappa[2]:.3g}, |restatement - exact| / bound "
          f"{worst[0]:.2f} {worst[1]:.2f} {worst[2]:.2f}, escaping {b.count}", flush=True)
    return b


def test_the_restatement_is_within_its_bound_of_exact_arithmetic(nb):
    """every case of the GPU tests at its initial state and at states drifted along the initial velocities (not states
    the engine visits -- those are the next test's -- but with the same scales and cancellations, and the bodies of interest
    cross the escape radius along the way): restatement within the derived bound of exact arithmetic, every decision clear"""
    seen = set()
    for name, c in oref.cases(nb).items():
        X, V, m = oref.state_of(c["ic"])
        for k in range(0, c["macros"] + 1, 2):
            Xk = X + V * (k * np.float32(c["dt"]))
            b = _check_against_exact(f"{name} @ {k}", Xk, V, m, c["G"], c["r_esc"])
            if b.count:
                seen.add(name)
                assert (b.count, b.lowest) == c["expect"], name
    assert seen == {n for n, c in oref.cases(nb).items() if c["expect"] is not None}


def _first_escape(tag, Xs, Vs, m, G, r_esc):
    """the boundaries the engine examines, in turn, up to the first escape: -> (macro index or 0, Bodies or None)"""
    for k in range(len(Xs)):
        b = _check_against_exact(f"{tag} after macro step {k + 1}", Xs[k], Vs[k], m, G, r_esc)
        if b.count:
            return k + 1, b
    return 0, None


def test_the_restatement_on_the_states_the_engine_reached(nb):
    """the same on the recorded states (tests/golden/hermite_batch_outcomes_states.npz: X and V after every macro step of
    every case and of the eight fly-bys, which the GPU test asserts the engine still reaches bit for bit): at every
    boundary up to the first escape the restatement lies within the derived bound of exact arithmetic and every decision
    is clear; the first escape is the one the case expects"""
    for k, (name, c) in enumerate(oref.cases(nb).items()):
        Xs, Vs, m = oref.recorded(k)
        assert Xs.shape == Vs.shape == (c["macros"], m.size, 3) and Xs.dtype == np.float64
        assert np.array_equal(m, c["ic"]["mass"]) and m.dtype == np.float32
        macro, b = _first_escape(name, Xs, Vs, m, c["G"], c["r_esc"])
        assert (None if b is None else (b.count, b.lowest)) == c["expect"], (name, macro)
    Xs, Vs, m = oref.recorded("fly")
    assert Xs.shape == (oref.FLY["macros"], 24, 3)
    for s, r_esc in enumerate(oref.FLY_RESC):
        if r_esc > 0:
            macro, b = _first_escape(f"fly-by {s}", Xs[:, 3 * s:3 * s + 3], Vs[:, 3 * s:3 * s + 3], m[3 * s:3 * s + 3], oref.FLY["G"], r_esc)
            assert macro == oref.FLY_MACRO[s] and (b is None or (b.count, b.lowest) == (1, 2)), (s, macro)


def test_clear_refuses_a_marginal_decision():
    """the condition has teeth: a body a few ulps beyond the radius, or with an energy that nearly cancels, is not clear"""
    X, V, m = _rows([[2, 0, 0, 0.5, 0, 0, 0.5], [-2, 0, 0, -0.5, 0, 0, 0.5]])
    bd = oref.bounds(X, V, m, 1.0)
    assert oref.clear(oref.evaluate(X, V, m, 1.0, 3.0), bd, 3.0).all()
    r_esc = float(np.nextafter(np.float32(4.0), np.float32(0.0)))  # the float below r = 4: a margin of 2.4e-7 is still clear
    assert oref.clear(oref.evaluate(X, V, m, 1.0, r_esc), bd, r_esc).all()
    Xc = X * (1 + 3e-12)                                           # 1.2e-11 beyond r_esc = 4: not clear
    b = oref.evaluate(Xc, V, m, 1.0, 4.0)
    assert b.count == 2 and not oref.clear(b, oref.bounds(Xc, V, m, 1.0), 4.0).any()
    Vc = V * math.sqrt(0.5) * (1 + 1e-12)                          # e = 1e-12 / 2: not clear
    b = oref.evaluate(X, Vc, m, 1.0, 3.0)
    assert b.count == 2 and 0 < b.e[0] < 1e-11 and not oref.clear(b, oref.bounds(X, Vc, m, 1.0), 3.0).any()


# ---- the shared arithmetic under the sanitizers -------------------------------------------------------------------------
def test_outcomes_check_builds_and_passes():
    r = subprocess.run(["make", "-C", CSRC, "outcomes_check"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "hermite_batch_outcomes_check: ok" in r.stdout and "FAIL" not in r.stdout
    mk = open(os.path.join(CSRC, "Makefile")).read()
    rule = mk[mk.index("../lib/hermite_batch_outcomes_check:"):]
    assert "-fsanitize=address,undefined -fno-sanitize-recover=all" in rule.split("\n\n")[0]
    assert re.search(r"^outcomes_check: \.\./lib/hermite_batch_outcomes_check$", mk, re.M)
    src = open(os.path.join(CSRC, "hermite_batch_outcomes_check.cpp")).read()
    assert re.search(r"^int main\(\)", src, re.M) and '#include "hermite_batch_outcomes_common.h"' in src
    common = re.sub(r"//.*", "", open(os.path.join(CSRC, "hermite_batch_outcomes_common.h")).read())
    for word in ("hip/", "__global__", "__shfl", "threadIdx", "float4"):  # plain C++: the kernel and the check share it
        assert word not in common, word
    kernel = open(os.path.join(CSRC, "hermite_batch.hip")).read()
    assert '#include "hermite_batch_outcomes_common.h"' in kernel and "outcome_body(" in kernel and "outcome_body_add(" in kernel


# ---- the null-handle answers ---------------------------------------------------------------------------------------------
def test_null_handle_answers(nb):
    lib = nb._lib.load()
    out = (nb.BatchOutcomeStruct * 2)()
    assert lib.nbody_hip_batch_outcomes_set(None, None, 0) == nb._lib.ERR_STATE
    assert lib.nbody_hip_last_error().startswith(b"null block-step Hermite ensemble")
    radii = (C.c_float * 2)(1.0, 1.0)
    assert lib.nbody_hip_batch_outcomes_set(None, C.cast(radii, C.c_void_p), 1) == nb._lib.ERR_STATE
    assert lib.nbody_hip_last_error().startswith(b"null block-step Hermite ensemble")
    assert lib.nbody_hip_batch_outcomes_get(None, C.cast(out, C.c_void_p), 2) == nb._lib.ERR_STATE
    assert lib.nbody_hip_last_error().startswith(b"null block-step Hermite ensemble")

"""The ensemble mergers (nbody_hip_batch_mergers_set / _apply / _get, EnsembleMergers), the parts that need no GPU: the
prototypes against the new header, the two structs' layouts through ctypes, numpy and the header, the flag values, the
Python-side validation and the refusals' wording, the null-handle answers, the numpy restatement
(tests/hermite_batch_mergers_ref.py) against exact rational arithmetic on the GPU test's cases, and the host check of the
shared arithmetic under the sanitizers (make mergers_check), whose printed cases the restatement reproduces."""
import ctypes as C
import os
import re
import subprocess
from fractions import Fraction

import numpy as np
import pytest

import hermite_batch_cases as bc
import hermite_batch_events_cases as ec
import hermite_batch_mergers_ref as mref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "n-body_amd", "csrc")
CTYPES = {"nbody_hip_hermite_batch*": C.c_void_p, "nbody_hip_batch_merger_state_t*": C.c_void_p,
          "nbody_hip_batch_merger_t*": C.c_void_p, "unsigned int*": C.c_void_p, "int": C.c_int, "size_t": C.c_size_t}
SYMS = ("nbody_hip_batch_mergers_set", "nbody_hip_batch_mergers_apply", "nbody_hip_batch_mergers_get")
STATE_OFFSETS = dict(n_live=0, n_mergers=4, flags=8, reserved=12)
ENTRY_OFFSETS = dict(slot_a=0, slot_b=4, id_a=8, id_b=12, moved_from=16, contact_tick=20, contact_macro=24, contact_d2=32,
                     radius=36, mass=40, delta_ke=48, delta_pe=56)


@pytest.fixture(autouse=True)
def _restates_this_interface(nb):
    """the restatement restates THIS interface: its "none", its flag and the fields of its log entries are the library's.
    Every test of the file starts here, those of the restatement's own arithmetic included."""
    assert mref.NONE == nb.BATCH_EVENT_NONE and nb.BATCH_MERGER_BAD_RECORD == 1
    s = mref.System(np.zeros((2, 3)), np.zeros((2, 3)), [1, 1], [0, 0])
    entry = mref.merge(s, 0, 1, 1.0, 0.0)
    assert set(nb.BATCH_MERGER_ENTRY_DTYPE.names) <= set(entry) and callable(nb.EnsembleMergers.apply)


def test_prototypes_are_bound_and_declared(nb):
    model = open(os.path.join(ROOT, "include", "nbody_hip.h")).read()
    header = open(os.path.join(ROOT, "include", "nbody_hip_mergers.h")).read()
    lib = nb._lib.load()
    for sym in SYMS:
        m = re.search(r"NBODY_HIP_API\s+int\s+" + sym + r"\s*\(([^)]*)\)", header)
        assert m, sym
        args = [re.sub(r"\s*\w+$", "", " ".join(a.split())) for a in m.group(1).split(",")]
        res, argtypes = nb._lib.PROTOTYPES[sym]
        want = [nb._lib.PROTOTYPES["nbody_hip_hermite_batch_advance"][1][1] if a == "nbody_particle_data*" else CTYPES[a]
                for a in args]
        assert res is C.c_int and argtypes == want, (sym, args)
        assert getattr(lib, sym).argtypes == argtypes and getattr(lib, sym).restype is C.c_int
        assert not sym.startswith("nbody_hip_hermite_")  # (that set of names is pinned by test_hermite_handles_cpu.py)
    order = [model.index("ensemble " + w) for w in ("EVENTS", "OUTCOMES", "HIERARCHIES", "MERGERS", "DIAGNOSTICS")]
    assert order == sorted(order)
    flat = " ".join(model.split())
    for word in ("sticky spheres", "not at the contact tick", "the volume rule", "keeps that slot's id",
                 "FROM THE VALUES AS STORED", "One merger per system per pass", "no mergers inside a launch",
                 "prime clears the log, the ids and the live counts", "set_layout drops the configuration"):
        assert word in flat, word


def test_flag_values_and_abi_version(nb):
    model = open(os.path.join(ROOT, "include", "nbody_hip.h")).read()
    assert re.search(r"^#define NBODY_HIP_BATCH_MERGERS_ON 1\s*$", model, re.M)
    assert re.search(r"^#define NBODY_HIP_BATCH_MERGER_BAD_RECORD 1\s*$", model, re.M)
    assert (nb._lib.BATCH_MERGERS_ON, nb.BATCH_MERGERS_ON, nb._lib.BATCH_MERGER_BAD_RECORD, nb.BATCH_MERGER_BAD_RECORD) == (1, 1, 1, 1)
    assert len(re.findall(r"^#define NBODY_HIP_ABI_VERSION 1\s*$", model, re.M)) == 1
    assert nb._lib.load().nbody_hip_abi_version() == 1
    assert nb.EnsembleMergers is nb.api.EnsembleMergers and nb.BatchMergerStruct is nb._lib.BatchMergerStruct
    assert nb.BatchMergerStateStruct is nb._lib.BatchMergerStateStruct


def _declared(model, name):
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), model, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    out = []
    for decl in body.split(";"):
        decl = " ".join(decl.split())
        if decl:
            ctype = re.match(r"(unsigned int|unsigned long long|double|float)\b", decl).group(1)
            out += [(n.strip(), ctype) for n in decl[len(ctype):].split(",")]
    return out


def test_struct_layouts(nb):
    model = open(os.path.join(ROOT, "include", "nbody_hip.h")).read()
    want = {"unsigned int": C.c_uint, "unsigned long long": C.c_ulonglong, "double": C.c_double, "float": C.c_float}
    S = nb._lib.BatchMergerStateStruct
    assert _declared(model, "nbody_hip_batch_merger_state_t") == [("n_live", "unsigned int"), ("n_mergers", "unsigned int"),
                                                                  ("flags", "unsigned int"), ("reserved[5]", "unsigned int")]
    assert [n for n, _ in S._fields_] == list(STATE_OFFSETS) and C.sizeof(S) == 32 and C.alignment(S) == 4
    assert {n: getattr(S, n).offset for n, _ in S._fields_} == STATE_OFFSETS
    dt = nb.BATCH_MERGER_STATE_DTYPE
    assert dt.itemsize == 32 and {n: dt.fields[n][1] for n in dt.names} == STATE_OFFSETS
    E = nb._lib.BatchMergerStruct
    assert [(n, want[t]) for n, t in _declared(model, "nbody_hip_batch_merger_t")] == list(E._fields_)
    assert C.sizeof(E) == 64 and C.alignment(E) == 8
    assert {n: getattr(E, n).offset for n, _ in E._fields_} == ENTRY_OFFSETS
    dt = nb.BATCH_MERGER_ENTRY_DTYPE
    assert dt.itemsize == 64 and {n: dt.fields[n][1] for n in dt.names} == ENTRY_OFFSETS
    assert [dt.fields[n][0].itemsize for n in dt.names] == [C.sizeof(t) for _, t in E._fields_]
    assert nb.BATCH_MERGER_DTYPE.names == ("system",) + dt.names
    # the kernel file and the facade assert the same layouts at compile time
    for f in (os.path.join(CSRC, "hermite_batch.hip"), os.path.join(ROOT, "n-body_amd", "facade", "src", "facade_device.cpp")):
        text = " ".join(open(f).read().split())
        assert re.search(r"static_assert\(sizeof\((nbody_hip_batch_merger_t|BatchMerger)\) == 64", text), f
        assert re.search(r"static_assert\(sizeof\((nbody_hip_batch_merger_state_t|BatchMergerState)\) == 32", text), f


def test_python_side_validation(nb):
    e = nb.BlockHermiteEnsemble()
    m = nb.EnsembleMergers(e)
    with pytest.raises(nb.ValidationException, match="needs a BlockHermiteEnsemble"):
        nb.EnsembleMergers(object())
    with pytest.raises(nb.StateException, match="no layout"):
        m.set()
    for call in (m.records, m.log, m.ids, m.alive, lambda: m.apply(None), lambda: m.run(None, 2)):
        with pytest.raises(nb.StateException, match="not primed"):
            call()
    e.setLayout([0, 3, 8, 9])
    for bad in (1, "yes", None, 2.0):
        with pytest.raises(nb.ValidationException, match="enabled must be True or False"):
            m.set(bad)
    assert e._mergers is None and e._h is None  # nothing was kept of a refused call, and none reached the library
    m.set()
    assert e._mergers == 1
    m.set(False)
    assert e._mergers is None
    m.set(True)
    e.setLayout([0, 4])  # a new layout drops the configuration
    assert e._mergers is None
    with pytest.raises(nb.ValidationException, match="every must be at least 1"):
        m.run(None, 4, every=0)
    # the refusals of apply before any call into the library: on a handle that looks primed
    e._h = object()
    try:
        with pytest.raises(nb.StateException, match="mergers are not configured"):
            m.apply(None)
        e._mergers = 1
        for events in (None, (None, None, 2), (np.zeros(4, np.float32), None, 1)):
            e._events = events
            with pytest.raises(nb.StateException, match="mergers need setEvents\\(radii, stop_on_contact=True\\)"):
                m.apply(None)
    finally:
        e._h, e._events, e._mergers = None, None, None
    # a send that fails leaves the configuration the handle has

    def refuse():
        raise nb.ValidationException("refused")
    e._h, e._layout_sent, e._send_mergers = object(), True, refuse
    try:
        with pytest.raises(nb.ValidationException, match="refused"):
            m.set(True)
        assert e._mergers is None
    finally:
        e._h, e._layout_sent = None, False
        del e._send_mergers
    assert sorted(n for n in dir(nb.EnsembleMergers) if not n.startswith("_")) == ["alive", "apply", "ids", "log", "records",
                                                                                   "run", "set"]


def test_null_handle_answers(nb):
    lib = nb._lib.load()
    state = (nb.BatchMergerStateStruct * 2)()
    assert lib.nbody_hip_batch_mergers_set(None, 1) == nb._lib.ERR_STATE
    assert lib.nbody_hip_last_error().startswith(b"null block-step Hermite ensemble")
    assert lib.nbody_hip_batch_mergers_apply(None, None) == nb._lib.ERR_STATE
    assert lib.nbody_hip_last_error().startswith(b"null block-step Hermite ensemble")
    assert lib.nbody_hip_batch_mergers_get(None, C.cast(state, C.c_void_p), 2, None, None, 5) == nb._lib.ERR_STATE
    assert lib.nbody_hip_last_error().startswith(b"null block-step Hermite ensemble")


# ---- the restatement ------------------------------------------------------------------------------------------------------
def test_slots_and_compaction_of_the_restatement():
    assert mref.slots(0, 1, 2) == (0, 1, mref.NONE, 1) and mref.slots(1, 0, 2) == (0, 1, mref.NONE, 1)
    assert mref.slots(0, 1, 3) == (0, 1, 2, 2) and mref.slots(2, 0, 3) == (0, 2, mref.NONE, 2) and mref.slots(1, 2, 3) == (1, 2, mref.NONE, 2)
    assert mref.slots(3, 255, 257) == (3, 255, 256, 256) and mref.slots(255, 3, 1025) == (3, 255, 1024, 1024)
    for bad in ((0, 0, 3), (0, 3, 3), (3, 0, 3), (mref.NONE, mref.NONE, 3), (0, mref.NONE, 3), (0, 1, 1), (0, 1, 0)):
        assert mref.slots(*bad) is None, bad
    assert mref.concerned(1, 0) and not any(mref.concerned(s, t) for s, t in ((0, 0), (2, 0), (3, 0), (4, 0), (1, 1), (1, 2)))
    # two equal bodies head-on: V exactly 0, X exactly the midpoint; the chain of ids over two mergers of three bodies
    pos, vel, m = ec.head_on()
    s = mref.System(pos, vel, m, [0.02, 0.02])
    e = mref.merge(s, 1, 0, 1.0, 0.05)
    assert s.n == 1 and s.pos[0].tolist() == [0, 0, 0] and s.vel[0].tolist() == [0, 0, 0] and s.mass.tolist() == [1.0, 0.0]
    assert s.ids.tolist() == [0, mref.NONE] and e["moved_from"] == mref.NONE and e["mass"] == 1.0
    assert e["radius"] == np.float32(np.cbrt(2 * np.float64(np.float32(0.02)) ** 3))
    assert e["delta_ke"] == -2 * 0.5 * (0.5 * 0.0625) and e["delta_pe"] == 0.25 / np.sqrt(1.0 + np.float64(np.float32(0.05) * np.float32(0.05)))
    s = mref.System(np.array([[0, 0, 0], [1, 0, 0], [2, 0, 0]]), np.zeros((3, 3)), [1, 1, 2], [0.6, 0.6, 0.6])
    e1 = mref.merge(s, 0, 1, 1.0, 0.0)
    assert (s.n, s.ids.tolist(), e1["moved_from"], s.mass.tolist(), s.pos[:2, 0].tolist()) == (2, [0, 2, mref.NONE], 2, [2, 2, 0], [0.5, 2.0])
    e2 = mref.merge(s, 1, 0, 1.0, 0.0)
    assert (s.n, s.ids.tolist(), e2["id_a"], e2["id_b"], s.mass[0], s.pos[0, 0]) == (1, [0, mref.NONE, mref.NONE], 0, 2, 4.0, 1.25)
    assert mref.merge(s, 0, 1, 1.0, 0.0) is None and len(s.log) == 2
    # two massless bodies: the plain mean
    s = mref.System([[1, 2, 3], [3, 2, -3]], [[1, 0, -1], [0, 1, 1]], [0, 0], [0, 0])
    mref.merge(s, 0, 1, 1.0, 0.0)
    assert s.pos[0].tolist() == [2, 2, 0] and s.vel[0].tolist() == [0.5, 0.5, 0] and s.mass[0] == 0


def _case_system(nb, name, n, pair, ext):
    pos, vel, m = bc.arrays_of(mref.case_ic(nb, n, pair))
    rng = np.random.default_rng(n)
    radii = mref.case_radii(n, pair)
    lo = (lambda a: (a * rng.uniform(-2.0 ** -25, 2.0 ** -25, a.shape)).astype(np.float32)) if ext else (lambda a: None)
    return mref.System(pos, vel, m, radii, lo(pos), lo(vel), ext=ext)


@pytest.mark.parametrize("name,n,pair", mref.CASES, ids=[c[0] for c in mref.CASES])
def test_the_restatement_is_within_its_bound_of_exact_arithmetic(nb, name, n, pair):
    for ext in (False, True):
        for G, eps in ((1.7, 0.05), (1.0, 0.0)):
            s = _case_system(nb, name, n, pair, ext)
            X, V, m = s.X().copy(), s.V().copy(), s.mass.astype(np.float64).copy()
            e = mref.merge(s, pair[1], pair[0], G, eps)
            lo, hi = e["slot_a"], e["slot_b"]
            M, Xm, Vm = mref.exact(X, V, m, lo, hi)
            assert Fraction(float(e["mass"])) == M and s.mass[lo] == np.float32(float(M))
            got = np.concatenate([s.X()[lo], s.V()[lo]])
            for c, want in enumerate(Xm + Vm):
                # one rounding of the stored precision: fp32, or 2^-46 |value| for hi + lo
                tol = abs(want) * (Fraction(2) ** -46 if ext else Fraction(2) ** -24)
                assert abs(Fraction(float(got[c])) - want) <= tol, (name, ext, c)
            eps2 = np.float64(np.float32(eps) * np.float32(eps))
            dke, dpe = mref.exact_deltas(s.mass[lo].astype(np.float64), s.X()[lo], s.V()[lo], X, V, m, n, lo, hi, G, eps2)
            assert abs(Fraction(float(e["delta_ke"])) - dke) <= Fraction(mref.ke_bound(e)), (name, ext)
            assert abs(Fraction(float(e["delta_pe"])) - dpe) <= Fraction(mref.pe_bound(e, G)), (name, ext)
            assert e["moved_from"] == (mref.NONE if hi == n - 1 else n - 1) and s.n == n - 1
            assert sorted(s.ids[:n - 1].tolist()) == [k for k in range(n) if k != hi] and s.ids[n - 1] == mref.NONE
            print(f"{name} ext {ext} eps {eps}: |dke - exact| / bound {float(abs(Fraction(float(e['delta_ke'])) - dke)) / max(mref.ke_bound(e), 1e-300):.3f}, "
                  f"|dpe - exact| / bound {float(abs(Fraction(float(e['delta_pe'])) - dpe)) / max(mref.pe_bound(e, G), 1e-300):.3f}", flush=True)


def test_the_triples_case_cannot_pass_vacuously():
    """300 colliding triples, by the restatement alone over the eight macro steps of the GPU test: at least 50 systems
    have a first contact (so they stop and merge) and at least 50 never touch; the first are exactly the flagged ones"""
    ics, radii, hit = ec.colliding_triples(300)
    assert all((r > 0).sum() == (2 if h else 0) for r, h in zip(radii, hit))
    c = bc.TRIPLE
    touched = np.zeros(300, bool)
    for s in range(300):
        pos, vel, m = bc.arrays_of(ics[s])
        tr, _ = ec.restatement_run(pos, vel, m, c["G"], c["eps"], c["dt_max"], c["max_level"], 8, radii=radii[s], until_contact=True)
        if tr.contact is not None:
            assert tr.contact[1] != tr.contact[2] and tr.contact[3] < 8, s  # (a star and anybody)
            touched[s] = True
    print("touch within 8 macro steps:", int(touched.sum()), "never:", int((~touched).sum()), flush=True)
    assert touched.sum() >= 50 and (~touched).sum() >= 50
    assert (touched == hit).all()  # (every flagged system touches in time: the GPU test's count is not left to chance)


# ---- the shared arithmetic under the sanitizers -------------------------------------------------------------------------
def test_mergers_check_builds_passes_and_agrees_with_the_restatement():
    r = subprocess.run(["make", "-C", CSRC, "mergers_check"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "hermite_batch_mergers_check: ok" in r.stdout and "FAIL" not in r.stdout
    mk = open(os.path.join(CSRC, "Makefile")).read()
    rule = mk[mk.index("../lib/hermite_batch_mergers_check:"):]
    assert "-fsanitize=address,undefined -fno-sanitize-recover=all" in rule.split("\n\n")[0]
    assert re.search(r"^mergers_check: \.\./lib/hermite_batch_mergers_check$", mk, re.M)
    src = open(os.path.join(CSRC, "hermite_batch_mergers_check.cpp")).read()
    assert re.search(r"^int main\(\)", src, re.M) and '#include "hermite_batch_mergers_common.h"' in src
    common = re.sub(r"//.*", "", open(os.path.join(CSRC, "hermite_batch_mergers_common.h")).read())
    for word in ("hip/", "__global__", "__shfl", "threadIdx", "float4"):  # plain C++: the kernel and the check share it
        assert word not in common, word
    kernel = open(os.path.join(CSRC, "hermite_batch.hip")).read()
    for word in ('#include "hermite_batch_mergers_common.h"', "merger_slots(", "merger_merge(", "merger_radius(",
                 "merger_delta_ke(", "merger_pair_delta(", "merger_delta_pe("):
        assert word in kernel, word
    cases = mref.parse_check_output(r.stdout)
    assert len(cases) == 32 and {c["n"] for c in cases} == {2, 3, 5, 257, 300, 1025}
    for c in cases:
        b = np.array(c["bodies"])
        assert b.shape == (c["n"], 14)
        s = mref.System(b[:, 0:3], b[:, 6:9], b[:, 12], b[:, 13], b[:, 3:6], b[:, 9:12], ext=bool(c["ext"]))
        e = mref.merge(s, c["i"], c["j"], c["G"], c["eps"])
        o, lo = c["out"], e["slot_a"]
        assert (o["lo"], o["hi"], o["moved"], o["dead"]) == (lo, e["slot_b"], -1 if e["moved_from"] == mref.NONE else e["moved_from"], c["n"] - 1)
        stored = [v for k in range(3) for v in (s.pos[lo, k], s.pos_lo[lo, k])] + [v for k in range(3) for v in (s.vel[lo, k], s.vel_lo[lo, k])]
        mine = [e["mass"], s.mass[lo]] + stored + [e["radius"], e["delta_ke"], e["others"], e["delta_pe"]]
        for k, (a, w) in enumerate(zip(mine, o["values"])):
            if k == 14:  # the radius: cbrt is no IEEE operation -- within one fp32 ulp
                assert abs(float(a) - w) <= np.spacing(np.float32(w)), (c["name"], a, w)
            else:  # everything else is the same sequence of IEEE operations: equal in its bits
                assert float(a) == w, (c["name"], c["ext"], k, float(a).hex(), w.hex())

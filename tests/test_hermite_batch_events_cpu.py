"""The ensemble events (nbody_hip_hermite_batch_set_events / _events / _running, BlockHermiteEnsemble.setEvents / events /
running), the parts that need no GPU: the prototypes against the headers, the record's layout through ctypes, the
Python-side validation, the key rule restated in numpy, the null-handle answers, and the conditions on the inputs that
tests/test_hermite_batch_events_gpu.py relies on, by the restatement alone."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import hermite_batch_events_cases as ec

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("set_events", "events", "running")
CTYPES = {"nbody_hip_hermite_batch*": C.c_void_p, "const float*": C.c_void_p, "const unsigned long long*": C.c_void_p,
          "nbody_hip_batch_event_t*": C.c_void_p, "int": C.c_int, "size_t": C.c_size_t, "size_t*": C.POINTER(C.c_size_t)}


def test_prototypes_are_bound_and_declared(nb):
    model = open(os.path.join(ROOT, "include", "nbody_hip.h")).read()
    header = open(os.path.join(ROOT, "include", "nbody_hip_events.h")).read()
    lib = nb._lib.load()
    for name in NAMES:
        sym = "nbody_hip_hermite_batch_" + name
        m = re.search(r"NBODY_HIP_API\s+int\s+" + sym + r"\s*\(([^)]*)\)", header)
        assert m, sym
        args = [re.sub(r"\s*\w+$", "", " ".join(a.split())) for a in m.group(1).split(",")]
        res, argtypes = nb._lib.PROTOTYPES[sym]
        assert res is C.c_int and argtypes == [CTYPES[a] for a in args], (sym, args)
        assert getattr(lib, sym).argtypes == argtypes and getattr(lib, sym).restype is C.c_int
    # the model, the flags and the struct stand next to the ensemble block; the version of the ABI is unchanged
    assert model.index("ensemble EVENTS") > model.index("nbody_hip_hermite_batch_get_state_f64(")
    assert re.search(r"^#define NBODY_HIP_BATCH_EVENTS_TRACK_CLOSEST 1\s*$", model, re.M)
    assert re.search(r"^#define NBODY_HIP_BATCH_EVENTS_STOP_ON_CONTACT 2\s*$", model, re.M)
    assert (nb._lib.BATCH_EVENTS_TRACK_CLOSEST, nb._lib.BATCH_EVENTS_STOP_ON_CONTACT) == (1, 2)
    assert len(re.findall(r"^#define NBODY_HIP_ABI_VERSION 1\s*$", model, re.M)) == 1
    for word in ("STRICTLY LESS", "fma(dx, dx, fma(dy, dy, dz * dz))", "bits(d2) << 32 | i << 12 | j", "ACTIVE side",
                 "COMPLETES the macro step", "prime clears all records"):
        assert word in model, word


def test_record_layout(nb):
    model = open(os.path.join(ROOT, "include", "nbody_hip.h")).read()
    body = re.search(r"typedef struct nbody_hip_batch_event_t \{(.*?)\} nbody_hip_batch_event_t;", model, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    declared = []
    for decl in body.split(";"):
        decl = " ".join(decl.split())
        if decl:
            ctype = re.match(r"(unsigned int|unsigned long long|float)\b", decl).group(1)
            declared += [(n.strip(), ctype) for n in decl[len(ctype):].split(",")]
    want = {"unsigned int": C.c_uint, "unsigned long long": C.c_ulonglong, "float": C.c_float}
    S = nb._lib.BatchEventStruct
    assert [(n, want[t]) for n, t in declared] == list(S._fields_)
    assert C.sizeof(S) == 64 and C.alignment(S) == 8
    offsets = dict(stopped=0, reserved=4, macro_steps_done=8, closest_d2=16, closest_i=20, closest_j=24, closest_tick=28,
                   closest_macro=32, contact_d2=40, contact_i=44, contact_j=48, contact_tick=52, contact_macro=56)
    assert {n: getattr(S, n).offset for n, _ in S._fields_} == offsets
    dt = nb.api.BATCH_EVENT_DTYPE
    assert dt.itemsize == 64 and {n: dt.fields[n][1] for n in dt.names} == offsets
    assert [dt.fields[n][0].itemsize for n in dt.names] == [C.sizeof(t) for _, t in S._fields_]
    assert nb.api.BATCH_EVENT_NONE == ec.NONE == 0xFFFFFFFF


def test_python_side_validation(nb):
    e = nb.BlockHermiteEnsemble()
    with pytest.raises(nb.StateException, match="no layout"):
        e.setEvents(track_closest=True)
    for call in (e.events, e.running):
        with pytest.raises(nb.StateException, match="not primed"):
            call()
    e.setLayout([0, 3, 8])
    ok = np.full(8, 0.25)
    for bad, what in ((ok[:7], "one per body"), (np.zeros((8, 1)), "one per body"), (np.zeros(9), "one per body"),
                      (np.array(["a"] * 8), "real numbers"), (ok.astype(complex), "real numbers"),
                      (np.zeros(8, bool), "real numbers")):
        with pytest.raises(nb.ValidationException, match=what):
            e.setEvents(radii=bad)
    for value in (-1e-6, float("nan"), float("inf"), -float("inf")):
        r = ok.copy()
        r[5] = value
        with pytest.raises(nb.ValidationException, match="radius of body 5 must be non-negative and finite"):
            e.setEvents(radii=r)
    for bad, what in (([1, 2, 3], "array of 2 values"), ([1.0, 2.0], "must be integers"), ([1, -1], "must not be negative"),
                      (np.zeros((2, 1), np.int32), "array of 2 values")):
        with pytest.raises(nb.ValidationException, match=what):
            e.setEvents(max_macro_steps=bad)
    with pytest.raises(nb.ValidationException, match="needs radii"):
        e.setEvents(stop_on_contact=True)
    assert e._events is None and e._h is None  # every refusal came before any call into the library
    e.setEvents(radii=ok, max_macro_steps=5, track_closest=True, stop_on_contact=True)
    r, lim, flags = e._events
    assert r.dtype == np.float32 and r.tolist() == [0.25] * 8 and lim.dtype == np.uint64 and lim.tolist() == [5, 5]
    assert flags == 3
    e.setEvents(max_macro_steps=np.array([0, 7], np.uint8))
    assert e._events[0] is None and e._events[1].tolist() == [0, 7] and e._events[2] == 0
    e.setEvents()
    assert e._events == (None, None, 0)
    e.setEvents(radii=ok)
    e.setLayout([0, 4, 8])  # a new layout drops the configuration
    assert e._events is None
    e.close()


def test_null_handle_is_a_state_error(nb):
    lib = nb._lib.load()
    r = np.zeros(4, np.float32)
    out = np.zeros(1, nb.api.BATCH_EVENT_DTYPE)
    n = C.c_size_t(7)
    for call in (lambda: lib.nbody_hip_hermite_batch_set_events(None, r.ctypes.data, None, 1),
                 lambda: lib.nbody_hip_hermite_batch_set_events(None, None, None, 0),
                 lambda: lib.nbody_hip_hermite_batch_events(None, out.ctypes.data, 1),
                 lambda: lib.nbody_hip_hermite_batch_running(None, C.byref(n))):
        assert call() == nb._lib.ERR_STATE
        assert b"null block-step Hermite ensemble" in lib.nbody_hip_last_error()
    assert n.value == 7 and not out.view(np.uint8).any()


# ---- the key rule ------------------------------------------------------------------------------------------------------
def test_key_rule():
    rng = np.random.default_rng(11)
    d2 = np.concatenate([rng.uniform(0, 4, 200).astype(np.float32), np.float32([0.0, 0.0, 1e-45, 1e-38, 3e38, 1.0, 1.0, 1.0])])
    i = np.concatenate([rng.integers(0, 4096, 200), [0, 4095, 1, 2, 3, 7, 7, 6]])
    j = np.concatenate([rng.integers(0, 4096, 200), [4095, 0, 1, 2, 3, 9, 8, 4095]])
    keys = [ec.key(a, b, c) for a, b, c in zip(d2, i, j)]
    # ordering by d2, then i, then j -- bits(d2) order as unsigned integers because d2 >= 0
    by_key = sorted(range(len(keys)), key=lambda k: keys[k])
    by_tuple = sorted(range(len(keys)), key=lambda k: (float(d2[k]), int(i[k]), int(j[k])))
    assert by_key == by_tuple
    for k in range(len(keys)):
        a, b, c = ec.unkey(keys[k])
        assert (a.view(np.uint32), b, c) == (d2[k].view(np.uint32), i[k], j[k])
        assert keys[k] < 2 ** 64 - 1  # (the "none" key is above every pair's)
    assert ec.key(0.0, 0, 1) < ec.key(0.0, 1, 0) < ec.key(1e-45, 0, 0)
    assert ec.key(np.float32(np.inf), 0, 0) >> 32 == 0x7F800000  # (a d2 that is not finite is never a key)


def test_folds_are_strictly_less_in_time():
    a, b = ec.key(0.25, 3, 5), ec.key(0.25, 3, 5)
    rec = ec.fold_closest(None, a, 0, 100)
    assert rec == (a, 0, 100)
    assert ec.fold_closest(rec, b, 0, 200) == rec  # a tie: the earliest block step keeps it
    assert ec.fold_closest(rec, ec.key(0.25, 3, 6), 1, 8) == rec
    assert ec.fold_closest(rec, ec.key(0.25, 3, 4), 1, 8) == (ec.key(0.25, 3, 4), 1, 8)  # the key, not d2 alone
    assert ec.fold_closest(rec, None, 2, 1) == rec
    first = ec.fold_contact(None, a, 4, 7)
    assert first == (a, 4, 7) and ec.fold_contact(first, ec.key(0.01, 0, 1), 4, 8) == first  # once
    assert ec.fold_contact(None, None, 0, 1) is None


def test_tracker_on_a_hand_made_schedule():
    """three bodies on a line, the Tracker shown two block steps: ties by (d, i, j), the mirror pair is no rival, the first
    contact is taken from the first block step that has one and is its smallest key"""
    x0 = np.array([[0.0, 0, 0], [1.0, 0, 0], [3.0, 0, 0]])
    tr = ec.Tracker(3, radii=[0.3, 0.3, 0.0])
    tr.step(0, 4, np.array([0, 1]), x0)  # (0, 1) and (1, 0) at d = 1: the key rule takes (0, 1)
    assert tr.closest == (1.0, 0, 1, 0, 4) and tr.contact is None and tr.runner_up == 2.0
    x1 = np.array([[0.0, 0, 0], [0.5, 0, 0], [0.75, 0, 0]])
    tr.step(0, 8, np.array([1, 2]), x1)  # (1, 2) and (2, 1) at 0.25; (1, 0) at 0.5 is in contact (rs = 0.6), (1, 2) is too
    assert tr.closest == (0.25, 1, 2, 0, 8) and tr.contact == (0.25, 1, 2, 0, 8)
    assert tr.runner_up == 0.5
    tr.step(1, 2, np.array([2]), x1)  # (2, 1) at 0.25 again, later: not strictly less
    assert tr.contact == (0.25, 1, 2, 0, 8) and tr.closest == (0.25, 1, 2, 0, 8)
    tr.step(1, 4, np.array([0]), x1 * 0.5)  # (0, 1) at 0.25: the same d2, a smaller key -- the fold compares keys
    assert tr.contact == (0.25, 1, 2, 0, 8) and tr.closest == (0.25, 0, 1, 1, 4)


# ---- the conditions on the inputs of the GPU cases, by the restatement alone -------------------------------------------
def test_head_on_copies_cross_their_thresholds_by_a_factor_of_two():
    c = ec.HEAD_ON
    t_cross = ec.head_on_crossing_time()
    radii, dts = ec.head_on_copies(t_cross)
    assert 0.5 < t_cross < 1.0 and len(set(radii[:6].tolist())) == 6
    pos, vel, m = ec.head_on()
    for s in range(8):
        tr, _ = ec.restatement_run(pos, vel, m, c["G"], c["eps"], float(dts[s]), c["max_level"], c["macros"],
                                   radii=[radii[s]] * 2, until_contact=True)
        rs = float(np.float32(radii[s]) + np.float32(radii[s]))
        if s < 6:
            assert tr.contact is not None and tr.contact[3] == s and tr.contact[1:3] == (0, 1), (s, tr.contact)
            assert all(d >= 2.0 * rs for mac, _, d in tr.samples if mac < s), s
            assert min(d for mac, _, d in tr.samples if mac == s) <= 0.5 * rs, s
        else:
            assert tr.contact is None and (rs == 0.0 or all(d >= 2.0 * rs for _, _, d in tr.samples)), s


def test_close_pairs_are_the_closest_by_a_margin(nb):
    for n, i, j in ((1025, 3, 1024), (600, 259, 515)):
        ic = dict(nb.ic.plummer(n, seed=42))
        ic = ec.with_close_pair(ic, i, j, 2e-3)
        pos = np.stack([ic["pos_x"], ic["pos_y"], ic["pos_z"]], 1).astype(np.float64)
        d = np.sqrt(((pos[:, None, :] - pos[None, :, :]) ** 2).sum(-1))
        d[np.arange(n), np.arange(n)] = np.inf
        assert np.unravel_index(d.argmin(), d.shape) == (i, j) and abs(d[i, j] - 2e-3) < 1e-6
        d[i, j] = d[j, i] = np.inf
        assert d.min() > 5 * 2e-3
    # where the source index j = bx 1024 + s 256 + lane puts them: (block bx, slot s, lane)
    where = lambda j: (j // 1024, (j % 1024) // 256, j % 256)  # noqa: E731
    assert (where(3), where(1024)) == ((0, 0, 3), (1, 0, 0)) and (where(259), where(515)) == ((0, 1, 3), (0, 2, 3))

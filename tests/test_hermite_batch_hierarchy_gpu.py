"""The ensemble HIERARCHIES (nbody_hip_batch_hierarchy_set / _get / _snapshot, EnsembleHierarchy; include/nbody_hip.h
"ensemble HIERARCHIES") on a real GPU.

Two oracles.  Bit equality: a system with hierarchies configured is, up to its stop, the plain ensemble's system, array
by array and counter by counter.  The restatement: tests/hermite_batch_hierarchy_ref.py runs the model in numpy fp64 on
the state the engine itself hands back (the primed state for the snapshots, advance(1) + getExtendedState of a plain
ensemble for the runs), so it predicts the forest, the resolved verdict, top_count and the first resolving boundary
exactly, and every node's mass, a, e, r, energy and min_sep within the bound it carries through its own operations (the
bound itself, no multiple of it; tests/test_hermite_batch_hierarchy_cpu.py holds the restatement to the same bound
against exact arithmetic on a CPU).  Every decision at every examined boundary must be clear by the restatement alone."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import hermite_batch_cases as bc
import hermite_batch_hierarchy_ref as href
import hermite_batch_outcomes_ref as oref
from gpu_util import to_device

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = ("pos_x", "pos_y", "pos_z", "vel_x", "vel_y", "vel_z", "acc_x", "acc_y", "acc_z", "acc_old_x", "acc_old_y", "acc_old_z",
     "mass")
COUNTERS = ("block_steps", "body_steps", "level_steps", "floor_hits", "macro_steps", "current_tick", "last_n_active",
            "max_level")
NONE = href.NONE


def _direct(nb, g, eps):
    c = nb.DirectForceCalculator()
    c.setGravitationalConstant(g)
    c.setSofteningParameter(eps)
    return c


def _ensemble(nb, ics, eps, precision="fp32", dt=1.0 / 16, max_level=16, g=1.0, hierarchy=None, outcomes=None, events=None,
              order="hoe"):
    """-> (d, ens, offsets, hier, out), primed; hierarchy / outcomes / events: the keywords of EnsembleHierarchy.set /
    EnsembleOutcomes.set / setEvents, sent after the layout and before the priming, in `order`"""
    ic, offsets = nb.ic.concat(ics)
    d, _ = to_device(nb, ic)
    ens = nb.BlockHermiteEnsemble()
    ens.setParameters(0.02, 0.01, max_level)
    ens.setStatePrecision(precision)
    ens.setLayout(offsets)
    hier, out = nb.EnsembleHierarchy(ens), nb.EnsembleOutcomes(ens)
    for which in order:
        if which == "h" and hierarchy is not None:
            hier.set(**hierarchy)
        if which == "o" and outcomes is not None:
            out.set(**outcomes)
        if which == "e" and events is not None:
            ens.setEvents(**events)
    ens.prime(d, _direct(nb, g, eps), dt)
    return d, ens, offsets, hier, out


def _whole(d, ens):
    out = {k: getattr(d, k).cpu().numpy().view(np.uint32).copy() for k in F}
    st = ens.getState()
    out.update(jerk=st["jerk"].view(np.uint32).copy(), levels=st["levels"].copy(), ticks=st["ticks"].copy(),
               want=st["want"].view(np.uint32).copy())
    if ens.getStatePrecision() == "extended":
        x, v = ens.getExtendedState(d)
        out.update(X=x.view(np.uint64).copy(), V=v.view(np.uint64).copy())
    info = ens.info()
    out["info"] = {k: info[k] for k in COUNTERS}
    return out


def _cut(whole, ens, offsets, s):
    a, b = int(offsets[s]), int(offsets[s + 1])
    one = {k: v[a:b] for k, v in whole.items() if k != "info"}
    info = ens.info(s)
    one["info"] = {k: info[k] for k in COUNTERS}
    return one


def _assert_equal(tag, got, ref):
    assert got.keys() == ref.keys(), tag
    for k in ref:
        if k == "info":
            assert got[k] == ref[k], (tag, got[k], ref[k])
        else:
            assert got[k].shape == ref[k].shape, (tag, k)
            bad = np.flatnonzero((got[k] != ref[k]).reshape(len(ref[k]), -1).any(axis=1))
            assert bad.size == 0, (tag, k, f"{bad.size} bodies differ, first {bad[:5]}")


def _same(tag, a, b):
    assert a.dtype == b.dtype and a.shape == b.shape, tag
    assert np.ascontiguousarray(a).tobytes() == np.ascontiguousarray(b).tobytes(), (tag, a, b)


def _table(nodes, off, s):
    return nodes[2 * int(off[s]):2 * int(off[s + 1])]


# ---- 1. the snapshot against the restatement on hand-made states ----------------------------------------------------------
@pytest.mark.parametrize("precision", ["fp32", "extended"])
def test_snapshot_against_the_restatement(nb, ctx, precision):
    cases = href.snapshot_cases()
    assert list(cases) == ["binary and a receding single", "the single approaching", "the single inside r_sep", "not isolated",
                           "permuted", "hierarchical triple", "mirrored 2+2", "three singles", "n = 2 bound", "n = 2 unbound",
                           "massless bound to massive", "two massless", "33 bodies", "cold chain of 64"]
    seen = 0
    for kappa in sorted({c["kappa"] for c in cases.values()}):
        names = [k for k, c in cases.items() if c["kappa"] == kappa]
        lone = href._ic([[5, 0, 0, 3, 0, 0, 1]])
        ics = [cases[k]["ic"] for k in names] + [lone, cases[names[0]]["ic"]]  # n = 1; and a system with r_sep = 0
        r_sep = np.array([cases[k]["r_sep"] for k in names] + [1.0, 0.0], np.float32)
        d, ens, off, hier, _ = _ensemble(nb, ics, 0.0, precision, hierarchy=dict(separation_radius=r_sep, isolation=kappa))
        own = hier.records()
        assert all(href.is_none(r) for r in own) and not np.frombuffer(hier.nodes().tobytes(), np.uint8).any()
        rec, nodes = hier.snapshot(d)
        assert rec.dtype == nb.BATCH_HIERARCHY_DTYPE and nodes.dtype == nb.BATCH_NODE_DTYPE and nodes.shape == (2 * int(off[-1]),)
        X, V = ens.getExtendedState(d)
        mass = d.mass.cpu().numpy()
        for s, name in enumerate(names + ["n = 1", "r_sep = 0"]):
            a, b = int(off[s]), int(off[s + 1])
            if name == "n = 1":
                assert href.is_none(rec[s]) and not np.frombuffer(_table(nodes, off, s).tobytes(), np.uint8).any()
                continue
            c = cases[names[0]] if name == "r_sep = 0" else cases[name]
            ev = href.evaluate(X[a:b], V[a:b], mass[a:b], 1.0, r_sep[s], kappa)
            bd = href.bounded(X[a:b], V[a:b], mass[a:b], 1.0, r_sep[s], kappa)
            ok, why = href.clear(bd)
            assert ok, (name, why)
            worst = href.check_table((name, precision), rec[s], _table(nodes, off, s), b - a, ev, bd, macro=0)
            text = hier.describe(s, nodes)
            print(f"{name} ({precision}): {text[:60]} K {ev.top_count} nodes {ev.node_count} resolved {ev.resolved}, "
                  f"|engine - restatement| {worst:.3g}", flush=True)
            assert text == href.forest(ev) == nb.hierarchy_string(_table(nodes, off, s), b - a)
            if name != "r_sep = 0":
                assert (ev.top_count, ev.node_count, ev.resolved) == (c["K"], c["nodes"], c["resolved"]), name
                assert c["forest"] is None or text == c["forest"], (name, text)
                seen += 1
            if name == "mirrored 2+2":  # bitwise equal a: the ids decide
                t = _table(nodes, off, s)
                assert t["a"][4] == t["a"][5] and (t["left"][4], t["right"][4], t["left"][5], t["right"][5]) == (0, 1, 2, 3)
            if name == "cold chain of 64":
                t = _table(nodes, off, s)
                assert (t["e"][64:127] == 1.0).all() and (t["bodies"][64:127] == np.arange(2, 65)).all() and rec[s]["largest"] == 64
        # the snapshot touched nothing of the run's own
        _same("own records after a snapshot", hier.records(), own)
        ens.close()
    assert seen == len(cases)


def test_snapshot_of_a_handle_never_configured_and_refusals(nb, ctx):
    cases = href.snapshot_cases()
    big = {k: np.resize(v, 65).astype(np.float32) for k, v in cases["33 bodies"]["ic"].items()}
    big["pos_x"] = (np.arange(65) * 3.0).astype(np.float32)
    ics = [cases["binary and a receding single"]["ic"], big]
    d, ens, off, hier, _ = _ensemble(nb, ics, 0.05)
    assert all(href.is_none(r) for r in hier.records()) and not np.frombuffer(hier.nodes().tobytes(), np.uint8).any()
    rec, nodes = hier.snapshot(d)  # r_sep = kappa = 0
    assert (rec["resolved"][0], rec["top_count"][0], rec["node_count"][0]) == (1, 2, 4) and hier.describe(0, nodes) == "[0 1] 2"
    assert href.is_none(rec[1]) and not np.frombuffer(_table(nodes, off, 1).tobytes(), np.uint8).any()  # n = 65: none
    # n = 65 with a radius: refused by name, in Python and at the C ABI
    with pytest.raises(nb.ValidationException, match="system 1 has 65 bodies"):
        hier.set([1.0, 1.0])
    lib = nb._lib.load()
    radii = np.array([1.0, 1.0], np.float32)
    assert lib.nbody_hip_batch_hierarchy_set(ens._h, radii.ctypes.data, 0.0, 0) == nb._lib.ERR_VALIDATION
    assert b"system 1 has 65 bodies" in lib.nbody_hip_last_error()
    for bad, word in ((np.array([-1.0, 0.0], np.float32), b"separation radius of system 0"),
                      (np.array([1.0, np.inf], np.float32), b"separation radius of system 1")):
        assert lib.nbody_hip_batch_hierarchy_set(ens._h, bad.ctypes.data, 0.0, 0) == nb._lib.ERR_VALIDATION
        assert word in lib.nbody_hip_last_error()
    ok = np.array([1.0, 0.0], np.float32)
    for kappa in (-1.0, float("nan"), float("inf")):
        assert lib.nbody_hip_batch_hierarchy_set(ens._h, ok.ctypes.data, kappa, 0) == nb._lib.ERR_VALIDATION
        assert b"kappa" in lib.nbody_hip_last_error()
    assert lib.nbody_hip_batch_hierarchy_set(ens._h, None, 0.0, 1) == nb._lib.ERR_VALIDATION
    assert b"STOP_ON_RESOLVED needs a separation radius > 0" in lib.nbody_hip_last_error()
    assert lib.nbody_hip_batch_hierarchy_set(ens._h, ok.ctypes.data, 0.0, 6) == nb._lib.ERR_VALIDATION
    assert b"unknown hierarchy flag bits 0x6" in lib.nbody_hip_last_error()
    out = np.zeros(2, nb.BATCH_HIERARCHY_DTYPE)
    tab = np.zeros(2 * 68, nb.BATCH_NODE_DTYPE)
    assert lib.nbody_hip_batch_hierarchy_get(ens._h, out.ctypes.data, 3, None, 0) == nb._lib.ERR_VALIDATION
    assert lib.nbody_hip_batch_hierarchy_get(ens._h, out.ctypes.data, 2, tab.ctypes.data, 135) == nb._lib.ERR_VALIDATION
    s = d.struct()
    assert lib.nbody_hip_batch_hierarchy_snapshot(ens._h, C.byref(s), out.ctypes.data, 2, tab.ctypes.data, 135) == nb._lib.ERR_VALIDATION
    assert lib.nbody_hip_batch_hierarchy_snapshot(ens._h, C.byref(s), out.ctypes.data, 2, None, 136) == nb._lib.ERR_VALIDATION
    with pytest.raises(nb.StateException, match="step graph"):
        with ctx.capture():
            hier.snapshot(d)
    hier.set([1.0, 0.0])  # accepted; a new layout drops it and unprimes
    ens.setLayout([0, 3, 68])
    assert ens._hierarchy is None
    with pytest.raises(nb.StateException, match="not primed"):
        hier.records()
    ens.close()


# ---- 2. configuring changes no bit -----------------------------------------------------------------------------------------
SIZES = [1, 2, 5, 64, 257]
FORMS = [("fp32", 0.05), ("fp32", 0.0), ("extended", 0.05), ("extended", 0.0)]
FORM_IDS = ["fp32-packed", "fp32-guard", "extended-packed", "extended-guard"]


def _kicked(nb, n, seed):
    ic = {k: np.array(v, np.float32) for k, v in nb.ic.plummer(n, seed=seed).items()}
    if n > 1:
        p = np.array([ic["pos_x"][-1], ic["pos_y"][-1], ic["pos_z"][-1]], np.float64)
        for k, c in zip(("vel_x", "vel_y", "vel_z"), 5.0 * p / np.linalg.norm(p)):
            ic[k][-1] = c
    return ic


@pytest.mark.parametrize("precision,eps", FORMS, ids=FORM_IDS)
def test_configuring_changes_no_bit(nb, ctx, precision, eps):
    ics = [_kicked(nb, n, 300 + k) for k, n in enumerate(SIZES)]
    d, ens, off, _, _ = _ensemble(nb, ics, eps, precision, g=1.7)
    assert [int(o) for o in off] == [0, 1, 3, 8, 72, 329]
    ens.advance(d, 3)
    plain, plain_ev = _whole(d, ens), ens.events()
    infos = [_cut(plain, ens, off, s)["info"] for s in range(len(SIZES))]
    ens.close()
    for tag, radius in (("huge", 1.0e6), ("tiny", 1.0e-3)):
        r = np.array([radius] * 4 + [0.0], np.float32)  # (the system of 257 bodies: no examination)
        d, ens, off, hier, _ = _ensemble(nb, ics, eps, precision, g=1.7, hierarchy=dict(separation_radius=r, isolation=1.0))
        ens.advance(d, 3)
        got = _whole(d, ens)
        _assert_equal((tag, precision, eps), got, plain)
        for s in range(len(SIZES)):
            assert _cut(got, ens, off, s)["info"] == infos[s], (tag, s)
        _same((tag, "event records"), ens.events(), plain_ev)
        rec, nodes = hier.records(), hier.nodes()
        assert href.is_none(rec[0]) and href.is_none(rec[4]) and ens.running() == len(SIZES)
        assert not np.frombuffer(_table(nodes, off, 0).tobytes(), np.uint8).any() and not np.frombuffer(_table(nodes, off, 4).tobytes(), np.uint8).any()
        print(f"{tag} {precision} eps {eps}: resolved {rec['resolved'].tolist()} K {rec['top_count'].tolist()} macro {rec['macro'].tolist()} "
              f"nodes {rec['node_count'].tolist()}", flush=True)
        for s in (1, 2, 3):
            assert 1 <= rec["macro"][s] <= 3 and rec["top_count"][s] + rec["node_count"][s] == 2 * SIZES[s]
            assert rec["macro"][s] == 3 or rec["resolved"][s] == 1
        if radius > 1.0:
            assert (rec["resolved"] == 0).all() and (rec["macro"][1:4] == 3).all()
        ens.close()


# ---- 3. the walk ------------------------------------------------------------------------------------------------------------
def _walk(nb, ics, r_seps, dts, kappa, macros, precision="extended", L=10):
    """a record-only ensemble walked one macro step at a time next to nothing else: after every step the record and the
    table of every examined system against the restatement on the state the engine hands back.  -> first resolving macro
    per system (0: never), the records at the end, the states"""
    d, ens, off, hier, _ = _ensemble(nb, ics, 0.0, precision, dt=np.asarray(dts, np.float32), max_level=L,
                                     hierarchy=dict(separation_radius=np.asarray(r_seps, np.float32), isolation=kappa))
    mass = d.mass.cpu().numpy()
    first, frozen = [0] * len(ics), {}
    Xs, Vs = [], []
    for k in range(1, macros + 1):
        ens.advance(d, 1)
        X, V = ens.getExtendedState(d)
        Xs.append(np.array(X, np.float64))
        Vs.append(np.array(V, np.float64))
        rec, nodes = hier.records(), hier.nodes()
        for s in range(len(ics)):
            a, b = int(off[s]), int(off[s + 1])
            if not r_seps[s] > 0:
                assert href.is_none(rec[s])
                continue
            if first[s]:
                _same(("frozen record", s, k), rec[s:s + 1], frozen[s][0])
                _same(("frozen table", s, k), _table(nodes, off, s), frozen[s][1])
                continue
            ev = href.evaluate(X[a:b], V[a:b], mass[a:b], 1.0, r_seps[s], kappa)
            bd = href.bounded(X[a:b], V[a:b], mass[a:b], 1.0, r_seps[s], kappa)
            ok, why = href.clear(bd)
            assert ok, (s, k, why)
            href.check_table((s, k), rec[s], _table(nodes, off, s), b - a, ev, bd, macro=k)
            if ev.resolved:
                first[s] = k
                frozen[s] = (rec[s:s + 1].copy(), _table(nodes, off, s).copy())
                print(f"system {s}: resolved after macro step {k} as {hier.describe(s, nodes)}", flush=True)
    assert (ens.events()["stopped"] == 0).all() and ens.running() == len(ics)
    out = (first, hier.records(), hier.nodes(), off, np.array(Xs), np.array(Vs), mass)
    ens.close()
    return out


def test_the_walk(nb, ctx):
    ics = [oref.flyby_ic(), href.two_plus_two_ic()]
    w = href.WALK
    first, rec, nodes, off, Xs, Vs, _ = _walk(nb, ics, w["r_sep"], [w["dt"]] * 2, w["kappa"], w["macros"])
    gX, gV, _ = href.recorded("walk")  # (the states the CPU test examines are the states the engine still reaches)
    assert np.array_equal(Xs.view(np.uint64), gX.view(np.uint64)) and np.array_equal(Vs.view(np.uint64), gV.view(np.uint64))
    assert first[0] >= 5 and first[1] >= 7, first  # beyond the radius on the far side, not before
    assert nb.hierarchy_string(_table(nodes, off, 0), 3) == "[0 1] 2"
    assert nb.hierarchy_string(_table(nodes, off, 1), 4) == "[0 1] [2 3]"
    assert rec["top_count"].tolist() == [2, 2] and rec["largest"].tolist() == [2, 2] and rec["macro"].tolist() == first


# ---- 4. stop when resolved ----------------------------------------------------------------------------------------------------
_FLY = {}


def _fly(nb):
    """the eight fly-bys: the record-only walk (its predictions asserted against the restatement step by step), and the plain
    ensemble's state after every macro step"""
    if not _FLY:
        ics = [oref.flyby_ic() for _ in range(8)]
        first, rec, nodes, off, _, _, _ = _walk(nb, ics, href.FLY_RSEP, href.FLY_DT, href.FLY["kappa"], href.FLY["macros"])
        d, ens, off, _, _ = _ensemble(nb, ics, 0.0, "extended", dt=np.array(href.FLY_DT, np.float32), max_level=10)
        states = []
        for _ in range(href.FLY["macros"]):
            ens.advance(d, 1)
            whole = _whole(d, ens)
            states.append([_cut(whole, ens, off, s) for s in range(8)])
        ens.close()
        _FLY.update(ics=ics, first=first, rec=rec, nodes=nodes, states=states)
        print("the eight fly-bys resolve after", first, flush=True)
        assert all(f > 0 for f in first[:6]) and first[6:] == [0, 0] and len(set(first[:6])) >= 4
    return _FLY


def _fly_ensemble(nb, ics, pick=slice(None), stop=True, **kw):
    return _ensemble(nb, ics[pick], 0.0, "extended", dt=np.array(href.FLY_DT, np.float32)[pick], max_level=10,
                     hierarchy=dict(separation_radius=np.array(href.FLY_RSEP, np.float32)[pick], isolation=href.FLY["kappa"],
                                    stop_on_resolved=stop), **kw)


def test_stop_when_resolved(nb, ctx):
    f = _fly(nb)
    M = href.FLY["macros"]
    first = f["first"]
    done = [m if m else M for m in first]
    d, ens, off, hier, _ = _fly_ensemble(nb, f["ics"])
    assert ens.running() == 8
    for k in range(1, M + 1):  # running() counts down
        ens.advance(d, 1)
        assert ens.running() == 8 - sum(1 for m in first if 0 < m <= k), k
    ev, rec, nodes = ens.events(), hier.records(), hier.nodes()
    assert nb.BATCH_STOPPED_RESOLVED == 4 and ev["stopped"].tolist() == [4 if m else 0 for m in first]
    assert ev["macro_steps_done"].tolist() == done and rec["macro"][:6].tolist() == first[:6]
    _same("stopping against record-only", rec, f["rec"])
    _same("stopping against record-only, tables", nodes, f["nodes"])
    whole = _whole(d, ens)
    for s in range(8):  # the state is that of the plain ensemble after macro_steps_done[s] macro steps, bit for bit
        _assert_equal(("stopped", s), _cut(whole, ens, off, s), f["states"][done[s] - 1][s])
    ens.advance(d, 4)  # four more macro steps leave the stopped systems untouched
    after = _whole(d, ens)
    for s in range(6):
        _assert_equal(("after 4 more", s), _cut(after, ens, off, s), f["states"][done[s] - 1][s])
    rec2, nodes2 = hier.records(), hier.nodes()
    _same("records after 4 more", rec2[:7], rec[:7])
    _same("tables after 4 more", nodes2[:2 * 3 * 7], nodes[:2 * 3 * 7])
    ev2 = ens.events()
    assert ev2["macro_steps_done"].tolist() == done[:6] + [M + 4, M + 4] and ev2["stopped"].tolist() == ev["stopped"].tolist()
    ens.close()
    d, ens, off, hier, _ = _fly_ensemble(nb, f["ics"], slice(None, None, -1))  # the reversed ensemble: the same records
    ens.advance(d, M)
    _same("reversed", hier.records()[::-1], rec)
    assert ens.events()["stopped"].tolist() == [4 if m else 0 for m in first][::-1]
    for s in range(8):
        _same(("reversed table", s), _table(hier.nodes(), off, 7 - s), _table(nodes, off, s))
    ens.close()


# ---- 5. priorities at one boundary --------------------------------------------------------------------------------------------
def test_priorities(nb, ctx):
    """contact, escape, resolved and the budget at one boundary: 1; escape, resolved and the budget: 3; resolved and the
    budget: 4.  The hierarchy record is on file whoever took the stop word."""
    ics = [oref.flyby_ic() for _ in range(3)]
    radii = np.zeros(9, np.float32)
    radii[0:2] = 0.3  # the binary of system 0 (separation 0.5) is in contact from its first block step
    d, ens, off, hier, out = _ensemble(nb, ics, 0.0, "fp32", dt=0.5, max_level=10,
                                       hierarchy=dict(separation_radius=1.2, isolation=1.0, stop_on_resolved=True),
                                       outcomes=dict(escape_radius=[1.2, 1.2, 0.0], stop_on_escape=True),
                                       events=dict(radii=radii, max_macro_steps=1, stop_on_contact=True))
    ens.advance(d, 3)
    ev, rec, nodes = ens.events(), hier.records(), hier.nodes()
    assert ev["stopped"].tolist() == [1, 3, 4] and ev["macro_steps_done"].tolist() == [1, 1, 1]
    assert out.records()["macro"].tolist() == [1, 1, 0]
    assert rec["resolved"].tolist() == [1, 1, 1] and rec["macro"].tolist() == [1, 1, 1] and rec["top_count"].tolist() == [2, 2, 2]
    for s in range(3):
        assert hier.describe(s, nodes) == "[0 1] 2"
        _same(("the same fly-by", s), rec[s:s + 1], rec[0:1])
        _same(("the same fly-by, table", s), _table(nodes, off, s), _table(nodes, off, 0))
    X, V = ens.getExtendedState(d)
    mass = d.mass.cpu().numpy()
    ev0, bd0 = href.evaluate(X[0:3], V[0:3], mass[0:3], 1.0, 1.2, 1.0), href.bounded(X[0:3], V[0:3], mass[0:3], 1.0, 1.2, 1.0)
    assert href.clear(bd0)[0]
    href.check_table("priorities", rec[0], _table(nodes, off, 0), 3, ev0, bd0, macro=1)
    ens.close()


# ---- 6. launch structure --------------------------------------------------------------------------------------------------------
def test_launch_structure(nb, ctx):
    f = _fly(nb)
    d, ens, _, hier, _ = _fly_ensemble(nb, f["ics"])
    ens.advance(d, 4)
    d2, ens2, _, hier2, _ = _fly_ensemble(nb, f["ics"])
    for _ in range(4):
        ens2.advance(d2, 1)
    _same("advance(4) against 4 advance(1)", hier.records(), hier2.records())
    _same("advance(4) against 4 advance(1), tables", hier.nodes(), hier2.nodes())
    assert ens.events().tobytes() == ens2.events().tobytes()
    _assert_equal("advance(4) against 4 advance(1)", _whole(d, ens), _whole(d2, ens2))
    d3, ens3, _, hier3, _ = _fly_ensemble(nb, f["ics"])
    with pytest.raises(nb.StateException, match="step graph"):  # refused until one eager advance has run
        with ctx.capture():
            ens3.advance(d3, 1)
    ens3.advance(d3, 1)
    with ctx.capture() as rec:
        ens3.advance(d3, 1)
    rec.graph.launch(3)
    _same("1 eager + 3 replayed", hier3.records(), hier.records())
    _same("1 eager + 3 replayed, tables", hier3.nodes(), hier.nodes())
    assert ens3.events().tobytes() == ens.events().tobytes()
    _assert_equal("1 eager + 3 replayed", _whole(d3, ens3), _whole(d, ens))
    rec.graph.close()
    hier3.set(None)  # a configuration changed since the last eager advance: refused until one has run
    with pytest.raises(nb.StateException, match="step graph"):
        with ctx.capture():
            ens3.advance(d3, 1)
    for e in (ens, ens2, ens3):
        e.close()


# ---- 7. more systems than compute units ---------------------------------------------------------------------------------------
def test_more_systems_than_compute_units(nb, ctx):
    """300 triples, a drawn third of which send their third body outward at speed 6: every record, table and event record
    equals that of the system run as a B = 1 ensemble"""
    c = bc.TRIPLE
    ics = bc.triples(c["systems"])
    hit = np.random.default_rng(91).random(len(ics)) < 1.0 / 3.0
    assert len(ics) == 300 and 60 < hit.sum() < 140
    for s in np.flatnonzero(hit):
        ic = ics[s]
        p = np.array([ic["pos_x"][2], ic["pos_y"][2], ic["pos_z"][2]], np.float64)
        for k, v in zip(("vel_x", "vel_y", "vel_z"), 6.0 * p / np.linalg.norm(p)):
            ic[k][2] = v
    kw = dict(dt=c["dt_max"], max_level=c["max_level"], g=c["G"],
              hierarchy=dict(separation_radius=4.0, isolation=1.0, stop_on_resolved=True))
    d, ens, off, hier, _ = _ensemble(nb, ics, c["eps"], **kw)
    ens.advance(d, 4)
    ev, rec, nodes = ens.events(), hier.records(), hier.nodes()
    print(f"{int(hit.sum())} systems kicked, {int((ev['stopped'] == 4).sum())} stopped, K {np.bincount(rec['top_count']).tolist()}", flush=True)
    assert ((ev["stopped"] == 4) == (rec["resolved"] == 1)).all() and (rec["macro"] >= 1).all()
    assert ens.running() == int((ev["stopped"] == 0).sum())
    pos = {k: getattr(d, k).cpu().numpy() for k in F[:6]}
    for s in range(300):
        d1, e1, _, h1, _ = _ensemble(nb, [ics[s]], c["eps"], **kw)
        e1.advance(d1, 4)
        _same(("triple", s), rec[s:s + 1], h1.records())
        _same(("triple table", s), _table(nodes, off, s), h1.nodes())
        assert ev[s:s + 1].tobytes() == e1.events().tobytes(), s
        a, b = int(off[s]), int(off[s + 1])
        for k in F[:6]:
            assert np.array_equal(pos[k][a:b].view(np.uint32), getattr(d1, k).cpu().numpy().view(np.uint32)), (s, k)
        e1.close()
    ens.close()


# ---- 8. independence, resetting, the facade -------------------------------------------------------------------------------------
@pytest.mark.parametrize("order", ["hoe", "eoh", "ohe"])
def test_independent_of_events_and_outcomes(nb, ctx, order):
    f = _fly(nb)
    radii = np.full(24, 1e-4, np.float32)
    d, ens, off, hier, out = _fly_ensemble(nb, f["ics"], order=order, outcomes=dict(escape_radius=100.0),
                                           events=dict(radii=radii, track_closest=True))
    ens.advance(d, href.FLY["macros"])
    _same(order, hier.records(), f["rec"])
    _same(order, hier.nodes(), f["nodes"])
    ev = ens.events()
    assert ev["stopped"].tolist() == [4 if m else 0 for m in f["first"]] and (ev["closest_i"] != NONE).all()
    assert (out.records()["escaped"] == 0).all()
    # hierarchies off: back to the outcomes form; a priming clears the records and the tables
    hier.set(None)
    assert ens._hierarchy is None
    ic, _ = nb.ic.concat(f["ics"])
    d, _ = to_device(nb, ic)
    ens.prime(d, _direct(nb, 1.0, 0.0), np.array(href.FLY_DT, np.float32))
    ens.advance(d, 2)
    assert all(href.is_none(r) for r in hier.records()) and not np.frombuffer(hier.nodes().tobytes(), np.uint8).any()
    assert (ens.events()["stopped"] == 0).all()
    ens.close()


def test_facade_program(nb, ctx):
    exe = os.path.join(ROOT, "n-body_amd", "lib", "hermite_batch_hierarchy_tests")
    assert os.path.exists(exe), "the facade test program has not been built"
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert re.search(r"^\d+ checks, 0 failed$", r.stdout, re.M)
    rows = [[-0.5, 0, 0, 0, -1, 0, 2], [0.5, 0, 0, 0, 1, 0, 2], [100, 0, 0, 5, 0, 0, 1],
            [-0.5, 0, 0, 0, -1, 0, 2], [0.5, 0, 0, 0, 1, 0, 2], [20, 0, 0, 0, 0.3, 0, 1],
            [0, 0, 0, 0, 0, 0, 1], [-1, 0, 0, -3, 0, 0, 1], [1, 0, 0, 3, 0, 0, 1]]
    ics = [href._ic(rows[0:3]), href._ic(rows[3:6]), href._ic(rows[6:7]), href._ic(rows[7:9])]
    d, ens, off, hier, _ = _ensemble(nb, ics, 0.0, dt=1.0 / 64, hierarchy=dict(separation_radius=[10, 10, 0, 1], isolation=5.0,
                                                                           stop_on_resolved=True))
    ens.advance(d, 4)
    ev, rec, nodes = ens.events(), hier.records(), hier.nodes()
    want = []
    for s in range(4):
        r_ = rec[s]
        want.append(f"hierarchy {s} {r_['resolved']} {r_['top_count']} {r_['macro']} {r_['node_count']} {r_['largest']} "
                    f"{_hexf(r_['min_sep'])} {r_['min_p']} {r_['min_q']} stopped {ev['stopped'][s]} done {ev['macro_steps_done'][s]}")
        t = _table(nodes, off, s)
        for k in range(int(off[s + 1] - off[s]), int(r_["node_count"])):
            want.append(f"node {s} {k} {t['left'][k]} {t['right'][k]} {t['bodies'][k]} " +
                        " ".join(_hexf(t[n][k]) for n in ("mass", "a", "e", "r", "energy")))
    got = [ln for ln in r.stdout.splitlines() if ln.startswith(("hierarchy ", "node "))]
    assert [_canon(ln) for ln in got] == [_canon(ln) for ln in want], (got, want)
    ens.close()


def _hexf(x):
    return float(x).hex()


def _canon(line):
    """the doubles of a line as floats (C's %a and Python's float.hex spell the same value differently)"""
    return [float.fromhex(w) if re.match(r"^-?(0x|inf|nan)", w) else w for w in line.split()]

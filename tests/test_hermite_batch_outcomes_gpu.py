"""The ensemble OUTCOMES (nbody_hip_batch_outcomes_set / _get, EnsembleOutcomes; include/nbody_hip.h "ensemble OUTCOMES",
DESIGN.md section 4.19) on a real GPU.

Two oracles.  Bit equality: a system with outcomes configured is, up to its stop, the plain ensemble's system, array by
array and counter by counter.  The restatement: tests/hermite_batch_outcomes_ref.py evaluates the model in numpy fp64 on
the state the engine itself hands back after every macro step (advance(1) + getExtendedState of a record-only ensemble),
so it predicts, per system, the first escaping boundary, the count and the lowest index exactly and r, vr, e and rest_mass
within the bound derived there from the operation count (the bound itself, no multiple of it: engine and restatement run
the same operations in the same order; tests/test_hermite_batch_outcomes_cpu.py holds the restatement to the same bound
against exact arithmetic on a CPU).  Every body at every examined boundary
must be clear by the restatement alone: its verdict is decided by margins above 1e6 times the bound."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import hermite_batch_cases as bc
import hermite_batch_outcomes_ref as oref
from gpu_util import to_device

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = ("pos_x", "pos_y", "pos_z", "vel_x", "vel_y", "vel_z", "acc_x", "acc_y", "acc_z", "acc_old_x", "acc_old_y", "acc_old_z",
     "mass")
COUNTERS = ("block_steps", "body_steps", "level_steps", "floor_hits", "macro_steps", "current_tick", "last_n_active",
            "max_level")
G, DT = 1.7, 1.0 / 16
NONE = oref.NONE


def _plummer(nb, n, seed=42):
    ic = dict(nb.ic.plummer(n, seed=seed))
    ic["mass"] = (ic["mass"] * np.random.default_rng(5 + seed).uniform(0.5, 2.0, ic["mass"].size)).astype(np.float32)
    return ic


def _direct(nb, g, eps):
    c = nb.DirectForceCalculator()
    c.setGravitationalConstant(g)
    c.setSofteningParameter(eps)
    return c


def _ensemble(nb, ics, eps, precision="fp32", dt=DT, max_level=16, g=G, outcomes=None, events=None, order=("o", "e")):
    """-> (d, ens, offsets, out), primed; outcomes / events: the keywords of EnsembleOutcomes.set / setEvents, sent after
    the layout and before the priming, in `order`"""
    ic, offsets = nb.ic.concat(ics)
    d, _ = to_device(nb, ic)
    ens = nb.BlockHermiteEnsemble()
    ens.setParameters(0.02, 0.01, max_level)
    ens.setStatePrecision(precision)
    ens.setLayout(offsets)
    out = nb.EnsembleOutcomes(ens)
    for which in order:
        if which == "o" and outcomes is not None:
            out.set(**outcomes)
        if which == "e" and events is not None:
            ens.setEvents(**events)
    ens.prime(d, _direct(nb, g, eps), dt)
    return d, ens, offsets, out


def _whole(d, ens):
    """every array of the ensemble as bits, and info(-1)"""
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


def _is_none(rec):
    return (rec["escaped"] == 0 and rec["escaper"] == NONE and rec["macro"] == 0 and
            all(rec[k] == 0.0 for k in ("r", "vr", "energy", "rest_mass", "reserved", "reserved2")))


def _same_records(tag, a, b):
    assert a.dtype == b.dtype
    assert np.ascontiguousarray(a).tobytes() == np.ascontiguousarray(b).tobytes(), (tag, a, b)


# ---- 1. configuring changes no bit -------------------------------------------------------------------------------------
# 1: no test; 2: a pair; 5: a wave with five bodies; 257: five waves; 1,025: a second body for thread 0.  Offsets 0, 1, 3, 8,
# 265.  The last body of every system of two or more is sent outward at speed 5, so that with a small escape radius
# something escapes.
SIZES = [1, 2, 5, 257, 1025]
FORMS = [("fp32", 0.05), ("fp32", 0.0), ("extended", 0.05), ("extended", 0.0)]
FORM_IDS = ["fp32-packed", "fp32-guard", "extended-packed", "extended-guard"]
_PLAIN = {}


def _kicked(nb, n, seed):
    ic = {k: np.array(v, np.float32) for k, v in _plummer(nb, n, seed).items()}
    if n > 1:
        p = np.array([ic["pos_x"][-1], ic["pos_y"][-1], ic["pos_z"][-1]], np.float64)
        for k, c in zip(("vel_x", "vel_y", "vel_z"), 5.0 * p / np.linalg.norm(p)):
            ic[k][-1] = c
    return ic


def _plain3(nb, precision, eps):
    """the plain handle's advance(3) of the SIZES batch, computed once per form and shared"""
    if (precision, eps) not in _PLAIN:
        ics = [_kicked(nb, n, 200 + k) for k, n in enumerate(SIZES)]
        d, ens, off, _ = _ensemble(nb, ics, eps, precision)
        assert [int(o) for o in off] == [0, 1, 3, 8, 265, 1290]
        ens.advance(d, 3)
        whole = _whole(d, ens)
        _PLAIN[(precision, eps)] = (ics, whole, [_cut(whole, ens, off, s)["info"] for s in range(len(SIZES))])
        ens.close()
    return _PLAIN[(precision, eps)]


@pytest.mark.parametrize("precision,eps", FORMS, ids=FORM_IDS)
def test_configuring_changes_no_bit(nb, ctx, precision, eps):
    ics, plain, infos = _plain3(nb, precision, eps)
    for tag, radius in (("nothing escapes", 1.0e6), ("record only", 1.0e-3)):
        d, ens, off, out = _ensemble(nb, ics, eps, precision, outcomes=dict(escape_radius=radius))
        ens.advance(d, 3)
        got = _whole(d, ens)
        _assert_equal((tag, precision, eps), got, plain)
        for s in range(len(SIZES)):
            assert _cut(got, ens, off, s)["info"] == infos[s], (tag, s)
        ev, rec = ens.events(), out.records()
        assert (ev["stopped"] == 0).all() and (ev["macro_steps_done"] == 3).all() and ens.running() == len(SIZES)
        assert _is_none(rec[0])  # (n = 1)
        if radius > 1.0:
            assert all(_is_none(r) for r in rec)
        else:
            hit = rec["escaped"] > 0
            print(f"{tag} {precision} eps {eps}: escaped {rec['escaped'].tolist()} escaper {rec['escaper'].tolist()} macro "
                  f"{rec['macro'].tolist()}")
            assert hit[1:].all()  # the kicked bodies at the latest
            assert (rec["escaper"][hit] < np.array(SIZES)[hit]).all() and (rec["macro"][hit] >= 1).all()
            assert (rec["r"][hit] > 1e-3).all() and (rec["vr"][hit] > 0).all() and (rec["energy"][hit] > 0).all()
        ens.close()


# ---- 2. the records against the restatement ----------------------------------------------------------------------------
_CASES = None


def _cases(nb):
    global _CASES
    if _CASES is None:
        _CASES = oref.cases(nb)
    return _CASES


CASE_NAMES = ["unbound pair", "bound e = 0.9 pair", "fly-by", "plummer 600, body 515", "plummer 1025, body 1024",
              "massless escaper", "whole mass in one body", "n = 1"]


def _walk(nb, ics, r_escs, dts, c, macros):
    """a record-only ensemble walked one macro step at a time: -> (records, predicted per system: None or (macro, Bodies,
    Bounds), the states X, V [macros, n, 3]).  Asserts that every body at every examined boundary is clear."""
    d, ens, off, out = _ensemble(nb, ics, c["eps"], c["precision"], dt=dts, max_level=c["L"], g=c["G"],
                                 outcomes=dict(escape_radius=np.asarray(r_escs, np.float32)))
    first = [None] * len(ics)
    mass = d.mass.cpu().numpy()
    Xs, Vs = [], []
    for k in range(1, macros + 1):
        ens.advance(d, 1)
        X, V = ens.getExtendedState(d)
        Xs.append(np.array(X, np.float64))
        Vs.append(np.array(V, np.float64))
        for s in range(len(ics)):
            a, b = int(off[s]), int(off[s + 1])
            if first[s] is not None or not r_escs[s] > 0 or b - a < 2:
                continue
            bodies = oref.evaluate(X[a:b], V[a:b], mass[a:b], c["G"], r_escs[s])
            bd = oref.bounds(X[a:b], V[a:b], mass[a:b], c["G"])
            ok = oref.clear(bodies, bd, r_escs[s])
            assert ok.all(), (s, k, np.flatnonzero(~ok)[:5], bodies.r[~ok][:5], bodies.dw[~ok][:5], bodies.e[~ok][:5])
            if bodies.count:
                first[s] = (k, bodies, bd)
    rec = out.records()
    assert (ens.events()["stopped"] == 0).all() and (ens.events()["macro_steps_done"] == macros).all()
    ens.close()
    return rec, first, (np.stack(Xs), np.stack(Vs), mass)


def _assert_recorded(tag, key, states):
    """the states on file, which the CPU test examines against exact arithmetic, are the ones the engine reaches"""
    for what, got, want in zip("XVm", states, oref.recorded(key)):
        assert got.dtype == want.dtype and got.shape == want.shape and got.tobytes() == want.tobytes(), (tag, what)


def _check_record(tag, rec, pred):
    if pred is None:
        assert _is_none(rec), (tag, rec)
        return
    k, b, bd = pred
    i = b.lowest
    diff = [abs(float(rec[f]) - float(v[i])) for f, v in (("r", b.r), ("vr", b.vr), ("energy", b.e), ("rest_mass", b.rest))]
    tol = [float(t[i]) for t in (bd.dr, bd.dvr, bd.de, bd.dM)]
    print(f"{tag}: first escape at macro {k}: count {b.count} lowest {i}; r {b.r[i]:.17g} (engine {rec['r']:.17g}) vr "
          f"{b.vr[i]:.17g} ({rec['vr']:.17g}) e {b.e[i]:.17g} ({rec['energy']:.17g}) rest {b.rest[i]:.17g} "
          f"({rec['rest_mass']:.17g}); |engine - restatement| {diff}, bound {tol}; kappa {bd.kappa[0]:.3g} {bd.kappa[1]:.3g} "
          f"{bd.kappa[2]:.3g}, rel {bd.rel[i]:.2e}", flush=True)
    assert (int(rec["macro"]), int(rec["escaped"]), int(rec["escaper"])) == (k, b.count, i), tag
    assert bd.rel[i] < oref.REL_MAX, tag  # (what the bound's second-order factor rests on)
    assert all(dv <= t for dv, t in zip(diff, tol)), (tag, diff, tol)
    assert rec["reserved"] == 0.0 and rec["reserved2"] == 0.0


@pytest.mark.parametrize("name", CASE_NAMES)
def test_records_against_the_restatement(nb, ctx, name):
    assert list(_cases(nb)) == CASE_NAMES
    c = _cases(nb)[name]
    rec, first, states = _walk(nb, [c["ic"]], [c["r_esc"]], c["dt"], c, c["macros"])
    _assert_recorded(name, CASE_NAMES.index(name), states)
    _check_record(name, rec[0], first[0])
    if c["expect"] is None:
        assert first[0] is None and _is_none(rec[0])
    else:
        assert first[0] is not None and (first[0][1].count, first[0][1].lowest) == c["expect"]


# ---- 3. stop on escape ---------------------------------------------------------------------------------------------------
# eight copies of the fly-by that differ in r_esc and dt_max (tests/hermite_batch_outcomes_ref.py)
FLY_DT, FLY_RESC, FLY_MACRO, FLY = oref.FLY_DT, oref.FLY_RESC, oref.FLY_MACRO, oref.FLY
_FLY = {}


def _fly(nb):
    """the record-only walk of the eight fly-bys (7 macro steps) and the plain ensemble's state after every macro step"""
    if not _FLY:
        ics = [oref.flyby_ic() for _ in FLY_DT]
        rec, first, states = _walk(nb, ics, FLY_RESC, np.array(FLY_DT, np.float32), FLY, FLY["macros"])
        _assert_recorded("fly-bys", "fly", states)
        assert [0 if f is None else f[0] for f in first] == FLY_MACRO
        d, ens, off, _ = _ensemble(nb, ics, FLY["eps"], FLY["precision"], dt=np.array(FLY_DT, np.float32), max_level=FLY["L"],
                                   g=FLY["G"])
        states = []
        for k in range(7):
            ens.advance(d, 1)
            whole = _whole(d, ens)
            states.append([_cut(whole, ens, off, s) for s in range(8)])
        ens.close()
        _FLY.update(ics=ics, rec=rec, first=first, states=states)
    return _FLY


def _fly_ensemble(nb, ics, pick=slice(None), stop=True, **kw):
    return _ensemble(nb, ics[pick], FLY["eps"], FLY["precision"], dt=np.array(FLY_DT, np.float32)[pick], max_level=FLY["L"],
                     g=FLY["G"], outcomes=dict(escape_radius=np.array(FLY_RESC, np.float32)[pick], stop_on_escape=stop), **kw)


def test_stop_on_escape(nb, ctx):
    f = _fly(nb)
    for s in range(8):
        _check_record(("fly-by", s), f["rec"][s], f["first"][s])
    d, ens, off, out = _fly_ensemble(nb, f["ics"])
    ens.advance(d, 7)
    ev, rec = ens.events(), out.records()
    done = [m if m else 7 for m in FLY_MACRO]
    assert ev["stopped"].tolist() == [3 if m else 0 for m in FLY_MACRO]
    assert ev["macro_steps_done"].tolist() == done and rec["macro"].tolist() == FLY_MACRO
    _same_records("stopping against record-only", rec, f["rec"])
    assert ens.running() == 2 and nb.BATCH_STOPPED_ESCAPE == 3
    # the state is that of the plain ensemble after macro_steps_done[s] macro steps, bit for bit
    whole = _whole(d, ens)
    for s in range(8):
        _assert_equal(("stopped", s), _cut(whole, ens, off, s), f["states"][done[s] - 1][s])
    # a further advance leaves the stopped systems' arrays and records untouched
    ens.advance(d, 4)
    after = _whole(d, ens)
    for s in range(6):
        _assert_equal(("after 4 more", s), _cut(after, ens, off, s), f["states"][done[s] - 1][s])
    _same_records("after 4 more", out.records(), rec)
    ev = ens.events()
    assert ev["macro_steps_done"].tolist() == done[:6] + [11, 11] and ev["stopped"].tolist()[:6] == [3] * 6
    ens.close()
    # the reversed ensemble: the same records
    d, ens, off, out = _fly_ensemble(nb, f["ics"], slice(None, None, -1))
    ens.advance(d, 7)
    _same_records("reversed", out.records()[::-1], rec)
    assert ens.events()["stopped"].tolist() == [3 if m else 0 for m in FLY_MACRO][::-1]
    ens.close()


def test_running_counts_down(nb, ctx):
    f = _fly(nb)
    d, ens, _, _ = _fly_ensemble(nb, f["ics"])
    assert ens.running() == 8
    for k in range(1, 8):
        ens.advance(d, 1)
        assert ens.running() == 8 - sum(1 for m in FLY_MACRO if 0 < m <= k), k
    ens.close()


def test_priorities(nb, ctx):
    """contact and escape (and the budget) at one boundary: 1; escape and the budget: 3; the budget alone: 2"""
    ics = [oref.flyby_ic() for _ in range(3)]
    radii = np.zeros(9, np.float32)
    radii[0:2] = 0.3  # the binary of system 0 (separation 0.5) is in contact from its first block step
    d, ens, _, out = _ensemble(nb, ics, 0.0, "fp32", dt=0.5, max_level=10, g=1.0,
                               outcomes=dict(escape_radius=[1.2, 1.2, 0.0], stop_on_escape=True),
                               events=dict(radii=radii, max_macro_steps=1, stop_on_contact=True))
    ens.advance(d, 3)
    ev, rec = ens.events(), out.records()
    assert ev["stopped"].tolist() == [1, 3, 2] and ev["macro_steps_done"].tolist() == [1, 1, 1]
    assert ev["contact_macro"][0] == 0 and ev["contact_i"][0] != NONE and ev["contact_i"][1] == NONE
    # the escape of system 0 is on record all the same: the test runs at every completed boundary
    assert rec["macro"].tolist() == [1, 1, 0] and rec["escaper"].tolist() == [2, 2, NONE]
    _same_records("with and without contact", rec[0:1], rec[1:2])
    ens.close()


# ---- 4. launch structure -------------------------------------------------------------------------------------------------
def test_one_launch_against_four(nb, ctx):
    f = _fly(nb)
    d, ens, _, out = _fly_ensemble(nb, f["ics"])
    ens.advance(d, 4)
    d2, ens2, _, out2 = _fly_ensemble(nb, f["ics"])
    for _ in range(4):
        ens2.advance(d2, 1)
    _same_records("advance(4) against 4 advance(1)", out.records(), out2.records())
    assert ens.events().tobytes() == ens2.events().tobytes()
    _assert_equal("advance(4) against 4 advance(1)", _whole(d, ens), _whole(d2, ens2))
    # one eager and three replayed advances
    d3, ens3, _, out3 = _fly_ensemble(nb, f["ics"])
    with pytest.raises(nb.StateException, match="step graph"):  # refused until one eager advance has run
        with ctx.capture():
            ens3.advance(d3, 1)
    ens3.advance(d3, 1)
    with ctx.capture() as rec:
        ens3.advance(d3, 1)
    rec.graph.launch(3)
    _same_records("1 eager + 3 replayed", out3.records(), out.records())
    assert ens3.events().tobytes() == ens.events().tobytes()
    _assert_equal("1 eager + 3 replayed", _whole(d3, ens3), _whole(d, ens))
    rec.graph.close()
    # a configuration changed since the last eager advance: the recording is refused until one has run
    out3.set(None)
    with pytest.raises(nb.StateException, match="step graph"):
        with ctx.capture():
            ens3.advance(d3, 1)
    for e in (ens, ens2, ens3):
        e.close()


def test_more_systems_than_compute_units(nb, ctx):
    """300 triples, a drawn third of which send their third body outward at speed 6: every record equals that of the system
    run as a B = 1 ensemble"""
    c = bc.TRIPLE
    ics = bc.triples(c["systems"])
    hit = np.random.default_rng(91).random(len(ics)) < 1.0 / 3.0
    assert len(ics) == 300 and 60 < hit.sum() < 140
    for s in np.flatnonzero(hit):
        ic = ics[s]
        p = np.array([ic["pos_x"][2], ic["pos_y"][2], ic["pos_z"][2]], np.float64)
        for k, v in zip(("vel_x", "vel_y", "vel_z"), 6.0 * p / np.linalg.norm(p)):
            ic[k][2] = v
    kw = dict(dt=c["dt_max"], max_level=c["max_level"], g=c["G"])
    d, ens, off, out = _ensemble(nb, ics, c["eps"], outcomes=dict(escape_radius=4.0, stop_on_escape=True), **kw)
    ens.advance(d, 4)
    ev, rec = ens.events(), out.records()
    print(f"{int(hit.sum())} systems kicked, {int((ev['stopped'] == 3).sum())} stopped, done "
          f"{sorted(set(ev['macro_steps_done'].tolist()))}")
    assert (ev["stopped"][~hit] == 0).all() and (rec["escaped"][~hit] == 0).all()
    assert (ev["stopped"][hit] == 3).sum() >= hit.sum() // 4 and ((ev["stopped"] == 3) == (rec["escaped"] > 0)).all()
    assert (rec["escaper"][rec["escaped"] > 0] == 2).all()
    assert ens.running() == int((ev["stopped"] == 0).sum())
    pos = {k: getattr(d, k).cpu().numpy() for k in F[:6]}
    for s in range(300):
        d1, e1, _, o1 = _ensemble(nb, [ics[s]], c["eps"], outcomes=dict(escape_radius=4.0, stop_on_escape=True), **kw)
        e1.advance(d1, 4)
        _same_records(("triple", s), rec[s:s + 1], o1.records())
        assert ev[s:s + 1].tobytes() == e1.events().tobytes(), s
        a, b = int(off[s]), int(off[s + 1])
        for k in F[:6]:
            assert np.array_equal(pos[k][a:b].view(np.uint32), getattr(d1, k).cpu().numpy().view(np.uint32)), (s, k)
        e1.close()
    ens.close()


# ---- 5. resetting and refusals -------------------------------------------------------------------------------------------
def test_prime_clears_and_layout_drops(nb, ctx):
    f = _fly(nb)
    d, ens, off, out = _fly_ensemble(nb, f["ics"])
    ens.advance(d, 7)
    assert ens.running() == 2 and (out.records()["escaped"] > 0).sum() == 6
    # prime clears the records and the stop words, and keeps the configuration
    ic, _ = nb.ic.concat(f["ics"])
    d2, _ = to_device(nb, ic)
    ens.invalidate()  # (extended precision: the residuals of the last run go, the new arrays are the state)
    ens.prime(d2, _direct(nb, FLY["G"], FLY["eps"]), np.array(FLY_DT, np.float32))
    assert all(_is_none(r) for r in out.records()) and ens.running() == 8 and (ens.events()["stopped"] == 0).all()
    ens.advance(d2, 7)
    _same_records("after a second priming", out.records(), f["rec"])
    # set(None): back to the previous (plain) form -- the records stay, nothing is tested, nothing stops
    d3, _ = to_device(nb, ic)
    ens.invalidate()
    ens.prime(d3, _direct(nb, FLY["G"], FLY["eps"]), np.array(FLY_DT, np.float32))
    out.set(None)
    ens.advance(d3, 7)
    assert all(_is_none(r) for r in out.records()) and ens.running() == 8
    whole = _whole(d3, ens)
    for s in range(8):
        _assert_equal(("plain again", s), _cut(whole, ens, off, s), f["states"][6][s])
    # a new layout drops the configuration
    out.set(FLY_RESC, stop_on_escape=True)
    ens.setLayout(off)
    assert ens._outcomes is None
    d4, _ = to_device(nb, ic)
    ens.invalidate()
    ens.prime(d4, _direct(nb, FLY["G"], FLY["eps"]), np.array(FLY_DT, np.float32))
    ens.advance(d4, 7)
    assert all(_is_none(r) for r in out.records()) and ens.running() == 8
    ens.close()


@pytest.mark.parametrize("order", [("o", "e"), ("e", "o")], ids=["outcomes-first", "events-first"])
def test_independent_of_set_events(nb, ctx, order):
    """both configured, in either order: the fly-bys' records and stops as with outcomes alone; the closest approach is
    tracked besides; setEvents() with nothing leaves the outcomes in force"""
    f = _fly(nb)
    d, ens, off, out = _fly_ensemble(nb, f["ics"], events=dict(track_closest=True), order=order)
    ens.advance(d, 7)
    _same_records(order, out.records(), f["rec"])
    ev = ens.events()
    assert ev["stopped"].tolist() == [3 if m else 0 for m in FLY_MACRO] and np.isfinite(ev["closest_d2"]).all()
    whole = _whole(d, ens)
    for s in range(8):
        _assert_equal((order, s), _cut(whole, ens, off, s), f["states"][(FLY_MACRO[s] or 7) - 1][s])
    ic, _ = nb.ic.concat(f["ics"])
    d2, _ = to_device(nb, ic)
    ens.invalidate()  # (extended precision: the residuals of the last run go, the new arrays are the state)
    ens.prime(d2, _direct(nb, FLY["G"], FLY["eps"]), np.array(FLY_DT, np.float32))
    ens.setEvents()  # events off, outcomes still on: a stop-word form
    ens.advance(d2, 7)
    _same_records((order, "events off"), out.records(), f["rec"])
    ev = ens.events()
    assert ev["stopped"].tolist() == [3 if m else 0 for m in FLY_MACRO] and np.isposinf(ev["closest_d2"]).all()
    ens.close()


def test_refusals_at_the_c_abi(nb, ctx):
    lib = nb._lib.load()
    ok = np.array([1.0, 0.0], np.float32)
    out = np.zeros(2, nb.BATCH_OUTCOME_DTYPE)
    h = C.c_void_p()
    nb._lib.check(lib.nbody_hip_hermite_batch_create(ctx.handle, 21, 2, C.byref(h)))
    try:
        assert lib.nbody_hip_batch_outcomes_set(h, ok.ctypes.data, 0) == nb._lib.ERR_STATE  # before a layout
        assert b"no layout" in lib.nbody_hip_last_error()
        off = np.array([0, 5, 21], np.uint64)
        nb._lib.check(lib.nbody_hip_hermite_batch_set_layout(h, off.ctypes.data, 2))
        for bad in (-0.5, float("nan"), float("inf")):
            r = np.array([1.0, bad], np.float32)
            assert lib.nbody_hip_batch_outcomes_set(h, r.ctypes.data, 0) == nb._lib.ERR_VALIDATION
            assert b"escape radius of system 1 must be non-negative and finite" in lib.nbody_hip_last_error()
        zero = np.zeros(2, np.float32)
        for radii in (zero.ctypes.data, None):
            assert lib.nbody_hip_batch_outcomes_set(h, radii, 1) == nb._lib.ERR_VALIDATION
            assert b"STOP_ON_ESCAPE needs an escape radius > 0" in lib.nbody_hip_last_error()
        assert lib.nbody_hip_batch_outcomes_set(h, ok.ctypes.data, 6) == nb._lib.ERR_VALIDATION
        assert b"unknown outcome flag bits 0x6" in lib.nbody_hip_last_error()
        assert lib.nbody_hip_batch_outcomes_get(h, out.ctypes.data, 2) == nb._lib.ERR_STATE  # unprimed
        assert b"not primed" in lib.nbody_hip_last_error()
        nb._lib.check(lib.nbody_hip_batch_outcomes_set(h, ok.ctypes.data, 1))
        nb._lib.check(lib.nbody_hip_batch_outcomes_set(h, None, 0))  # off again
        # set_events is what it was
        assert lib.nbody_hip_hermite_batch_set_events(h, None, None, 4) == nb._lib.ERR_VALIDATION
        assert b"unknown event flag bits 0x4" in lib.nbody_hip_last_error()
    finally:
        lib.nbody_hip_hermite_batch_destroy(h)
    # on a primed ensemble: a wrong n_systems; "none" on a handle that never had outcomes configured
    ics = [_plummer(nb, n, seed=300 + k) for k, n in enumerate([5, 16])]
    d, ens, _, o = _ensemble(nb, ics, 0.05)
    ens.advance(d, 1)
    assert all(_is_none(r) for r in o.records())
    with pytest.raises(nb.ValidationException, match="layout has 2 systems"):
        nb._lib.check(lib.nbody_hip_batch_outcomes_get(ens._h, np.zeros(3, nb.BATCH_OUTCOME_DTYPE).ctypes.data, 3))
    ens.close()


# ---- 6. both hosts -------------------------------------------------------------------------------------------------------
def test_facade_program(nb, ctx):
    exe = os.path.join(ROOT, "n-body_amd", "lib", "hermite_batch_outcomes_tests")
    assert os.path.exists(exe), "build with __graft_entry__.build()"
    env = dict(os.environ)
    env["LD_LIBRARY_PATH"] = os.path.dirname(exe) + os.pathsep + env.get("LD_LIBRARY_PATH", "")
    r = subprocess.run([exe], cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    print(r.stdout)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    theirs = re.findall(r"^(outcome .*)$", r.stdout, re.M)
    assert len(theirs) == 3
    # the same ensemble through the Python host
    n = 300
    hst = nb.ParticleData()
    nb.ParticleDataManager.allocateHost(hst, n)
    nb.ParticleInitializer.initUniform(hst, nb.UniformDistParams((-1, -1, -1), (1, 1, 1), 0.5, 1.5), 7)
    hst.vel_x[:] = np.float32(0.1) * hst.pos_y
    hst.vel_y[:] = np.float32(-0.1) * hst.pos_x
    for i, speed in ((0, 8.0), (259, 64.0)):
        hst.pos_x[i], hst.pos_y[i], hst.pos_z[i] = 2.0, 0.0, 0.0
        hst.vel_x[i], hst.vel_y[i], hst.vel_z[i] = speed, 0.0, 0.0
    d = nb.ParticleData()
    nb.ParticleDataManager.allocateDevice(d, n)
    nb.ParticleDataManager.copyToDevice(d, hst)
    ens = nb.BlockHermiteEnsemble()
    ens.setLayout([0, 3, 260, 300])
    out = nb.EnsembleOutcomes(ens)
    out.set([2.5, 2.5, 0.0], stop_on_escape=True)
    ens.prime(d, _direct(nb, float(np.float32(1.7)), float(np.float32(0.05))), 1.0 / 64)
    ens.advance(d, 12)
    ev, rec = ens.events(), out.records()
    ours = ["outcome %d %d %d %d %s %s %s %s stopped %d done %d" % (
        s, rec["escaped"][s], rec["escaper"][s], rec["macro"][s], float(rec["r"][s]).hex(), float(rec["vr"][s]).hex(),
        float(rec["energy"][s]).hex(), float(rec["rest_mass"][s]).hex(), ev["stopped"][s], ev["macro_steps_done"][s])
        for s in range(3)]

    def fields(line):  # ("%a" and float.hex spell the same number differently: compare the values)
        w = line.split()
        return [int(x) for x in w[1:5]] + [float.fromhex(x) for x in w[5:9]] + [w[9], int(w[10]), w[11], int(w[12])]

    assert [fields(a) for a in theirs] == [fields(b) for b in ours], (theirs, ours)
    ens.close()

"""The ensemble MERGERS (nbody_hip_batch_mergers_set / _apply / _get, EnsembleMergers; include/nbody_hip.h "ensemble
MERGERS") on a real GPU.

Three oracles.  Bit equality: a system that does not merge is, array by array, counter by counter and record by record,
the system of a handle on which apply was never called; a merged system is, from its priming on, a FRESH ensemble of its
live bodies.  The restatement (tests/hermite_batch_mergers_ref.py, whose own error tests/test_hermite_batch_mergers_cpu.py
holds against exact arithmetic): slots, ids, counts and the copied contact exactly, the stored merged body within one unit
in the last place of the stored precision, the deltas within the fp64 rounding of their sums.  The ledger: the ensemble
diagnostics before and after a pass differ by the logged deltas.

The bounds of the ledger (u = 2^-53, every term of a sum has the same sign, so sum |terms| is the sum itself):
  diagnostics: KE is a sum of n terms of 7 operations and PE one of n (n - 1) / 2 terms of 9; a thread adds at most
      q = ceil(ceil(n / 2) (n - 1) / 256) pair terms (n / 256 body terms) one after the other, then 6 shuffle stages and 4
      waves: |error| <= (q + 10 + 9) u (KE + |PE|), for each of the two evaluations;
  the log: mref.ke_bound + mref.pe_bound (the restatement's docstring), which hold for the engine's evaluation too;
  mass: the stored mass is (float)M: |M - (float)M| <= 2^-24 M, and the diagnostics' sum of n masses rounds (n + 10) u sum m;
  momentum, per component c: the stored V_c is one rounding of the stored precision from V_c (2^-24 |V_c| in fp32 mode,
      2^-46 |V_c| for hi + lo), the stored mass 2^-24 M from M, V_c itself 4 u (|ma Va_c| + |mb Vb_c|) / M from exact:
      |M_s V_s - (ma Va + mb Vb)|_c <= (2^-24 + ulp_state) M |V_c| (1 + 2^-23) + 4 u (|ma Va_c| + |mb Vb_c|), plus the
      diagnostics' (n + 10) u sum |m v_c| for each of the two evaluations."""
import math
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import hermite_batch_cases as bc
import hermite_batch_events_cases as ec
import hermite_batch_mergers_ref as mref
from gpu_util import to_device

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = ("pos_x", "pos_y", "pos_z", "vel_x", "vel_y", "vel_z", "acc_x", "acc_y", "acc_z", "acc_old_x", "acc_old_y", "acc_old_z",
     "mass")
COUNTERS = ("block_steps", "body_steps", "level_steps", "floor_hits", "macro_steps", "current_tick", "last_n_active",
            "max_level")
G, DT, L = float(np.float32(1.7)), 1.0 / 64, 10  # (G as the handle holds it: fp32)
NONE = mref.NONE
U = 2.0 ** -53
FORMS = [("fp32", 0.05), ("fp32", 0.0), ("extended", 0.05), ("extended", 0.0)]
FORM_IDS = ["fp32-packed", "fp32-guard", "extended-packed", "extended-guard"]


def _direct(nb, g, eps):
    c = nb.DirectForceCalculator()
    c.setGravitationalConstant(g)
    c.setSofteningParameter(eps)
    return c


def _ensemble(nb, ics, radii, eps, precision="fp32", dt=DT, max_level=L, g=G, mergers=True, state64=None):
    """-> (d, ens, mg, offsets), primed, with the events set to stop on contact; state64: (X, V) for setExtendedState"""
    ic, offsets = nb.ic.concat(ics)
    d, _ = to_device(nb, ic)
    ens = nb.BlockHermiteEnsemble()
    ens.setParameters(0.02, 0.01, max_level)
    ens.setStatePrecision(precision)
    ens.setLayout(offsets)
    ens.setEvents(radii=np.concatenate(radii).astype(np.float32), stop_on_contact=True)
    mg = nb.EnsembleMergers(ens)
    if mergers:
        mg.set()
    fc = _direct(nb, g, eps)
    if state64 is not None:
        ens.setExtendedState(d, state64[0], state64[1], fc)
    ens.prime(d, fc, dt)
    return d, ens, mg, np.asarray(offsets).astype(np.int64)


def _whole(d, ens, mg=None):
    """every array of the ensemble as bits, the event records, and (mg) the merger state, ids and log table"""
    out = {k: getattr(d, k).cpu().numpy().view(np.uint32).copy() for k in F}
    st = ens.getState()
    out.update(jerk=st["jerk"].view(np.uint32).copy(), levels=st["levels"].copy(), ticks=st["ticks"].copy(),
               want=st["want"].view(np.uint32).copy())
    x, v = ens.getExtendedState(d)
    out.update(X=x.view(np.uint64).copy(), V=v.view(np.uint64).copy())
    out["events"] = ens.events()
    if mg is not None:
        out["mstate"], out["mlog"], out["ids"] = mg._get(True, True)
    return out


PER_SYSTEM = ("events", "mstate")


def _light(d, ens, mg):
    """state, records, log and ids: what the comparison of 300 systems with their B = 1 runs reads"""
    out = {k: getattr(d, k).cpu().numpy().view(np.uint32).copy() for k in F[:6] + ("mass",)}
    out["events"] = ens.events()
    out["mstate"], out["mlog"], out["ids"] = mg._get(True, True)
    return out


def _cut(whole, ens, offsets, s):
    a, b = int(offsets[s]), int(offsets[s + 1])
    one = {k: (v[s:s + 1] if k in PER_SYSTEM else v[a:b]) for k, v in whole.items()}
    info = ens.info(s)
    one["info"] = {k: info[k] for k in COUNTERS}
    return one


def _assert_equal(tag, got, ref, skip=()):
    assert got.keys() == ref.keys(), tag
    for k in ref:
        if k in skip:
            continue
        if k == "info":
            assert got[k] == ref[k], (tag, got[k], ref[k])
        else:
            assert got[k].shape == ref[k].shape and got[k].tobytes() == ref[k].tobytes(), (tag, k)


def _case_systems(nb):
    ics = [mref.case_ic(nb, n, pair) for _, n, pair in mref.CASES]
    radii = [mref.case_radii(n, pair) for _, n, pair in mref.CASES]
    return ics, radii


# ---- 1. nothing else moves ------------------------------------------------------------------------------------------------
def test_nothing_else_moves(nb, ctx):
    """systems that stop on contact (a triple whose pair is the last slot, a 257 whose last body moves) between systems
    that do not (no radii): after apply the latter equal a handle on which apply was never called, in every array,
    counter and record, and go on equal; mergers configured but never applied is the STOP_ON_CONTACT run"""
    quiet5, quiet2 = dict(nb.ic.plummer(5, seed=11)), dict(nb.ic.plummer(2, seed=12))
    ics = [quiet5, mref.case_ic(nb, 3, (0, 2)), quiet2, mref.case_ic(nb, 257, (3, 255)), dict(nb.ic.plummer(64, seed=13))]
    radii = [np.zeros(5), mref.case_radii(3, (0, 2)), np.zeros(2), mref.case_radii(257, (3, 255)), np.zeros(64)]
    merging = (1, 3)
    for precision, eps in (("fp32", 0.05), ("extended", 0.0)):
        da, ea, ma, off = _ensemble(nb, ics, radii, eps, precision)
        db, eb, mb, _ = _ensemble(nb, ics, radii, eps, precision)
        dc, ec_, _, _ = _ensemble(nb, ics, radii, eps, precision, mergers=False)
        for e, d in ((ea, da), (eb, db), (ec_, dc)):
            e.advance(d, 2)
        ma.apply(da)
        a, b, c = _whole(da, ea, ma), _whole(db, eb, mb), _whole(dc, ec_)
        _assert_equal("configured, never applied", {k: v for k, v in b.items() if k not in ("mstate", "mlog", "ids")}, c)
        assert (b["mstate"]["n_mergers"] == 0).all() and (b["mlog"]["mass"] == 0).all()
        for s in range(len(ics)):
            if s in merging:
                assert b["events"]["stopped"][s] == 1 and a["events"]["stopped"][s] == 0
                assert a["mstate"]["n_mergers"][s] == 1 and a["mstate"]["n_live"][s] == len(radii[s]) - 1
            else:
                _assert_equal(("untouched", precision, s), _cut(a, ea, off, s), _cut(b, eb, off, s))
        assert ea.running() == len(ics) and eb.running() == len(ics) - len(merging)
        ea.advance(da, 2)
        eb.advance(db, 2)
        a, b = _whole(da, ea, ma), _whole(db, eb, mb)
        for s in range(len(ics)):
            if s not in merging:
                _assert_equal(("untouched, two more", precision, s), _cut(a, ea, off, s), _cut(b, eb, off, s))
        for e in (ea, eb, ec_):
            e.close()


# ---- 2, 3, 4. the merge arithmetic, the priming, the ledger: one run per form, shared -----------------------------------------
_RUNS = {}


def _plain_diagnostics(nb, ctx, d, offsets, eps, whole, rows, ext):
    """nb.systems_diagnostics -- the plain kernel, which knows no live counts -- of the particle data d with the given
    offsets; the residuals (extended mode) are those of the rows `rows` of `whole`: X - (double)pos, exact in fp32"""
    lo = [None, None]
    if ext:
        for k, (f, p) in enumerate((("X", "pos_"), ("V", "vel_"))):
            hi = np.stack([whole[p + c][rows].view(np.float32) for c in "xyz"], 1).astype(np.float64)
            r = np.zeros((len(rows), 4), np.float32)
            r[:, :3] = whole[f][rows].view(np.float64) - hi
            assert (hi + r[:, :3].astype(np.float64) == whole[f][rows].view(np.float64)).all()
            lo[k] = torch.from_numpy(r).to(d.pos_x.device)
    return nb.systems_diagnostics(ctx, d, np.asarray(offsets, np.int64), G, eps, lo[0], lo[1])


def _run(nb, ctx, precision, eps):
    """the seven systems of mref.CASES in one ensemble: advance(1) (every pair is in contact at the first block step),
    the state, apply, the state; then a FRESH ensemble of the live bodies (no mergers configured on it), primed, and
    advance(3) on both.  diag: the handle's diagnostics before and after the pass (the kernel with live counts), and the
    plain kernel's of the whole data before it and of the compacted copy of the live bodies after it"""
    key = (precision, eps)
    if key in _RUNS:
        return _RUNS[key]
    ext = precision == "extended"
    ics, radii = _case_systems(nb)
    d, ens, mg, off = _ensemble(nb, ics, radii, eps, precision)
    ens.advance(d, 1)
    before, diag0 = _whole(d, ens, mg), ens.diagnostics(d)
    plain0 = _plain_diagnostics(nb, ctx, d, off, eps, before, np.arange(int(off[-1])), ext)
    mg.apply(d)
    after, diag1 = _whole(d, ens, mg), ens.diagnostics(d)
    log = mg.log()
    # the restatement, system by system, driven by the engine's contact records
    refs = []
    for s in range(len(ics)):
        a, b = int(off[s]), int(off[s + 1])
        ev = before["events"][s]
        X, V = before["X"][a:b].view(np.float64), before["V"][a:b].view(np.float64)
        sysr = mref.System.from_f64(X, V, before["mass"][a:b].view(np.float32), radii[s], ext)
        lo = min(int(ev["contact_i"]), int(ev["contact_j"]))
        stored = (after["mass"][a + lo:a + lo + 1].view(np.float32)[0],) + tuple(
            np.array([after[p + c][a + lo] for c in "xyz"], np.uint32).view(np.float32) for p in ("pos_", "vel_"))
        Xa, Va = after["X"][a + lo].view(np.float64), after["V"][a + lo].view(np.float64)
        hi_p, hi_v = stored[1].astype(np.float64), stored[2].astype(np.float64)
        stored = (stored[0], stored[1], (Xa - hi_p).astype(np.float32), stored[2], (Va - hi_v).astype(np.float32))
        e = mref.merge(sysr, ev["contact_i"], ev["contact_j"], G, eps,
                       (ev["contact_d2"], ev["contact_tick"], ev["contact_macro"]), stored=stored)
        refs.append((sysr, e))
    # the fresh ensemble of the live bodies
    live = np.concatenate([np.arange(off[s], off[s] + after["mstate"]["n_live"][s]) for s in range(len(ics))])
    fresh_ics = []
    for s in range(len(ics)):
        a, n1 = int(off[s]), int(after["mstate"]["n_live"][s])
        fresh_ics.append({k: after[k][a:a + n1].view(np.float32).copy() for k in F[:6] + ("mass",)})
    fresh_radii = [r.radii[:r.n] for r, _ in refs]
    for (r, e), s in zip(refs, range(len(ics))):
        fresh_radii[s] = fresh_radii[s].copy()
        fresh_radii[s][e["slot_a"]] = log["radius"][log["system"] == s][0]  # (the engine's, asserted within an ulp of r's)
    state64 = (after["X"][live].view(np.float64), after["V"][live].view(np.float64)) if ext else None
    d2, ens2, mg2, off2 = _ensemble(nb, fresh_ics, fresh_radii, eps, precision, mergers=False, state64=state64)
    primed2 = _whole(d2, ens2, mg2)
    plain1 = _plain_diagnostics(nb, ctx, d2, off2, eps, after, live, ext)  # (d2: the compacted copy of the live bodies)
    ens.advance(d, 3)
    ens2.advance(d2, 3)
    later, later2 = _whole(d, ens, mg), _whole(d2, ens2, mg2)
    _RUNS[key] = dict(off=off, off2=off2, before=before, after=after, log=log, refs=refs, live=live, primed2=primed2,
                      later=later, later2=later2, diag=(diag0, diag1, plain0, plain1), radii=radii)
    ens.close()
    ens2.close()
    return _RUNS[key]


@pytest.mark.parametrize("precision,eps", FORMS, ids=FORM_IDS)
def test_the_merge_arithmetic(nb, ctx, precision, eps):
    r = _run(nb, ctx, precision, eps)
    ext = precision == "extended"
    off, before, after, log = r["off"], r["before"], r["after"], r["log"]
    assert log["system"].tolist() == list(range(len(mref.CASES))) and (after["mstate"]["n_mergers"] == 1).all()
    assert (after["mstate"]["flags"] == 0).all()
    for s, (name, n, pair) in enumerate(mref.CASES):
        a, b = int(off[s]), int(off[s + 1])
        sysr, e = r["refs"][s]
        ev0, ev1, g = before["events"][s], after["events"][s], log[s]
        assert {int(ev0["contact_i"]), int(ev0["contact_j"])} == set(pair) and ev0["stopped"] == 1, name
        # exactly: slots, ids, counts, the move, the copied contact, the event record
        assert (g["slot_a"], g["slot_b"], g["id_a"], g["id_b"], g["moved_from"]) == (
            e["slot_a"], e["slot_b"], e["id_a"], e["id_b"], e["moved_from"]), name
        assert e["moved_from"] == (NONE if pair[1] == n - 1 else n - 1) and (g["slot_a"], g["slot_b"]) == pair
        assert (g["contact_tick"], g["contact_macro"]) == (ev0["contact_tick"], ev0["contact_macro"])
        assert g["contact_d2"].tobytes() == ev0["contact_d2"].tobytes() and np.isfinite(g["contact_d2"])
        assert after["mstate"]["n_live"][s] == n - 1 == sysr.n
        assert after["ids"][a:b].tolist() == sysr.ids.tolist() and after["ids"][b - 1] == NONE
        assert ev1["stopped"] == 0 and ev1["macro_steps_done"] == ev0["macro_steps_done"] == 1
        assert np.isposinf(ev1["contact_d2"]) and np.isposinf(ev1["closest_d2"])
        assert ev1["contact_i"] == ev1["contact_j"] == ev1["closest_i"] == ev1["closest_j"] == NONE
        assert ev1["contact_tick"] == ev1["closest_tick"] == 0 and ev1["contact_macro"] == ev1["closest_macro"] == 0
        # the merged body: M exactly (one fp64 sum), the stored values within one unit in the last place
        lo = e["slot_a"]
        own_m, own_ph, own_pl, own_vh, own_vl = e["own"]
        assert g["mass"] == e["mass"] and after["mass"][a + lo].view(np.float32) == own_m, name
        Xg, Vg = after["X"][a + lo].view(np.float64), after["V"][a + lo].view(np.float64)
        Xr = own_ph.astype(np.float64) + own_pl.astype(np.float64)
        Vr = own_vh.astype(np.float64) + own_vl.astype(np.float64)
        for got, want in ((Xg, Xr), (Vg, Vr)):
            tol = 2.0 ** -46 * np.abs(want) if ext else np.spacing(np.abs(want).astype(np.float32)).astype(np.float64)
            assert (np.abs(got - want) <= tol).all(), (name, got, want)
        if not ext:  # fp32 mode holds no residual
            hi = np.array([after["pos_" + c][a + lo] for c in "xyz"], np.uint32).view(np.float32).astype(np.float64)
            assert (Xg == hi).all()
        assert abs(float(g["radius"]) - float(e["radius"])) <= np.spacing(e["radius"]), name
        # everybody else: the slots of the restatement, bit for bit; the dead slot
        for k in range(n - 1):
            if k == lo:
                continue
            assert (after["X"][a + k].view(np.float64) == sysr.X()[k]).all() and (after["V"][a + k].view(np.float64) == sysr.V()[k]).all(), (name, k)
            assert after["mass"][a + k].view(np.float32) == sysr.mass[k], (name, k)
        dead = b - 1
        assert after["mass"][dead] == 0 and all(after[f][dead] == 0 for f in F[3:9]) and (after["V"][dead] == 0).all()
        assert all(after[f][dead] == before[f][dead] for f in F[:3])  # (its position stays)
        # the deltas, from the values as stored
        assert abs(g["delta_ke"] - e["delta_ke"]) <= 2 * mref.ke_bound(e), (name, g["delta_ke"], e["delta_ke"])
        assert abs(g["delta_pe"] - e["delta_pe"]) <= 2 * mref.pe_bound(e, G), (name, g["delta_pe"], e["delta_pe"])
        print(f"{name} {precision} eps {eps}: dke {g['delta_ke']:.6e} (|diff| {abs(g['delta_ke'] - e['delta_ke']):.1e}), dpe "
              f"{g['delta_pe']:.6e} (|diff| {abs(g['delta_pe'] - e['delta_pe']):.1e}, bound {2 * mref.pe_bound(e, G):.1e})", flush=True)


def test_two_equal_bodies_head_on(nb, ctx):
    """ec.head_on with radii that touch from the start: V exactly 0, X exactly the midpoint, in both precisions"""
    pos, vel, m = ec.head_on()
    for precision in ("fp32", "extended"):
        d, ens, mg, _ = _ensemble(nb, [bc.ic_of(pos, vel, m)], [np.array([0.6, 0.6])], 0.05, precision, dt=1.0 / 16, g=1.0)
        ens.advance(d, 1)
        x0, v0 = ens.getExtendedState(d)
        assert (x0[0] == -x0[1]).all() and (v0[0] == -v0[1]).all() and ens.events()["stopped"][0] == 1
        mg.apply(d)
        x, v = ens.getExtendedState(d)
        assert (x[0] == 0).all() and (v[0] == 0).all() and d.mass.cpu().numpy().tolist() == [1.0, 0.0]
        rec, log = mg.records(), mg.log()
        assert (rec["n_live"][0], rec["n_mergers"][0]) == (1, 1) and log["mass"][0] == 1.0 and mg.alive().tolist() == [True, False]
        ens.close()


@pytest.mark.parametrize("precision,eps", FORMS, ids=FORM_IDS)
def test_priming_again_is_the_priming(nb, ctx, precision, eps):
    """n_live = 1, 2, 2, 2, 4, 256, 1,024: a, jerk, levels, ticks and want of the merged systems equal a fresh ensemble of
    their live bodies bit for bit, and after advance(3) on both every array does"""
    r = _run(nb, ctx, precision, eps)
    live, after, fresh = r["live"], r["after"], r["primed2"]
    assert sorted(set(after["mstate"]["n_live"].tolist())) == [1, 2, 4, 256, 1024]
    for k in ("acc_x", "acc_y", "acc_z", "jerk", "levels", "ticks", "want", "pos_x", "pos_y", "pos_z", "vel_x", "vel_y",
              "vel_z", "mass", "X", "V"):
        assert after[k][live].tobytes() == fresh[k].tobytes(), ("primed", k)
    assert (after["ticks"][live] == 0).all()
    later, later2 = r["later"], r["later2"]
    assert (later["events"]["stopped"] == 0).all() and (later2["events"]["stopped"] == 0).all()
    assert (later["events"]["macro_steps_done"] == 4).all() and (later2["events"]["macro_steps_done"] == 3).all()
    for k in F + ("jerk", "levels", "ticks", "want", "X", "V"):
        assert later[k][live].tobytes() == later2[k].tobytes(), ("advance(3)", k)


@pytest.mark.parametrize("precision,eps", FORMS, ids=FORM_IDS)
def test_the_energy_ledger(nb, ctx, precision, eps):
    r = _run(nb, ctx, precision, eps)
    ext = precision == "extended"
    d0, d1, p0, p1 = r["diag"]
    ulp_state = 2.0 ** -46 if ext else 2.0 ** -24
    for s, (name, n, _) in enumerate(mref.CASES):
        sysr, e = r["refs"][s]
        g = r["log"][s]
        # the live bodies only, and bit for bit what the plain kernel (nb.systems_diagnostics, which knows no live
        # counts) gives for a compacted copy of them; before the pass (live count = slot count) for the whole data
        assert d1["n"][s] == n - 1 and d0["n"][s] == n and d1["status"][s] == 0
        assert d1[s].tobytes() == p1[s].tobytes() and d0[s].tobytes() == p0[s].tobytes(), name
        q = math.ceil(math.ceil(n / 2) * (n - 1) / 256)
        e0, e1 = d0["kinetic"][s] + d0["potential"][s], d1["kinetic"][s] + d1["potential"][s]
        sums = d0["kinetic"][s] + abs(d0["potential"][s]) + d1["kinetic"][s] + abs(d1["potential"][s])
        bound = (q + 19) * U * sums + mref.ke_bound(e) + mref.pe_bound(e, G)
        got, want = e1 - e0, g["delta_ke"] + g["delta_pe"]
        print(f"{name} {precision} eps {eps}: dE {got:.9e} logged {want:.9e} |diff| {abs(got - want):.2e} bound {bound:.2e}", flush=True)
        assert abs(got - want) <= bound, name
        M = e["mass"]
        assert abs(d1["mass"][s] - d0["mass"][s]) <= 2.0 ** -24 * M + 2 * (n + 10) * U * d0["mass"][s], name
        Vm = sysr.V()[e["slot_a"]]
        for c in range(3):
            sum_mv = float(np.abs(sysr.mass[:sysr.n].astype(np.float64) * sysr.V()[:sysr.n, c]).sum()) + float(e["momentum_terms"][c])
            tol = (2.0 ** -24 + ulp_state) * M * abs(Vm[c]) * (1 + 2.0 ** -23) + 4 * U * e["momentum_terms"][c] + 2 * (n + 10) * U * sum_mv
            assert abs(d1["momentum"][s][c] - d0["momentum"][s][c]) <= tol, (name, c)


# ---- 5. chains ---------------------------------------------------------------------------------------------------------------
def test_chains(nb, ctx):
    """three collinear overlapping bodies beside a system that never touches: two advance; apply rounds give one body, two
    entries and the ids the restatement predicts; the single body runs on"""
    pos = np.array([[0.0, 0, 0], [0.01, 0, 0], [0.025, 0, 0]], np.float32)
    chain = bc.ic_of(pos, np.zeros((3, 3), np.float32), np.array([1.0, 0.5, 0.25], np.float32))
    ics, radii = [chain, dict(nb.ic.plummer(4, seed=21))], [np.full(3, 0.02, np.float32), np.zeros(4, np.float32)]
    d, ens, mg, off = _ensemble(nb, ics, radii, 0.05, g=1.0)
    sysr = mref.System(pos, np.zeros((3, 3)), chain["mass"], radii[0])
    for rnd in range(2):
        ens.advance(d, 1)
        ev = ens.events()
        assert ev["stopped"].tolist() == [1, 0] and ens.running() == 1
        w = _whole(d, ens, mg)
        sysr.pos, sysr.vel = (np.stack([w[p + c][:3].view(np.float32) for c in "xyz"], 1) for p in ("pos_", "vel_"))
        assert mref.merge(sysr, ev["contact_i"][0], ev["contact_j"][0], 1.0, 0.05) is not None
        mg.apply(d)
        assert ens.running() == 2  # the revived system counts again
        rec = mg.records()
        assert (rec["n_live"][0], rec["n_mergers"][0], rec["flags"][0]) == (2 - rnd, rnd + 1, 0)
        assert mg.ids()[:3].tolist() == sysr.ids.tolist()
    log = mg.log()
    assert log["system"].tolist() == [0, 0] and [(g["id_a"], g["id_b"]) for g in log] == [(e["id_a"], e["id_b"]) for e in sysr.log]
    assert log["mass"].tolist() == [e["mass"] for e in sysr.log] and log["mass"][1] == 1.75
    assert mg.ids()[:3].tolist() == [0, NONE, NONE] and mg.alive().tolist() == [True, False, False, True, True, True, True]
    assert d.mass.cpu().numpy()[:3].tolist() == [1.75, 0.0, 0.0]
    ens.advance(d, 2)
    ev = ens.events()
    assert ev["stopped"].tolist() == [0, 0] and ev["macro_steps_done"].tolist() == [4, 4] and ens.running() == 2
    assert ens.info(0)["macro_steps"] == 4 and np.isfinite(d.pos_x.cpu().numpy()).all()
    # a pass with nobody stopped changes nothing
    w0 = _whole(d, ens, mg)
    mg.apply(d)
    _assert_equal("idle pass", _whole(d, ens, mg), w0)
    ens.close()


# ---- 6. place in the batch and launch structure -------------------------------------------------------------------------------
def _triples(nb, ics, radii, systems):
    c = bc.TRIPLE
    return _ensemble(nb, [ics[s] for s in systems], [radii[s] for s in systems], c["eps"], dt=c["dt_max"],
                     max_level=c["max_level"], g=float(np.float32(c["G"])))


def test_more_systems_than_compute_units_and_the_launch_structure(nb, ctx):
    ics, radii, hit = ec.colliding_triples(300)
    every = list(range(300))
    d, ens, mg, off = _triples(nb, ics, radii, every)
    mg.run(d, 8, every=1)
    whole = _whole(d, ens, mg)
    merged = whole["mstate"]["n_mergers"] > 0
    print("merged", int(merged.sum()), "twice", int((whole["mstate"]["n_mergers"] > 1).sum()), "never touched", int((~hit).sum()))
    assert merged.sum() >= 50 and (~merged & ~hit).sum() >= 50 and not merged[~hit].any()
    assert (whole["mstate"]["n_live"] + whole["mstate"]["n_mergers"] == 3).all() and (whole["mstate"]["flags"] == 0).all()
    # run() is the eager loop
    d2, ens2, mg2, _ = _triples(nb, ics, radii, every)
    for _ in range(8):
        ens2.advance(d2, 1)
        mg2.apply(d2)
    _assert_equal("run == loop", whole, _whole(d2, ens2, mg2))
    ens2.close()
    # every system is the system run alone
    for s in every:
        d1, e1, m1, _ = _triples(nb, ics, radii, [s])
        m1.run(d1, 8, every=1)
        one = _light(d1, e1, m1)
        a, b = int(off[s]), int(off[s + 1])
        for k, v in one.items():
            mine = whole[k][s:s + 1] if k in PER_SYSTEM else whole[k][a:b]
            assert mine.tobytes() == v.tobytes(), (s, k)
        e1.close()
    ens.close()


def test_the_pass_in_a_step_graph(nb, ctx):
    """one eager round and three replays of a recorded [advance(1), apply] equal four eager rounds; a recording before
    the first eager apply is refused"""
    ics, radii, hit = ec.colliding_triples(40)
    every = list(range(40))
    d, ens, mg, _ = _triples(nb, ics, radii, every)
    ens.advance(d, 1)
    with pytest.raises(nb.StateException, match="step graph"):
        with ctx.capture():
            mg.apply(d)
    mg.apply(d)  # eagerly first
    with ctx.capture() as rec:
        ens.advance(d, 1)
        mg.apply(d)
    rec.graph.launch(3)
    d2, ens2, mg2, _ = _triples(nb, ics, radii, every)
    mg2.run(d2, 4, every=1)
    got, want = _whole(d, ens, mg), _whole(d2, ens2, mg2)
    assert (want["mstate"]["n_mergers"] > 0).sum() >= 5
    _assert_equal("1 eager + 3 replayed", got, want)
    rec.graph.close()
    ens.close()
    ens2.close()


# ---- 7. resetting and refusals --------------------------------------------------------------------------------------------------
def test_resetting_and_refusals(nb, ctx):
    ics, radii = [mref.case_ic(nb, 3, (0, 1)), dict(nb.ic.plummer(5, seed=31))], [mref.case_radii(3, (0, 1)), np.zeros(5, np.float32)]
    d, ens, mg, off = _ensemble(nb, ics, radii, 0.05)
    rec, log, ids = mg._get(True, True)
    assert rec["n_live"].tolist() == [3, 5] and ids.tolist() == [0, 1, 2, 0, 1, 2, 3, 4] and mg.log().size == 0
    ens.advance(d, 1)
    mg.apply(d)
    assert mg.records()["n_live"].tolist() == [2, 5] and mg.log().size == 1 and mg.ids()[:3].tolist() == [0, 2, NONE]
    # prime restores n, ids and an empty log (the data and the radii are set again: the pass changed both)
    d, _ = to_device(nb, nb.ic.concat(ics)[0])
    ens.setEvents(radii=np.concatenate(radii), stop_on_contact=True)
    fc = _direct(nb, G, 0.05)
    ens.prime(d, fc, DT)
    rec, log, ids = mg._get(True, True)
    assert rec["n_live"].tolist() == [3, 5] and rec["n_mergers"].tolist() == [0, 0] and ids.tolist() == [0, 1, 2, 0, 1, 2, 3, 4]
    assert (log["mass"] == 0).all() and mg.log().size == 0 and mg.alive().all()
    ens.advance(d, 1)
    assert ens.events()["stopped"].tolist() == [1, 0]  # (three bodies again: the same contact)
    # the library's refusals (the Python layer's own come first and are lifted here)
    lib, s = nb._lib.load(), d.struct()
    import ctypes as C
    mg.set(False)
    assert lib.nbody_hip_batch_mergers_apply(ens._h, C.byref(s)) == nb._lib.ERR_STATE
    assert b"mergers are not configured" in lib.nbody_hip_last_error()
    assert lib.nbody_hip_batch_mergers_set(ens._h, 6) == nb._lib.ERR_VALIDATION and b"unknown merger flag bits 0x6" in lib.nbody_hip_last_error()
    mg.set(True)
    for kw in (dict(), dict(radii=np.concatenate(radii), track_closest=True)):  # no events; events without STOP_ON_CONTACT
        ens.setEvents(**kw)
        assert lib.nbody_hip_batch_mergers_apply(ens._h, C.byref(s)) == nb._lib.ERR_STATE
        assert b"STOP_ON_CONTACT" in lib.nbody_hip_last_error()
        with pytest.raises(nb.StateException, match="stop_on_contact=True"):
            mg.apply(d)
    ens.setEvents(radii=np.concatenate(radii), stop_on_contact=True)
    other, _ = to_device(nb, nb.ic.concat(ics)[0])
    with pytest.raises(nb.StateException, match="differ from the primed ones"):
        mg.apply(other)
    bad = (nb.BatchMergerStateStruct * 3)()
    assert lib.nbody_hip_batch_mergers_get(ens._h, C.cast(bad, C.c_void_p), 3, None, None, 8) == nb._lib.ERR_VALIDATION
    assert lib.nbody_hip_batch_mergers_get(ens._h, C.cast(bad, C.c_void_p), 2, None, None, 7) == nb._lib.ERR_VALIDATION
    # set_layout drops the configuration: the Python layer forgets it, and so does the handle
    ens.setLayout(off)
    assert ens._mergers is None
    ens.setEvents(radii=np.concatenate(radii), stop_on_contact=True)
    ens.prime(d, fc, DT)
    assert lib.nbody_hip_batch_mergers_apply(ens._h, C.byref(s)) == nb._lib.ERR_STATE
    assert b"mergers are not configured" in lib.nbody_hip_last_error()
    # unprimed
    mg.set()
    ens.invalidate()
    assert lib.nbody_hip_batch_mergers_apply(ens._h, C.byref(s)) == nb._lib.ERR_STATE and b"not primed" in lib.nbody_hip_last_error()
    ens.close()
    # a handle that never had mergers configured: n_live = n, no entries, ids 0 .. n-1
    d, ens, mg, off = _ensemble(nb, ics, radii, 0.05, mergers=False)
    rec, log, ids = mg._get(True, True)
    assert rec["n_live"].tolist() == [3, 5] and rec["n_mergers"].tolist() == [0, 0] and ids.tolist() == [0, 1, 2, 0, 1, 2, 3, 4]
    assert (log["mass"] == 0).all() and mg.alive().all()
    ens.close()


# ---- 8. the facade -------------------------------------------------------------------------------------------------------------
def test_facade_program(nb, ctx):
    exe = os.path.join(ROOT, "n-body_amd", "lib", "hermite_batch_mergers_tests")
    assert os.path.exists(exe), "build with __graft_entry__.build()"
    env = dict(os.environ)
    env["LD_LIBRARY_PATH"] = os.path.dirname(exe) + os.pathsep + env.get("LD_LIBRARY_PATH", "")
    r = subprocess.run([exe], cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    print(r.stdout)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    theirs = re.findall(r"^((?:mstate|merger|ids) .*)$", r.stdout, re.M)
    assert len(theirs) == 8
    # the same ensemble through the Python host
    n = 300
    hst = nb.ParticleData()
    nb.ParticleDataManager.allocateHost(hst, n)
    nb.ParticleInitializer.initUniform(hst, nb.UniformDistParams((-1, -1, -1), (1, 1, 1), 0.5, 1.5), 7)
    hst.vel_x[:] = np.float32(0.1) * hst.pos_y
    hst.vel_y[:] = np.float32(-0.1) * hst.pos_x
    radii = np.zeros(n, np.float32)
    for i, j in ((0, 2), (6, 258)):
        for k, dx in ((i, -0.005), (j, 0.005)):
            hst.pos_x[k], hst.pos_y[k], hst.pos_z[k] = np.float32(2.0) + np.float32(dx), 0.0, 0.0
            hst.vel_x[k], hst.vel_y[k], hst.vel_z[k] = 0.0, 0.0, 0.0
            radii[k] = 0.02
    d = nb.ParticleData()
    nb.ParticleDataManager.allocateDevice(d, n)
    nb.ParticleDataManager.copyToDevice(d, hst)
    off = [0, 3, 260, 300]
    ens = nb.BlockHermiteEnsemble()
    ens.setLayout(off)
    ens.setEvents(radii=radii, stop_on_contact=True)
    mg = nb.EnsembleMergers(ens)
    mg.set()
    ens.prime(d, _direct(nb, float(np.float32(1.7)), float(np.float32(0.05))), 1.0 / 64)
    mg.run(d, 2, every=1)
    rec, log, ids, ev = mg.records(), mg.log(), mg.ids(), ens.events()
    ours = []
    for s in range(3):
        ours.append("mstate %d %d %d %d stopped %d done %d" % (s, rec["n_live"][s], rec["n_mergers"][s], rec["flags"][s],
                                                               ev["stopped"][s], ev["macro_steps_done"][s]))
        for g in log[log["system"] == s]:
            ours.append("merger %d %d %d %d %d %d %d %d %s %s %s %s %s" % (
                s, g["slot_a"], g["slot_b"], g["id_a"], g["id_b"], g["moved_from"], g["contact_tick"], g["contact_macro"],
                float(g["contact_d2"]).hex(), float(g["radius"]).hex(), float(g["mass"]).hex(), float(g["delta_ke"]).hex(),
                float(g["delta_pe"]).hex()))
        mine = ids[off[s]:off[s + 1]]
        ours.append("ids %d %d %s" % (s, int((mine == NONE).sum()), " ".join(str(int(mine[k])) for k in (0, 1, 2, 3, 255, 256) if k < mine.size)))

    def fields(line):  # ("%a" and float.hex spell the same number differently: compare the values)
        w = line.split()
        if w[0] == "merger":
            return w[:1] + [int(x) for x in w[1:9]] + [float.fromhex(x) for x in w[9:]]
        return [int(x) if x.isdigit() else x for x in w]

    assert [fields(a) for a in theirs] == [fields(b) for b in ours], (theirs, ours)
    ens.close()

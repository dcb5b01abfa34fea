"""The ensemble EVENTS (nbody_hip_hermite_batch_set_events / _events / _running, BlockHermiteEnsemble.setEvents / events /
running; include/nbody_hip.h "ensemble EVENTS") on a real GPU.

Two oracles.  Bit equality: a system with events configured is, up to its stop, the plain ensemble's system, array by array
and counter by counter.  The restatement: tests/hermite_block_ref.py driven ONE BLOCK STEP AT A TIME beside a
single-system BlockHermiteIntegrator in its narrow host-scheduled form -- which the ensemble equals bit for bit
(tests/test_hermite_batch_gpu.py, tests/test_hermite_block_resident_gpu.py) -- seeded with the engine's primed a, j and
levels and fed the engine's own a1, j1 as tests/test_hermite_block_gpu.py does, so that both walk the same schedule; the
closest approach and the first contact are then formed in fp64 from the restatement's predicted positions
(tests/hermite_batch_events_cases.py).  Macro index, tick, i and j must be equal exactly; the separation within
|d_engine - d_ref| <= 2 sqrt(3) delta + 4 u d, u = 2^-24, with delta = 6e-8 the absolute per-coordinate tolerance
tests/test_hermite_block_gpu.py grants the engine's state against this restatement after a block step (`dv <= 6e-8`;
positions equal in their bits) at these cases' O(1) coordinates."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import hermite_batch_cases as bc
import hermite_batch_events_cases as ec
import hermite_block_ref as br
from gpu_util import to_device

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = ("pos_x", "pos_y", "pos_z", "vel_x", "vel_y", "vel_z", "acc_x", "acc_y", "acc_z", "acc_old_x", "acc_old_y", "acc_old_z",
     "mass")
COUNTERS = ("block_steps", "body_steps", "level_steps", "floor_hits", "macro_steps", "current_tick", "last_n_active",
            "max_level")
REC = ("closest_d2", "closest_i", "closest_j", "closest_macro", "closest_tick", "contact_d2", "contact_i", "contact_j",
       "contact_macro", "contact_tick")
G, DT = 1.7, 1.0 / 16
NONE = ec.NONE


def _plummer(nb, n, seed=42):
    ic = dict(nb.ic.plummer(n, seed=seed))
    ic["mass"] = (ic["mass"] * np.random.default_rng(5 + seed).uniform(0.5, 2.0, ic["mass"].size)).astype(np.float32)
    return ic


def _direct(nb, g, eps):
    c = nb.DirectForceCalculator()
    c.setGravitationalConstant(g)
    c.setSofteningParameter(eps)
    return c


def _ensemble(nb, ics, eps, precision="fp32", dt=DT, max_level=16, g=G, events=None):
    """-> (d, ens, offsets), primed; events: the keywords of setEvents (sent after the layout, before the priming)"""
    ic, offsets = nb.ic.concat(ics)
    d, _ = to_device(nb, ic)
    ens = nb.BlockHermiteEnsemble()
    ens.setParameters(0.02, 0.01, max_level)
    ens.setStatePrecision(precision)
    ens.setLayout(offsets)
    if events is not None:
        ens.setEvents(**events)
    ens.prime(d, _direct(nb, g, eps), dt)
    return d, ens, offsets


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


def _none(ev, what):
    assert np.isposinf(ev[what + "_d2"]) and ev[what + "_i"] == NONE and ev[what + "_j"] == NONE
    assert ev[what + "_macro"] == 0 and ev[what + "_tick"] == 0


def _same_records(tag, a, b, fields=("stopped", "macro_steps_done") + REC):
    for k in fields:
        assert np.ascontiguousarray(a[k]).tobytes() == np.ascontiguousarray(b[k]).tobytes(), (tag, k, a[k], b[k])


# ---- 1. tracking changes no bit ----------------------------------------------------------------------------------------
# 1: no pair; 2: the packed pair; 5: padding inside a group of four; 257: two sub-blocks' worth of sources; 1,025: a second
# 1,024-source block holding one body.  Offsets 0, 1, 6, 263, 265, 1290: none but the first a multiple of 4.
SIZES = [1, 5, 257, 2, 1025]
FORMS = [("fp32", 0.05), ("fp32", 0.0), ("extended", 0.05), ("extended", 0.0)]
FORM_IDS = ["fp32-packed", "fp32-guard", "extended-packed", "extended-guard"]
_PLAIN = {}


def _plain3(nb, precision, eps):
    """the plain handle's advance(3) of the SIZES batch, computed once per form and shared"""
    if (precision, eps) not in _PLAIN:
        ics = [_plummer(nb, n, seed=200 + k) for k, n in enumerate(SIZES)]
        d, ens, off = _ensemble(nb, ics, eps, precision)
        assert [int(o) for o in off] == [0, 1, 6, 263, 265, 1290]
        ens.advance(d, 3)
        whole = _whole(d, ens)
        _PLAIN[(precision, eps)] = (ics, whole, [_cut(whole, ens, off, s)["info"] for s in range(len(SIZES))])
        ens.close()
    return _PLAIN[(precision, eps)]


@pytest.mark.parametrize("precision,eps", FORMS, ids=FORM_IDS)
def test_tracking_changes_no_bit(nb, ctx, precision, eps):
    ics, plain, infos = _plain3(nb, precision, eps)
    total = sum(SIZES)
    d, ens, off = _ensemble(nb, ics, eps, precision,
                            events=dict(radii=np.zeros(total, np.float32), max_macro_steps=np.zeros(len(SIZES), np.int64),
                                        track_closest=True))
    ens.advance(d, 3)
    got = _whole(d, ens)
    _assert_equal(("tracked", precision, eps), got, plain)
    for s in range(len(SIZES)):
        assert _cut(got, ens, off, s)["info"] == infos[s], s
    ev = ens.events()
    assert (ev["stopped"] == 0).all() and (ev["macro_steps_done"] == 3).all() and ens.running() == len(SIZES)
    _none(ev[0], "closest")  # (n = 1)
    for s in range(len(SIZES)):
        _none(ev[s], "contact")  # (radii 0: rs > 0 never holds)
        if SIZES[s] > 1:
            assert ev["closest_i"][s] < SIZES[s] and ev["closest_j"][s] < SIZES[s] and np.isfinite(ev["closest_d2"][s])
            assert ev["closest_macro"][s] < 3 and 1 <= ev["closest_tick"][s] <= 2 ** 16


# ---- 2. the closest-approach record against the restatement ------------------------------------------------------------
def _lockstep(nb, ic, g, eps, dt, L, macros, radii=None, until_contact=False):
    """the restatement beside the engine's narrow host-scheduled block steps (the module docstring): -> Tracker"""
    pos, vel, m = bc.arrays_of(ic)
    d, _ = to_device(nb, ic)
    fc = _direct(nb, g, eps)
    blk = nb.BlockHermiteIntegrator()
    blk.setParameters(0.02, 0.01, L)
    blk.setTuning(1 << 30)  # always the narrow form: the sums of the resident forms
    blk.prime(d, fc, dt)
    st0 = blk.getState()
    a0 = np.stack([d.acc_x.cpu().numpy(), d.acc_y.cpu().numpy(), d.acc_z.cpu().numpy()], 1).astype(np.float64)
    fields = [getattr(d, k) for k in F[:9]]

    def advance(run, t, A):
        blk.block_step(d, fc, dt, 1)
        s = torch.stack(fields).cpu().numpy().astype(np.float64)  # x, v, a of every body after the step
        j1 = blk.getState()["jerk"][A, :3].astype(np.float64)
        run.correct(A, t, s[6:9, A].T, j1)
        # (the corrector's x is the engine's to the bit and its v within 6e-8, tests/test_hermite_block_gpu.py: taken
        # over, so that the predicted positions below are those of the engine's state and not of a drifting twin)
        run.x[A], run.v[A] = s[0:3, A].T, s[3:6, A].T

    tr, run = ec.restatement_run(pos, vel, m, g, eps, dt, L, macros, radii=radii, advance=advance, acc=a0,
                                 jerk=st0["jerk"][:, :3].astype(np.float64), levels=st0["levels"],
                                 until_contact=until_contact)
    end = blk.getState()
    assert np.array_equal(end["levels"], run.level) and not end["ticks"].any()  # both walked one schedule
    assert blk.info()["block_steps"] == run.block_steps == len(tr.samples) or len(m) < 2
    blk.close()
    return tr


def _check_closest(tag, ev, tr):
    """one system's record against the Tracker's closest approach, under the condition on the inputs"""
    d_ref, i, j, macro, tick = tr.closest
    bound = ec.d_bound(d_ref)
    d_eng = float(np.sqrt(np.float64(ev["closest_d2"])))
    print(f"{tag}: closest d {d_ref:.9e} (engine {d_eng:.9e}, |diff| {abs(d_eng - d_ref):.2e}, bound {bound:.2e}) pair "
          f"({i}, {j}) macro {macro} tick {tick}; runner-up further by {tr.runner_up - d_ref:.3e}; {len(tr.samples)} block "
          f"steps", flush=True)
    # the condition on the inputs: otherwise the identity of the pair and of the block step is not decidable
    assert tr.runner_up - d_ref > 2.0 * bound, (tag, tr.runner_up - d_ref, bound)
    assert (int(ev["closest_i"]), int(ev["closest_j"]), int(ev["closest_macro"]), int(ev["closest_tick"])) == (i, j, macro, tick)
    assert abs(d_eng - d_ref) <= bound, (tag, d_eng, d_ref, bound)


def _closest_case(nb, tag, ic, g, eps, dt, L, macros):
    n = ic["mass"].size
    d, ens, _ = _ensemble(nb, [ic], eps, dt=dt, max_level=L, g=g,
                          events=dict(radii=np.zeros(n, np.float32), track_closest=True))
    ens.advance(d, macros)
    ev = ens.events()[0]
    assert ev["stopped"] == 0 and ev["macro_steps_done"] == macros
    tr = _lockstep(nb, ic, g, eps, dt, L, macros)
    _check_closest(tag, ev, tr)
    return ev, tr


def test_closest_approach_binary_over_a_period(nb, ctx):
    """the e = 0.9 binary with a perturber (n = 3, max_level 10) over one full period: the pericentre passage falls
    between two call boundaries (macro steps of a fifteenth of the period)"""
    c = br.BINARY
    ic = bc.ic_of(*br.binary_case())
    ev, tr = _closest_case(nb, "binary", ic, 1.0, c["eps"], c["T"] / 15, 10, 15)  # (15 macro steps: pericentre inside one)
    assert 0.09 < tr.closest[0] < 0.11 and {tr.closest[1], tr.closest[2]} == {0, 1}  # a (1 - e) = 0.1
    assert 0 < ev["closest_tick"] < 2 ** 10 and ev["closest_macro"] == 7  # inside the eighth macro step: half the period


def test_closest_approach_plummer_16(nb, ctx):
    _closest_case(nb, "plummer 16", _plummer(nb, 16, seed=42), G, 0.05, DT, 10, 2)


@pytest.mark.parametrize("n,i,j", [(1025, 3, 1024), (600, 259, 515)], ids=["second-source-block", "source-slot"])
def test_closest_approach_index_arithmetic(nb, ctx, n, i, j):
    """the closest pair placed where the source index j = bx 1024 + s 256 + lane decides the answer: j = 1,024 is the only
    source of the second block; 259 and 515 are lane 3 of slots s = 1 and s = 2"""
    ic = ec.with_close_pair(_plummer(nb, n, seed=42), i, j, 2e-3)
    _, tr = _closest_case(nb, f"n {n} pair ({i}, {j})", ic, G, 0.05, DT, 6, 1)
    assert tr.closest[1:3] == (i, j)


# ---- 3. padding and self pairs -----------------------------------------------------------------------------------------
def test_padded_sources_never_enter(nb, ctx):
    """n = 5: the padded sources 5..1023 sit at the origin with m = 0; one body at 1e-3 from it, the others at >= 1"""
    pos = np.array([[1e-3, 0, 0], [1.5, 0, 0], [0, -1.25, 0], [0, 0, 2.0], [-1.0, -1.0, 1.0]], np.float32)
    vel = np.zeros((5, 3), np.float32)
    ic = bc.ic_of(pos, vel, np.full(5, 0.2, np.float32))
    ev, tr = _closest_case(nb, "n 5", ic, G, 0.05, DT, 8, 1)
    assert ev["closest_j"] < 5 and ev["closest_d2"] > 0.9  # (a padded source would have given d = 1e-3)


def test_one_body_and_a_coincident_pair(nb, ctx):
    one = bc.ic_of(np.zeros((1, 3), np.float32), np.zeros((1, 3), np.float32), np.ones(1, np.float32))
    p = np.array([[0.25, -0.5, 0.125]] * 2, np.float32)
    two = bc.ic_of(p, np.zeros((2, 3), np.float32), np.array([1.0, 2.0], np.float32))
    d, ens, _ = _ensemble(nb, [one, two], 0.05, events=dict(track_closest=True))
    ens.advance(d, 2)
    ev = ens.events()
    _none(ev[0], "closest")
    _none(ev[0], "contact")
    # two different bodies at one place at rest: d2 = 0 from both sides in the first block step; the key rule orders
    # (d2, i, j), so (0, 1) beats (1, 0); later block steps tie and strictly-less keeps the first
    assert ec.key(0.0, 0, 1) < ec.key(0.0, 1, 0)
    assert ev["closest_d2"][1] == 0.0 and (ev["closest_i"][1], ev["closest_j"][1]) == (0, 1)
    # (softened and coincident: a = j = 0, want = +inf, level 0 -- the first block step is the whole macro step)
    assert ev["closest_macro"][1] == 0 and ev["closest_tick"][1] == 2 ** 16


# ---- 4. stop on contact ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def head_on(nb):
    """the eight copies, and per copy the restatement's verdict beside the engine's block steps: (contact or None,
    samples); computed once"""
    c = ec.HEAD_ON
    t_cross = ec.head_on_crossing_time()
    radii, dts = ec.head_on_copies(t_cross)
    ic = bc.ic_of(*ec.head_on())
    verdict = []
    for s in range(8):
        tr = _lockstep(nb, ic, c["G"], c["eps"], float(dts[s]), c["max_level"], c["macros"],
                       radii=np.array([radii[s]] * 2, np.float32), until_contact=True)
        verdict.append((tr.contact, tr.samples))
    return ic, radii, dts, verdict


def _head_on_run(nb, ic, radii, dts, order, stop=True):
    c = ec.HEAD_ON
    r = np.repeat(radii[order], 2)
    return _ensemble(nb, [ic] * len(order), c["eps"], dt=dts[order], max_level=c["max_level"], g=c["G"],
                     events=dict(radii=r, track_closest=True, stop_on_contact=stop))


def test_stop_on_contact(nb, ctx, head_on):
    c = ec.HEAD_ON
    ic, radii, dts, verdict = head_on
    # the prediction, and the condition on it: inside the deciding macro step the separation crosses the threshold by a
    # factor of at least 2 either way (every earlier sample >= 2 rs, a sample of that macro step <= rs / 2)
    want_macro = []
    for s, (contact, samples) in enumerate(verdict):
        rs = float(np.float32(radii[s]) + np.float32(radii[s]))
        if s < 6:
            assert contact is not None and contact[3] == s, (s, contact)
            assert all(d >= 2.0 * rs for m, _, d in samples if m < s), s
            assert min(d for m, _, d in samples if m == s) <= 0.5 * rs, s
            want_macro.append(s)
        else:
            assert contact is None and (rs == 0.0 or all(d >= 2.0 * rs for _, _, d in samples)), s
            want_macro.append(None)
    order = np.arange(8)
    d, ens, off = _head_on_run(nb, ic, radii, dts, order)
    ens.advance(d, c["macros"])
    ev = ens.events()
    got = _whole(d, ens)
    print("stopped", ev["stopped"], "done", ev["macro_steps_done"], "contact tick", ev["contact_tick"])
    plain = {}
    for s in range(8):
        contact = verdict[s][0]
        done = c["macros"] if contact is None else contact[3] + 1
        assert ev["stopped"][s] == (0 if contact is None else 1) and ev["macro_steps_done"][s] == done, s
        if contact is None:
            _none(ev[s], "contact")
        else:
            assert (ev["contact_macro"][s], ev["contact_tick"][s]) == (contact[3], contact[4]), (s, contact)
            assert (ev["contact_i"][s], ev["contact_j"][s]) == (contact[1], contact[2])
            assert abs(np.sqrt(np.float64(ev["contact_d2"][s])) - contact[0]) <= ec.d_bound(contact[0])
        # the state: bitwise that of a plain ensemble advanced `done` macro steps
        if done not in plain:
            dp, ep, offp = _ensemble(nb, [ic] * 8, c["eps"], dt=dts, max_level=c["max_level"], g=c["G"])
            ep.advance(dp, done)
            plain[done] = (_whole(dp, ep), ep, offp)
        _assert_equal(("stopped at", done, s), _cut(got, ens, off, s), _cut(*plain[done], s))
    assert ens.running() == 2
    # the same eight in reversed order: the same record per system
    d2, ens2, _ = _head_on_run(nb, ic, radii, dts, order[::-1])
    ens2.advance(d2, c["macros"])
    ev2 = ens2.events()
    for s in range(8):
        _same_records(("reversed", s), ev[s], ev2[7 - s])
    # a further advance(4): stopped systems untouched in arrays and records, the two running ones move
    ens.advance(d, 4)
    ev4, got4 = ens.events(), _whole(d, ens)
    for s in range(8):
        if ev["stopped"][s]:
            _same_records(("untouched", s), ev[s], ev4[s])
            _assert_equal(("untouched", s), _cut(got4, ens, off, s), _cut(got, ens, off, s))
        else:
            assert ev4["stopped"][s] == 0 and ev4["macro_steps_done"][s] == c["macros"] + 4
            a, b = int(off[s]), int(off[s + 1])
            assert (got4["pos_x"][a:b] != got["pos_x"][a:b]).any()
    assert ens.info()["macro_steps"] == int(ev4["macro_steps_done"].sum())  # info(-1) sums what was done


# ---- 5. budgets --------------------------------------------------------------------------------------------------------
def test_budgets(nb, ctx):
    ics = [_plummer(nb, n, seed=300 + k) for k, n in enumerate([5, 16, 3, 7])]
    limits = [1, 2, 5, 0]
    d, ens, off = _ensemble(nb, ics, 0.05, events=dict(max_macro_steps=limits))
    ens.advance(d, 8)
    ev = ens.events()
    assert ev["stopped"].tolist() == [2, 2, 2, 0] and ev["macro_steps_done"].tolist() == [1, 2, 5, 8]
    assert ens.running() == 1
    got = _whole(d, ens)
    for s, done in enumerate([1, 2, 5, 8]):
        dp, ep, offp = _ensemble(nb, ics, 0.05)
        ep.advance(dp, done)
        _assert_equal(("budget", s), _cut(got, ens, off, s), _cut(_whole(dp, ep), ep, offp, s))
        _none(ev[s], "closest")  # (not tracked)
        _none(ev[s], "contact")
    assert ens.info()["macro_steps"] == 16


# ---- 6. launch structure -----------------------------------------------------------------------------------------------
def _structure_case(nb):
    ics = [_plummer(nb, n, seed=100 + k) for k, n in enumerate([257, 5])] + [bc.ic_of(*ec.head_on())]
    radii = np.concatenate([np.zeros(262, np.float32), np.array([0.49, 0.49], np.float32)])  # (the pair touches at 0.98)
    events = dict(radii=radii, max_macro_steps=[0, 3, 0], track_closest=True, stop_on_contact=True)
    return ics, events


def test_advance_4_equals_four_advances(nb, ctx):
    ics, events = _structure_case(nb)
    d, ens, _ = _ensemble(nb, ics, 0.05, events=events)
    ens.advance(d, 4)
    d2, ens2, _ = _ensemble(nb, ics, 0.05, events=events)
    for _ in range(4):
        ens2.advance(d2, 1)
    ev, ev2 = ens.events(), ens2.events()
    print("stopped", ev["stopped"], "done", ev["macro_steps_done"])
    _same_records("advance(4)", ev, ev2)
    _assert_equal("advance(4)", _whole(d, ens), _whole(d2, ens2))
    assert ev["stopped"][1] == 2 and ev["macro_steps_done"][1] == 3 and ev["stopped"][0] == 0
    assert ev["stopped"][2] == 1 and ev["macro_steps_done"][2] == ev["contact_macro"][2] + 1 < 4


def test_events_in_a_step_graph(nb, ctx):
    """the pattern of tests/test_hermite_batch_gpu.py::test_advance_in_a_step_graph: one eager advance(1), one more
    recorded and replayed three times, against four eager ones"""
    ics, events = _structure_case(nb)
    d, ens, _ = _ensemble(nb, ics, 0.05, events=events)
    ens.advance(d, 1)  # eagerly first
    with ctx.capture() as rec:
        ens.advance(d, 1)
    rec.graph.launch(3)
    d2, ens2, _ = _ensemble(nb, ics, 0.05, events=events)
    ens2.advance(d2, 4)
    _same_records("1 eager + 3 replayed", ens.events(), ens2.events())
    _assert_equal("1 eager + 3 replayed", _whole(d, ens), _whole(d2, ens2))
    rec.graph.close()
    # a configuration changed since the last eager advance: the recording is refused until one has run
    ens2.setEvents()
    with pytest.raises(nb.StateException, match="step graph"):
        with ctx.capture():
            ens2.advance(d2, 1)


def test_more_systems_than_compute_units(nb, ctx):
    """300 triples, a drawn third with radii that collide: every record equals that of the system run as a B = 1 ensemble"""
    c = bc.TRIPLE
    ics, radii, hit = ec.colliding_triples(c["systems"])
    assert len(ics) == 300 and 60 < hit.sum() < 140
    kw = dict(dt=c["dt_max"], max_level=c["max_level"], g=c["G"])
    d, ens, off = _ensemble(nb, ics, c["eps"], events=dict(radii=np.concatenate(radii), track_closest=True,
                                                           stop_on_contact=True), **kw)
    ens.advance(d, 4)
    ev = ens.events()
    print(f"{int(hit.sum())} systems with radii, {int((ev['stopped'] == 1).sum())} stopped, done "
          f"{sorted(set(ev['macro_steps_done'].tolist()))}")
    assert (ev["stopped"][~hit] == 0).all() and (ev["stopped"][hit] == 1).sum() >= hit.sum() // 2
    assert ens.running() == int((ev["stopped"] == 0).sum())
    pos = {k: getattr(d, k).cpu().numpy() for k in F[:6]}
    for s in range(300):
        d1, e1, _ = _ensemble(nb, [ics[s]], c["eps"], events=dict(radii=radii[s], track_closest=True, stop_on_contact=True),
                              **kw)
        e1.advance(d1, 4)
        _same_records(("triple", s), ev[s], e1.events()[0])
        a, b = int(off[s]), int(off[s + 1])
        for k in F[:6]:
            assert np.array_equal(pos[k][a:b].view(np.uint32), getattr(d1, k).cpu().numpy().view(np.uint32)), (s, k)
        e1.close()
    total = ens.info()
    assert total["macro_steps"] == int(ev["macro_steps_done"].sum()) < 1200


# ---- 7. resetting and refusals -----------------------------------------------------------------------------------------
def test_prime_clears_and_nothing_is_the_plain_path(nb, ctx):
    precision, eps = FORMS[0]
    ics, plain, infos = _plain3(nb, precision, eps)
    total = sum(SIZES)
    d, ens, off = _ensemble(nb, ics, eps, precision, events=dict(radii=np.full(total, 0.5, np.float32),
                                                               max_macro_steps=1, track_closest=True))
    ens.advance(d, 2)
    ev = ens.events()
    assert (ev["stopped"] == 2).all() and (ev["macro_steps_done"] == 1).all() and ens.running() == 0
    assert np.isfinite(ev["contact_d2"][[2, 4]]).all()  # (radii of 0.5 in Plummer spheres of 257 and 1,025: contacts)
    # prime clears records and stop words
    d2, _ = to_device(nb, nb.ic.concat(ics)[0])
    ens.prime(d2, _direct(nb, G, eps), DT)
    ev = ens.events()
    assert (ev["stopped"] == 0).all() and (ev["macro_steps_done"] == 0).all() and ens.running() == len(SIZES)
    for s in range(len(SIZES)):
        _none(ev[s], "closest")
        _none(ev[s], "contact")
    # setEvents() with nothing: the plain kernel, to the bits of the plain handle
    ens.setEvents()
    ens.advance(d2, 3)
    _assert_equal("back on the plain path", _whole(d2, ens), plain)
    ev = ens.events()
    assert (ev["macro_steps_done"] == 3).all() and (ev["stopped"] == 0).all()
    for s in range(len(SIZES)):
        _none(ev[s], "closest")


def test_refusals(nb, ctx):
    ics = [_plummer(nb, n, seed=300 + k) for k, n in enumerate([5, 16])]
    lib = nb._lib.load()
    e = nb.BlockHermiteEnsemble()
    with pytest.raises(nb.StateException, match="no layout"):  # a call before a layout
        e.setEvents(track_closest=True)
    with pytest.raises(nb.StateException, match="not primed"):
        e.events()
    e.setLayout([0, 5, 21])
    ok = np.full(21, 0.1, np.float32)
    for bad, what in ((-0.1, "body 7"), (float("nan"), "body 7"), (float("inf"), "body 7")):
        r = ok.copy()
        r[7] = bad
        with pytest.raises(nb.ValidationException, match=what):
            e.setEvents(radii=r)
    for r in (ok[:20], np.zeros((21, 1), np.float32), np.zeros(22, np.float32)):
        with pytest.raises(nb.ValidationException, match="one per body"):
            e.setEvents(radii=r)
    with pytest.raises(nb.ValidationException, match="array of 2 values"):
        e.setEvents(max_macro_steps=[1, 2, 3])
    with pytest.raises(nb.ValidationException, match="needs radii"):
        e.setEvents(stop_on_contact=True)
    # the C call: the same refusals with the library's wording, unknown flag bits, a handle without a layout, no handle
    h = C.c_void_p()
    nb._lib.check(lib.nbody_hip_hermite_batch_create(ctx.handle, 21, 2, C.byref(h)))
    try:
        assert lib.nbody_hip_hermite_batch_set_events(h, ok.ctypes.data, None, 1) == nb._lib.ERR_STATE
        assert b"no layout" in lib.nbody_hip_last_error()
        off = np.array([0, 5, 21], np.uint64)
        nb._lib.check(lib.nbody_hip_hermite_batch_set_layout(h, off.ctypes.data, 2))
        assert lib.nbody_hip_hermite_batch_set_events(h, ok.ctypes.data, None, 4) == nb._lib.ERR_VALIDATION
        assert b"unknown event flag bits 0x4" in lib.nbody_hip_last_error()
        assert lib.nbody_hip_hermite_batch_set_events(h, None, None, 2) == nb._lib.ERR_VALIDATION
        assert b"needs radii" in lib.nbody_hip_last_error()
        r = ok.copy()
        r[7] = -0.1
        assert lib.nbody_hip_hermite_batch_set_events(h, r.ctypes.data, None, 0) == nb._lib.ERR_VALIDATION
        assert b"body 7 (body 2 of system 1)" in lib.nbody_hip_last_error()
        r[7] = np.nan
        assert lib.nbody_hip_hermite_batch_set_events(h, r.ctypes.data, None, 0) == nb._lib.ERR_VALIDATION
        out = np.zeros(2, nb.api.BATCH_EVENT_DTYPE)
        n = C.c_size_t(9)
        assert lib.nbody_hip_hermite_batch_events(h, out.ctypes.data, 2) == nb._lib.ERR_STATE  # unprimed
        assert b"not primed" in lib.nbody_hip_last_error()
        assert lib.nbody_hip_hermite_batch_running(h, C.byref(n)) == nb._lib.ERR_STATE and n.value == 9
        nb._lib.check(lib.nbody_hip_hermite_batch_set_events(h, ok.ctypes.data, None, 3))
    finally:
        lib.nbody_hip_hermite_batch_destroy(h)
    assert lib.nbody_hip_hermite_batch_set_events(None, ok.ctypes.data, None, 0) == nb._lib.ERR_STATE
    assert b"null block-step Hermite ensemble" in lib.nbody_hip_last_error()
    # none of it left a mark: the ensemble configures, primes and runs; a new layout drops the configuration
    e.setEvents(radii=ok, max_macro_steps=[1, 0])
    d, _ = to_device(nb, nb.ic.concat(ics)[0])
    e.prime(d, _direct(nb, G, 0.05), DT)
    e.advance(d, 2)
    assert e.events()["stopped"].tolist() == [2, 0] and e.running() == 1
    with pytest.raises(nb.ValidationException, match="layout has 2 systems"):
        nb._lib.check(lib.nbody_hip_hermite_batch_events(e._h, np.zeros(3, nb.api.BATCH_EVENT_DTYPE).ctypes.data, 3))
    e.setLayout([0, 5, 21])
    assert e._events is None
    e.prime(d, _direct(nb, G, 0.05), DT)
    e.advance(d, 2)
    assert e.events()["stopped"].tolist() == [0, 0] and e.events()["macro_steps_done"].tolist() == [2, 2]


# ---- 8. both hosts -----------------------------------------------------------------------------------------------------
def test_facade_program(nb, ctx):
    exe = os.path.join(ROOT, "n-body_amd", "lib", "hermite_batch_events_tests")
    assert os.path.exists(exe), "build with __graft_entry__.build()"
    env = dict(os.environ)
    env["LD_LIBRARY_PATH"] = os.path.dirname(exe) + os.pathsep + env.get("LD_LIBRARY_PATH", "")
    r = subprocess.run([exe], cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    print(r.stdout)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    theirs = re.findall(r"^(hermite_batch_events .*)$", r.stdout, re.M)
    assert len(theirs) == 4
    # the same ensemble through the Python host
    n = 300
    hst = nb.ParticleData()
    nb.ParticleDataManager.allocateHost(hst, n)
    nb.ParticleInitializer.initUniform(hst, nb.UniformDistParams((-1, -1, -1), (1, 1, 1), 0.5, 1.5), 7)
    hst.vel_x[:] = np.float32(0.1) * hst.pos_y
    hst.vel_y[:] = np.float32(-0.1) * hst.pos_x
    d = nb.ParticleData()
    nb.ParticleDataManager.allocateDevice(d, n)
    nb.ParticleDataManager.copyToDevice(d, hst)
    ens = nb.BlockHermiteEnsemble()
    ens.setLayout([0, 3, 260, 300])
    ens.setEvents(radii=np.full(n, np.float32(0.04)), max_macro_steps=[0, 0, 2], track_closest=True, stop_on_contact=True)
    ens.prime(d, _direct(nb, float(np.float32(1.7)), float(np.float32(0.05))), 1.0 / 64)
    ens.advance(d, 4)
    ev = ens.events()
    ours = []
    for s in range(3):
        e = ev[s]
        ours.append("hermite_batch_events %d stopped %d done %d closest %08x %d %d %d %d contact %08x %d %d %d %d" % (
            s, e["stopped"], e["macro_steps_done"], e["closest_d2"].view(np.uint32), e["closest_i"], e["closest_j"],
            e["closest_macro"], e["closest_tick"], e["contact_d2"].view(np.uint32), e["contact_i"], e["contact_j"],
            e["contact_macro"], e["contact_tick"]))
    ours.append("hermite_batch_events running %d" % ens.running())
    assert theirs == ours

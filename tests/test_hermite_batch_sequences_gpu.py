"""The host state machine of the ensemble integrator on a live handle: ONE reused ensemble goes
through a sequence of configurations -- events on, outcomes on, hierarchies on, events off, outcomes off, hierarchies off,
a new layout, events with radii and stop_on_contact plus mergers with a pass after every advance, mergers off -- and after
every step everything it holds equals, bit for bit, a FRESH ensemble given only the configuration in force and primed the
same way: the state, events(), the outcome records, the hierarchy records and node tables, the merger state, log and ids,
info().  What the reused handle carries over and the fresh one does not: every feature's device memory once it has been
allocated (cleared by the priming whether the feature is on or not, against the host's "none" records of a handle that
never had it), the records of the steps before, the live counts of merged systems, flags and kappa of a feature turned off.

Between two steps the bodies go back to their initial state, the handle is invalidated and primed again, and two macro
steps run as two launches.  After each change of a feature's on-bit the recording rule is asserted on the reused handle
(primed, and run eagerly in the step before): a recording of the advance is refused until one eager advance has run, and
is taken after it.  The mergers' own word likewise for the pass; turning the mergers off does not touch the advance's.

Systems of 2, 3, 5, 257 and 513 bodies: the smallest that give two source tiles (257) and two target blocks (513) of the
priming sweep, and systems under the hierarchies' limit of 64; the new layout is the same systems in reverse order.  Every
system has one light pair 0.01 apart (tests/hermite_batch_mergers_ref.py), so that with radii every system merges."""
import numpy as np
import pytest

import hermite_batch_mergers_ref as mref
from gpu_util import to_device

pytestmark = pytest.mark.gpu
F = ("pos_x", "pos_y", "pos_z", "vel_x", "vel_y", "vel_z", "acc_x", "acc_y", "acc_z", "acc_old_x", "acc_old_y", "acc_old_z",
     "mass")
G, DT, L = 1.7, 1.0 / 64, 10
SYSTEMS = [(2, (0, 1)), (3, (0, 2)), (5, (1, 3)), (257, (3, 255)), (513, (3, 511))]
ADVANCE_REFUSED = "a block-step Hermite ensemble advance cannot be recorded into a step graph before it has run once eagerly"
PASS_REFUSED = "a merger pass cannot be recorded into a step graph before it has run once eagerly since the priming"
OFF = dict(events=None, outcomes=None, hierarchy=None, mergers=False)


class Layout:
    """the bodies, the offsets and ONE object per setting of a feature (a configuration is compared by identity)"""

    def __init__(self, nb, systems):
        self.ic, self.offsets = nb.ic.concat([mref.case_ic(nb, n, pair) for n, pair in systems])
        radii = np.concatenate([mref.case_radii(n, pair) for n, pair in systems]).astype(np.float32)
        self.track = dict(track_closest=True, max_macro_steps=[0, 1, 0, 0, 5])
        self.contact = dict(radii=radii, stop_on_contact=True)
        self.outcomes = dict(escape_radius=np.full(len(systems), 3.0, np.float32), stop_on_escape=True)
        self.hierarchy = dict(separation_radius=np.array([1.0 if n <= 64 else 0.0 for n, _ in systems], np.float32),
                              isolation=1.5, stop_on_resolved=True)

    def cfg(self, events=None, outcomes=False, hierarchy=False, mergers=False):
        return dict(events=events, outcomes=self.outcomes if outcomes else None,
                    hierarchy=self.hierarchy if hierarchy else None, mergers=mergers)


class Handle:
    """an ensemble with its three companions, its own bodies on the device, and the configuration it was given"""

    def __init__(self, nb, fc, precision):
        self.nb, self.fc = nb, fc
        self.ens = nb.BlockHermiteEnsemble()
        self.ens.setParameters(0.02, 0.01, L)
        self.ens.setStatePrecision(precision)
        self.out, self.hier, self.mg = nb.EnsembleOutcomes(self.ens), nb.EnsembleHierarchy(self.ens), nb.EnsembleMergers(self.ens)
        self.cfg = dict(OFF)

    def layout(self, lay):
        self.lay = lay
        self.d, self.h = to_device(self.nb, lay.ic)
        self.ens.setLayout(lay.offsets)
        self.cfg = dict(OFF)

    def configure(self, cfg):
        """only what differs from the configuration in force is sent (the events: always, where they are on -- a pass
        changes the radii on the device)"""
        for key, send in (("events", lambda v: self.ens.setEvents(**(v or {}))), ("outcomes", lambda v: self.out.set(**(v or {}))),
                          ("hierarchy", lambda v: self.hier.set(**(v or {}))), ("mergers", lambda v: self.mg.set(bool(v)))):
            if cfg[key] is not self.cfg[key] or (key == "events" and cfg[key]):
                send(cfg[key])
        self.cfg = dict(cfg)

    def prime(self):
        self.nb.ParticleDataManager.copyToDevice(self.d, self.h)  # the bodies as they were
        self.ens.invalidate()                                     # (extended: the residuals back to 0)
        self.ens.prime(self.d, self.fc, DT)

    def macro_step(self):
        self.ens.advance(self.d, 1)
        if self.cfg["mergers"]:
            self.mg.apply(self.d)

    def everything(self):
        d, ens = self.d, self.ens
        out = {k: getattr(d, k).cpu().numpy().view(np.uint32).copy() for k in F}
        st = ens.getState()
        out.update(jerk=st["jerk"].view(np.uint32).copy(), levels=st["levels"].copy(), ticks=st["ticks"].copy(),
                   want=st["want"].view(np.uint32).copy())
        x, v = ens.getExtendedState(d)
        out.update(X=x.view(np.uint64).copy(), V=v.view(np.uint64).copy(), events=ens.events(), outcomes=self.out.records(),
                   hierarchy=self.hier.records(), nodes=self.hier.nodes())
        out["mstate"], out["mlog"], out["ids"] = self.mg._get(True, True)
        info = [ens.info(s) for s in range(len(SYSTEMS))] + [ens.info()]
        return out, info


def _refused(nb, ctx, call, message):
    with pytest.raises(nb.StateException, match=message):
        with ctx.capture():
            call()


def _recorded(ctx, call):
    with ctx.capture() as rec:
        call()
    rec.graph.close()  # (never launched: the sequence goes on eagerly)


def _same(label, got, want):
    (a, ia), (b, ib) = got, want
    assert a.keys() == b.keys(), label
    for k in b:
        assert a[k].dtype == b[k].dtype and a[k].shape == b[k].shape and a[k].tobytes() == b[k].tobytes(), (label, k)
    assert ia == ib, label


@pytest.mark.parametrize("precision, eps", [("fp32", 0.05), ("extended", 0.0)], ids=["fp32-packed", "extended-guard"])
def test_reused_ensemble_equals_fresh_ensembles(nb, ctx, precision, eps):
    fc = nb.DirectForceCalculator()
    fc.setGravitationalConstant(G)
    fc.setSofteningParameter(eps)
    A, B = Layout(nb, SYSTEMS), Layout(nb, SYSTEMS[::-1])
    # label, the layout, the configuration in force after the step, what of the recording rule is asserted
    steps = [("1 events on", A, A.cfg(A.track), "advance"),
             ("2 outcomes on", A, A.cfg(A.track, outcomes=True), "advance"),
             ("3 hierarchies on", A, A.cfg(A.track, outcomes=True, hierarchy=True), "advance"),
             ("4 events off", A, A.cfg(outcomes=True, hierarchy=True), "advance"),
             ("5 outcomes off", A, A.cfg(hierarchy=True), "advance"),
             ("6 hierarchies off", A, A.cfg(), "advance"),
             ("7 a new layout", B, B.cfg(), None),
             ("8 events with radii and stop_on_contact, mergers on", B, B.cfg(B.contact, mergers=True), "advance and pass"),
             ("9 mergers off", B, B.cfg(B.contact), "mergers off")]
    one = Handle(nb, fc, precision)
    one.layout(A)
    one.prime()
    one.macro_step()  # (primed, and run eagerly: what every step finds)
    merged = 0
    for label, lay, want, rule in steps:
        if lay is not one.lay:
            one.out.set(escape_radius=3.0)  # (a configuration for the new layout to drop)
            one.layout(lay)
        one.configure(want)
        if rule == "mergers off":
            _recorded(ctx, lambda: one.ens.advance(one.d, 1))  # (the advance's word is not the mergers' to clear)
        elif rule:
            _refused(nb, ctx, lambda: one.ens.advance(one.d, 1), ADVANCE_REFUSED)
        one.prime()
        if rule == "advance and pass":
            _refused(nb, ctx, lambda: one.mg.apply(one.d), PASS_REFUSED)
        one.macro_step()
        if rule:
            _recorded(ctx, lambda: one.ens.advance(one.d, 1))
        if rule == "advance and pass":
            _recorded(ctx, lambda: one.mg.apply(one.d))
        one.macro_step()
        fresh = Handle(nb, fc, precision)
        fresh.layout(lay)
        fresh.configure(want)
        fresh.prime()
        fresh.macro_step()
        fresh.macro_step()
        got = one.everything()
        _same(label, got, fresh.everything())
        fresh.ens.close()
        if want["mergers"]:
            merged = int(got[0]["mstate"]["n_mergers"].sum())
    assert merged == len(SYSTEMS)  # every system of step 8 met its contact and merged: the pass did run
    one.ens.close()

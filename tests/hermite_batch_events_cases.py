"""What the ensemble-event tests (tests/test_hermite_batch_events_*.py) share: the key rule restated in numpy, the folds of
the closest approach and of the first contact over the block steps of the restatement (tests/hermite_block_ref.py), the
error bound of a recorded separation and the systems of the cases.  numpy only; the GPU tests drive `Tracker` with the
engine's own block steps, the CPU tests with the restatement alone."""
import numpy as np

import hermite_batch_cases as bc
import hermite_block_ref as br
import hermite_ref as hr

U = hr.U  # 2^-24
NONE = 0xFFFFFFFF
# The absolute per-coordinate tolerance tests/test_hermite_block_gpu.py grants the engine's state against the restatement
# after a block step at O(1) coordinates (`assert dv <= 6e-8`, positions equal in their bits): half an fp32 ulp at 1.
DELTA = 6e-8


def d_bound(d, delta=DELTA):
    """|d_engine - d_ref| <= 2 sqrt(3) delta + 4 u d: two positions off by delta in three coordinates, and the fp32
    evaluation of d2 = fma(dx, dx, fma(dy, dy, dz dz)) from fp32 differences"""
    return 2.0 * np.sqrt(3.0) * delta + 4.0 * U * d


def key(d2, i, j):
    """bits(d2) << 32 | i << 12 | j as a Python int (d2: one fp32 value >= 0)"""
    return (int(np.float32(d2).view(np.uint32)) << 32) | (int(i) << 12) | int(j)


def unkey(k):
    return np.uint32(k >> 32).view(np.float32), (k >> 12) & 0xFFFFF, k & 0xFFF


def fold_closest(record, step_key, macro, tick):
    """record: None or (key, macro, tick).  STRICTLY less: the earliest block step keeps a tie."""
    if step_key is not None and (record is None or step_key < record[0]):
        return (step_key, macro, tick)
    return record


def fold_contact(record, step_key, macro, tick):
    """the first block step with a contact, once"""
    if record is None and step_key is not None:
        return (step_key, macro, tick)
    return record


class Tracker:
    """The events of ONE system in fp64 from the restatement's predicted positions: call step(macro, t, A, xp) for every
    block step in order.  closest / contact: (d, i, j, macro, tick) or None, ties by (d, i, j) and strictly-less in time;
    runner_up: the smallest d of any other candidate of the closest approach -- another block step's minimum, or another
    pair of the same block step (the mirror (j, i) of the pair, which has the same d to the bit and loses by the key
    rule, is no rival); samples: (macro, tick, smallest d of the block step)."""

    def __init__(self, n, radii=None):
        self.n = n
        self.r = None if radii is None else np.asarray(radii, np.float32)
        self.closest = self.contact = None
        self.rivals = []
        self.samples = []

    def step(self, macro, t, A, xp):
        if self.n < 2:
            return
        A = np.asarray(A)
        dv = xp[None, :, :] - xp[A, None, :]
        d = np.sqrt((dv * dv).sum(-1))  # [|A|, n]
        d[np.arange(len(A)), A] = np.inf  # j != i
        bd, bi, bj = self._smallest(d, A)
        self.samples.append((macro, t, bd))
        others = d.copy()
        others[np.flatnonzero(A == bi)[0], bj] = np.inf
        mirror = np.flatnonzero(A == bj)
        if mirror.size:
            others[mirror[0], bi] = np.inf
        self.rivals.append(float(others.min()))
        if self.closest is None or (bd, bi, bj) < self.closest[:3]:
            if self.closest is not None:
                self.rivals.append(self.closest[0])
            self.closest = (bd, bi, bj, macro, t)
        else:
            self.rivals.append(bd)
        if self.r is not None and self.contact is None:
            rs = (self.r[A][:, None] + self.r[None, :]).astype(np.float32).astype(np.float64)
            hit = (rs > 0) & (d < rs)
            if hit.any():
                self.contact = self._smallest(np.where(hit, d, np.inf), A) + (macro, t)

    @staticmethod
    def _smallest(d, A):
        """the smallest entry of d [|A|, n] by (d, i, j): -> (d, i, j)"""
        rows, cols = np.nonzero(d == d.min())
        i = A[rows]
        pick = np.lexsort((cols, i))[0]
        return float(d[rows[pick], cols[pick]]), int(i[pick]), int(cols[pick])

    @property
    def runner_up(self):
        return min(self.rivals) if self.rivals else np.inf


def restatement_run(pos, vel, m, G, eps, dt_max, max_level, macros, radii=None, advance=None, acc=None, jerk=None,
                    levels=None, until_contact=False):
    """`macros` macro steps of the restatement, every block step shown to a Tracker: -> (Tracker, BlockHermite).
    advance(run, t, A): replaces the restatement's own force evaluation and corrector -- the GPU tests take the engine's
    block step there, seeded with its primed acc, jerk and levels, as tests/test_hermite_block_gpu.py does.
    until_contact: the run ends with the macro step that holds the first contact."""
    run = br.BlockHermite(pos, vel, m, G, eps, dt_max, max_level=max_level, acc=acc, jerk=jerk, levels=levels)
    tr = Tracker(len(m), radii)
    guard = 0
    while run.macro_steps < macros and not (until_contact and tr.contact and run.macro_steps > tr.contact[3]):
        macro = run.macro_steps
        t, A = run.schedule()
        xp, _ = run.predicted(t)
        tr.step(macro, t, A, xp)
        if advance is None:
            run.step()
        else:
            advance(run, t, A)
        guard += 1
        assert guard <= macros * (2 ** max_level + 1)
    return tr, run


# ---- the systems of the cases ------------------------------------------------------------------------------------------
def with_close_pair(ic, i, j, sep, at=(0.31, -0.22, 0.17)):
    """bodies i and j of `ic` moved to `at` -/+ sep / 2 along x, at rest relative to each other: the closest pair of the
    system by construction (the caller asserts it on the restatement)"""
    ic = {k: v.copy() for k, v in ic.items()}
    for k, c in zip(("pos_x", "pos_y", "pos_z"), at):
        ic[k][i] = ic[k][j] = np.float32(c)
    ic["pos_x"][i] = np.float32(at[0] - 0.5 * sep)
    ic["pos_x"][j] = np.float32(at[0] + 0.5 * sep)
    for k in ("vel_x", "vel_y", "vel_z"):
        ic[k][i] = ic[k][j] = np.float32(0.0)
    return ic


# Head-on: two bodies of mass 1/2 at x = -/+ 1/2 approaching at -/+ 1/4 (at rest j = 0 and the priming would put both on
# level 0: one block step of dt_max), G = 1, eps = 0.05: they fall through each other at T_CROSS.
# One trajectory cannot cross six thresholds by a factor of four (two either way) in six EQUAL macro steps -- its
# separation would have to fall geometrically -- so the eight copies differ in their radius AND in dt_max, which is per
# system: copy s < 6 has dt_max = T_CROSS / (s + 1/2), so the bodies cross in its macro step s (0-based); copy 6 has
# radius 0 and copy 7 a dt_max so short that eight macro steps end long before the threshold.
HEAD_ON = dict(G=1.0, eps=0.05, max_level=12, macros=8)


def head_on():
    pos = np.array([[-0.5, 0.0, 0.0], [0.5, 0.0, 0.0]], np.float32)
    vel = np.array([[0.25, 0.0, 0.0], [-0.25, 0.0, 0.0]], np.float32)
    return pos, vel, np.array([0.5, 0.5], np.float32)


def head_on_crossing_time():
    """the time at which the separation first falls below 0.01, by the restatement with fine shared-length macro steps"""
    c = HEAD_ON
    pos, vel, m = head_on()
    dt = 1.0 / 64
    run = br.BlockHermite(pos, vel, m, c["G"], c["eps"], dt, max_level=c["max_level"])
    for _ in range(100000):
        t, A = run.schedule()
        xp, _ = run.predicted(t)
        if np.linalg.norm(xp[1] - xp[0]) < 0.01:
            return run.macro_steps * dt + t * dt / 2 ** c["max_level"]
        run.step()
    raise AssertionError("no crossing")


def head_on_copies(t_cross):
    """-> (radius per copy [8], dt_max per copy [8])"""
    radii = np.array([0.020 + 0.002 * s for s in range(6)] + [0.0, 0.020], np.float32)
    dts = np.array([t_cross / (s + 0.5) for s in range(6)] + [t_cross / 10.0, t_cross / 40.0], np.float32)
    return radii, dts


def colliding_triples(count, seed=77, fraction=1.0 / 3.0):
    """bc.triples(count) and radii per body: a drawn `fraction` of the systems get stars of radius 0.949, whose sum 1.898
    is just under the binary's apocentre separation 1.9 -- they touch within the first macro steps; the others have none"""
    ics = bc.triples(count)
    rng = np.random.default_rng(seed)
    hit = rng.random(count) < fraction
    radii = [np.array([0.949, 0.949, 0.0], np.float32) if h else np.zeros(3, np.float32) for h in hit]
    return ics, radii, hit

"""The host state machine of the spatial hash on a live handle (tests/grid_sequence.py): ONE reused grid goes through
builds at scale 1 / 1.6 / 1 / 4 / 1 of the same bodies (start array by position, by the two-level search in a regrown
array with other key bits, by position again over dirty scratch counters and a wrong speculation, no start array at
all), ten calls in a row of the automatic form and of the wave-per-cell form (which makes its work list for the
statistics and then takes it), every tuning at eps 0.05 / 0 and cutoff 1 / 1.7, the potential, the field over a growing
point workspace, a slab with the two-grid and layer entries on a backend's reused handle, and a cell size set WITHOUT a
build -- and after every step its result equals, bit for bit, that of a fresh grid given only the settings in force,
whatever the reused handle carried over (capacities, counters, hint words, key bits, a pending cell size).

4,096 bodies in a box of half-width 8 at cell 1 plus 300 in one cell: the smallest set that is below two cells per body at
scale 1, between two and sixteen at 1.6, beyond at 4, and has a cell of more than 64 bodies.  The regimes are asserted
from what the grid reports, not trusted."""
import numpy as np
import pytest

import grid_sequence as gs

pytestmark = pytest.mark.gpu


def same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


@pytest.fixture(scope="module")
def run(nb, ctx):
    """every record of the sequence beside the fresh grid's answer (computed once per distinct question)"""
    data = gs.prepare(nb)
    cache, rows = {}, []
    for label, s, kind, args, got in gs.sequence(nb, ctx, data):
        key = (kind, args) + tuple(sorted(s.items()))
        if key not in cache:
            cache[key] = gs.fresh(nb, ctx, data, s, kind, args)
        rows.append((label, s, kind, args, got, cache[key]))
    return rows


def test_reused_grid_equals_fresh_grids(run):
    for label, s, kind, args, got, want in run:
        assert set(got) == set(want), label
        for name, a in got.items():
            assert same(a, want[name]), f"{label}: {name} differs from a fresh grid with {s} {args}"
        if kind == "forces":
            assert np.isfinite(got["acc"]).all(), label
    kinds = [r[2] for r in run]
    # 6 builds x (cells, start array, forces) + 20 calls in a row + 9 tunings x 2 x 2 + 6 before and 6 after setCellSize
    assert kinds.count("cells") == 6 and kinds.count("start") == 6 and kinds.count("slab") == 2
    assert kinds.count("forces") == 6 + 20 + 36 + 4 and kinds.count("potential") == 3 + 4 and kinds.count("field") == 3 + 4


def test_every_regime_of_the_start_array_was_reached(run):
    n = gs.N + gs.CROWD
    by = {label: got for label, _, _, _, got, _ in run}
    regime = {}
    for label, got in by.items():
        if label.endswith(": cells"):
            start = by[label[:-len("cells")] + "start array"]
            total = int(got["total"])
            assert total == int(np.prod(got["dims"]))
            regime[label[0:2].strip()] = (total, int(start["has"]))
            if int(start["has"]):
                assert int(start["base"]) == 0 and int(start["count"]) == total and start["lb"].size == total + 1
                assert start["lb"][0] == 0 and start["lb"][-1] == n and (np.diff(start["lb"]) >= 0).all()
    t1, t2, t3, t4, t5, t11 = (regime[k] for k in ("1", "2", "3", "4", "5", "11"))
    assert t1[1] and t1[0] <= 2 * n                                   # by position
    assert t2[1] and 2 * n < t2[0] <= 16 * n + 4096                   # two-level search ...
    assert t2[0] + 1 > (t1[0] + 1) + (t1[0] + 1) // 2                 # ... in an array that had to grow
    assert t3 == t1 and t5 == t1
    assert not t4[1] and t4[0] > 16 * n + 4096                        # no start array
    bits = [int(t[0] - 1).bit_length() for t in (t1, t2, t4)]
    assert len(set(bits)) == 3, bits                                  # every rebuild speculated on other key bits
    assert t11[1] and t11[0] < t1[0]                                  # the build after setCellSize(2.0) gave the coarser grid
    # a cell of more than 64 bodies: what makes the second call of a kind take the work list
    lb = by["5 scale 1 once more: start array"]["lb"]
    assert np.diff(lb).max() > 64


def test_calls_in_a_row_do_not_move_a_bit(run):
    for form in ("automatic", "tuning 3"):
        accs = [got["acc"] for label, _, _, _, got, _ in run if label.startswith(f"6 {form}, call")]
        assert len(accs) == 10
        for k, a in enumerate(accs):
            assert same(a, accs[0]), f"{form}: call {k + 1} differs from call 1"


def test_a_pending_cell_size_does_not_reach_the_grid_as_built(run):
    """setCellSize(2.0) without a build, cutoff 1.5: between the built cell 1 and the pending 2.  Tuning 1 is the cell-run
    kernel, whose STRICT instantiation (cutoff > cell: only x-adjacent cells interact) is a different pair set."""
    by = {label: (s, got) for label, s, _, _, got, _ in run}
    checked = 0
    for label, (s, got) in by.items():
        if not label.startswith("10 after setCellSize without a build"):
            continue
        before = by[label.replace("after setCellSize without a build", "before setCellSize")][1]
        assert s["cell"] == 1.0
        for name, a in got.items():
            assert same(a, before[name]), f"{label}: {name} moved"
        checked += 1
    assert checked == 6
    assert by["11 build at cell 2: cells"][0]["cell"] == 2.0

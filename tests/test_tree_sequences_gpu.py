"""The host state machine of the Barnes-Hut tree on a live handle (tests/tree_sequence.py): one reused tree goes through
build / walk / walk / build beside the queued schedule / walk / range walks / whole walk / counting / form 3 / form 1 /
depth 10 / depth 20 at order 2 with the potential / the order-changed error / build / walk, and after every step its
result equals, bit for bit, that of a fresh tree given only the settings in force -- whatever the reused handle carried
over (recorded costs, a pending schedule, aligned ids, reshaped node arrays, moments).

131,072 bodies = 2,048 waves is the smallest size at which every branch exists (the pair walk, its cost-ordered schedule,
the schedule queued beside the build); 6,000 bodies take the other side of each: replicas, plain ids, and the refusal of
the pair walk asked for after a build with plain ids."""
import numpy as np
import pytest

import tree_sequence as ts
from gpu_util import to_device

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("n", [131072, 6000])
def test_reused_tree_equals_fresh_trees(nb, ctx, n):
    ic = nb.ic.two_galaxies(n, seed=31)
    d, _ = to_device(nb, ic)
    cache, kinds, visits = {}, [], {}
    for label, s, kind, got in ts.sequence(nb, ctx, d, n):
        kinds.append(kind)
        if kind == "error":
            continue
        if kind == "visits":
            visits[s["form"]] = int(got["visits"])
            continue
        key = (kind,) + tuple(sorted(s.items()))
        if key not in cache:
            cache[key] = ts.fresh(nb, ctx, d, n, s, kind)
        want = cache[key]
        for name, a in got.items():
            assert np.isfinite(a).all(), (label, name)
            assert np.array_equal(a, want[name]), f"{label}: {name} differs from a fresh tree with {s}"
    # every step ran: 9 walks + 3 counted ones, the range walks, the potential, the refused walk(s)
    small = n < ts.PAIR_FROM
    assert kinds.count("walk") == 12 and kinds.count("ranges") == 1 and kinds.count("potential") == 1
    assert kinds.count("error") == (2 if small else 1)
    # the three forms visit the same nodes
    assert set(visits) == {0, 3, 1} and visits[0] > 0
    assert visits[3] == visits[0] and visits[1] == visits[0], visits

"""tests/grid_ref.py checked without a GPU: the crafted grids get exactly the keys they were written for (by the oracle),
every case sits in the builder regime it was written for, and the references of the start array, the layer export and
the work list agree with an independent count (bincount + cumsum, a plain loop) and with hand-counted examples."""
import numpy as np
import pytest

import grid_ref as gr
import sort_ref as sr


def crafted_cases():
    out = {}
    for name, (h, _) in gr.line_cases().items():
        out["line " + name] = ((h.size, 1, 1), h, False)
    out["line many runs"] = ((199000, 1, 1), gr.hist_many_runs(), False)
    out["line no array"] = ((gr.hist_no_array().size, 1, 1), gr.hist_no_array(), gr.NO_ARRAY_JITTER)
    for dims in gr.SLAB_GRIDS:
        for slab in gr.slabs_of(dims[2]):
            for outside in (False, True):
                if gr.covered(dims, slab) is None and not outside:
                    continue
                out[f"slab {dims} {slab} outside {outside}"] = (dims, gr.hist_slab(dims, slab, outside, 7), False)
    out["layer 363 x 363 x 2"] = ((363, 363, 2), np.bincount(np.random.default_rng(3).integers(0, 363 * 363 * 2, 20000),
                                                              minlength=363 * 363 * 2), False)
    for chunk, min_cnt, _ in gr.UNIT_SETTINGS:
        out[f"units 2049 chunk {chunk} min {min_cnt}"] = ((2049, 1, 1), gr.hist_units(2049, chunk, min_cnt, 1), False)
        out[f"units (5, 3, 9) chunk {chunk} min {min_cnt}"] = ((5, 3, 9), gr.hist_units(135, chunk, min_cnt, 2), False)
    return out


CASES = crafted_cases()


@pytest.mark.parametrize("name", sorted(CASES))
def test_crafted_grids_get_the_intended_keys(oracle, name):
    dims, hist, jitter = CASES[name]
    c = gr.Crafted(dims, hist, seed=5, jitter=jitter)
    odims, okeys = c.oracle_keys(oracle)
    assert odims == c.dims, f"the oracle's grid {odims} against {c.dims}"
    assert np.array_equal(okeys, c.keys)
    assert np.array_equal(np.bincount(c.keys, minlength=c.total), hist)
    assert np.unique(c.ic["mass"]).size == c.n
    # the start array against an independent count
    cov = gr.covered(c.dims)
    lb = gr.start_array(c.sorted_keys, cov)
    assert lb.dtype == np.int32 and lb.size == c.total + 1
    assert np.array_equal(lb, np.concatenate([[0], np.cumsum(hist)]))


@pytest.mark.parametrize("name", sorted(gr.line_cases()))
def test_line_cases_sit_in_their_regime(name):
    h, want = gr.line_cases()[name]
    n, cov = int(h.sum()), (0, h.size)
    assert gr.builder(n, cov) == want
    assert gr.builder(n, cov, "cell") == ("cell" if want == "position" else want)


def test_regimes_at_the_thresholds():
    assert gr.builder(500, (0, 1000)) == "position" and gr.builder(500, (0, 1001)) == "two-level"
    assert gr.builder(100, (0, 5696)) == "two-level" and gr.builder(100, (0, 5697)) is None
    assert gr.builder(100, None) is None and not gr.has_array(100, (0, 0))
    h = gr.hist_no_array()
    assert gr.builder(int(h.sum()), (0, h.size)) is None and h.sum() == 100
    h = gr.hist_many_runs()
    c = gr.Crafted((h.size, 1, 1), h)
    assert gr.builder(c.n, (0, h.size)) == "position"
    assert gr.long_runs(c.sorted_keys, (0, h.size)) == 3015 > 512 * 4
    # the run lengths around kGapInline: 63 empty cells and the occupied one behind them are filled inline, 64 empty cells
    # make a list entry (RUNS holds five such lengths); at the edges the same, for the threads k == 0 and k == n
    for e, want in ((0, 5), (62, 5), (63, 5), (64, 7), (129, 7)):
        c = gr.Crafted((gr.hist_runs(e, 64).size, 1, 1), gr.hist_runs(e, 64))
        assert gr.long_runs(c.sorted_keys, gr.covered(c.dims)) == want, e


def test_start_array_of_two_hand_counted_grids():
    # cells 0..6 hold 2, 0, 0, 1, 0, 3, 0 bodies
    sk = np.array([0, 0, 3, 5, 5, 5])
    assert gr.start_array(sk, (0, 7)).tolist() == [0, 2, 2, 2, 3, 3, 6, 6]
    # (2, 2, 3): layers of 4 cells holding (1, 0, 2, 0 | 0, 0, 0, 1 | 3, 0, 0, 0); the slab of layer 1 alone, bodies outside it
    sk = np.array([0, 2, 2, 7, 8, 8, 8])
    assert gr.covered((2, 2, 3), (1, 1)) == (4, 4)
    assert gr.start_array(sk, (4, 4)).tolist() == [3, 3, 3, 3, 4]
    assert gr.start_array(sk, (0, 12)).tolist() == [0, 1, 1, 3, 3, 3, 3, 3, 4, 7, 7, 7, 7]


def test_slab_clipping():
    dims = (5, 3, 9)
    assert gr.covered(dims) == gr.covered(dims, (0, 0)) == (0, 135)
    assert gr.covered(dims, (0, 1)) == (0, 15) and gr.covered(dims, (2, 3)) == (30, 45)
    assert gr.covered(dims, (8, 1)) == (120, 15) and gr.covered(dims, (7, 5)) == (105, 30)
    assert gr.covered(dims, (-1, 3)) == (0, 30) and gr.covered(dims, (9, 2)) is None
    for d in gr.SLAB_GRIDS:
        for slab in gr.slabs_of(d[2]):
            for outside in (False, True):
                cov = gr.covered(d, slab)
                if cov is None and not outside:
                    continue
                h = gr.hist_slab(d, slab, outside, 7)
                c = gr.Crafted(d, h)
                if cov is None:
                    continue
                assert gr.builder(c.n, cov) == "position"
                below, above = h[:cov[0]].sum(), h[cov[0] + cov[1]:].sum()
                whole = cov == (0, c.total)
                assert (below + above > 0) == (outside and not whole)
                lb = gr.start_array(c.sorted_keys, cov)
                assert lb[0] == below and lb[-1] == c.n - above
                assert np.array_equal(np.diff(lb), h[cov[0]:cov[0] + cov[1]])


def test_layer_export_reference():
    dims = (2, 2, 3)
    h = np.array([1, 0, 2, 0, 0, 0, 0, 1, 3, 0, 0, 0])
    c = gr.Crafted(dims, h)
    cov = gr.covered(dims)
    lb = gr.start_array(c.sorted_keys, cov)
    want = {0: [0, 1, 1, 3, 3], 1: [0, 0, 0, 0, 1], 2: [0, 3, 3, 3, 3]}
    for z in range(3):
        bodies, lbz = gr.layer_export(lb, cov, dims, z, c.sorted_posm)
        assert lbz.tolist() == want[z]
        keys = sr.grid_keys  # noqa: F841  (the bodies of the layer are those whose key lies in it, in stable order)
        sel = np.flatnonzero(c.keys // 4 == z)
        sel = sel[np.argsort(c.keys[sel], kind="stable")]
        assert np.array_equal(bodies, c.posm[sel])
    cov1 = gr.covered(dims, (1, 1))
    lb1 = gr.start_array(c.sorted_keys, cov1)
    assert gr.layer_export(lb1, cov1, dims, 0, c.sorted_posm) is None and gr.layer_export(lb1, cov1, dims, 2, c.sorted_posm) is None
    assert gr.layer_export(lb1, cov1, dims, 1, c.sorted_posm)[1].tolist() == [0, 0, 0, 0, 1]   # rebased: the array itself starts at 3


def loop_unit_list(cnt, lo0, chunk, min_cnt, mode):
    heavy, other, light, pos = [], [], [], lo0
    for c, k in enumerate(cnt):
        if k >= min_cnt:
            (heavy if k > gr.HEAVY else other).extend((c, q) for q in range(-(-k // chunk)))
        elif mode == gr.BODIES:
            light.extend(range(pos, pos + k))
        elif mode == gr.PAIRS:
            light.extend((pos + q) | (0x80000000 if q + 1 >= k else 0) for q in range(0, k, 2))
        pos += k
    return heavy, other, sorted(light)


def test_unit_list_of_a_hand_counted_example():
    cnt = [0, 1, 48, 49, 64, 65, 128, 129, 300]
    lb = np.concatenate([[0], np.cumsum(cnt)]).astype(np.int32)
    cov = (0, len(cnt))
    u = gr.unit_list(lb, cov, 0, 9, 128)
    # chunks of 128: 1 and 48 -> one light unit each; 49, 64, 65, 128 -> one heavy unit each; 129 -> 2; 300 -> 3
    assert u["counts"].tolist() == [9, 300, 2, 0]
    assert u["other"].tolist() == [[1, 0], [2, 0]]
    assert u["heavy"].tolist() == [[3, 0], [4, 0], [5, 0], [6, 0], [7, 0], [7, 1], [8, 0], [8, 1], [8, 2]]
    u = gr.unit_list(lb, cov, 0, 9, 64)
    assert u["counts"].tolist() == [1 + 1 + 2 + 2 + 3 + 5, 300, 2, 0]
    # without the cell of 300, and without the one of 129: the most crowded cell is reported above 64 only
    assert gr.unit_list(lb, cov, 0, 8, 128)["counts"][1] == 129 and gr.unit_list(lb, cov, 0, 5, 128)["counts"][1] == 0
    assert gr.unit_list(lb, cov, 0, 6, 128)["counts"][1] == 65
    # a range that starts inside the array: cells are numbered from cell_first
    u = gr.unit_list(lb, cov, 7, 9, 128)
    assert u["heavy"].tolist() == [[0, 0], [0, 1], [1, 0], [1, 1], [1, 2]] and u["counts"].tolist() == [5, 300, 0, 0]
    # the split forms: cells below 49 bodies are light
    u = gr.unit_list(lb, cov, 0, 9, 128, 49, gr.BODIES)
    assert u["counts"].tolist() == [9, 300, 0, 49] and u["light"].tolist() == list(range(49))
    u = gr.unit_list(lb, cov, 0, 9, 128, 49, gr.PAIRS)
    assert u["counts"].tolist() == [9, 300, 0, 1 + 24]
    assert u["light"].tolist() == sorted([0 | 0x80000000] + list(range(1, 49, 2)))   # the single body is its cell's odd last one
    u = gr.unit_list(lb, cov, 0, 4, 128, gr.INT_MAX, gr.PAIRS)   # 0, 1, 48, 49: the 49th body carries the top bit
    assert u["counts"].tolist() == [0, 0, 0, 1 + 24 + 25] and (49 + 48) | 0x80000000 in u["light"].tolist()
    for chunk, min_cnt, mode in gr.UNIT_SETTINGS:
        u = gr.unit_list(lb, cov, 0, 9, chunk, min_cnt, mode)
        heavy, other, light = loop_unit_list(cnt, 0, chunk, min_cnt, mode)
        assert u["heavy"].tolist() == [list(r) for r in heavy] and u["other"].tolist() == [list(r) for r in other]
        assert u["light"].tolist() == light


@pytest.mark.parametrize("chunk,min_cnt,mode", gr.UNIT_SETTINGS)
def test_unit_list_cases_hold_their_populations(chunk, min_cnt, mode):
    pops = gr.unit_populations(chunk, min_cnt)
    assert {0, 1, 48, 49, 63, 64, 65, chunk - 1, chunk, chunk + 1, 2 * chunk + 1, 300} <= set(pops)
    if min_cnt < gr.INT_MAX:
        assert {min_cnt - 1, min_cnt} <= set(pops)
    for total in gr.UNIT_LINES + (135, 192):
        h = gr.hist_units(total, chunk, min_cnt, 1)
        assert set(pops) <= set(h.tolist()) and h[0] in pops and h[-1] in pops
        n = int(h.sum())
        assert n < (1 << 17) and gr.builder(n, (0, total)) == "position"
        lb = np.concatenate([[0], np.cumsum(h)]).astype(np.int32)
        u = gr.unit_list(lb, (0, total), 0, total, chunk, min_cnt, mode)
        heavy, other, light = loop_unit_list(h.tolist(), 0, chunk, min_cnt, mode)
        assert u["heavy"].tolist() == [list(r) for r in heavy] and u["other"].tolist() == [list(r) for r in other]
        assert u["light"].tolist() == light
        assert u["counts"][0] + u["counts"][2] <= n + n // 64 + 1024     # the capacity the slots are counted against


def test_no_array_case_has_a_force_on_every_body(oracle):
    h = gr.hist_no_array()
    c = gr.Crafted((h.size, 1, 1), h, seed=13, jitter=gr.NO_ARRAY_JITTER)
    ic = c.ic
    a = np.stack(oracle.spatial_hash_forces_grid(ic["pos_x"], ic["pos_y"], ic["pos_z"], ic["mass"], c.n, 1.0,
                                                 float(np.float32(0.05) ** 2), 1.0, 1.0, c.bounds[:3], c.dims), 1)
    assert np.all(np.linalg.norm(a, axis=1) > 0)


@pytest.mark.parametrize("dims", gr.RIM_GRIDS)
@pytest.mark.parametrize("cutoff", [1.0, 1.7])
def test_rim_cases_have_few_bodies_without_a_force(oracle, dims, cutoff):
    """at most 10 % of a case's bodies may have a zero reference force (they are compared for exact zero only)"""
    ic, bounds = gr.rim_bodies(dims)
    lo, odims = sr.grid_geometry(oracle, ic, 1.0, bounds)
    assert tuple(odims) == dims
    keys = sr.grid_keys(oracle, ic, 1.0, lo, odims)
    total = dims[0] * dims[1] * dims[2]
    assert keys.min() == 0 and keys.max() == total - 1 and np.unique(keys).size >= 0.95 * total   # both corners hold bodies
    for eps in (0.05, 0.0):
        a = np.stack(oracle.spatial_hash_forces_grid(ic["pos_x"], ic["pos_y"], ic["pos_z"], ic["mass"], gr.RIM_N, 1.0,
                                                     float(np.float32(eps) ** 2), 1.0, cutoff, lo, odims), 1)
        assert np.all(np.isfinite(a))
        assert (np.linalg.norm(a, axis=1) == 0).mean() <= 0.10

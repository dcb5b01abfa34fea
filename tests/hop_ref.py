"""The model of include/nbody_hip_hop.h restated in numpy (no GPU, no library): next, peak, the saddle table, the union
of the viable peaks, the attachment rounds, the catalogue and group_peak.  `reference` returns the device outputs and,
beyond them, `rounds`, the dropped peaks, the edge table and the number of unions, so a test can tell what its input
exercised.  HAND_CASES are graphs of at most 12 bodies whose answers are written out by hand."""
import numpy as np

MAX_K = 32


def defaults(delta_outer, delta_saddle=None, delta_peak=None):
    """HOP's defaults: 2.5 and 3 times delta_outer"""
    return (float(delta_outer), 2.5 * delta_outer if delta_saddle is None else float(delta_saddle),
            3.0 * delta_outer if delta_peak is None else float(delta_peak))


def lower_median(rho):
    """the default delta_outer of the hopGroups calls: the lower median of the densities that are no NaN (of an even
    number, the lower of the two in the middle)"""
    v = np.sort(np.asarray(rho, np.float64)[~np.isnan(rho)])
    return float(v[(v.size - 1) // 2]) if v.size else 0.0


def _empty(n, status):
    return dict(labels=np.full(n, -1, np.int32), peak=np.full(n, -1, np.int32), offsets=np.zeros(1, np.int32),
                members=np.zeros(0, np.int32), group_peak=np.zeros(0, np.int32),
                counts=np.array([0, 0, 0, 0, status], np.int64), rounds=0, dropped=np.zeros(0, np.int32),
                edges=np.zeros((0, 2), np.int32), saddles=np.zeros(0, np.float64), unions=0, next=None, anchor=None)


def reference(index, rho, n_hop, n_merge, delta_outer, delta_saddle=None, delta_peak=None, min_members=1):
    index = np.asarray(index, np.int32)
    rho = np.asarray(rho, np.float64)
    n, k = index.shape
    assert rho.shape == (n,) and 1 <= k <= MAX_K and 1 <= n_hop <= k and 0 <= n_merge <= k and min_members >= 1
    d_outer, d_saddle, d_peak = defaults(delta_outer, delta_saddle, delta_peak)
    assert 0 <= d_outer <= d_saddle <= d_peak < np.inf
    if (index[:, :max(n_hop, n_merge)] >= n).any():
        return _empty(n, 1)
    me = np.arange(n, dtype=np.int64)
    # hop: the slots in order, each replacing b while better(j, b)
    b, rb = me.copy(), rho.copy()
    for s in range(n_hop):
        j = index[:, s].astype(np.int64)
        ok = j >= 0
        jj = np.where(ok, j, 0)
        rj = rho[jj]
        better = ok & ((rj > rb) | ((rj == rb) & (jj < b)))  # (every compare with a NaN is False)
        b, rb = np.where(better, jj, b), np.where(better, rj, rb)
    nxt = b
    peak = nxt.copy()
    while True:
        twice = peak[peak]
        if (twice == peak).all():
            break
        peak = twice
    live = rho >= d_outer
    is_peak = peak == me
    # saddles: undirected {P, Q}, the maximum of b over the pairs found from either side
    Ps, Qs, Bs = [], [], []
    for s in range(n_merge):
        j = index[:, s].astype(np.int64)
        ok = j >= 0
        jj = np.where(ok, j, 0)
        take = live & ok & live[jj] & (peak != peak[jj])
        i = me[take]
        jt = jj[take]
        bound = (rho[i] + rho[jt]) * 0.5 + 0.0  # (+ 0.0: a -0 becomes the +0 it equals)
        Ps.append(np.minimum(peak[i], peak[jt]))
        Qs.append(np.maximum(peak[i], peak[jt]))
        Bs.append(bound)
    P = np.concatenate(Ps) if Ps else np.zeros(0, np.int64)
    Q = np.concatenate(Qs) if Qs else np.zeros(0, np.int64)
    B = np.concatenate(Bs) if Bs else np.zeros(0, np.float64)
    n_records = 2 * P.size
    if P.size:
        order = np.lexsort((Q, P))
        P, Q, B = P[order], Q[order], B[order]
        head = np.r_[True, (P[1:] != P[:-1]) | (Q[1:] != Q[:-1])]
        first = np.nonzero(head)[0]
        eP, eQ, eS = P[first], Q[first], np.maximum.reduceat(B, first)
    else:
        eP, eQ, eS = P, Q, B
    # 1. the viable peaks, united where the saddle reaches delta_saddle; the root is the lowest peak of a component
    viable = is_peak & live & (rho >= d_peak)
    root = me.copy()
    link = viable[eP] & viable[eQ] & (eS >= d_saddle)
    lp, lq = eP[link], eQ[link]
    while lp.size:
        low = np.minimum(root[lp], root[lq])
        before = root.copy()
        np.minimum.at(root, lp, low)
        np.minimum.at(root, lq, low)
        root = root[root]
        if (root == before).all():
            break
    unions = int(viable.sum() - np.unique(root[viable]).size)
    anchor = np.where(viable, 0, -1)
    # 2. the rounds: both directions of every edge, P the peak that looks, Q the one it looks at
    dP, dQ, dS = np.r_[eP, eQ], np.r_[eQ, eP], np.r_[eS, eS]
    candidate = is_peak & live & ~viable
    rounds = 0
    while True:
        rounds += 1
        can = candidate[dP] & (anchor[dP] < 0) & (anchor[dQ] >= 0)  # (whatever is anchored now was anchored before this round)
        if not can.any():
            break
        p, q, s = dP[can], dQ[can], dS[can]
        order = np.lexsort((q, -s, p))  # per P: the greatest S first, ties to the lowest Q
        p, q = p[order], q[order]
        first = np.r_[True, p[1:] != p[:-1]]
        root[p[first]] = root[q[first]]
        anchor[p[first]] = rounds
    dropped = me[candidate & (anchor < 0)]
    labels = np.where(live & (anchor[peak] >= 0), root[peak], -1)
    # the catalogue
    sizes = np.bincount(labels[labels >= 0], minlength=n)
    kept = (labels >= 0) & (sizes[np.maximum(labels, 0)] >= min_members)
    members = me[kept][np.argsort(labels[kept], kind="stable")]
    group_labels, group_sizes = np.unique(labels[kept], return_counts=True)
    offsets = np.r_[0, np.cumsum(group_sizes)]
    group_peak = np.zeros(group_labels.size, np.int64)
    anchored_peaks = me[is_peak & (anchor >= 0)]
    for g, lab in enumerate(group_labels):
        ps = anchored_peaks[root[anchored_peaks] == lab]
        top = ps[rho[ps] == rho[ps].max()]
        group_peak[g] = top.min()
    counts = np.array([group_labels.size, members.size, int(is_peak.sum()), rounds, 0], np.int64)
    return dict(labels=labels.astype(np.int32), peak=peak.astype(np.int32), offsets=offsets.astype(np.int32),
                members=members.astype(np.int32), group_peak=group_peak.astype(np.int32), counts=counts, rounds=rounds,
                dropped=dropped.astype(np.int32), edges=np.stack([eP, eQ], 1).astype(np.int32), saddles=eS, unions=unions,
                next=nxt.astype(np.int32), anchor=anchor.astype(np.int32), n_records=n_records)


OUTPUTS = ("labels", "peak", "offsets", "members", "group_peak", "counts")


def rows(lists, k, fill=-1):
    """rows of at most k entries -> index [n, k] int32, the unused slots `fill`"""
    out = np.full((len(lists), k), fill, np.int32)
    for i, r in enumerate(lists):
        out[i, :len(r)] = r
    return out


def line_graph(n):
    """index[i] = [i + 1, i - 1], k = 2; the ends have one neighbour and a -1"""
    i = np.arange(n, dtype=np.int32)
    up, down = i + 1, i - 1
    up[-1] = -1
    return np.stack([up, down], 1).astype(np.int32)


def _below(x):
    return float(np.nextafter(np.float64(x), -np.inf))


def hand_cases():
    """name -> (arguments of `reference`, the answers written out by hand: any of labels, peak, offsets, members,
    group_peak, rounds, dropped, n_peaks, edges, saddles)"""
    nan = float("nan")
    cases = {}
    # a tie in rho: bodies 1 and 2 share the top density; the lower index wins, for every body
    cases["tie"] = (dict(index=rows([[1, 2], [0, 2], [0, 1], [2, 1]], 2), rho=[1.0, 5.0, 5.0, 1.0], n_hop=2, n_merge=2,
                         delta_outer=0.5, delta_saddle=1.0, delta_peak=2.0),
                    dict(peak=[1, 1, 1, 1], labels=[1, 1, 1, 1], offsets=[0, 4], members=[0, 1, 2, 3], group_peak=[1],
                         rounds=1, n_peaks=1, dropped=[], edges=[]))
    # a NaN: body 2 is its own peak, nobody's target, dead; body 3 names only the NaN and stays its own (dead) peak
    cases["nan"] = (dict(index=rows([[2, 1], [2, 0], [0, 1], [2]], 2), rho=[1.0, 4.0, nan, 0.1], n_hop=2, n_merge=2,
                         delta_outer=0.5, delta_saddle=1.0, delta_peak=2.0),
                    dict(peak=[1, 1, 2, 3], labels=[1, 1, -1, -1], offsets=[0, 2], members=[0, 1], group_peak=[1],
                         rounds=1, n_peaks=3, dropped=[], edges=[]))
    # a -1 slot in front of the neighbour that counts
    cases["minus_one"] = (dict(index=rows([[-1, 1], [-1, -1], [-1, 1]], 2), rho=[1.0, 2.0, 1.5], n_hop=2, n_merge=2,
                               delta_outer=0.0, delta_saddle=0.0, delta_peak=0.0),
                          dict(peak=[1, 1, 1], labels=[1, 1, 1], offsets=[0, 3], members=[0, 1, 2], group_peak=[1], rounds=1,
                               n_peaks=1))
    # n_hop < k: the denser body 2 sits in slot 1 of row 0 and is not read by the hop (n_hop = 1), but n_merge = 2 reads
    # it as a boundary: peaks 1 and 2, S = (1 + 9) / 2 = 5 >= delta_saddle = 3, both viable: united under 1
    cases["n_hop_below_k"] = (dict(index=rows([[1, 2], [0, -1], [-1, -1]], 2), rho=[1.0, 3.0, 9.0], n_hop=1, n_merge=2,
                                   delta_outer=0.5, delta_saddle=3.0, delta_peak=3.0),
                              dict(peak=[1, 1, 2], labels=[1, 1, 1], offsets=[0, 3], members=[0, 1, 2], group_peak=[2],
                                   rounds=1, n_peaks=2, edges=[[1, 2]], saddles=[5.0]))
    # a saddle exactly at delta_saddle merges (>=) ...  peaks 0 (rho 8) and 3 (rho 6); the boundary pair (1, 2) has
    # b = (1 + 3) / 2 = 2, both operations exact
    at = dict(index=rows([[1], [0, 2], [3, 1], [2]], 2), rho=[8.0, 1.0, 3.0, 6.0], n_hop=2, n_merge=2, delta_outer=1.0,
              delta_saddle=2.0, delta_peak=5.0)
    cases["saddle_at"] = (at, dict(peak=[0, 0, 3, 3], labels=[0, 0, 0, 0], offsets=[0, 4], members=[0, 1, 2, 3],
                                   group_peak=[0], rounds=1, n_peaks=2, edges=[[0, 3]], saddles=[2.0]))
    # ... and one ulp below it does not: rho[2] one ulp under 3 gives 1 + rho[2] = 4 - 2^-51 (a double) and b one ulp
    # under 2
    under = dict(at, rho=[8.0, 1.0, _below(3.0), 6.0])
    assert (1.0 + under["rho"][2]) * 0.5 == _below(2.0)
    cases["saddle_below"] = (under, dict(peak=[0, 0, 3, 3], labels=[0, 0, 3, 3], offsets=[0, 2, 4], members=[0, 1, 2, 3],
                                         group_peak=[0, 3], rounds=1, n_peaks=2, edges=[[0, 3]], saddles=[_below(2.0)]))
    # a non-viable pair that prefer each other, no viable neighbour: both dropped; body 4 is a viable peak far away
    cases["dropped_pair"] = (dict(index=rows([[1], [0, 2], [3, 1], [2], [-1]], 2), rho=[3.0, 1.0, 1.5, 3.5, 9.0], n_hop=2,
                                  n_merge=2, delta_outer=0.5, delta_saddle=2.0, delta_peak=5.0),
                             dict(peak=[0, 0, 3, 3, 4], labels=[-1, -1, -1, -1, 4], offsets=[0, 1], members=[4], group_peak=[4],
                                  rounds=1, n_peaks=3, dropped=[0, 3], edges=[[0, 3]], saddles=[1.25]))
    # a chain of three non-viable peaks reaching a viable one: peaks 0 (viable, rho 9), 2, 4, 6 (rho 3); the bodies
    # between them (1, 3, 5, rho 1) hop up to the lower-indexed peak and name the next: edges {0,2}, {2,4}, {4,6}.
    # Round 1 anchors 2, round 2 anchors 4, round 3 anchors 6, round 4 anchors nothing: rounds == 4
    cases["chain_of_three"] = (dict(index=rows([[-1], [0, 2], [-1], [2, 4], [-1], [4, 6], [-1]], 2),
                                    rho=[9.0, 1.0, 3.0, 1.0, 3.0, 1.0, 3.0], n_hop=1, n_merge=2, delta_outer=0.5,
                                    delta_saddle=4.0, delta_peak=5.0),
                               dict(peak=[0, 0, 2, 2, 4, 4, 6], labels=[0] * 7, offsets=[0, 7], members=list(range(7)),
                                    group_peak=[0], rounds=4, n_peaks=4, dropped=[], edges=[[0, 2], [2, 4], [4, 6]],
                                    saddles=[2.0, 2.0, 2.0]))
    # an asymmetric list: 1 is in 0's row but 0 is not in 1's; 0 (rho 6) and 1 (rho 7) are both peaks because n_hop = 1
    # reads only slot 0 (-1); the edge {0, 1} exists from 0's side alone: S = 6.5 >= delta_saddle, united under 0
    cases["asymmetric"] = (dict(index=rows([[-1, 1], [-1, -1]], 2), rho=[6.0, 7.0], n_hop=1, n_merge=2, delta_outer=1.0,
                                delta_saddle=6.0, delta_peak=6.0),
                           dict(peak=[0, 1], labels=[0, 0], offsets=[0, 2], members=[0, 1], group_peak=[1], rounds=1, n_peaks=2,
                                edges=[[0, 1]], saddles=[6.5]))
    # the attachment choice.  Peaks 0 (rho 9) and 1 (rho 8) are viable and not united; the non-viable peak 2 (rho 3) has
    # S = (1 + 9) / 2 = 5 to 0 (body 4) and S = (2 + 8) / 2 = 5 to 1 (body 5): the tie goes to the lowest Q, 0.  The
    # non-viable peak 3 has S = 5 to 0 (body 6) and S = (2.5 + 8) / 2 = 5.25 to 1 (body 7): the greatest S wins, 1
    cases["attach_choice"] = (dict(index=rows([[-1, -1], [-1, -1], [-1, -1], [-1, -1], [2, 0], [2, 1], [3, 0], [3, 1]], 2),
                                   rho=[9.0, 8.0, 3.0, 3.0, 1.0, 2.0, 1.0, 2.5], n_hop=1, n_merge=2, delta_outer=0.5,
                                   delta_saddle=5.0, delta_peak=5.0),
                              dict(peak=[0, 1, 2, 3, 2, 2, 3, 3], labels=[0, 1, 0, 1, 0, 0, 1, 1], offsets=[0, 4, 8],
                                   members=[0, 2, 4, 5, 1, 3, 6, 7], group_peak=[0, 1], rounds=2, n_peaks=4, dropped=[],
                                   edges=[[0, 2], [0, 3], [1, 2], [1, 3]], saddles=[5.0, 5.0, 5.0, 5.25]))
    # not the greedy sweep.  Peaks V = 0 (rho 20) and V2 = 1 (rho 18) viable and not united,
    # Q = 2 (rho 10) and P = 3 (rho 9) not viable.  S{Q, V} = (4 + 8) / 2 = 6 (bodies 4 and 6), S{P, Q} = (6 + 4) / 2 = 5
    # (bodies 5 and 4), S{P, V2} = (2 + 6) / 2 = 4 (bodies 7 and 8).  Round 1: Q goes to V, and P -- which sees only what
    # was anchored before the round -- to V2 at 4, not through Q at 5 to V as a descending sweep would send it
    cases["not_the_greedy_sweep"] = (dict(index=rows([[-1], [-1], [-1], [-1], [2, 6], [3, 4], [0], [3, 8], [1]], 2),
                                          rho=[20.0, 18.0, 10.0, 9.0, 4.0, 6.0, 8.0, 2.0, 6.0], n_hop=1, n_merge=2,
                                          delta_outer=1.0, delta_saddle=15.0, delta_peak=15.0),
                                     dict(peak=[0, 1, 2, 3, 2, 3, 0, 3, 1], labels=[0, 1, 0, 1, 0, 1, 0, 1, 1],
                                          offsets=[0, 4, 9], members=[0, 2, 4, 6, 1, 3, 5, 7, 8], group_peak=[0, 1], rounds=2,
                                          n_peaks=4, dropped=[], edges=[[0, 2], [1, 3], [2, 3]], saddles=[6.0, 4.0, 5.0]))
    return cases


def random_graph(n, k, levels, seed, missing=0.1):
    """index [n, k] drawn uniformly (a share `missing` of the slots -1, self-references allowed) and rho drawn from
    `levels` distinct values: massive ties"""
    rng = np.random.default_rng(seed)
    index = rng.integers(0, n, size=(n, k)).astype(np.int32)
    index[rng.random((n, k)) < missing] = -1
    rho = (1.0 + rng.integers(0, levels, size=n)).astype(np.float64)
    return index, rho


def local_graph(n, k, levels, seed, reach=6):
    """neighbours within `reach` places along a line, so that basins are local and peaks are many: the graph on which the
    regrouping has rounds to run"""
    rng = np.random.default_rng(seed)
    i = np.arange(n)[:, None]
    step = rng.integers(1, reach + 1, size=(n, k)) * rng.choice([-1, 1], size=(n, k))
    index = (i + step).astype(np.int64)
    index[(index < 0) | (index >= n)] = -1
    rho = (1.0 + rng.integers(0, levels, size=n)).astype(np.float64)
    return index.astype(np.int32), rho


def regroup_case():
    """the random graph of 3,000 bodies (k = 8, 16 distinct densities) on which the regrouping has work of every kind:
    the arguments of `reference`"""
    index, rho = random_graph(3000, 8, 16, 7)
    return dict(index=index, rho=rho, n_hop=4, n_merge=2, delta_outer=6.0, delta_saddle=12.0, delta_peak=16.0, min_members=1)

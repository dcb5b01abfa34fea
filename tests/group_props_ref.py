"""The group properties (include/nbody_hip_group_props.h: nbody_hip_group_props) restated in numpy, the exact-lattice recipe
of the tests, and the error bounds of the general-data comparison.  No GPU, no package import: the CPU tests hold this
file against a plain-Python loop, the GPU tests hold the kernels against it."""
import numpy as np

# the two sizes of group_props_plan.h, mirrored (tests/test_group_props_plan_cpu.py reads the header and compares)
S = 32      # kGroupSmall: at most S members -> one lane, serial
C = 1024    # kGroupChunk: members per chunk of a larger group

DTYPE = np.dtype([("mass", "<f8"), ("com", "<f8", (3,)), ("vel", "<f8", (3,)), ("ang_mom", "<f8", (3,)),
                  ("kinetic", "<f8"), ("inertia", "<f8", (6,)), ("r_max", "<f8"), ("potential", "<f8"),
                  ("phi_min", "<f8"), ("n", "<i4"), ("label", "<i4"), ("r_max_body", "<i4"),
                  ("phi_min_body", "<i4"), ("status", "<i4"), ("reserved", "<i4", (3,))])
assert DTYPE.itemsize == 192

POS = ("pos_x", "pos_y", "pos_z")
VEL = ("vel_x", "vel_y", "vel_z")
BIG = np.iinfo(np.int64).max


def _segments(offsets, n_members):
    """-> (legal [G] bool, pos [T] positions in members of the legal groups one after another, seg [L] where each legal
    group starts in pos, gid [T] the row of the group in the catalogue)"""
    off = np.asarray(offsets, np.int64)
    o0, o1 = off[:-1], off[1:]
    legal = (o0 >= 0) & (o0 < o1) & (o1 <= n_members)
    n = np.where(legal, o1 - o0, 0)
    rows = np.nonzero(legal)[0]
    nl = n[rows]
    seg = np.concatenate(([0], np.cumsum(nl)))[:-1]
    total = int(nl.sum())
    pos = np.repeat(o0[rows] - seg, nl) + np.arange(total, dtype=np.int64)
    return legal, pos, seg, np.repeat(rows, nl), np.repeat(np.arange(rows.size), nl), rows


def reference(fields, offsets, members, phi=None, count=None, wide=False):
    """The structs of the catalogue (DTYPE), in fp64 -- or, with wide=True, summed in numpy's long double and rounded to
    fp64 once (the general-data reference: its own summation error is then 2^-11 of an fp64 sum's).  Also returns the
    per-group quantities the error bounds are made of.  fields: dict of float32 arrays pos_*, vel_*, mass."""
    F = np.longdouble if wide else np.float64
    members = np.asarray(members, np.int64)
    count = int(fields["mass"].size if count is None else count)
    G = len(offsets) - 1
    out = np.zeros(G, DTYPE)
    aux = {}
    if G == 0:
        return out, aux
    legal, pos, seg, gid_rows, gid, rows = _segments(offsets, members.size)
    out["status"] = 1
    if rows.size == 0:
        return out, aux
    idx = members[pos]
    bad_member = (idx < 0) | (idx >= count)
    safe = np.where(bad_member, 0, idx)
    bad_group = np.logical_or.reduceat(bad_member, seg)
    m = fields["mass"][safe].astype(np.float64)
    x = [fields[k][safe].astype(np.float64) for k in POS]
    v = [fields[k][safe].astype(np.float64) for k in VEL]

    def gsum(t):  # t: fp64 terms (each rounded as the model rounds it); the sum in F, rounded to fp64
        return np.add.reduceat(t.astype(F), seg).astype(np.float64)

    M = gsum(m)
    zero = M == 0.0
    Ms = np.where(zero, 1.0, M)
    X = [np.where(zero, 0.0, gsum(m * x[a]) / Ms) for a in range(3)]
    V = [np.where(zero, 0.0, gsum(m * v[a]) / Ms) for a in range(3)]
    d = [x[a] - X[a][gid] for a in range(3)]
    u = [v[a] - V[a][gid] for a in range(3)]
    L = [gsum(m * ((d[1] * u[2]) - (d[2] * u[1]))), gsum(m * ((d[2] * u[0]) - (d[0] * u[2]))),
         gsum(m * ((d[0] * u[1]) - (d[1] * u[0])))]
    T = gsum(m * (((u[0] * u[0]) + (u[1] * u[1])) + (u[2] * u[2])))
    pairs = ((0, 0), (1, 1), (2, 2), (0, 1), (0, 2), (1, 2))
    I = [gsum(m * (d[a] * d[b])) for a, b in pairs]
    r2 = ((d[0] * d[0]) + (d[1] * d[1])) + (d[2] * d[2])
    r2max = np.maximum.reduceat(r2, seg)
    r2body = np.minimum.reduceat(np.where(r2 == r2max[gid], idx, BIG), seg)
    # the runner-up: the largest r2 among the members that are not the winning body
    second = np.maximum.reduceat(np.where(idx == r2body[gid], -np.inf, r2), seg)
    good = ~bad_group
    o = np.zeros(rows.size, DTYPE)
    o["mass"] = M
    for a in range(3):
        o["com"][:, a], o["vel"][:, a], o["ang_mom"][:, a] = X[a], V[a], L[a]
    o["kinetic"] = 0.5 * T
    for k in range(6):
        o["inertia"][:, k] = I[k]
    o["r_max"] = np.sqrt(r2max)
    o["r_max_body"] = r2body
    o["phi_min_body"] = -1
    if phi is not None:
        ph = np.asarray(phi, np.float32)[safe].astype(np.float64)
        o["potential"] = 0.5 * gsum(m * ph)
        pmin = np.minimum.reduceat(ph, seg)
        o["phi_min"] = pmin
        o["phi_min_body"] = np.minimum.reduceat(np.where(ph == pmin[gid], idx, BIG), seg)
    off = np.asarray(offsets, np.int64)
    o["n"] = (off[1:] - off[:-1])[rows]
    o["label"] = safe[seg]
    o[~good] = np.zeros(1, DTYPE)
    o["status"] = np.where(good, 0, 1)
    out[rows] = o

    def asum(t):
        return np.add.reduceat(np.abs(t), seg)

    # the absolute sums the bounds are made of (rows of the LEGAL groups scattered back to catalogue rows)
    def scatter(a, fill=0.0):
        r = np.full(G, fill, np.float64)
        r[rows] = a
        return r

    aux = {
        "abs_mx": [scatter(asum(m * x[a])) for a in range(3)],
        "abs_mv": [scatter(asum(m * v[a])) for a in range(3)],
        "abs_L": [scatter(asum(m * (np.abs(d[1] * u[2]) + np.abs(d[2] * u[1])))),
                  scatter(asum(m * (np.abs(d[2] * u[0]) + np.abs(d[0] * u[2])))),
                  scatter(asum(m * (np.abs(d[0] * u[1]) + np.abs(d[1] * u[0]))))],
        "abs_T": scatter(asum(m * (u[0] * u[0] + u[1] * u[1] + u[2] * u[2]))),
        "abs_I": [scatter(asum(m * (d[a] * d[b]))) for a, b in pairs],
        "abs_W": scatter(asum(m * ph)) if phi is not None else np.zeros(G),
        "A_d": scatter(asum(m * (np.abs(d[0]) + np.abs(d[1]) + np.abs(d[2])))),
        "A_u": scatter(asum(m * (np.abs(u[0]) + np.abs(u[1]) + np.abs(u[2])))),
        "r_second": scatter(np.sqrt(np.maximum(second, 0.0)), fill=-np.inf),
        "has_second": scatter(np.isfinite(second).astype(np.float64)) > 0,
    }
    return out, aux


def plain_python(fields, offsets, members, phi=None):
    """The model as three nested Python loops (groups, members, axes) over Python floats, in member order: for legal
    catalogues of a few members.  -> list of dicts."""
    f = {k: [float(t) for t in a] for k, a in fields.items()}
    res = []
    for g in range(len(offsets) - 1):
        mem = [int(i) for i in members[offsets[g]:offsets[g + 1]]]
        M, P, Q = 0.0, [0.0] * 3, [0.0] * 3
        for i in mem:
            M = M + f["mass"][i]
            for a in range(3):
                P[a] = P[a] + f["mass"][i] * f[POS[a]][i]
                Q[a] = Q[a] + f["mass"][i] * f[VEL[a]][i]
        X = [P[a] / M if M != 0.0 else 0.0 for a in range(3)]
        V = [Q[a] / M if M != 0.0 else 0.0 for a in range(3)]
        L, T, I, W = [0.0] * 3, 0.0, [0.0] * 6, 0.0
        rbest, rbody, pbest, pbody = -1.0, None, float("inf"), None
        for i in mem:
            m = f["mass"][i]
            d = [f[POS[a]][i] - X[a] for a in range(3)]
            u = [f[VEL[a]][i] - V[a] for a in range(3)]
            for a in range(3):
                b, c = (a + 1) % 3, (a + 2) % 3
                L[a] = L[a] + m * ((d[b] * u[c]) - (d[c] * u[b]))
            T = T + m * (((u[0] * u[0]) + (u[1] * u[1])) + (u[2] * u[2]))
            for k, (a, b) in enumerate(((0, 0), (1, 1), (2, 2), (0, 1), (0, 2), (1, 2))):
                I[k] = I[k] + m * (d[a] * d[b])
            r2 = ((d[0] * d[0]) + (d[1] * d[1])) + (d[2] * d[2])
            if r2 > rbest or (r2 == rbest and i < rbody):
                rbest, rbody = r2, i
            if phi is not None:
                p = float(phi[i])
                W = W + m * p
                if p < pbest or (p == pbest and i < pbody):
                    pbest, pbody = p, i
        res.append(dict(mass=M, com=X, vel=V, ang_mom=L, kinetic=0.5 * T, inertia=I, r_max=rbest ** 0.5,
                        potential=0.5 * W if phi is not None else 0.0, phi_min=pbest if phi is not None else 0.0,
                        n=len(mem), label=mem[0], r_max_body=rbody, phi_min_body=pbody if phi is not None else -1,
                        status=0))
    return res


# ---- the exact lattice -------------------------------------------------------------------------------------------------
MASSES = np.array([0.5, 1.0, 2.0, 4.0], np.float32)


def lattice_sizes(small_before=1500, small_after=1500, seed=5):
    """the group sizes of the GPU lattice test: every size at which the pass takes another path, one group of 64 C + 3,
    and a few thousand small groups before and after it"""
    rng = np.random.default_rng(seed)
    edge = [1, 2, 3, S - 1, S, S + 1, C - 1, C, C + 1, 2 * C, 2 * C + 1]
    return (list(rng.integers(1, 7, small_before)) + edge[:6] + [64 * C + 3] + edge[6:]
            + list(rng.integers(1, 7, small_after)))


def lattice(sizes, count, seed=1):
    """A catalogue in which every quantity of the model is exact in fp64 whatever the order of the sums.  Group g of n
    members: n // 2 mirrored pairs about an integer centre c (|c| <= 512) -- offsets +-o, integer |o_a| <= 32, relative
    velocities +-w, integer |w_a| <= 8, one mass of {0.5, 1, 2, 4} for both bodies of a pair -- and, for an odd n, one
    body at c with the bulk velocity V (integer, |V_a| <= 16).  phi: multiples of 1/8 in [-64, 0], repeated within the
    small groups so that the minimum ties.  The groups' bodies are scattered over [0, count) by a seeded permutation;
    the bodies no group holds are background; the last member of the last group is body count - 1.
    -> (fields, offsets int32, members int32, phi float32)"""
    rng = np.random.default_rng(seed)
    sizes = np.asarray(sizes, np.int64)
    total = int(sizes.sum())
    assert total < count
    G = sizes.size
    gid = np.repeat(np.arange(G), sizes)
    start = np.concatenate(([0], np.cumsum(sizes)))
    k = np.arange(total) - start[gid]           # position in the group
    pair = k // 2
    odd_one = (k == sizes[gid] - 1) & (sizes[gid] % 2 == 1)
    sign = np.where(odd_one, 0, np.where(k % 2 == 0, 1, -1))
    c = rng.integers(-512, 513, (G, 3))
    Vg = rng.integers(-16, 17, (G, 3))
    # per (group, pair) draws: index them by the first body of the pair
    first = start[gid] + 2 * pair
    o_all = rng.integers(-32, 33, (total, 3))
    w_all = rng.integers(-8, 9, (total, 3))
    m_all = MASSES[rng.integers(0, 4, total)]
    first = np.minimum(first, total - 1)
    o, w, m = o_all[first], w_all[first], m_all[first]
    x = c[gid] + sign[:, None] * o
    v = Vg[gid] + sign[:, None] * w
    m = np.where(odd_one, m_all[np.arange(total)], m)
    # phi: few distinct values per small group (ties), any of the 513 in the large ones
    base = rng.integers(-512, 1, G)
    step = rng.integers(0, 3, total)
    ph_small = np.clip(base[gid] + step, -512, 0)
    ph = np.where(sizes[gid] <= S, ph_small, rng.integers(-512, 1, total)) / 8.0
    perm = rng.permutation(count)
    where = np.nonzero(perm[:total] == count - 1)[0]
    if where.size:
        perm[where[0]], perm[total - 1] = perm[total - 1], perm[where[0]]
    else:
        j = np.nonzero(perm == count - 1)[0][0]
        perm[j], perm[total - 1] = perm[total - 1], perm[j]
    members = perm[:total].astype(np.int32)
    fields = {}
    bg = rng.integers(-600, 601, (count, 7)).astype(np.float32)  # the background: bodies of no group
    for a in range(3):
        fields[POS[a]] = bg[:, a].copy()
        fields[VEL[a]] = (bg[:, 3 + a] / 32).astype(np.float32)
        fields[POS[a]][members] = x[:, a]
        fields[VEL[a]][members] = v[:, a]
    fields["mass"] = np.abs(bg[:, 6]) + 1
    fields["mass"][members] = m
    phi = (rng.integers(-512, 1, count) / 8.0).astype(np.float32)
    phi[members] = ph
    return fields, start.astype(np.int32), members, phi


# ---- general data --------------------------------------------------------------------------------------------------------
N_PLUMMER, N_BACKGROUND, LINK = 20000, 10000, 0.2


def general_fields(ic):
    """A Plummer sphere in a uniform background (ic: the package's initial-condition module).  The masses are spread by
    a seeded factor in [0.5, 1.5): with equal masses the two bodies of every pair would be equally far from their centre
    up to rounding, and r_max_body would be undecided in every group of two."""
    a = ic.plummer(N_PLUMMER, seed=3)
    b = ic.uniform_box(N_BACKGROUND, seed=4, lo=-6.0, hi=6.0)
    f = {k: np.concatenate([np.asarray(a[k], np.float32), np.asarray(b[k], np.float32)]) for k in POS + VEL + ("mass",)}
    f["mass"] = (f["mass"] * np.random.default_rng(7).uniform(0.5, 1.5, f["mass"].size)).astype(np.float32)
    return f


def r_max_decided(ref, aux, bound):
    """the groups in which r_max_body is asserted: one member, or the reference's runner-up further from the winner than
    the two bounds together can move them"""
    return ~aux["has_second"] | (ref["r_max"] - aux["r_second"] > 2 * bound["r_max"])


R_MAX_UNDECIDED_CAP = 0.01  # at most 1 % of the groups may be left out of the r_max_body comparison


# ---- the bounds of the general-data comparison ------------------------------------------------------------------------
U = 2.0 ** -53
# (n + K) u sum|t| bounds |device - reference| of one sum of n terms:
#   n - 1  roundings of the device's additions, in any order (each at most u times the running absolute sum <= sum|t|);
#   6      roundings at most inside one term (the deepest is T: u = v - V, u * u, two additions, m * ..: 1 + 1 + 2 + 1 = 5
#          relative to the term's products taken absolutely; ang_mom: 1 (d) + 1 (u) + 1 (product) + 1 (difference) +
#          1 (m * ..) = 5; 6 covers the second-order remainder of the products of these factors);
#   1      the reference's own rounding of its long double sum to fp64;
#   the reference's long double summation, (n + 6) 2^-64 sum|t| = (n + 6) / 2048 u sum|t|: at most 17 for n <= 2^15.
# 6 - 1 + 1 + 17 = 23 <= K = 24.  sum|t| is the reference's sum of m times the ABSOLUTE products of the term.
K = 24
N_MAX = 2 ** 15


def bounds(ref, aux):
    """Per group and field, the bound on |device - reference| of the general-data test, from the reference's own absolute
    sums: the rounding of each sum, carried through the two divisions into com and vel (dX, dV), the effect of dX and dV
    on every central sum, and the square root of r_max.  -> dict of arrays shaped like the fields."""
    n = ref["n"].astype(np.float64)
    assert n.max() <= N_MAX and np.finfo(np.longdouble).eps <= 2.0 ** -63
    e = (n + K) * U
    M = ref["mass"]
    Ms = np.where(M > 0, M, 1.0)
    b = {"mass": e * M}
    dX = np.zeros((n.size, 3))
    dV = np.zeros((n.size, 3))
    for a in range(3):
        # X = fl(P / M): |dP| <= e sum|m x|, |dM| <= e M; first order in both, the quotient's rounding and the
        # reference's own (2 u |X|), and the second-order remainder as the factor 1 / (1 - e)
        dX[:, a] = (e * aux["abs_mx"][a] + np.abs(ref["com"][:, a]) * e * M) / (Ms * (1 - e)) + 2 * U * np.abs(ref["com"][:, a])
        dV[:, a] = (e * aux["abs_mv"][a] + np.abs(ref["vel"][:, a]) * e * M) / (Ms * (1 - e)) + 2 * U * np.abs(ref["vel"][:, a])
    b["com"], b["vel"] = dX, dV
    dx, dv = dX.max(axis=1), dV.max(axis=1)   # every component of dX (dV) is at most dx (dv)
    A_d, A_u = aux["A_d"], aux["A_u"]
    # ang_mom_a = sum m (d_b u_c - d_c u_b): moving X by dX and V by dV changes a term by at most
    # m (dx (|u_c| + |u_b|) + dv (|d_b| + |d_c|) + 2 dx dv)
    shift_L = dx * A_u + dv * A_d + 2 * M * dx * dv
    b["ang_mom"] = np.stack([e * aux["abs_L"][a] + shift_L for a in range(3)], 1)
    # kinetic = 1/2 sum m |u|^2: |u + dv|^2 - |u|^2 <= 2 dv (|ux| + |uy| + |uz|) + 3 dv^2
    b["kinetic"] = 0.5 * (e * aux["abs_T"] + 2 * dv * A_u + 3 * M * dv * dv)
    # inertia_ab = sum m d_a d_b: (d_a + dx)(d_b + dx) - d_a d_b <= dx (|d_a| + |d_b|) + dx^2
    b["inertia"] = np.stack([e * aux["abs_I"][k] + 2 * dx * A_d + M * dx * dx for k in range(6)], 1)
    b["potential"] = 0.5 * e * aux["abs_W"]
    # r_max = sqrt(max |d|^2): | |d + dX| - |d| | <= |dX| <= sqrt(3) dx for every member, so for the maxima; r2 carries
    # 1 (d) + 1 (square) + 2 (additions) roundings relative to itself on each side and the root halves them and adds
    # one: (2.5 + 2.5) u r_max <= 8 u r_max
    b["r_max"] = np.sqrt(3.0) * dx + 8 * U * ref["r_max"]
    return b

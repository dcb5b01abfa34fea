"""One reused Barnes-Hut tree driven through every branch of its host state machine (csrc/tree_plan.h: walk plan,
schedule queued beside a build, range walks, counting, walk forms, reshaped node arrays, multipole order), step by step.

sequence() yields one record per observable result; tests/test_tree_sequences_gpu.py compares each with a fresh tree that
was given only the settings in force at that step, tools/tree_parity.py records them (and the host copies of the tree) to
compare two builds of the library bit for bit."""
import numpy as np
import torch

from gpu_util import acc_of

THETA, G, EPS = 0.5, 1.0, 0.02
PAIR_FROM = 98304          # kPairFrom: trees from this many bodies get the even-aligned ids of the pair walk
DEFAULTS = {"depth": 20, "leaf": 1, "order": 1, "form": 0, "count": False}


def apply(tree, s):
    """the settings of `s` on a tree that has the defaults"""
    if (s["depth"], s["leaf"]) != (DEFAULTS["depth"], DEFAULTS["leaf"]):
        tree.setParams(s["depth"], s["leaf"])
    if s["order"] != 1:
        tree.setMultipoleOrder(s["order"])
    if s["form"] != 0:
        tree.walkForm(s["form"])
    if s["count"]:
        tree.countVisits(True)


def walk(tree, d):
    tree.computeForces(d, THETA, G, EPS)
    return acc_of(d)


def range_walks(ctx, tree, n):
    """[0, n/2) and [n/2, n) of the sorted bodies through the packed entry point: (n, 4) rows at the original indices"""
    from nbody_amd._lib import check
    out = torch.full((n, 4), float("nan"), dtype=torch.float32, device="cuda")
    for lo, hi in ((0, n // 2), (n // 2, n)):
        check(ctx._lib.nbody_hip_tree_compute_forces_packed(tree._h, lo, hi - lo, THETA, G, EPS, out.data_ptr()))
    return out.cpu().numpy()


def potential(tree, d, n):
    phi = torch.zeros(n, dtype=torch.float32, device="cuda")
    pe = tree.computePotential(d, THETA, G, EPS, phi)
    return phi.cpu().numpy(), np.float64(pe)


def host_copies(tree, points=None):
    """what the inspection calls hand back after a build (tools/tree_parity.py)"""
    st = tree.stats()
    aligned, ids = tree.idLayout()
    out = {"stats": np.array([st["node_count"], st["nodes_visited"]] + st["level_base"], np.int64),
           "root_mass": np.float32(st["root_mass"]), "id_layout": np.array([int(aligned)] + ids, np.int64),
           "nodes": tree.copyNodesToHost().view(np.uint8), "sorted_indices": tree.sorted_indices_.copy()}
    if tree.getMultipoleOrder() == 2:
        out["moments"] = tree.copyMomentsToHost()
    if points is not None:
        out["field"] = tree.computeField(points, THETA, G, EPS).cpu().numpy()
    return out


def sequence(nb, ctx, d, n, inspect=None):
    """yields (label, settings, kind, arrays): kind "walk" / "ranges" / "potential" hold results a fresh tree with
    `settings` must reproduce, "visits" the node visits of a counted walk, "error" the message of a refused call, "host"
    (only with inspect = the field points) the host copies after a build"""
    s = dict(DEFAULTS)
    tree = nb.BarnesHutTree(n)

    def build(label):
        tree.build(d)
        if inspect is not None:
            yield label + ": host copies", dict(s), "host", host_copies(tree, inspect)

    def walked(label):
        return label, dict(s), "walk", {"acc": walk(tree, d)}

    def counted(label):
        tree.countVisits(True)
        s["count"] = True
        yield walked(label + ", counting")
        yield label + ": node visits", dict(s), "visits", {"visits": np.int64(tree.stats()["nodes_visited"])}
        tree.countVisits(False)
        s["count"] = False

    def refused(label, match):
        try:
            walk(tree, d)
        except nb.StateException as e:
            assert match in str(e), str(e)
            return label, dict(s), "error", {"message": np.array(match)}
        raise AssertionError(label + ": the walk was not refused")

    yield from build("1 build")
    yield walked("2 walk")
    yield walked("3 second walk of the build")
    yield from build("4 build beside the queued schedule")
    yield walked("5 walk")
    yield "6 range walks", dict(s), "ranges", {"acc4": range_walks(ctx, tree, n)}
    yield walked("7 whole walk")
    yield from counted("8 walk")
    tree.walkForm(3)
    s["form"] = 3
    if n < PAIR_FROM:   # the build gave plain ids: the pair walk is refused until a build with the form set
        yield refused("9 form 3 on plain ids", "before the build")
        yield from build("9 build with form 3")
    yield walked("9 form 3")
    yield from counted("9 form 3")
    tree.walkForm(1)
    s["form"] = 1
    yield walked("10 form 1")
    yield from counted("10 form 1")
    tree.walkForm(0)
    tree.setParams(10, 1)
    s.update(form=0, depth=10)
    yield from build("11 build at depth 10")
    yield walked("11 depth 10")
    tree.setParams(20, 1)
    tree.setMultipoleOrder(2)
    s.update(depth=20, order=2)
    yield from build("12 build at order 2")
    yield walked("12 order 2")
    phi, pe = potential(tree, d, n)
    yield "12 potential", dict(s), "potential", {"phi": phi, "pe": pe}
    tree.setMultipoleOrder(1)
    s["order"] = 1
    yield refused("13 order 1 without a rebuild", "rebuild the tree")
    yield from build("14 build")
    yield walked("14 walk")
    tree.close()


def fresh(nb, ctx, d, n, s, kind):
    """the result of `kind` on a new tree given only the settings `s`: one build, one call"""
    tree = nb.BarnesHutTree(n)
    apply(tree, s)
    tree.build(d)
    if kind == "walk":
        out = {"acc": walk(tree, d)}
    elif kind == "ranges":
        out = {"acc4": range_walks(ctx, tree, n)}
    elif kind == "potential":
        phi, pe = potential(tree, d, n)
        out = {"phi": phi, "pe": pe}
    else:
        raise ValueError(kind)
    tree.close()
    return out

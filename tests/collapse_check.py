"""Shared pieces of the BVH2 -> BVH4 collapse's tests (test_collapse_cpu.py, test_gpu_collapse.py, test_gpu_rebuild_bvh4.py): the
scenes and hand-made node arrays the collapse is checked on, and a plain numpy walk of a collapsed tree that gives what the upload
derives from it (live ids, quad records, root entries, stack need, largest leaf).  The walk calls neither implementation."""
import numpy as np

import rebuild_check as RB
import test_groundtruth_cpu as C
from magr_ray_tracer_amd import _lib as W
from magr_ray_tracer_amd.scene import _view
from magr_ray_tracer_amd.scenes import Scene, _std_materials

INV = -1


def raw(a):
    return np.ascontiguousarray(a).view(np.uint8)


def same_bytes(got, want, what):
    assert len(got) == len(want), f"{what}: {len(got)} records, expected {len(want)}"
    if not np.array_equal(raw(got), raw(want)):
        bad = [i for i in range(len(got)) if raw(got[i:i + 1]).tobytes() != raw(want[i:i + 1]).tobytes()]
        raise AssertionError(f"{what}: records {bad[:8]} differ ({len(bad)} of {len(got)})")


# ---- scenes (the reference-exact collapse is Scene.BuildBVH4) --------------------------------------------------------------------------
def soup_scene(counts, seed=0, alpha=1.0, builder="sah"):
    """One BLAS per entry of `counts`, each a random triangle soup in its own corner."""
    s = Scene()
    _std_materials(s)
    rng = np.random.default_rng(seed)
    start = 0
    for k, n in enumerate(counts):
        s.AddTriangles(C._soup(rng, n, 3.0 * k - 1.0, 3.0 * k + 1.0, 0.3), "sand" if k else "white-light")
        if builder == "lbvh":
            s.BuildBLAS(start, builder="lbvh", device=None)
        else:
            s.BuildBLAS(start, alpha=alpha)
        start += n
    return s


def tiny_scene():
    """Three BLAS: a soup, one triangle (its root is a leaf) and two triangles (a leaf root as well)."""
    s = Scene()
    _std_materials(s)
    rng = np.random.default_rng(5)
    s.AddTriangles(C._soup(rng, 60, -1.0, 1.0, 0.3), "sand")
    y = 3.0
    for v in ([(-1, y, -1), (1, y, -1), (1, y, 1)], [(1, y, 1), (-1, y, 1), (-1, y, -1)]):
        s.AddTriangle(*[np.array(p, np.float32) for p in v], "white-light")
    s.BuildBLAS(0)
    s.AddTriangles(C._soup(rng, 1, 1.5, 2.0, 0.3), "green")
    s.BuildBLAS(62)
    s.AddTriangles(C._soup(rng, 2, -2.0, -1.5, 0.3), "red")
    s.BuildBLAS(63)
    return s


SCENES = {
    "1-triangle": lambda: soup_scene([1]), "2-triangles": lambda: soup_scene([2]), "3-triangles": lambda: soup_scene([3]),
    "7-triangles": lambda: soup_scene([7]), "600-triangles": lambda: soup_scene([600]),
    "three-blas-leaf-roots": tiny_scene,
    "four-blas": lambda: soup_scene([40, 9, 70, 5], seed=3),
    "sbvh-alpha0": lambda: soup_scene([150], seed=4, alpha=0.0),
    "lbvh": lambda: soup_scene([200], seed=6, builder="lbvh"),
    "ladder-64": lambda: RB.ladder_scene(-88),
}


def inputs(s):
    """(BVH2 nodes, roots, primIdx slots, the reference-exact BVH4 array) of a Scene."""
    sa = s.arrays(bvh4=True)
    return sa.bvh2, sa.blas["bvhIdx"].astype(np.uint32), len(sa.primIdx), sa.bvh4


def scene_bvh4(s):
    return _view(s._lib.rth_bvh4_nodes, s._h, W.BVHNode4)


def from_nodes(n2):
    """BVH4::Convert + Collapse on hand-made nodes, one BLAS rooted at node 0 (rth_bvh4_from_nodes)."""
    out = np.zeros(len(n2), W.BVHNode4)
    assert W.host_lib().rth_bvh4_from_nodes(W.ptr(n2), len(n2), W.ptr(out)) == 0, W.host_lib().rth_last_error()
    return out


# ---- hand-made BVH2 arrays, one BLAS rooted at node 0 -----------------------------------------------------------------------------------
def _interior(n2, i, first, lo, hi):
    n2["aabbMin"][i][:3], n2["aabbMax"][i][:3] = lo, hi
    n2["first"][i], n2["count"][i] = first, 0


def _leaf(n2, i, first, count, lo=0.0, hi=0.0):
    n2["aabbMin"][i][:3], n2["aabbMax"][i][:3] = lo, hi
    n2["first"][i], n2["count"][i] = first, count


def fixture13():
    """The reference's hand-built 13-node BVH2 (src/bvh.cpp:615-674; tests/test_oracle_cpu.py works its collapse out by hand)."""
    n2 = np.zeros(13, W.BVHNode2)
    for i, first, half in ((0, 1, 20), (1, 3, 9), (2, 5, 12), (3, 7, 8), (6, 9, 10), (9, 11, 9)):
        _interior(n2, i, first, -half, half)
    for k in (4, 5, 7, 8, 10, 11):
        n2["first"][k], n2["count"][k] = k, k
    n2["first"][12], n2["count"][12] = 0, 12
    return n2, 24


def complete(levels, box=lambda i: (-1.0, 1.0)):
    """A complete BVH2 of `levels` interior levels in pair order (children of the r-th interior node at 2r + 1, 2r + 2), one-primitive
    leaves; box(i) gives node i's (lo, hi)."""
    interiors = 2 ** levels - 1
    n2 = np.zeros(2 * interiors + 1, W.BVHNode2)
    slot = 0
    for i in range(len(n2)):
        lo, hi = box(i)
        if i < interiors:
            _interior(n2, i, 2 * i + 1, lo, hi)
        else:
            _leaf(n2, i, slot, 1, lo, hi)
            slot += 1
    return n2, slot


def lattice():
    """Every box identical: every area ties and only "the first of equal areas wins" decides."""
    return complete(5)


def nan_child():
    """Node 1 (an interior child of the root) has a NaN extent: its area is NaN, it is never absorbed, and it survives with two slots."""
    def box(i):
        return (-1.0, np.nan) if i == 1 else (-1.0 - 0.01 * i, 1.0 + 0.01 * i)
    return complete(4, box)


def unreachable():
    """fixture13 with three more records that no root leads to: an interior one (converted too) and its two leaves."""
    n2, n_idx = fixture13()
    more = np.zeros(3, W.BVHNode2)
    _interior(more, 0, 14, -3.0, 3.0)
    _leaf(more, 1, 1, 2, -1.0, 1.0)
    _leaf(more, 2, 3, 4, -2.0, 2.0)
    return np.concatenate([n2, more]), n_idx


def deep_chain(h):
    """A BVH2 caterpillar of height h (interior N_k at 2k - 1, its leaf sibling at 2k; N_0 = node 0)."""
    n2 = np.zeros(2 * h + 1, W.BVHNode2)
    at = lambda k: 0 if k == 0 else 2 * k - 1
    for k in range(h):
        _interior(n2, at(k), 2 * k + 1, -1.0 - k, 1.0 + k)
        _leaf(n2, 2 * k + 2, k, 1)
    _leaf(n2, at(h), h, 1)
    return n2, h + 1


def comb2(levels):
    """A BVH2 whose collapse is capacity_check's BVH4 comb: level node X = (A, B), A = (S1, S2), B = (S3, Y) with Y the next level
    (the last level: B = (S3, S4)); every S a stub of two one-primitive leaves.  The boxes are written so that area(A) > area(B) >
    area(S): X absorbs A, then B, and is full as (S1, S3, S2, Y) - three stubs pending under the next level, which sits in the last
    slot: a stack need of 3 (levels - 1) + 4."""
    nodes, slot = [], [0]

    def new(n=1):
        nodes.extend([None] * n)
        return len(nodes) - n

    def stub(i):
        c = new(2)
        nodes[i] = ("i", c, 1.0)
        for k in range(2):
            nodes[c + k] = ("l", slot[0], 0.5)
            slot[0] += 1

    def level(x, l):
        c = new(2)
        nodes[x] = ("i", c, 10.0 if l else 20.0)
        a, b = c, c + 1
        ca, cb = new(2), new(2)
        nodes[a], nodes[b] = ("i", ca, 9.0), ("i", cb, 8.0)
        stub(ca), stub(ca + 1), stub(cb)
        if l + 1 < levels:
            level(cb + 1, l + 1)
        else:
            stub(cb + 1)

    level(new(), 0)
    n2 = np.zeros(len(nodes), W.BVHNode2)
    for i, (kind, first, half) in enumerate(nodes):
        if kind == "i":
            _interior(n2, i, first, -half, half)
        else:
            _leaf(n2, i, first, 1, -half, half)
    return n2, slot[0]


HAND = {"fixture13": fixture13, "lattice": lattice, "nan-child": nan_child, "unreachable": unreachable,
        "comb2(3)": lambda: comb2(3), "comb2(21)": lambda: comb2(21)}


# ---- the numpy walk ----------------------------------------------------------------------------------------------------------------------
def recursive_collapse(n2, roots):
    """BVH4::Convert / Collapse restated in Python (accel_build.cpp): every root in turn, a root named twice collapsed twice; float32
    areas in the reference's order.  (The recursion into the surviving children is a work list: they do not depend on each other.)"""
    n = len(n2)
    q = np.zeros(n, W.BVHNode4)
    for i in range(n):
        if n2["count"][i] > 0:
            continue
        for k in range(2):
            c = int(n2["first"][i]) + k
            q["aabbMin"][i][k], q["aabbMax"][i][k] = n2["aabbMin"][c], n2["aabbMax"][c]
            q["first"][i][k], q["count"][i][k] = (n2["first"][c], n2["count"][c]) if n2["count"][c] > 0 else (c, 0)
        q["first"][i][2:], q["count"][i][2:] = INV, INV

    def kids(i):
        c = 0
        while c < 4 and q["count"][i][c] != INV:
            c += 1
        return c

    def collapse(i):
        work = [i]
        while work:
            i = work.pop()
            while True:
                cnt, best, pick = kids(i), np.float32(-np.inf), INV
                for k in range(cnt):
                    if q["count"][i][k] > 0 or not (cnt - 1 + kids(int(q["first"][i][k])) <= 4):
                        continue
                    d = (q["aabbMax"][i][k] - q["aabbMin"][i][k]).astype(np.float32)
                    with np.errstate(all="ignore"):
                        half = np.float32(np.float32(np.float32(d[0] * d[1]) + np.float32(d[1] * d[2])) + np.float32(d[2] * d[0]))
                    if half > best:
                        best, pick = half, k
                if pick == INV:
                    break
                ch = q[int(q["first"][i][pick])].copy()
                nc = 0
                while nc < 4 and ch["count"][nc] != INV:
                    nc += 1
                for f in ("aabbMin", "aabbMax", "first", "count"):
                    q[f][i][pick] = ch[f][0]
                    for k in range(1, nc):
                        q[f][i][cnt - 1 + k] = ch[f][k]
            work += [int(q["first"][i][k]) for k in range(4) if q["count"][i][k] == 0 and q["first"][i][k] != INV]

    for root in roots:
        root = int(root)
        if n2["count"][root] > 0:
            q["aabbMin"][root][0], q["aabbMax"][root][0] = n2["aabbMin"][root], n2["aabbMax"][root]
            q["first"][root][0], q["count"][root][0] = n2["first"][root], n2["count"][root]
            q["first"][root][1:], q["count"][root][1:] = INV, INV
        else:
            collapse(root)
    return q


def walk(n4, roots, n_idx):
    """What the upload derives from a collapsed tree, by a breadth-first walk BLAS by BLAS in the order in which the roots are first
    named: {order (live id -> node), entry (per root), quads (live, 8, 4) float32, live_nodes, levels, stack_need, largest_leaf}."""
    new_id, order, levels, need, leaf = {}, [], 0, 0, 0
    for root in roots:
        root = int(root)
        if root in new_id:
            continue
        front, l = [(root, 0)], 0
        while front:
            nxt = []
            for node, base in front:
                new_id[node] = len(order)
                order.append(node)
                j = 0
                for k in range(4):
                    f, c = int(n4["first"][node][k]), int(n4["count"][node][k])
                    if f == INV:
                        continue
                    if c > 0:
                        leaf = max(leaf, c)
                    else:
                        nxt.append((f, base + j))
                        j += 1
                need = max(need, base + j)
            l += 1
            front = nxt
        levels = max(levels, l)
    quads = np.zeros((len(order), 8, 4), np.float32)
    bits = quads.view(np.uint32)
    for q, node in enumerate(order):
        b = np.zeros(24, np.float32)
        for k in range(4):
            b[k * 6:k * 6 + 3], b[k * 6 + 3:k * 6 + 6] = n4["aabbMin"][node][k][:3], n4["aabbMax"][node][k][:3]
            f, c = int(n4["first"][node][k]), int(n4["count"][node][k])
            bits[q, 6, k] = 0xffffffff if f == INV else ((0x80000000 | (c << 24) | f) if c > 0 else new_id[f])
        quads[q, :6] = b.reshape(6, 4)
    return dict(order=np.array(order, np.uint32), entry=np.array([new_id[int(r)] for r in roots], np.uint32), quads=quads,
                live_nodes=len(order), levels=levels, stack_need=need, largest_leaf=leaf)


def check_derived(stats, quads, entry, qnode, want, what):
    for k in ("live_nodes", "levels", "stack_need", "largest_leaf"):
        assert stats[k] == want[k], f"{what}: {k} = {stats[k]}, the walk says {want[k]}"
    assert np.array_equal(qnode, want["order"]) and np.array_equal(entry, want["entry"]), f"{what}: live ids differ"
    same_bytes(quads, want["quads"], f"{what}: quads")

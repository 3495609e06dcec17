"""Shared pieces of the per-range rebuild's tests (test_ranges_cpu.py, test_gpu_ranges.py): one scene of three distinct BLAS of 1, 37
and 220 primitives under four instances, built twice by the same calls as refit_check builds its scenes - once as bound, once with a
deformation (refit_check's: deform(kind, b, value)) - and the host restatement of a rebuild under a plan (Scene.RebuildRanges)."""
import numpy as np

import rebuild_check as RB
import refit_check as R
import test_groundtruth_cpu as C
from magr_ray_tracer_amd import _lib as W
from magr_ray_tracer_amd import scene as SC
from magr_ray_tracer_amd.scenes import Scene, _std_materials

COUNTS = (1, 37, 220)                         # primitives of the three BLAS, in range order
FIRST = (0, 1, 38)
X_OF = {"sah": "sah", "lbvh": "lbvh", "sbvh": "sbvh_gpu"}   # the plan word that builds what a first build of RB.FIRST_BUILDS built
SHIFT = C.invT(np.eye(3), (1.4, -0.6, 0.5))   # the second instance of BLAS 0
VIEW = dict(origin=(0.1, 0.6, 10.0), forward=(0.0, 0.05, 1.0), fov=64.0, aperture=0.01)


def scene(deform=R.identity, first_build="sah"):
    """BLAS 0: one light triangle (its root is a leaf: one node, no interior).  BLAS 1: 35 triangles and 2 spheres.  BLAS 2: 220
    triangles.  Instances, in this order: BLAS 2, BLAS 1 under RB.ROT, BLAS 0, BLAS 0 again under SHIFT - so the instances name the
    BLAS in another order than the ranges, which is the order pair ids go by.  The random draws do not depend on `deform`."""
    alpha, b0 = RB.FIRST_BUILDS[first_build]
    rng = np.random.default_rng(11)
    s = Scene()
    _std_materials(s)

    def blas(start):
        if b0 == "lbvh":
            s.BuildBLAS(start, builder="lbvh", device=None)
        else:
            s.BuildBLAS(start, alpha=alpha)

    y = 4.2
    v = deform("light", 0, np.array([(-1.5, y, -1.5), (1.5, y, -1.5), (0.0, y, 1.5)], np.float32))
    s.AddTriangle(v[0], v[1], v[2], "white-light")
    blas(FIRST[0])
    c = np.array(R.CENTRES[1])
    s.AddTriangles(deform("tris", 1, C._soup(rng, 35, c - 1.2, c + 1.2, 0.45)), "green")
    for k in range(2):
        pos, r = c + rng.uniform(-1.0, 1.0, 3), float(rng.uniform(0.2, 0.45))
        pos, r = deform("sphere", 1, (pos, r))
        s.AddSphere(pos, r, "mirror" if k else "red")
    blas(FIRST[1])
    c = np.array(R.CENTRES[0])
    s.AddTriangles(deform("tris", 2, C._soup(rng, 220, c - 1.6, c + 1.6, 0.3)), "sand")
    blas(FIRST[2])
    s.SetInstanceTransform(1, RB.ROT)
    s.AddInstance(0, SHIFT)
    s.SwapInstances(0, 2)
    return s


def only(r, deform):
    """`deform` applied to BLAS r alone."""
    return lambda kind, b, x: deform(kind, b, x) if b == r else x


def squash(factor):
    """Every triangle of a soup scaled about its own centroid: small triangles sit apart, large ones overlap - the builders' leaf
    sizes, and with them the node counts, follow."""
    def d(kind, b, x):
        if kind == "tris":
            m = x.mean(axis=1, keepdims=True)
            return (m + (x - m) * np.float32(factor)).astype(np.float32)
        return x
    return d


def ranges(sa):
    """The distinct BLAS ranges [(first, count)] in increasing order."""
    return sorted(set(SC.blas_ranges(sa)))


def blocks(sa):
    """[(root, nodes, idxLo, idxSlots)] of the distinct BLAS in range order, walked from the roots (all of them compact: asserted)."""
    n, out = sa.bvh2, {}
    for (first, _), root in zip(SC.blas_ranges(sa), sa.blas["bvhIdx"]):
        ids, leaves, st = [], [], [int(root)]
        while st:
            i = st.pop()
            ids.append(i)
            if n["count"][i] > 0:
                leaves.append((int(n["first"][i]), int(n["count"][i])))
            else:
                st += [int(n["first"][i]), int(n["first"][i]) + 1]
        leaves.sort()
        assert sorted(ids) == list(range(int(root), int(root) + len(ids))) and len(ids) % 2 == 1, "the nodes are not one block"
        assert all(a[0] + a[1] == b[0] for a, b in zip(leaves, leaves[1:])), "the leaves do not tile one interval"
        out[first] = (int(root), len(ids), leaves[0][0], sum(c for _, c in leaves))
    return [out[k] for k in sorted(out)]


def check_wire(sa):
    """The wire arrays are what appending BLAS after BLAS gives: the blocks of nodes and of index slots tile both arrays in range order,
    every slot of a BLAS names a primitive of its range and every primitive of the range is named."""
    node, slot = 0, 0
    for (root, m, lo, s), (first, count) in zip(blocks(sa), ranges(sa)):
        assert (root, lo) == (node, slot), ((root, lo), (node, slot))
        ids = sa.primIdx[lo:lo + s]
        assert ids.min() == first and ids.max() == first + count - 1 and len(np.unique(ids)) == count
        node, slot = node + m, slot + s
    assert node == len(sa.bvh2) and slot == len(sa.primIdx)
    RB.validate(sa)


def host_ranges(s, plan, prims=None, first=0, inst=None, bvh4=False, **options):
    """The host restatement of rt_rebuild_ranges on Scene `s` (SetPrimitives + the transforms + RebuildRanges + BuildTLAS); its arrays."""
    if prims is not None:
        s.SetPrimitives(first, prims)
    if inst is not None:
        for b, r in enumerate(inst):
            s.SetInstanceTransform(b, r["invT"].reshape(4, 4))
    s.RebuildRanges(plan, **options)
    return s.arrays(bvh4=bvh4)


def ranges_check(n_prims, rng_list, plan, first=0, count=0, compact=None, n_ranges=None, **options):
    """rt_rebuild_ranges_check; returns (code, message)."""
    L = W.device_lib()
    rf = np.array([a for a, _ in rng_list], np.int32)
    rc_ = np.array([b for _, b in rng_list], np.int32)
    cp = None if compact is None else np.array(compact, np.int32)
    words = None if plan is None else np.array([SC.PLAN_WORDS.get(w, w) for w in plan], np.int32)
    opts = SC.build_options(**options)
    rc = L.rt_rebuild_ranges_check(n_prims, W.ptr(rf), W.ptr(rc_), None if cp is None else W.ptr(cp), len(rng_list),
                                   None if words is None else W.ptr(words), (0 if words is None else len(words)) if n_ranges is None else n_ranges,
                                   first, count, W.ptr(opts))
    return rc, L.rt_last_error().decode()

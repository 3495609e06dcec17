"""Odd but legal scenes: hand-made wire arrays that the builders do not emit, that rt_validate_scene accepts and whose access audit
(wire_audit.py) is empty.  test_validate_cpu.py holds each to that, and to the float64 ground truth through the oracle;
test_gpu_validate.py runs each on every traversal path that applies.

Every entry starts from a scene of the repository's builders whose primitives went through geom64.GTScene (which gives the float64
ground truth its primitive sets), then rewrites node arrays, indices or counts by hand.  The ground truth follows the primitives
alone, so it does not care how the arrays reach them - only which instance sees which set.

  bvh4-holes            unused BVH4 slots in every position: the slots of node i are rotated by i % 4 (slot 0 unused with slot 2 used
                        occurs)
  leaf-127 / leaf-128   a BVH2 leaf / BVH4 leaf slot of 127 primitives (the largest packed entry) and of 128 (layout 0 for all)
  shared-subtree        a BVH2 ladder of three levels in which both nodes of a level name the SAME pair of children: 7 nodes, every
                        leaf reached over 4 paths, 15 visits - inside bvh2_depth's budget of 2 * nNodes + 2 = 16
  unreachable-zeros     all-zero records behind the last BVH node (both accels) and behind the last TLAS node
  tlas-leaf-root        a one-node TLAS whose root is a leaf naming instance 1 of 2: the single-BLAS fast path through one_instance
  two-on-one-root       three instances, two of them on one BLAS root, under a hand-written TLAS
  leaf-root-blas        a BLAS whose root is a leaf (one triangle) beside two ordinary ones
  primidx-repeats       a leaf whose primIdx range names each of its primitives twice (appended behind the builder's indices)
  lights-duplicate      the first light listed twice
  no-lights             nLights = 0 under next-event estimation
  texture-1x1           a 1 x 1 texture at texIdx 0"""
import copy
from dataclasses import dataclass

import numpy as np

import capacity_check as CC
import geom64 as G
import test_groundtruth_cpu as C
from magr_ray_tracer_amd import _lib as W
from magr_ray_tracer_amd.scenes import Scene, _std_materials, box_tris

B2, B4 = W.ACCEL_BVH2, W.ACCEL_BVH4


@dataclass
class Entry:
    name: str
    gt: object
    sa: object
    kind: str                    # "one": the TLAS root is a leaf; "multi": a TLAS walk (test_gpu_groundtruth.CASES)
    accels: tuple
    view: dict = None            # a camera: frames apply; None: `rays` only
    rays: np.ndarray = None      # extend rays of the capacity trees
    layout0_only: bool = False   # a leaf too large for the packed entry: every variant runs layout 0


def _regt(gt, sa, sets=None):
    """The ground truth of the same primitives behind other arrays (sets: which primitive set each instance of sa.blas sees)."""
    g = copy.copy(gt)
    g.sa, g.sets, g._cache = sa, list(gt.sets if sets is None else sets), {}
    return g


def _with(sa, **arrays):
    s = copy.copy(sa)
    for k, v in arrays.items():
        setattr(s, k, v)
    return s


_EMPTY = dict(tri=np.zeros((0, 3, 3)), tri_idx=np.zeros(0, np.int64), sph_c=np.zeros((0, 3)), sph_r=np.zeros(0), sph_idx=np.zeros(0, np.int64))
VIEW = dict(origin=(0.2, 0.3, 9.0), forward=(0.0, 0.0, 1.0), fov=62.0, aperture=0.01)


def _one(extra_blas=(), transforms=()):
    """A 140-triangle soup, a light with its wall and occluder, a closed room: one BLAS (nearly every ray hits: long bounce queues).
    extra_blas: further BLAS, each a function adding its primitives; transforms: (instance, invT)."""
    rng = np.random.default_rng(19)
    gt = G.GTScene(Scene())
    _std_materials(gt.s)
    gt.triangles(C._soup(rng, 140, -3, 3, 0.5), "sand")
    C._lights_and_walls(gt, 4.2)
    gt.triangles(box_tris((-6, -5, -6), (6, 6, 11)), "white")
    gt.build_blas(1.0)
    for add in extra_blas:
        add(gt, rng)
        gt.build_blas(1.0)
    for b, T in transforms:
        gt.s.SetInstanceTransform(b, T)
    return gt, gt.finish()


def _second(gt, rng):
    gt.triangles(C._soup(rng, 90, (-2, -3.5, 2), (2, -1, 6), 0.45), "green")


def _single_triangle(gt, rng):
    gt.triangles(np.array([[(-2.5, -2, 7), (2.5, -2, 7), (0, 2.5, 7)]], np.float32), "red")


def _multi():
    return _one((_second,), [(1, C.invT(C.rot(1, 17.0), (0.2, -0.1, 0.3)))])


def _tlas_leaves(sa):
    """instance -> the TLAS leaf record that names it, of the nodes reachable from the root."""
    out, todo = {}, [0]
    while todo:
        i = todo.pop()
        lr = int(sa.tlas["leftRight"][i])
        if lr == 0:
            out[int(sa.tlas["BLASidx"][i])] = sa.tlas[i]
        else:
            todo += [lr & 0xffff, lr >> 16]
    return out


# ---- the entries ------------------------------------------------------------------------------------------------------------------------
def bvh4_holes():
    gt, sa = _one()
    n = sa.bvh4.copy()
    for i in range(len(n)):
        for f in ("aabbMin", "aabbMax", "first", "count"):
            n[f][i] = np.roll(sa.bvh4[f][i], i % 4, axis=0)
    used = n["first"] != -1
    assert (~used[:, 0] & used[:, 2]).any() and all((~used[:, k]).any() and used[:, k].any() for k in range(4))
    return Entry("bvh4-holes", _regt(gt, sa), _with(sa, bvh4=n), "one", (B4,), VIEW)


def fat_leaf(m):
    c = CC.chain(5, fat=m)
    return Entry(f"leaf-{m}", c.gt, c.sa, "one", (B2, B4), rays=c.rays, layout0_only=m > CC.LEAF_MAX)


def _box_of(prims):
    v = np.concatenate([prims["v0"][:, :3], prims["v1"][:, :3], prims["v2"][:, :3]])
    return v.min(0) - 1e-3, v.max(0) + 1e-3


def shared_ladder(levels, gt=None, sa=None):
    """BVH2 of 2 * levels + 1 nodes: node 0 -> (1, 2); both nodes of a level name the next level's pair; the last pair are leaves over
    the two halves of the primitives.  1 + 2 + ... + 2^levels visits."""
    if gt is None:
        gt, sa = _one()
    assert (sa.prims["objType"] == W.PRIM_TRIANGLE).all()
    n = np.zeros(2 * levels + 1, W.BVHNode2)
    half = len(sa.prims) // 2
    lo, hi = _box_of(sa.prims)
    n["aabbMin"][:, :3], n["aabbMax"][:, :3] = lo, hi
    for i in range(2 * levels - 1):
        n["first"][i], n["count"][i] = (1 if i == 0 else 2 * ((i + 1) // 2) + 1), 0
    for k, (f, c) in enumerate(((0, half), (half, len(sa.prims) - half))):
        i = 2 * levels - 1 + k
        n["first"][i], n["count"][i] = f, c
        n["aabbMin"][i][:3], n["aabbMax"][i][:3] = _box_of(sa.prims[f:f + c])
    blas = sa.blas.copy()
    blas["bvhIdx"][0] = 0
    out = _with(sa, bvh2=n, primIdx=np.arange(len(sa.prims), dtype=np.uint32), blas=blas)
    return Entry(f"shared-subtree({levels})", _regt(gt, out), out, "one", (B2,), VIEW)


def unreachable_zeros():
    gt, sa = _multi()
    out = _with(sa, bvh2=np.concatenate([sa.bvh2, np.zeros(2, W.BVHNode2)]), bvh4=np.concatenate([sa.bvh4, np.zeros(2, W.BVHNode4)]),
                tlas=np.concatenate([sa.tlas, np.zeros(2, W.TLASNode)]))
    return Entry("unreachable-zeros", _regt(gt, out), out, "multi", (B2, B4), VIEW)


def tlas_leaf_root():
    gt, sa = _multi()
    t = np.array([_tlas_leaves(sa)[1]], W.TLASNode)
    out = _with(sa, tlas=t)
    view = dict(origin=(0.0, -2.0, 9.5), forward=(0.0, 0.0, 1.0), fov=50.0, aperture=0.01)
    return Entry("tlas-leaf-root", _regt(gt, out, [_EMPTY, gt.sets[1]]), out, "one", (B2, B4), view)


def two_on_one_root():
    gt, sa = _multi()
    shift = np.array([0.0, 2.2, -1.5])
    blas = np.concatenate([sa.blas, sa.blas[1:2]])
    T = blas["invT"][2].reshape(4, 4).copy()
    T[:3, 3] -= T[:3, :3] @ shift.astype(np.float32)         # p' = A (p - shift) + t
    blas["invT"][2] = T.ravel()
    leaf = _tlas_leaves(sa)
    t = np.zeros(5, W.TLASNode)
    t[1], t[2] = leaf[0], leaf[1]
    t[3] = leaf[1]
    t["BLASidx"][3] = 2
    t["aabbMin"][3][:3] = leaf[1]["aabbMin"][:3] + shift - 1e-3
    t["aabbMax"][3][:3] = leaf[1]["aabbMax"][:3] + shift + 1e-3
    for i, (a, b) in ((4, (2, 3)), (0, (1, 4))):
        t["leftRight"][i] = a | (b << 16)
        t["aabbMin"][i][:3] = np.minimum(t["aabbMin"][a][:3], t["aabbMin"][b][:3])
        t["aabbMax"][i][:3] = np.maximum(t["aabbMax"][a][:3], t["aabbMax"][b][:3])
    out = _with(sa, blas=blas, tlas=t)
    assert blas["bvhIdx"][1] == blas["bvhIdx"][2]
    return Entry("two-on-one-root", _regt(gt, out, [gt.sets[0], gt.sets[1], gt.sets[1]]), out, "multi", (B2, B4), VIEW)


def leaf_root_blas():
    gt, sa = _one((_second, _single_triangle))
    root = int(sa.blas["bvhIdx"][2])
    assert sa.bvh2["count"][root] == 1 and len(sa.blas) == 3
    return Entry("leaf-root-blas", gt, sa, "multi", (B2, B4), VIEW)


def primidx_repeats():
    gt, sa = _one()
    i = int(np.where(sa.bvh2["count"] > 1)[0][0])
    f, c = int(sa.bvh2["first"][i]), int(sa.bvh2["count"][i])
    idx = np.concatenate([sa.primIdx, np.repeat(sa.primIdx[f:f + c], 2)])
    n2, n4 = sa.bvh2.copy(), sa.bvh4.copy()
    n2["first"][i], n2["count"][i] = len(sa.primIdx), 2 * c
    slot = (sa.bvh4["first"] == f) & (sa.bvh4["count"] == c)
    assert slot.any()
    n4["first"][slot], n4["count"][slot] = len(sa.primIdx), 2 * c
    out = _with(sa, bvh2=n2, bvh4=n4, primIdx=idx)
    return Entry("primidx-repeats", _regt(gt, out), out, "one", (B2, B4), VIEW)


def lights_duplicate():
    gt, sa = _one()
    out = _with(sa, lights=np.concatenate([sa.lights, sa.lights[:1]]))
    return Entry("lights-duplicate", _regt(gt, out), out, "one", (B2, B4), VIEW)


def no_lights():
    gt, sa = _one()
    out = _with(sa, lights=np.zeros(0, np.uint32))
    return Entry("no-lights", _regt(gt, out), out, "one", (B2, B4), VIEW)


def texture_1x1():
    gt, sa = _one()
    mats = sa.mats.copy()
    m = int(sa.prims["matIdx"][0])                            # the soup's material
    mats["texIdx"][m], mats["texW"][m], mats["texH"][m] = 0, 1, 1
    out = _with(sa, mats=mats, tex=np.array([[0.3, 0.6, 0.9, 0.0]], np.float32))
    return Entry("texture-1x1", _regt(gt, out), out, "one", (B2, B4), VIEW)


CATALOGUE = {
    "bvh4-holes": bvh4_holes, "leaf-127": lambda: fat_leaf(127), "leaf-128": lambda: fat_leaf(128), "shared-subtree": lambda: shared_ladder(3),
    "unreachable-zeros": unreachable_zeros, "tlas-leaf-root": tlas_leaf_root, "two-on-one-root": two_on_one_root,
    "leaf-root-blas": leaf_root_blas, "primidx-repeats": primidx_repeats, "lights-duplicate": lights_duplicate, "no-lights": no_lights,
    "texture-1x1": texture_1x1,
}
_BUILT = {}


def entry(name):
    if name not in _BUILT:
        _BUILT[name] = CATALOGUE[name]()
    return _BUILT[name]

"""BVH2 trees built by hand over a handful of triangles, and rays against them (shared by test_gpu_top_descent.py, anyhit_check.py and
the modules that use it).

Primitive 0 is a floor triangle in the plane y = 0, primitive 1 a light above it that faces down, the others stand in a row along x.
Two placements of the light and the row:

row_prims    light in the plane y = 2, the row beside the floor (x >= 6) at y in [2, 3].  A shadow ray from the floor to the light starts
             above the floor's (flat) box and ends below the plane y = 2 that bounds every other box from below: where the root's two
             children are the floor and everything else it misses both - a ray finished at the root with tmax shorter than the entry
             distance.  No shadow ray of this placement is occluded.
slat_prims   light in the plane y = 4, the row OVER the floor (x = 1, 1.75, 2.5, ...) at y in [2, 3]: slats between floor and light, so
             that the shadow rays of floor points behind them are occluded and the others are not."""
import dataclasses

import numpy as np

import geom64 as G
from magr_ray_tracer_amd import _lib as W
from magr_ray_tracer_amd.scenes import Scene, _std_materials

FLOOR = [(-4, 0, -4), (4, 0, 4), (4, 0, -4)]


def _row(x0, dx, n):
    """Triangle k of the row: base (x, 2, -1) - (x, 2, 1), apex (x + 0.25, 3, 0) with x = x0 + k dx.  The line y = 2.5, z = 0 crosses it
    at x + 0.125 (u = 0.5, v = 0.25); the line y = 2.5, z = 0.9 passes its box but misses it (u + v = 1.2)."""
    return [[(x0 + dx * k, 2, -1), (x0 + dx * k + 0.25, 3, 0), (x0 + dx * k, 2, 1)] for k in range(n)]


def row_prims(n):
    t = [FLOOR, [(-0.5, 2, -0.5), (0.5, 2, -0.5), (0.5, 2, 0.5)]] + _row(6.0, 1.5, max(n - 2, 0))
    return np.array(t[:n], np.float32)


def slat_prims(n):
    t = [FLOOR, [(-0.5, 4, -0.5), (0.5, 4, -0.5), (0.5, 4, 0.5)]] + _row(1.0, 0.75, max(n - 2, 0))
    return np.array(t[:n], np.float32)


def hand_scene(n, tree, prims=row_prims):
    """n primitives under the BVH2 `tree`: a list of primitive ids is a leaf, a pair (left, right) an interior node.  Nodes as BVH2's
    builders lay them out (root 0, node 1 unused, the two children of a node side by side), boxes from the vertices.  A primitive may
    sit in more than one leaf (as under an SBVH)."""
    tris = prims(n)
    s = Scene()
    _std_materials(s)
    s.AddTriangles(tris[:1], "sand")
    if n > 1:
        s.AddTriangles(tris[1:2], "white-light")
    if n > 2:
        s.AddTriangles(tris[2:], "green")
    s.BuildBLAS(0)
    sa = s.arrays()
    nodes, idx = [None, None], []

    def fill(at, t):
        nd = np.zeros((), W.BVHNode2)
        if isinstance(t, list):
            nd["first"], nd["count"] = len(idx), len(t)
            idx.extend(t)
            v = tris[t].reshape(-1, 3)
        else:
            k = len(nodes)
            nodes.extend([None, None])
            nd["first"], nd["count"] = k, 0
            v = np.concatenate([fill(k, t[0]), fill(k + 1, t[1])])
        nd["aabbMin"][:3], nd["aabbMax"][:3] = v.min(0), v.max(0)
        nodes[at] = nd
        return v

    fill(0, tree)
    nodes[1] = np.zeros((), W.BVHNode2)
    bvh2 = np.array(nodes, dtype=W.BVHNode2)
    assert int(sa.blas["bvhIdx"][0]) == 0 and len(sa.blas) == 1
    assert np.array_equal(bvh2["aabbMin"][0], sa.bvh2["aabbMin"][0]) and np.array_equal(bvh2["aabbMax"][0], sa.bvh2["aabbMax"][0])
    return dataclasses.replace(sa, bvh2=bvh2, primIdx=np.array(idx, np.uint32))


def ladder(ids):
    """Every interior node has one leaf child and one interior child, the leaf on alternating sides; the last one two leaves."""
    t = ([ids[-2]], [ids[-1]])
    for k, i in enumerate(reversed(ids[:-2])):
        t = ([i], t) if k % 2 else (t, [i])
    return t


def balanced(ids):
    return list(ids) if len(ids) == 1 else (balanced(ids[:len(ids) // 2]), balanced(ids[len(ids) // 2:]))


def tree(name, L):
    if name == "one-triangle":
        return 1, [0]
    if name == "two-triangles":
        return 2, ([0], [1])
    if name == "ladder-8":                     # eight interior nodes, one per level; root = (floor, everything else)
        return 9, ([0], ladder(list(range(1, 9))))
    d = L + {"depth-L-1": -1, "depth-L": 0, "depth-L+1": 1}[name]
    return 1 << d, balanced(list(range(1 << d)))      # complete: d levels of interior nodes over 2^d single-triangle leaves


def hand_rays(n):
    """Rays against the row_prims scenes: away from everything (both root children missed), down at the floor (one child; their shadow
    rays run to the light), along the row from either end and across it (both children, far child pushed and popped later), random."""
    rng = np.random.default_rng(17)
    xmax = 6.0 + 1.5 * max(n - 2, 1)
    O, D = [], []
    k = 160
    O.append(np.c_[rng.uniform(-4, xmax, k), np.full(k, 5.0), rng.uniform(-1, 1, k)]); D.append(np.tile([0.0, 1.0, 0.0], (k, 1)) + rng.normal(scale=0.2, size=(k, 3)))
    P = np.c_[rng.uniform(-3.5, 3.5, 3 * k), np.zeros(3 * k), rng.uniform(-3.5, 3.5, 3 * k)]
    o = np.c_[rng.uniform(-3, 3, 3 * k), np.full(3 * k, 6.0), rng.uniform(-3, 3, 3 * k)]
    O.append(o); D.append(P - o)
    for x0, sx in ((-5.0, 1.0), (xmax + 3.0, -1.0)):
        o = np.c_[np.full(k, x0), rng.uniform(2.0, 3.0, k), rng.uniform(-1, 1, k)]
        O.append(o); D.append(np.c_[np.full(k, sx), rng.normal(scale=0.03, size=k), rng.normal(scale=0.03, size=k)])
    o = np.c_[rng.uniform(-4, xmax, 2 * k), rng.uniform(3.5, 6, 2 * k), rng.uniform(-3, 3, 2 * k)]
    t = np.c_[rng.uniform(-4, xmax, 2 * k), rng.uniform(0, 3, 2 * k), rng.uniform(-1, 1, 2 * k)]
    O.append(o); D.append(t - o)
    o = rng.uniform([-6, -1, -5], [xmax + 2, 7, 5], (4 * k, 3))
    O.append(o); D.append(rng.normal(size=(4 * k, 3)))
    O, D = np.concatenate(O), np.concatenate(D)
    return G.make_rays(O, D / np.linalg.norm(D, axis=1)[:, None])


def floor_rays(n, seed=29):
    """n rays from above to points inside the floor triangle: nearly every one of them sends a shadow ray to the light."""
    rng = np.random.default_rng(seed)
    u, v = rng.uniform(0.03, 0.94, n), rng.uniform(0.03, 0.94, n)
    over = u + v > 0.97
    u[over], v[over] = 0.97 - v[over], 0.97 - u[over]
    A, B, Cc = np.array([-4.0, 0, -4]), np.array([4.0, 0, 4]), np.array([4.0, 0, -4])
    P = A + u[:, None] * (B - A) + v[:, None] * (Cc - A)
    o = P + np.c_[rng.uniform(-1, 1, n), np.full(n, 6.0), rng.uniform(-1, 1, n)]
    D = P - o
    return G.make_rays(o, D / np.linalg.norm(D, axis=1)[:, None])

"""Shared pieces of the BVH4 refit's tests (test_refit_bvh4_cpu.py, test_gpu_refit_bvh4.py): the host restatement of the in-place
collapse (rth_bvh4_refit) around numpy arrays, deformations of a Scene's primitives, and the two named fixtures the GPU tests render:
`keep` (the same deformation applied twice: the second refit finds identical boxes, so it is in place by construction) and `flip` (a
hand-made two-cluster soup in which scaling one cluster swaps which child the root absorbs first, so slots change)."""
import ctypes as C_

import numpy as np

import collapse_check as K
import refit_check as R
import test_groundtruth_cpu as C
from magr_ray_tracer_amd import _lib as W
from magr_ray_tracer_amd.scene import BuildError, build_bvh4_gpu
from magr_ray_tracer_amd.scenes import Scene, _std_materials


def collapse(n2, roots, n_idx):
    """The level-wise collapse on the host: (BVHNode4 array, stats, live id -> node)."""
    n4, st, _, _, qnode = build_bvh4_gpu(n2, roots, n_idx, device=None, derived=True)
    return n4.copy(), st, qnode


def bvh4_refit(n2_refit, roots, n_idx, n4_bound, qnode):
    """rth_bvh4_refit on copies: (the new BVHNode4 array, changedNodes)."""
    L = W.host_lib()
    n2 = np.ascontiguousarray(n2_refit, W.BVHNode2)
    r = np.ascontiguousarray(roots, np.uint32)
    q = np.ascontiguousarray(qnode, np.uint32)
    out = np.ascontiguousarray(n4_bound, W.BVHNode4).copy()
    changed = C_.c_int32(-1)
    rc = L.rth_bvh4_refit(W.ptr(n2), len(n2), int(n_idx), W.ptr(r), len(r), W.ptr(out), W.ptr(q), len(q), C_.byref(changed))
    if rc != 0:
        raise BuildError(rc, L.rth_last_error().decode())
    return out, changed.value


def slots(n4, order):
    return np.concatenate([n4["first"][order], n4["count"][order]], axis=1)


def slots_agree(n4_a, order_a, n4_b, order_b):
    """Do two collapses have the same live nodes with the same (first, count) in every slot?"""
    return len(order_a) == len(order_b) and np.array_equal(order_a, order_b) and np.array_equal(slots(n4_a, order_a), slots(n4_b, order_b))


def wire(s):
    """(BVH2 nodes, roots, primIdx slots) of a Scene, copied (the views die with the next change)."""
    sa = s.arrays(bvh4=False)
    return sa.bvh2.copy(), sa.blas["bvhIdx"].astype(np.uint32), len(sa.primIdx)


def jittered(prims, amp, seed):
    """Every triangle vertex moved by a normal draw of scale `amp`."""
    rng = np.random.default_rng(seed)
    p = prims.copy()
    tri = p["objType"] == W.PRIM_TRIANGLE
    for v in ("v0", "v1", "v2"):
        p[v][tri, :3] += rng.normal(scale=amp, size=(int(tri.sum()), 3)).astype(np.float32)
    return p


# ---- the named fixtures ------------------------------------------------------------------------------------------------------------------
CLUSTER_A, CLUSTER_B = np.array([-3.0, 0.0, 0.0]), np.array([3.0, 0.0, 0.0])
# the factor cluster B is scaled by about its centre.  swap: B becomes the larger child, the root absorbs it first and its last two slots
# change places; shrink: other children win the greedy steps below the root, and the collapse has 9 live nodes instead of 11
FLIP_VARIANTS = {"swap": 1.3, "shrink": 0.5}


def flip_scene(extra_blas=0):
    """BLAS 0: two clusters of 20 triangles each, 6 apart, A inside a box of half extent 1.0 and B of 0.8, so the SAH root splits
    between them and the root's record absorbs A (the larger area) before B.  extra_blas more soups follow as BLAS of their own."""
    s = Scene()
    _std_materials(s)
    rng = np.random.default_rng(21)
    s.AddTriangles(C._soup(rng, 20, CLUSTER_A - 1.0, CLUSTER_A + 1.0, 0.3), "white-light")
    s.AddTriangles(C._soup(rng, 20, CLUSTER_B - 0.8, CLUSTER_B + 0.8, 0.3), "green")
    s.BuildBLAS(0)
    for k in range(extra_blas):
        c = np.array([0.0, 3.0 + 3.0 * k, 0.0])
        s.AddTriangles(C._soup(rng, 30, c - 1.0, c + 1.0, 0.3), "sand")
        s.BuildBLAS(40 + 30 * k)
    return s


def flip_prims(prims, variant):
    """Cluster B (primitives 20..39) scaled about its centre."""
    f = np.float32(FLIP_VARIANTS[variant])
    p = prims.copy()
    c = CLUSTER_B.astype(np.float32)
    for v in ("v0", "v1", "v2"):
        p[v][20:40, :3] = (p[v][20:40, :3] - c) * f + c
    return p


FLIP_VIEW = dict(origin=(0.0, 1.5, 11.0), forward=(0.0, 0.05, 1.0), fov=64.0, aperture=0.01)


def keep_scene(blas, spheres=2, tris=220, transforms=None):
    """(Scene, its arrays, the view, the deformed primitives): R.build's scene and a jitter of it; handing the same primitives over
    twice makes the second refit the guaranteed in-place case."""
    gt, sa, view = R.build(blas=blas, spheres=spheres, tris=tris, transforms=transforms)
    prims = R.build(R.jitter(0.05, seed=4), blas=blas, spheres=spheres, tris=tris, transforms=transforms)[1].prims.copy()
    return gt.s, sa, view, prims


def host_refit(s, prims=None, inst=None):
    """The host restatement of rebuild_scene(builder="refit") on Scene `s`: its arrays, the BVH4 collapsed by BuildBVH4."""
    if prims is not None:
        s.SetPrimitives(0, prims)
    if inst is not None:
        for b, r in enumerate(inst):
            s.SetInstanceTransform(b, r["invT"].reshape(4, 4))
    s.Refit()
    return s.arrays(bvh4=True)


def host_live(sa):
    """(live nodes, stack need) of the collapse of sa.bvh2, by the host restatement."""
    _, st, qnode = collapse(sa.bvh2, sa.blas["bvhIdx"].astype(np.uint32), len(sa.primIdx))
    return len(qnode), st["stack_need"]

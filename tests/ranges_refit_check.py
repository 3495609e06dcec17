"""Shared pieces of the tests of the per-range refit and of the relocated derived records (test_ranges_refit_cpu.py,
test_gpu_ranges_refit.py): snapshots of host arrays, deformations composed BLAS by BLAS on ranges_check's scene, and the two
device-free entries that pin the relocation of pair records (rt_debug_derive_pairs, rt_debug_relocate_pairs)."""
import ctypes as C

import numpy as np

import ranges_check as RC
import refit_check as R
import test_ranges_cpu as CPU
from magr_ray_tracer_amd import _lib as W
from magr_ray_tracer_amd.scene import SceneArrays

RANGES = list(zip(RC.FIRST, RC.COUNTS))
FIELDS = ("prims", "mats", "tex", "lights", "bvh2", "bvh4", "primIdx", "tlas", "blas")


def snap(sa):
    """A copy of host arrays: Scene.arrays() returns views, which a later rebuild of the Scene leaves dangling."""
    return SceneArrays(**{k: np.array(getattr(sa, k)) for k in FIELDS})


def per_blas(*deforms):
    """deforms[b] (None: identity) applied to BLAS b alone."""
    def d(kind, b, x):
        f = deforms[b] if b < len(deforms) else None
        return f(kind, b, x) if f else x
    return d


def prims_of(deform):
    """The primitives of the test scene under `deform` (they do not depend on the first build)."""
    return np.array(RC.scene(deform, "sah").arrays(bvh4=False).prims)


def node_bytes(sa, k):
    """The node records of BLAS k (range order) as bytes."""
    root, m, _, _ = RC.blocks(sa)[k]
    return np.ascontiguousarray(sa.bvh2[root:root + m]).view(np.uint8).reshape(m, -1)


def keep_and_build_last(fb, move):
    """test_ranges_cpu.keep_and_build for range 2: BLAS 2 - the first the instances name, so the first run of pair ids - changes its
    node count, and the pair ids of BLAS 1 move although its nodes, which lie in front of BLAS 2's, do not."""
    d0, d1 = (RC.only(2, f()) for f in CPU.MOVES[move])
    s = RC.scene(d0, fb)
    sa0 = snap(s.arrays(bvh4=False))
    prims = prims_of(d1)
    full = RC.scene(d0, fb)
    full.SetPrimitives(0, prims)
    full.Rebuild(RC.X_OF[fb], **CPU.OPT[fb])
    return s, sa0, prims[38:], ["keep", "keep", RC.X_OF[fb]], snap(full.arrays(bvh4=False))


def derive_pairs(sa):
    """rt_debug_derive_pairs of wire arrays: (pair records as (n, 4, 4) uint32, pairNode, rootEntry per instance)."""
    L = W.device_lib()
    nodes, inst = np.ascontiguousarray(sa.bvh2, W.BVHNode2), np.ascontiguousarray(sa.blas, W.BVHInstance)
    cap = max(len(nodes) // 2, 1)
    pairs, pair_node, roots, n = np.zeros((cap, 4, 4), np.uint32), np.zeros(cap, np.uint32), np.zeros(len(inst), np.uint32), C.c_int32(0)
    rc = L.rt_debug_derive_pairs(W.ptr(nodes), len(nodes), W.ptr(inst), len(inst), W.ptr(pairs), W.ptr(pair_node), cap, W.ptr(roots), C.byref(n))
    assert rc == 0, L.rt_last_error().decode()
    return pairs[:n.value].copy(), pair_node[:n.value].copy(), roots


def relocate_pairs(recs, pair_delta, idx_delta):
    """rt_debug_relocate_pairs of (n, 4, 4) uint32 records; the deltas are taken modulo 2^32."""
    L = W.device_lib()
    src = np.ascontiguousarray(recs, np.uint32)
    out = np.zeros_like(src)
    rc = L.rt_debug_relocate_pairs(W.ptr(src) if len(src) else None, len(src), int(pair_delta) % 2**32, int(idx_delta) % 2**32,
                                   W.ptr(out) if len(src) else None)
    assert rc == 0, L.rt_last_error().decode()
    return out


def pair_run(pair_node, root, m):
    """(start, count) of the run of pair ids whose nodes lie in the block [root, root + m): one run, asserted."""
    at = np.flatnonzero((pair_node >= root) & (pair_node < root + m))
    assert len(at) == (m - 1) // 2 and (len(at) == 0 or at[-1] - at[0] + 1 == len(at)), "the pair ids of a BLAS are not one run"
    return (int(at[0]) if len(at) else 0), len(at)

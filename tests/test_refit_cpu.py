"""The host restatement of rt_update_scene (rth_set_primitives + rth_refit, csrc/refit_common.h): what it leaves unchanged, the float64
ground truth of tests/geom64.py after deformations, and its refusals.  The device update must reproduce these arrays bit for bit
(test_gpu_refit.py)."""
import numpy as np
import pytest

import geom64 as G
import refit_check as R
import test_groundtruth_cpu as C
from magr_ray_tracer_amd import _lib as W, scenes
from magr_ray_tracer_amd.scene import Scene
from oracle.oracle_py import Oracle


def _refit_unchanged(gt):
    before = gt.s.arrays(bvh4=False).bvh2
    gt.s.Refit()
    after = gt.s.arrays(bvh4=False).bvh2
    return before, after


@pytest.mark.parametrize("builder", ["sah", "lbvh", ("sah", "lbvh"), ("lbvh", "sah")], ids=["sah", "lbvh", "sah-lbvh", "lbvh-sah"])
def test_refit_of_unchanged_geometry_reproduces_the_builder(builder):
    """SAH (alpha 1), LBVH and mixed-builder trees: a refit of the unchanged primitives gives back the builder's node arrays.  Both
    builders bound a node by the union of its primitives' unclipped boxes; they differ from the refit only in how a union treats
    +-0 (fminf / fmaxf against lb_min / lb_max), so the values are compared, not the bits."""
    gt, sa, _ = R.build(blas=4 if isinstance(builder, tuple) else 1, spheres=3, builder=builder)
    before, after = _refit_unchanged(gt)
    assert R.nodes_equal(before, after)
    assert R.check_bounds(gt.s.arrays(bvh4=False)) > 10


def test_refit_of_sbvh_trees_contains_the_old_boxes():
    """SBVH (alpha 0) leaves that held clipped fragments get their primitives' full boxes: every node box contains the box the builder
    gave it and every primitive box below it (the tree stays correct, only looser).  One exception, by one ulp: the builder pads a
    clipped fragment's box outward by one ulp per side (accel_build.cpp, RefBounds), so where a fragment reaches its primitive's own
    extreme the builder's box lies one ulp beyond the primitive's exact box, which is what the refit takes."""
    gt, sa, _ = R.build(alpha=0.0, blas=2, spheres=3)
    assert gt.s.stats()["spatial_splits"] > 0
    before, after = _refit_unchanged(gt)
    reach = np.unique(np.concatenate([[0], np.where(before["count"] > 0)[0], before["first"][before["count"] == 0]]))
    bmn, bmx = before["aabbMin"][reach, :3], before["aabbMax"][reach, :3]
    amn, amx = after["aabbMin"][reach, :3], after["aabbMax"][reach, :3]
    assert np.all(amn <= np.nextafter(bmn, np.float32(np.inf))) and np.all(amx >= np.nextafter(bmx, np.float32(-np.inf)))
    assert np.any(amn < bmn) or np.any(amx > bmx)
    assert np.array_equal(before["first"], after["first"]) and np.array_equal(before["count"], after["count"])
    R.check_bounds(gt.s.arrays(bvh4=False), "sbvh")
    assert not R.nodes_equal(before, after)   # some leaf did hold fragments


ROT = C.invT(C.rot(1, 23.0) @ C.rot(0, -11.0), (0.31, -0.17, 0.45))
SCALE = C.invT(np.diag([1.7, 0.6, 1.15]), (0.2, 0.1, -0.3))
MIRROR = C.invT(C.rot(2, 9.0) @ np.diag([-1.0, 1.0, 1.0]), (-0.25, 0.05, 0.1))
# (kind, blas, alpha, spheres, deformation); spheres stay under identity / rigid instances (the sphere test assumes a unit D)
DEFORMS = {
    "jitter-sah": (1, 1.0, 0, lambda: R.jitter()),
    "jitter-sbvh": (1, 0.0, 3, lambda: R.jitter(seed=4)),
    "rigid-blas": (4, 1.0, 3, lambda: R.rigid_blas(1)),
    "scrambled": (1, 1.0, 0, lambda: R.scramble()),
    "spheres": (2, 0.0, 4, lambda: R.spheres_moved()),
    "lights": (1, 1.0, 2, lambda: R.lights_moved()),
    "instances": (4, 1.0, 2, lambda: R.transforms([None, ROT, SCALE, MIRROR])),
    "instances-back": (4, 0.0, 2, lambda: R.transforms([ROT, None, MIRROR, SCALE])),
}
_UPD = {}


def updated(name):
    """(ground truth of the deformed scene, arrays of the original scene updated to it on the host, view)."""
    if name not in _UPD:
        blas, alpha, spheres, mk = DEFORMS[name]
        start = [None, None, SCALE, MIRROR] if name == "instances-back" else None
        gt0, sa0, view = R.build(alpha=alpha, blas=blas, spheres=spheres, transforms=start)
        gt1, sa1, _ = R.build(mk(), alpha=alpha, blas=blas, spheres=spheres, transforms=start)
        sa = R.host_update(gt0, gt1, sa1)
        assert np.array_equal(sa.prims.view(np.uint8), sa1.prims.view(np.uint8))
        assert np.array_equal(sa.primIdx, sa0.primIdx) and np.array_equal(sa.bvh2["first"], sa0.bvh2["first"])
        assert W.device_lib().rt_validate_scene(W.ACCEL_BVH2, *_val_args(sa)) == 0, W.device_lib().rt_last_error()
        _UPD[name] = (gt1, sa, view)
    return _UPD[name]


def _val_args(sa):
    P = W.ptr
    return (P(sa.prims), len(sa.prims), P(sa.mats), len(sa.mats), P(sa.tex) if len(sa.tex) else None, len(sa.tex),
            P(sa.lights) if len(sa.lights) else None, len(sa.lights), P(sa.bvh2), len(sa.bvh2), P(sa.primIdx), len(sa.primIdx),
            P(sa.tlas), len(sa.tlas), P(sa.blas), len(sa.blas))


@pytest.mark.parametrize("accel", [W.ACCEL_BVH2, W.ACCEL_BVH4], ids=["bvh2", "bvh4"])
@pytest.mark.parametrize("name", list(DEFORMS))
def test_oracle_after_a_refit_matches_float64_closest_hit(name, accel, monkeypatch):
    """Camera rays and the adversarial sets of geom64 through the oracle over the refit trees: the deformed scene's true closest hit
    on every decidable ray."""
    gt, sa, view = updated(name)
    R.check_bounds(sa, name)
    monkeypatch.setattr(C, "_CACHE", {(name, 0.0): (gt, sa, view)})
    C.test_extend_matches_float64_closest_hit((name, 0.0), accel)


# (the sphere and light cases are covered by the closest-hit test above: their open scenes leave bounce queues of a few dozen rays,
# too few for the ground truth's floor on the decidable share)
@pytest.mark.parametrize("name", ["jitter-sah", "rigid-blas", "instances"])
def test_oracle_frames_after_a_refit_match_float64(name, monkeypatch):
    """Bounce rays of real frames against the float64 closest hit, every shadow ray against the float64 any-hit."""
    gt, sa, view = updated(name)
    monkeypatch.setattr(C, "_CACHE", {(name, 0.0): (gt, sa, view)})
    C.test_frames_bounces_and_connect_match_float64((name, 0.0))


def test_refit_loosens_but_keeps_the_tree():
    """Scrambled vertices: the tree keeps its shape (node count, children, leaf ranges) while its boxes grow."""
    gt, sa, _ = updated("scrambled")
    _, sa0, _ = R.build()
    assert len(sa.bvh2) == len(sa0.bvh2)
    area = lambda n: np.prod(n["aabbMax"][0, :3] - n["aabbMin"][0, :3])
    assert area(sa.bvh2) >= area(sa0.bvh2) * 0.5
    lo, hi = R.prim_boxes(sa.prims)
    leaves = sa.bvh2["count"] > 0
    grow = np.mean([np.prod(hi[sa.primIdx[f:f + c]].max(0) - lo[sa.primIdx[f:f + c]].min(0))
                    for f, c in zip(sa.bvh2["first"][leaves], sa.bvh2["count"][leaves])])
    lo, hi = R.prim_boxes(sa0.prims)
    grow0 = np.mean([np.prod(hi[sa0.primIdx[f:f + c]].max(0) - lo[sa0.primIdx[f:f + c]].min(0))
                     for f, c in zip(sa0.bvh2["first"][sa0.bvh2["count"] > 0], sa0.bvh2["count"][sa0.bvh2["count"] > 0])])
    assert grow > 2 * grow0


def test_refusals_leave_the_scene_unchanged():
    gt, sa, _ = R.build(spheres=2)
    s = gt.s
    before = s.arrays(bvh4=False)
    p = sa.prims.copy()
    bad_type = p[:4].copy()
    bad_type["objType"][2] = W.PRIM_SPHERE if bad_type["objType"][2] != W.PRIM_SPHERE else W.PRIM_TRIANGLE
    bad_mat = p[:4].copy()
    bad_mat["matIdx"][1] += 1
    L = W.host_lib()
    for first, recs, what in ((0, bad_type, "objType"), (0, bad_mat, "matIdx"), (len(p) - 2, p[:4], "range"), (-1, p[:2], "range")):
        with pytest.raises(RuntimeError) as e:
            s.SetPrimitives(first, recs)
        assert what in str(e.value) or "outside" in str(e.value), str(e.value)
    assert L.rth_set_primitives(s._h, 0, 3, None) == W.RT_E_INVALID
    after = s.arrays(bvh4=False)
    assert np.array_equal(before.prims.view(np.uint8), after.prims.view(np.uint8))
    assert np.array_equal(before.bvh2.view(np.uint8), after.bvh2.view(np.uint8))
    empty = Scene()
    scenes._std_materials(empty)
    empty.AddSphere((0, 0, 0), 1.0, "red")
    with pytest.raises(RuntimeError, match="no BLAS"):
        empty.Refit()
    # a singular instance transform: TLAS::Build refuses it after the refit, as rt_update_scene refuses it
    gt4, sa4, _ = R.build(blas=2)
    gt4.s.SetInstanceTransform(1, np.diag([1.0, 0.0, 1.0, 1.0]).astype(np.float32))
    gt4.s.Refit()
    with pytest.raises(RuntimeError, match="singular"):
        gt4.s.BuildTLAS()
    gt4.s.close()

"""The state of a scene copy carried across commits of different kinds on the MI355X: one copy, held by two contexts, goes through
update_scene, rebuild_ranges, update_materials, resize_scene, the whole-scene refit, rebuild_ranges and update_scene again.  After every
step its device arrays (sizes included) are those of a fresh upload of the host mirror's scene, and both holders report the kernels, the
BLAS blocks and the traversal facts of that fresh context.  All comparisons are byte for byte."""
import numpy as np
import pytest

import ranges_check as RC
import rebuild_check as RB
import refit_check as R
import resize_check as RZ
import test_groundtruth_cpu as C
from ranges_refit_check import snap
from magr_ray_tracer_amd import _lib as W, scenes
from magr_ray_tracer_amd.renderer import Device, RtError
from magr_ray_tracer_amd.scenes import Scene, _std_materials

pytestmark = pytest.mark.gpu

Wd, Hd = 64, 48
KINDS = {"bvh2": {}, "layout0": {"extend_variant": 1}, "bvh4": {"accel": W.ACCEL_BVH4}}
NAMES = [*RZ.ARRAYS, "rootEntry", *W.SCENE_ARRAYS_MATERIALS]
NAMES4 = [*RZ.ARRAYS_BVH4, *W.SCENE_ARRAYS_MATERIALS]
N0, N1, MORE = 30, 40, 8                      # soup triangles of BLAS 0 (behind its light triangle) and of BLAS 1; what the resize adds to BLAS 1
FIRST1 = 1 + N0                               # the first primitive of BLAS 1
LIGHT = np.array([(-1.5, 4.2, -1.5), (1.5, 4.2, -1.5), (0.0, 4.2, 1.5)], np.float32)
FOURTH = C.invT(C.rot(2, 15.0), (-0.8, 0.5, 0.9))
HOST_SAH = dict(builder="sah_gpu", device=None)   # the host form of the builder the resize names


def _soups():
    rng = np.random.default_rng(21)
    c0, c1 = np.array(R.CENTRES[0]), np.array(R.CENTRES[1])
    return C._soup(rng, N0, c0 - 1.4, c0 + 1.4, 0.4), C._soup(rng, N1 + MORE, c1 - 1.2, c1 + 1.2, 0.4)


def _jitter(t, seed):
    return (t + np.random.default_rng(seed).normal(0.0, 0.05, t.shape)).astype(np.float32)


def _scene(t0, t1, lit=(), fourth=False, **host):
    """BLAS 0: a light triangle and the soup t0; BLAS 1: the soup t1, its triangles `lit` emissive.  Instances: BLAS 0, BLAS 1 under
    RB.ROT, BLAS 0 again under RC.SHIFT, and (fourth) BLAS 1 again under FOURTH."""
    s = Scene()
    _std_materials(s)
    s.AddTriangle(LIGHT[0], LIGHT[1], LIGHT[2], "white-light")
    s.AddTriangles(t0, "sand")
    s.BuildBLAS(0, **host)
    for j, t in enumerate(t1):
        s.AddTriangle(t[0], t[1], t[2], "white-light" if j in lit else "green")
    s.BuildBLAS(FIRST1, **host)
    s.SetInstanceTransform(1, RB.ROT)
    s.AddInstance(0, RC.SHIFT)
    if fourth:
        s.AddInstance(1, FOURTH)
    return s


def _prims(t0, t1, lit=()):
    return np.array(_scene(t0, t1, lit).arrays(bvh4=False).prims)


def _moved(sa, b, T):
    inst = np.array(sa.blas)
    inst["invT"][b] = np.asarray(T, np.float32).reshape(inst["invT"][b].shape)
    return inst


def _state(d, names):
    facts = d.traversal_facts()
    facts.pop("xcdFirst")
    return {k: d.scene_array(k) for k in names}, (d.kernel_info(), d.blas_blocks(), facts)


@pytest.mark.parametrize("kind", list(KINDS))
def test_the_state_of_a_copy_across_commits_of_every_kind(kind):
    kw, bvh4 = KINDS[kind], kind == "bvh4"
    names = NAMES4 if bvh4 else NAMES
    t0, t1all = _soups()
    t1 = t1all[:N1]
    s = _scene(t0, t1)
    cam = scenes.camera_for(RC.VIEW, Wd, Hd)
    a, b = Device(Wd, Hd, **kw), Device(Wd, Hd, **kw)
    fresh = None

    def mirror():
        return snap(s.arrays(bvh4=bvh4))

    def check(what):
        """A's arrays are a fresh upload's; A, the sharing partner and the fresh context report the same kernels, blocks and facts."""
        nonlocal fresh
        if fresh is not None:
            fresh.close()
        fresh = Device(Wd, Hd, **kw)
        fresh.upload(mirror(), from_bvh2=bvh4)
        want, told = _state(fresh, names)
        got, told_a = _state(a, names)
        RZ.same(got, want, f"{kind}: {what}")
        assert told_a == told, (kind, what, told_a, told)
        assert _state(b, ())[1] == told, (kind, what, "the sharing partner", _state(b, ())[1], told)

    def update(what, prims, first, inst, apply):
        """rt_update_scene, which a BVH4 context refuses: then nothing may have changed."""
        if bvh4:
            with pytest.raises(RtError, match="BVH4 contexts cannot refit"):
                a.update_scene(prims, first, inst)
        else:
            a.update_scene(prims, first, inst)
            apply()
            s.Refit()
        check(what)

    try:
        a.upload(mirror(), from_bvh2=bvh4)
        b.share_scene(a)
        check("the upload")
        assert len(a.blas_blocks()) == 2 and all(blk["nodes"] > 1 for blk in a.blas_blocks())

        # (a) update_scene: a window in BLAS 1 and a new transform of instance 2
        lo, hi = FIRST1 + 5, FIRST1 + 25
        p = _prims(t0, _jitter(t1, 1))
        T = C.invT(C.rot(1, 40.0), (0.2, 0.1, -0.3))
        update("(a) update_scene", p[lo:hi], lo, _moved(mirror(), 2, T), lambda: (s.SetPrimitives(lo, p[lo:hi]), s.SetInstanceTransform(2, T)))

        # (b) BLAS 0 kept, BLAS 1 built by the linear builder
        a.rebuild_ranges(["keep", "lbvh"])
        s.RebuildRanges(["keep", "lbvh"])
        check("(b) rebuild_ranges keep, lbvh")

        # (c) one more emissive triangle: the light count changes
        lights = len(mirror().lights)
        emissive = np.array([mirror().prims["matIdx"][0]], np.int32)
        st = a.update_materials(prim_mat=emissive, prim_first=FIRST1 + 3)
        s.SetPrimMaterials(FIRST1 + 3, emissive)
        assert st["lights"] == lights + 1 == len(mirror().lights)
        check("(c) update_materials")

        # (d) resize: eight more triangles in BLAS 1, a fourth instance
        t1 = t1all
        s = _scene(t0, t1, lit={3}, fourth=True, **HOST_SAH)
        sa = mirror()
        counts, inst_range, inst = RZ.shape_of(sa, [FIRST1, N1 + MORE])
        st = a.resize_scene(sa.prims, counts, inst_range, inst, builder="sah")
        assert st["prims"] == FIRST1 + N1 + MORE and len(sa.blas) == 4
        check("(d) resize_scene")

        # (e) the whole-scene refit with a window over the end of BLAS 0 and the start of BLAS 1
        lo, hi = FIRST1 - 10, FIRST1 + 20
        p = _prims(_jitter(t0, 2), _jitter(t1, 3), lit={3})
        a.rebuild_scene(p[lo:hi], lo, None, builder="refit")
        s.SetPrimitives(lo, p[lo:hi])
        s.Refit()
        check("(e) rebuild_scene refit")

        # (f) BLAS 0 refit under a window of its own, BLAS 1 kept
        lo, hi = 0, 12
        p = _prims(_jitter(t0, 4), t1, lit={3})
        a.rebuild_ranges(["refit", "keep"], p[lo:hi], lo)
        s.SetPrimitives(lo, p[lo:hi])
        s.RebuildRanges(["refit", "keep"])
        check("(f) rebuild_ranges refit, keep")

        # (g) update_scene again: the added triangles and the fourth instance
        lo, hi = FIRST1 + N1 - 4, FIRST1 + N1 + MORE
        p = _prims(t0, _jitter(t1, 5), lit={3})
        T = C.invT(C.rot(0, -25.0), (0.6, -0.2, 0.4))
        update("(g) update_scene", p[lo:hi], lo, _moved(mirror(), 3, T), lambda: (s.SetPrimitives(lo, p[lo:hi]), s.SetInstanceTransform(3, T)))

        frames = []
        for d in (a, b, fresh):
            d.seed_default()
            d.reset()
            d.render(cam, 1)
            frames.append(d.read_accum())
        assert frames[0].any()
        for f, who in zip(frames[1:], ("the sharing partner", "the fresh context")):
            assert np.array_equal(frames[0].view(np.uint32), f.view(np.uint32)), f"{kind}: the frame of {who} differs from A's"
    finally:
        if fresh is not None:
            fresh.close()
        b.close()
        a.close()

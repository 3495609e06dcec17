"""The host restatement of rt_rebuild_scene (Scene.Rebuild = rth_rebuild, csrc/rebuild_common.h): a rebuild after SetPrimitives gives,
array for array, the deformed scene built from scratch with the same builder; the rebuilt scenes answer rays like the float64 ground
truth; BLAS range detection; refit after rebuild; refusals.  The device rebuild must reproduce these arrays bit for bit
(test_gpu_rebuild.py)."""
import ctypes

import numpy as np
import pytest

import rebuild_check as RB
import refit_check as R
import test_groundtruth_cpu as C
from magr_ray_tracer_amd import _lib as W
from magr_ray_tracer_amd.scene import BuildError, SceneArrays, blas_ranges

_DONE = {}


def rebuilt(deform, first_build, builder, blas):
    """(ground truth of the deformed scene, arrays of the first scene rebuilt to it on the host, arrays built from scratch, view)."""
    key = (deform, first_build, builder, blas)
    if key not in _DONE:
        mk, spheres = RB.DEFORMS[deform]
        (gt0, sa0), (gt1, sa1), view = RB.pair(mk(), first_build, builder, blas, spheres=spheres)
        sa = RB.host_rebuild(gt0.s, sa1.prims, builder=builder, bvh4=True)
        gt1.sa = sa
        _DONE[key] = (gt1, sa, sa1, sa0, view)
    return _DONE[key]


@pytest.mark.parametrize("builder", RB.BUILDERS)
@pytest.mark.parametrize("blas", [1, 2, 4])
@pytest.mark.parametrize("first_build", list(RB.FIRST_BUILDS))
@pytest.mark.parametrize("deform", list(RB.DEFORMS))
def test_rebuild_equals_a_build_from_scratch(deform, first_build, builder, blas):
    gt, sa, want, sa0, _ = rebuilt(deform, first_build, builder, blas)
    RB.same_wire_arrays(sa, want, f"{deform} / first built {first_build} / rebuilt {builder} / {blas} BLAS")
    RB.validate(sa)
    if first_build == "sbvh":
        assert len(sa.primIdx) <= len(sa0.primIdx) and len(sa.primIdx) == sum(c for _, c in blas_ranges(sa))


def test_an_sbvh_scene_shrinks_its_primidx():
    """The SBVH build references some primitives several times; the rebuilt trees reference each once."""
    _, sa, _, sa0, _ = rebuilt("jitter", "sbvh", "sah", 4)
    assert len(sa0.primIdx) > len(sa0.prims) and len(sa.primIdx) == len(sa.prims) < len(sa0.primIdx)


@pytest.mark.parametrize("builder", RB.BUILDERS)
@pytest.mark.parametrize("deform,first_build,blas", [("scramble", "sah", 1), ("jitter", "sbvh", 2), ("rigid_blas", "lbvh", 4),
                                                      ("spheres_moved", "sbvh", 2)])
def test_rebuilt_scene_matches_float64_closest_hit(deform, first_build, builder, blas, monkeypatch):
    """Camera rays and the adversarial sets of geom64 through the oracle over the rebuilt trees: the deformed scene's true closest
    hit on every decidable ray; every node box contains what lies below it."""
    gt, sa, _, _, view = rebuilt(deform, first_build, builder, blas)
    assert R.check_bounds(sa, deform) > 10
    name = f"rebuild-{deform}-{first_build}-{builder}-{blas}"
    monkeypatch.setattr(C, "_CACHE", {(name, 0.0): (gt, sa, view)})
    C.test_extend_matches_float64_closest_hit((name, 0.0), W.ACCEL_BVH2)


# ---- BLAS ranges ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("first_build", list(RB.FIRST_BUILDS))
def test_blas_ranges_of_built_scenes(first_build):
    alpha, b0 = RB.FIRST_BUILDS[first_build]
    gt, sa, _ = R.build(alpha=alpha, blas=4, spheres=2, builder=b0)
    want = [(0, 226), (226, 222), (448, 220), (668, 220)]
    assert blas_ranges(sa) == want and gt.s.blas_ranges() == want
    assert sum(c for _, c in want) == len(sa.prims)
    if first_build == "sbvh":
        assert len(sa.primIdx) > len(sa.prims)   # some primitive is referenced twice: the set is still a range


def _hand_made(leaves, roots=None):
    """One BLAS per entry of `leaves` (a root with two leaves over the given primitive ids), BLAS k rooted at node 3 * k unless `roots`
    says otherwise."""
    n = len(leaves)
    roots = list(range(0, 3 * n, 3)) if roots is None else roots
    nodes = np.zeros(3 * n, W.BVHNode2)
    idx = []
    for k, (a, b) in enumerate(leaves):
        r = roots[k]
        nodes["first"][r], nodes["count"][r] = r + 1, 0
        for j, ids in enumerate((a, b)):
            nodes["first"][r + 1 + j], nodes["count"][r + 1 + j] = len(idx), len(ids)
            idx += list(ids)
    inst = np.zeros(n, W.BVHInstance)
    inst["bvhIdx"] = roots
    nprims = max(idx) + 1
    return SceneArrays(prims=np.zeros(nprims, W.Primitive), mats=None, tex=None, lights=None, bvh2=nodes, bvh4=None,
                       primIdx=np.asarray(idx, np.uint32), tlas=None, blas=inst)


def test_blas_ranges_refuses_what_cannot_be_rebuilt():
    ok = _hand_made([((0, 1), (2, 1)), ((3,), (4, 5))])
    assert blas_ranges(ok) == [(0, 3), (3, 3)]
    shared = _hand_made([((0, 1), (2,)), ((3,), (4, 5))])
    shared.blas = np.concatenate([shared.blas, shared.blas[:1]])           # a third instance of BLAS 0
    assert blas_ranges(shared) == [(0, 3), (3, 3), (0, 3)]
    for what, sa in (("interleaved", _hand_made([((0,), (2,)), ((1,), (3,))])),
                     ("overlapping", _hand_made([((0, 1), (2,)), ((2,), (3, 4))])),
                     ("out of root order", _hand_made([((3,), (4, 5)), ((0, 1), (2,))])),
                     ("a hole", _hand_made([((0,), (1,)), ((2,), (4,))]))):
        with pytest.raises(BuildError) as e:
            blas_ranges(sa)
        assert e.value.code == W.RT_E_UNSUPPORTED, what
    # roots in the other order, ranges following them: fine (instance order does not matter)
    swapped = _hand_made([((3,), (4, 5)), ((0, 1), (2,))], roots=[3, 0])
    assert blas_ranges(swapped) == [(3, 3), (0, 3)]


# ---- chaining ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("builder", RB.BUILDERS)
def test_rebuild_then_refit_equals_a_fresh_build_then_refit(builder):
    (gt0, sa0), (gt1, sa1), _ = RB.pair(R.scramble(), "sbvh", builder, 4)
    RB.host_rebuild(gt0.s, sa1.prims, builder=builder)
    p2 = R.build(R.jitter(0.03, seed=7), blas=4, spheres=2)[1].prims
    a = RB.host_refit(gt0.s, p2)
    b = RB.host_refit(gt1.s, p2)
    RB.same_wire_arrays(a, b, "refit after a rebuild")
    R.check_bounds(a, "refit after a rebuild")


def test_rebuild_without_new_primitives_changes_the_builder():
    gt_l, sa_l, _ = R.build(blas=2, spheres=2, builder="lbvh")
    _, sa_s, _ = R.build(blas=2, spheres=2, builder="sah")
    RB.same_wire_arrays(RB.host_rebuild(gt_l.s, None, builder="sah"), sa_s, "lbvh scene rebuilt with sah")
    RB.same_wire_arrays(RB.host_rebuild(gt_l.s, None, builder="lbvh"), sa_l, "and back")
    other = RB.host_rebuild(gt_l.s, None, builder="lbvh", max_leaf=2)
    assert len(other.bvh2) > len(sa_l.bvh2)


def test_instance_transforms_survive_a_rebuild():
    T = [None, RB.ROT]
    (gt0, sa0), (gt1, sa1), _ = RB.pair(R.jitter(), "sah", "sah", 2, transforms=T)
    sa = RB.host_rebuild(gt0.s, sa1.prims)
    RB.same_wire_arrays(sa, sa1, "instances")
    assert not np.array_equal(sa.blas["invT"][1], sa.blas["invT"][0])


# ---- refusals ---------------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_scene_unchanged():
    gt, sa, _ = R.build(blas=2, spheres=2)
    s = gt.s
    before = s.arrays(bvh4=False)
    bad_type = sa.prims[:4].copy()
    bad_type["objType"][2] = W.PRIM_SPHERE
    with pytest.raises(RuntimeError):
        s.SetPrimitives(0, bad_type)
    RB.same_wire_arrays(s.arrays(bvh4=False), before, "after the refused objType change")
    nan = sa.prims.copy()
    nan["v1"][300, 1] = np.inf
    s.SetPrimitives(0, nan)           # the records are taken (objType / matIdx kept) ...
    with pytest.raises(BuildError) as e:
        s.Rebuild("sah")              # ... and the builder refuses them
    assert e.value.code == W.RT_E_UNSUPPORTED
    s.SetPrimitives(0, sa.prims)
    RB.same_wire_arrays(s.arrays(bvh4=False), before, "after the refused rebuild")
    with pytest.raises(ValueError):
        s.Rebuild("sbvh")
    with pytest.raises(BuildError) as e:
        s.Rebuild("lbvh", max_leaf=1000)
    assert e.value.code == W.RT_E_INVALID
    assert W.host_lib().rth_rebuild(s._h, 7, None) == W.RT_E_INVALID
    RB.same_wire_arrays(s.arrays(bvh4=False), before, "after the refused options")


def test_a_blas_deeper_than_the_stack_is_refused_at_65_levels():
    """The 64-entry stack rule (rebuild_common.h, exceeds_stack) at its boundary, on geometry: a rebuild to a tree 64 levels deep is
    taken, one to 65 levels is refused with RT_E_UNSUPPORTED - by the restatement as by rt_upload_scene's checks - and changes nothing."""
    s = RB.ladder_scene(-90)
    sa64 = s.arrays(bvh4=False)
    assert RB.depth(sa64) == 64
    RB.validate(sa64)
    sa65 = RB.ladder_scene(-93).arrays(bvh4=False)
    assert RB.depth(sa65) == 65 and len(sa65.prims) == len(sa64.prims)
    L = W.device_lib()
    P = W.ptr
    assert L.rt_validate_scene(W.ACCEL_BVH2, P(sa65.prims), len(sa65.prims), P(sa65.mats), len(sa65.mats), None, 0, P(sa65.lights), len(sa65.lights),
                               P(sa65.bvh2), len(sa65.bvh2), P(sa65.primIdx), len(sa65.primIdx), P(sa65.tlas), len(sa65.tlas), P(sa65.blas),
                               len(sa65.blas)) == W.RT_E_UNSUPPORTED
    s.SetPrimitives(0, sa65.prims)
    before = s.arrays(bvh4=False)
    with pytest.raises(BuildError, match="65 stack entries") as e:
        s.Rebuild("sah")
    assert e.value.code == W.RT_E_UNSUPPORTED
    RB.same_wire_arrays(s.arrays(bvh4=False), before, "after the refused 65-level rebuild")
    other = RB.ladder_scene(-88).arrays(bvh4=False)
    RB.same_wire_arrays(RB.host_rebuild(s, other.prims, builder="sah"), other, "a 64-level rebuild")
    assert RB.depth(other) == 64
    deep = RB.host_rebuild(s, sa65.prims, builder="lbvh")          # the linear builder's trees are at most 63 levels deep
    assert RB.depth(deep) <= 63
    RB.validate(deep)


def test_the_entry_points_exist_and_refuse_a_null_context():
    L = W.device_lib()
    for name in ("rt_rebuild_scene", "rt_group_rebuild_scene", "rt_blas_ranges"):
        assert hasattr(L, name)
    st = np.zeros((), W.RebuildStats)
    assert L.rt_rebuild_scene(None, None, 0, 0, None, 0, W.REBUILD_SAH, None, W.ptr(st)) == W.RT_E_INVALID
    assert b"null context" in L.rt_last_error()
    assert L.rt_group_rebuild_scene(None, None, 0, 0, None, 0, W.REBUILD_LBVH, None, None) == W.RT_E_INVALID
    assert ctypes.sizeof(ctypes.c_double) * 7 + 4 * 10 == W.RebuildStats.itemsize and W.RebuildStats.itemsize % 8 == 0

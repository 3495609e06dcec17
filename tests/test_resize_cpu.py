"""The host side of rt_resize_scene, without a GPU: the light-list rule of csrc/resize_common.h against Scene's own list, Scene.AddInstance
against hand-worked TLAS leaves (what the host needs to state a scene with more instances than BLAS), and the argument refusals that
need no device, one case per message (rt_resize_check)."""
import numpy as np
import pytest

import rebuild_check as RB
import resize_check as Z
import test_groundtruth_cpu as C
from magr_ray_tracer_amd import _lib as W
from magr_ray_tracer_amd.scene import BuildError, build_options, light_list

SCENES = {
    "one-blas": dict(tris=(57,), lights=2),
    "no-light": dict(tris=(40,), lights=0),
    "one-light": dict(tris=(12,), lights=1),
    "many-lights": dict(tris=(30, 20), spheres=(2, 1), lights=7),
    "lights-in-the-last-blas": dict(tris=(9, 301, 5), spheres=(1, 0, 0), lights=3, light_blas=2),
}


@pytest.mark.parametrize("name", list(SCENES))
def test_light_list_rule_equals_the_scenes_own(name):
    _, sa, counts = Z.build(**SCENES[name])
    got = light_list(sa.prims, sa.mats)
    assert got.dtype == np.uint32 and np.array_equal(got, sa.lights), (got, sa.lights)
    assert np.all(np.diff(got.astype(np.int64)) > 0)                     # increasing
    assert len(got) == SCENES[name]["lights"] and sum(counts) == len(sa.prims)


def test_light_list_at_the_ends_everywhere_and_nowhere():
    for runs in ([(1, "white-light"), (200, "sand"), (1, "red-light")], [(64, "green-light")], [(64, "sand")]):
        sa, _ = Z.build_runs(runs)
        assert np.array_equal(light_list(sa.prims, sa.mats), sa.lights)
    sa, _ = Z.build_runs([(1, "white-light"), (200, "sand"), (1, "red-light")])
    assert list(sa.lights) == [0, 201]


def test_light_list_refuses_a_record_out_of_range():
    sa, _ = Z.build_runs([(5, "sand")])
    for field, value in (("matIdx", len(sa.mats)), ("matIdx", -1), ("objType", 3), ("objType", -1)):
        p = sa.prims.copy()
        p[field][4] = value
        with pytest.raises(BuildError, match="primitive 4") as e:
            light_list(p, sa.mats)
        assert e.value.code == W.RT_E_INVALID


def _world_box(invT, mn, mx):
    """refit::instance_world_box for a transform whose linear part is diagonal with powers of two (every product exact in float64)."""
    T = np.asarray(invT, np.float64).reshape(4, 4)
    s, t = 1.0 / np.diag(T)[:3], T[:3, 3]
    a, b = (mn[:3].astype(np.float64) - t) * s, (mx[:3].astype(np.float64) - t) * s
    lo, hi = np.minimum(a, b), np.maximum(a, b)
    pad = 1e-5 * (hi - lo) + 1e-6 * np.maximum(np.abs(lo), np.abs(hi)) + 1e-30
    fl = np.nextafter((lo - pad).astype(np.float32), np.float32(-np.inf))
    fh = np.nextafter((hi + pad).astype(np.float32), np.float32(np.inf))
    return fl, fh


def test_add_instance_against_hand_worked_tlas_leaves():
    T1 = C.invT(np.diag([0.5, 2.0, 1.0]), (3.0, -1.25, 0.5))
    gt, sa, counts = Z.build(tris=(30, 12), lights=1, extra=[(0, T1), (1, None), (0, None)])
    s = gt.s
    assert len(sa.blas) == 5 and len(sa.tlas) == 10
    roots = sa.blas["bvhIdx"]
    assert roots[2] == roots[0] and roots[3] == roots[1] and roots[4] == roots[0] and roots[0] != roots[1]
    ident = np.eye(4, dtype=np.float32).ravel()
    assert np.array_equal(sa.blas["invT"][2], np.asarray(T1, np.float32).ravel())
    assert np.array_equal(sa.blas["invT"][3], ident) and np.array_equal(sa.blas["invT"][4], ident)
    for i in range(5):                                                  # leaf i of TLAS::Build is node 1 + i
        leaf, root = sa.tlas[1 + i], sa.bvh2[roots[i]]
        assert leaf["leftRight"] == 0 and leaf["BLASidx"] == i
        if i == 2:
            lo, hi = _world_box(T1, root["aabbMin"], root["aabbMax"])
            assert np.array_equal(leaf["aabbMin"][:3], lo) and np.array_equal(leaf["aabbMax"][:3], hi), (leaf, lo, hi)
        else:                                                           # the identity: the root's box bit for bit
            assert leaf["aabbMin"].tobytes() == root["aabbMin"].tobytes() and leaf["aabbMax"].tobytes() == root["aabbMax"].tobytes()
    RB.validate(sa)                                                     # rt_validate_scene accepts it ...
    want = [(0, counts[0]), (counts[0], counts[1])]
    assert s.blas_ranges() == [want[0], want[1], want[0], want[1], want[0]]   # ... and rt_blas_ranges reports the ranges and the map
    rc, ir, inst = Z.shape_of(sa, counts)
    assert list(rc) == counts and list(ir) == [0, 1, 0, 1, 0] and Z.check_args(len(sa.prims), rc, ir, inst)[0] == 0


def test_add_instance_refusals():
    gt, sa, _ = Z.build(tris=(8,), lights=0)
    with pytest.raises(RuntimeError, match="bad index"):
        gt.s.AddInstance(1)
    with pytest.raises(RuntimeError, match="singular"):
        gt.s.AddInstance(0, np.diag([1.0, 0.0, 1.0, 1.0]))
    for _ in range(255):
        gt.s.AddInstance(0)
    with pytest.raises(RuntimeError, match="256"):
        gt.s.AddInstance(0)


_SING = np.zeros(2, W.BVHInstance)
_SING["invT"][0] = np.eye(4, dtype=np.float32).ravel()
_SING["invT"][1] = np.diag([1.0, 1.0, 0.0, 1.0]).astype(np.float32).ravel()
REFUSALS = {
    "no-primitives": (dict(n_prims=0, counts=[1], inst_range=[0]), "nPrims must be positive"),
    "no-range": (dict(n_prims=5, counts=[], inst_range=[0]), "at least one BLAS range"),
    "zero-count": (dict(n_prims=5, counts=[5, 0], inst_range=[0, 1]), "range 1 holds 0 primitives"),
    "sum-one-short": (dict(n_prims=10, counts=[4, 5], inst_range=[0, 1]), "9 primitives in all, nPrims is 10"),
    "sum-one-over": (dict(n_prims=10, counts=[6, 5], inst_range=[0, 1]), "11 primitives in all, nPrims is 10"),
    "instRange-high": (dict(n_prims=10, counts=[5, 5], inst_range=[0, 2]), r"instance 1: instRange 2 outside \[0, 2\)"),
    "instRange-negative": (dict(n_prims=10, counts=[5, 5], inst_range=[-1, 1]), r"instance 0: instRange -1 outside"),
    "unnamed-range": (dict(n_prims=10, counts=[5, 5], inst_range=[0, 0]), "range 1 is named by no instance"),
    "no-instance": (dict(n_prims=5, counts=[5], inst_range=[]), "0 instances: 1..256"),
    "257-instances": (dict(n_prims=5, counts=[5], inst_range=[0] * 257), "257 instances: 1..256"),
    "singular": (dict(n_prims=5, counts=[5], inst_range=[0, 0], instances=_SING), "instance 1: the transform is singular"),
    "unknown-builder": (dict(n_prims=5, counts=[5], inst_range=[0], builder=7), "unknown builder 7"),
    "refit": (dict(n_prims=5, counts=[5], inst_range=[0], builder=W.REBUILD_REFIT), "no tree to refit"),
    "alpha": (dict(n_prims=5, counts=[5], inst_range=[0], builder=W.REBUILD_SBVH, opts=build_options(alpha=1.5)), r"alpha must lie in \[0, 1\]"),
    "alpha-nan": (dict(n_prims=5, counts=[5], inst_range=[0], builder=W.REBUILD_SBVH, opts=build_options(alpha=float("nan"))), "alpha must lie"),
    "lbvh-options": (dict(n_prims=5, counts=[5], inst_range=[0], builder=W.REBUILD_LBVH, opts=build_options(max_leaf=0)), "max_leaf"),
}


@pytest.mark.parametrize("name", list(REFUSALS))
def test_argument_refusals_need_no_device(name):
    import re
    kw, pattern = REFUSALS[name]
    rc, msg = Z.check_args(**kw)
    assert rc == W.RT_E_INVALID and msg.startswith("rt_resize_scene: ") and re.search(pattern, msg), (rc, msg)


def test_a_null_shape_is_refused_and_good_arguments_pass():
    L = W.device_lib()
    assert L.rt_resize_check(5, None, W.REBUILD_SAH, None) == W.RT_E_INVALID and b"null shape" in L.rt_last_error()
    for builder, opts in ((W.REBUILD_SAH, None), (W.REBUILD_LBVH, None), (W.REBUILD_LBVH, build_options(max_leaf=4)),
                          (W.REBUILD_SBVH, None), (W.REBUILD_SBVH, build_options(alpha=0.5))):
        assert Z.check_args(10, [1, 2, 7], [2, 0, 1, 1], builder=builder, opts=opts) == (0, "")

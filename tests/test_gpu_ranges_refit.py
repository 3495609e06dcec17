"""The per-range refit (plan word "refit") and the relocated derived records of kept and refit BLAS on the MI355X: after every call the
device arrays (sizes included), the root entries and kernel_info are those of a fresh upload of the host mirror's scene, and what reads
the relocated refit topology afterwards - update_scene, the whole-scene refit, a further plan - gives the host's arrays too.  All
comparisons are byte for byte."""
import numpy as np
import pytest

import ranges_check as RC
import ranges_refit_check as RR
import rebuild_check as RB
import refit_check as R
import test_groundtruth_cpu as C
import test_ranges_cpu as CPU
from helpers import DEFAULT, assert_bits
from magr_ray_tracer_amd import _lib as W, scenes
from magr_ray_tracer_amd.renderer import Device, Group, RtError
from oracle.oracle_py import Oracle, seed_stream

pytestmark = pytest.mark.gpu

Wd, Hd = 160, 120
NAMES = {**W.SCENE_ARRAYS, "rootEntry": W.SCENE_ARRAYS_BVH4["rootEntry"]}
NAMES4 = {**W.SCENE_ARRAYS, **W.SCENE_ARRAYS_BVH4}
KINDS = {"bvh2": {}, "layout0": {"extend_variant": 1}, "bvh4": {"accel": W.ACCEL_BVH4}}


def _arrays(d, names=NAMES):
    return {k: d.scene_array(k) for k in names}


def _same(got, want, what):
    for k in want:
        assert len(got[k]) == len(want[k]) and np.array_equal(got[k], want[k]), f"{what}: {k} differs ({len(got[k])} / {len(want[k])} bytes)"


def _fresh(sa, names=NAMES, from_bvh2=False, **kw):
    d = Device(Wd, Hd, **kw)
    try:
        d.upload(sa, from_bvh2=from_bvh2)
        return _arrays(d, names), d.kernel_info()
    finally:
        d.close()


def _check(d, sa_want, what, names=NAMES, from_bvh2=False, **kw):
    """The reference: a fresh upload of the host mirror's arrays (test_gpu_ranges._check's, with the root entries)."""
    want, info = _fresh(sa_want, names, from_bvh2, **kw)
    _same(_arrays(d, names), want, what)
    assert d.kernel_info() == info, (what, d.kernel_info(), info)
    return want


def _interiors(sa):
    return [(m - 1) // 2 for _, m, _, _ in RC.blocks(sa)]


@pytest.mark.parametrize("kind", list(KINDS))
@pytest.mark.parametrize("fb", CPU.XS)
def test_refit_and_kept_ranges_give_the_arrays_of_the_host_mirror(fb, kind):
    """["keep", X, "refit"]: BLAS 1 scrambled and rebuilt, so BLAS 2 moves, and BLAS 2 jittered and refit.  Then ["refit", "keep", X] with
    the light moved: the leaf root is refit (a leaf root entry, the light records), BLAS 1 - built by the first call - is kept."""
    kw = KINDS[kind]
    bvh4 = kind == "bvh4"
    names = NAMES4 if bvh4 else NAMES
    x, opt = RC.X_OF[fb], CPU.OPT[fb]
    s = RC.scene(first_build=fb)
    sa0 = RR.snap(s.arrays(bvh4=bvh4))
    p1 = RR.prims_of(RR.per_blas(None, R.scramble(), R.jitter(0.05)))
    p2 = RR.prims_of(R.lights_moved())
    d = Device(Wd, Hd, **kw)
    try:
        d.upload(sa0, from_bvh2=bvh4)
        st = d.rebuild_ranges(["keep", x, "refit"], p1[1:], 1, **opt)
        want = RR.snap(RC.host_ranges(s, ["keep", x, "refit"], p1[1:], 1, bvh4=bvh4, **opt))
        assert RC.blocks(want)[2][0] != RC.blocks(sa0)[2][0]                       # the refit block moved
        assert st["blas_built"] == 1 and st["nodes"] == len(want.bvh2) and st["n_idx"] == len(want.primIdx)
        _check(d, want, f"{fb} / {kind}: keep, {x}, refit", names, from_bvh2=bvh4, **kw)
        info = d.ranges_info()
        assert (info["built"], info["kept"], info["refit"]) == (1, 1, 1) and info["leaves_refit"] == _interiors(want)[2] + 1, info
        st = d.rebuild_ranges(["refit", "keep", x], p2[:1], 0, **opt)
        want = RR.snap(RC.host_ranges(s, ["refit", "keep", x], p2[:1], 0, bvh4=bvh4, **opt))
        assert st["blas_built"] == 1
        _check(d, want, f"{fb} / {kind}: refit, keep, {x}", names, from_bvh2=bvh4, **kw)
        assert d.ranges_info()["leaves_refit"] == 1
    finally:
        d.close()


def test_refitting_every_range_is_the_whole_scene_refit_and_the_update():
    s = RC.scene(first_build="sbvh")
    sa0 = RR.snap(s.arrays(bvh4=False))
    p = RR.prims_of(R.jitter(0.05))
    inst = sa0.blas.copy()
    inst["invT"][1] = np.asarray(C.invT(C.rot(1, 40.0), (0.2, 0.1, -0.3)), np.float32).reshape(inst["invT"][1].shape)
    devs = [Device(Wd, Hd) for _ in range(3)]
    try:
        for d in devs:
            d.upload(sa0)
        devs[0].rebuild_ranges(["refit"] * 3, p, 0, inst)
        devs[1].rebuild_scene(p, 0, inst, builder="refit")
        devs[2].update_scene(p, 0, inst)
        ref = _check(devs[0], RB.host_refit(s, p, inst), "three refits")
        _same(_arrays(devs[1]), ref, "rebuild_scene(builder='refit')")
        _same(_arrays(devs[2]), ref, "update_scene")
        info = devs[0].ranges_info()
        assert (info["built"], info["kept"], info["refit"], info["nodes_numbered"], info["pairs_derived"]) == (0, 0, 3, 0, 0), info
        assert all(v == 0 for v in devs[1].ranges_info().values())                  # (no rebuild_ranges call there)
    finally:
        for d in devs:
            d.close()


@pytest.mark.parametrize("move", list(CPU.MOVES))
def test_what_reads_the_relocated_topology(move):
    """After ["keep", X, "keep"] the parent links, the leaf runs and pairNode of BLAS 0 and 2 are relocated copies: update_scene and the
    whole-scene refit climb them, and a second plan keeps blocks whose leaf runs are now in rebuild order."""
    d0, d1 = (f() for f in CPU.MOVES[move])
    s = RC.scene(RC.only(1, d0), "sbvh")
    sa0 = RR.snap(s.arrays(bvh4=False))
    p1 = RR.prims_of(RC.only(1, d1))
    d = Device(Wd, Hd)
    try:
        d.upload(sa0)
        d.rebuild_ranges(["keep", "sbvh_gpu", "keep"], p1[1:38], 1, alpha=0.0)
        _check(d, RC.host_ranges(s, ["keep", "sbvh_gpu", "keep"], p1[1:38], 1, alpha=0.0), f"{move}: keep, sbvh_gpu, keep")
        p2 = RR.prims_of(R.jitter(0.05))                                            # every primitive moves
        d.update_scene(p2, 0)
        _check(d, RB.host_refit(s, p2), f"{move}: update_scene on the relocated topology")
        p3 = RR.prims_of(R.jitter(0.03, seed=5))
        d.rebuild_scene(p3, 0, None, builder="refit")
        _check(d, RB.host_refit(s, p3), f"{move}: the whole-scene refit on the relocated topology")
        p4 = RR.prims_of(R.lights_moved())
        d.rebuild_ranges(["refit", "keep", "keep"], p4[:1], 0)
        _check(d, RC.host_ranges(s, ["refit", "keep", "keep"], p4[:1], 0), f"{move}: refit, keep, keep")
    finally:
        d.close()


def test_ranges_info_counts_what_was_queued():
    s = RC.scene(first_build="sah")
    sa0 = RR.snap(s.arrays(bvh4=False))
    p1 = RR.prims_of(RC.only(1, R.scramble()))
    d = Device(Wd, Hd)
    try:
        d.upload(sa0)
        assert all(v == 0 for v in d.ranges_info().values())
        d.rebuild_ranges(["keep", "sah", "keep"], p1[1:38], 1)
        want = RR.snap(RC.host_ranges(s, ["keep", "sah", "keep"], p1[1:38], 1))
        blk, ints = RC.blocks(want), _interiors(want)
        assert d.ranges_info() == dict(built=1, kept=2, refit=0, pairs_derived=ints[1], pairs_relocated=ints[0] + ints[2], slots_derived=blk[1][3],
                                       slots_relocated=blk[0][3] + blk[2][3], nodes_numbered=blk[1][1], leaves_refit=0), d.ranges_info()
        _check(d, want, "keep, sah, keep")
        # the rigid-body frame: every tree kept, new instance transforms
        inst = want.blas.copy()
        inst["invT"][0] = np.asarray(C.invT(C.rot(1, 40.0), (0.2, 0.1, -0.3)), np.float32).reshape(inst["invT"][0].shape)
        inst["invT"][3] = np.asarray(C.invT(np.eye(3), (-1.0, 0.4, 0.2)), np.float32).reshape(inst["invT"][3].shape)
        d.rebuild_ranges(["keep"] * 3, None, 0, inst)
        info = d.ranges_info()
        assert (info["built"], info["kept"], info["pairs_derived"], info["slots_derived"], info["nodes_numbered"]) == (0, 3, 0, 0, 0), info
        assert info["pairs_relocated"] == sum(ints) and info["slots_relocated"] == len(want.primIdx)
        _check(d, RC.host_ranges(s, ["keep"] * 3, inst=inst), "three kept ranges under new transforms")
        d.rebuild_ranges(["sah", "lbvh", "sah"])
        want = RR.snap(RC.host_ranges(s, ["sah", "lbvh", "sah"]))
        info = d.ranges_info()
        assert (info["built"], info["kept"], info["refit"], info["pairs_relocated"], info["slots_relocated"]) == (3, 0, 0, 0, 0), info
        assert info["pairs_derived"] == sum(_interiors(want)) and info["nodes_numbered"] == len(want.bvh2) and info["slots_derived"] == len(want.primIdx)
        _check(d, want, "an all-built plan")
    finally:
        d.close()


PLAN = ["keep", "refit", "lbvh"]


def test_a_frame_and_traced_rays_after_a_plan_with_a_refit_range():
    s = RC.scene(first_build="sbvh")
    sa0 = RR.snap(s.arrays(bvh4=False))
    p = RR.prims_of(R.jitter(0.05))
    cam = scenes.camera_for(RC.VIEW, Wd, Hd)
    d, f = Device(Wd, Hd, **DEFAULT), Device(Wd, Hd, **DEFAULT)
    try:
        d.upload(sa0)
        d.rebuild_ranges(PLAN, p[1:], 1)
        want = RR.snap(RC.host_ranges(s, PLAN, p[1:], 1, bvh4=True))
        d.seed_default()
        d.render(cam, 1)
        assert_bits(d.read_accum(), Oracle(want, Wd, Hd, **DEFAULT).render(cam, 1)[0], "one frame after keep, refit, lbvh vs the oracle")
        f.upload(want)
        rng = np.random.default_rng(4)
        o = rng.uniform(-3, 3, (4096, 3)).astype(np.float32) + np.float32([0, 0, 8])
        dirs = rng.normal(size=(4096, 3)).astype(np.float32) - np.float32([0, 0, 2])
        dirs /= np.linalg.norm(dirs, axis=1, keepdims=True)
        got, ref = d.trace(o, dirs)["hit"], f.trace(o, dirs)["hit"]
        assert np.array_equal(got.view(np.uint8), ref.view(np.uint8)), "closest hits differ from a fresh context's"
        assert (ref["primIdx"] >= 0).sum() >= 100
    finally:
        f.close()
        d.close()


def test_a_sharing_partner_and_a_group_render_the_refit_scene():
    s = RC.scene(first_build="sbvh")
    sa0 = RR.snap(s.arrays(bvh4=False))
    p = RR.prims_of(R.jitter(0.05))
    cam = scenes.camera_for(RC.VIEW, Wd, Hd)
    a, b = Device(Wd, Hd, **DEFAULT), Device(Wd, Hd, **DEFAULT)
    g = Group(Wd, Hd, lanes=2)
    try:
        a.upload(sa0)
        b.share_scene(a)
        g.upload(sa0)
        b.seed_default()
        b.render(cam, 1)          # a frame in flight on a holder that is not the one rebuilding
        a.rebuild_ranges(PLAN, p[1:], 1)
        g.rebuild_ranges(PLAN, p[1:], 1)
        want = RR.snap(RC.host_ranges(s, PLAN, p[1:], 1, bvh4=True))
        ref_arrays, info = _fresh(want, **DEFAULT)
        _same(_arrays(b), ref_arrays, "the sharing partner's arrays")
        _same(_arrays(g.devs[1]), ref_arrays, "lane 1's arrays")
        assert b.kernel_info() == info
        b.seed_default()
        b.reset()
        b.render(cam, 1)
        assert_bits(b.read_accum(), Oracle(want, Wd, Hd, **DEFAULT).render(cam, 1)[0], "the sharing partner's next frame")
    finally:
        g.close()
        b.close()
        a.close()


def test_refusals_change_nothing():
    s = RC.scene(first_build="sbvh")
    sa0 = RR.snap(s.arrays(bvh4=False))
    p = RR.prims_of(R.jitter(0.05))
    cam = scenes.camera_for(RC.VIEW, Wd, Hd)
    d = Device(Wd, Hd, **DEFAULT)
    try:
        d.upload(sa0)
        before = _arrays(d)
        for what, code, match, args in [
            ("word 3", W.RT_E_INVALID, "RT_REBUILD_REFIT", (["keep", W.REBUILD_REFIT, "refit"],)),
            ("a window in a kept range beside a refit one", W.RT_E_INVALID, "intersect BLAS 2", (["keep", "refit", "keep"], p[30:50], 30)),
        ]:
            with pytest.raises(RtError, match=match) as e:
                d.rebuild_ranges(*args)
            assert e.value.code == code, what
            _same(_arrays(d), before, what)
        assert all(v == 0 for v in d.ranges_info().values())
        d.seed_default()
        d.render(cam, 1)
        assert_bits(d.read_accum(), Oracle(s.arrays(), Wd, Hd, **DEFAULT).render(cam, 1)[0], "the next frame after the refusals")
    finally:
        d.close()
    _, holed = CPU.with_a_hole()
    d = Device(Wd, Hd, **DEFAULT)
    try:
        d.upload(holed)
        before = _arrays(d)
        with pytest.raises(RtError, match=r"BLAS 1 \(primitives \[1, 38\)\)") as e:
            d.rebuild_ranges(["keep", "refit", "keep"])
        assert e.value.code == W.RT_E_UNSUPPORTED
        _same(_arrays(d), before, "a refused refit of a BLAS that is not compact")
        d.seed_default()
        d.render(cam, 1)
        assert_bits(d.read_accum(), Oracle(RC.scene().arrays(), Wd, Hd, **DEFAULT).render(cam, 1)[0], "the next frame after the refused refit")
    finally:
        d.close()


@pytest.mark.parametrize("cap", [None, "16"], ids=["default", "initial-cap-16"])
def test_alternating_plans_with_refit_ranges_stop_allocating(cap, monkeypatch):
    if cap:
        monkeypatch.setenv("RT355_REBUILD_INITIAL_CAP", cap)
    s = RC.scene(first_build="sbvh")
    d = Device(Wd, Hd)
    try:
        d.upload(RR.snap(s.arrays(bvh4=False)))
        plans = (["keep", "refit", "lbvh"], ["sah", "keep", "refit"])
        counts = []
        for visit in range(4):
            for plan in plans:
                d.rebuild_ranges(plan)
                want = RR.snap(RC.host_ranges(s, plan))
                counts.append(d.rebuild_allocations())
        _check(d, want, f"after {len(counts)} alternating plans")
        assert counts[4] == counts[-1], counts
    finally:
        d.close()

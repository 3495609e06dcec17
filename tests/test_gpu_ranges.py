"""Per-range rebuild plans on the MI355X (rt_rebuild_ranges / rt_group_rebuild_ranges): a BLAS the plan keeps is moved by
k_blas_relocate, the others are built, and afterwards the device arrays (sizes included) and kernel_info are those of a fresh upload of
the host mirror's scene - which for "keep what did not change" is the scene a full rebuild gives.  All comparisons are byte for byte."""
import numpy as np
import pytest

import ranges_check as RC
import rebuild_check as RB
import refit_check as R
import test_ranges_cpu as CPU
from helpers import DEFAULT, assert_bits
from magr_ray_tracer_amd import _lib as W, scenes
from magr_ray_tracer_amd.renderer import Device, Group, RtError
from oracle.oracle_py import Oracle, seed_stream

pytestmark = pytest.mark.gpu

Wd, Hd = 160, 120
MIXED = {"sah": ["lbvh", "keep", "sbvh_gpu"], "sbvh": ["lbvh", "keep", "sah"], "lbvh": ["keep", "sah", "keep"]}


def _arrays(d, names=W.SCENE_ARRAYS):
    return {k: d.scene_array(k) for k in names}


def _same(got, want, what):
    for k in want:
        assert len(got[k]) == len(want[k]) and np.array_equal(got[k], want[k]), f"{what}: {k} differs ({len(got[k])} / {len(want[k])} bytes)"


def _fresh(sa, names=W.SCENE_ARRAYS, from_bvh2=False, **kw):
    d = Device(Wd, Hd, **kw)
    try:
        d.upload(sa, from_bvh2=from_bvh2)
        return _arrays(d, names), d.kernel_info()
    finally:
        d.close()


def _check(d, sa_want, what, names=W.SCENE_ARRAYS, from_bvh2=False, **kw):
    want, info = _fresh(sa_want, names, from_bvh2, **kw)
    _same(_arrays(d, names), want, what)
    assert d.kernel_info() == info, (what, d.kernel_info(), info)
    return want


@pytest.mark.parametrize("fb,r,move", CPU.CASES, ids=[f"{a}-r{b}-{c}" for a, b, c in CPU.CASES])
def test_keeping_the_unchanged_blas_equals_rebuilding_everything(fb, r, move):
    """Context A rebuilds everything, context B keeps what did not change: both hold the arrays of a fresh upload of the scene rebuilt
    on the host, which rests on the builders alone."""
    s, sa0, window, plan, want = CPU.keep_and_build(fb, r, move)
    a, b = Device(Wd, Hd), Device(Wd, Hd)
    try:
        a.upload(sa0)
        b.upload(sa0)
        assert [(k["prim_first"], k["prim_count"], k["compact"]) for k in b.blas_blocks()] == [(f, c, True) for f, c in zip(RC.FIRST, RC.COUNTS)]
        a.rebuild_scene(window, RC.FIRST[r], None, builder=RC.X_OF[fb], **CPU.OPT[fb])
        st = b.rebuild_ranges(plan, window, RC.FIRST[r], **CPU.OPT[fb])
        assert st["blas_built"] == 1 and st["nodes"] == len(want.bvh2) and st["n_idx"] == len(want.primIdx)
        ref = _check(b, want, f"{fb}: keep all but range {r} ({move})")
        _same(_arrays(a), ref, "the full rebuild")
        assert a.kernel_info() == b.kernel_info()
        assert [(k["nodes"], k["idx_slots"]) for k in b.blas_blocks()] == [(m, n) for _, m, _, n in RC.blocks(want)]
    finally:
        b.close()
        a.close()


@pytest.mark.parametrize("accel", [W.ACCEL_BVH2, W.ACCEL_BVH4], ids=["bvh2", "bvh4"])
@pytest.mark.parametrize("fb", CPU.XS)
def test_mixed_plans_give_the_arrays_of_the_host_mirror(fb, accel):
    """Builders differ from BLAS to BLAS in one call, next to a kept BLAS; a BVH4 context bound with its BVH2 collapses the result."""
    bvh4 = accel == W.ACCEL_BVH4
    names = {**W.SCENE_ARRAYS, **W.SCENE_ARRAYS_BVH4} if bvh4 else W.SCENE_ARRAYS
    s = RC.scene(first_build=fb)
    sa0 = s.arrays(bvh4=bvh4)
    prims = RC.scene(R.jitter(0.05), "sah").arrays(bvh4=False).prims
    plan = MIXED[fb]
    last = max(k for k in range(3) if plan[k] != "keep")   # the replaced primitives: those of the last built BLAS (triangles: jitter moves them)
    lo, hi = RC.FIRST[last], RC.FIRST[last] + RC.COUNTS[last]
    opt = {"alpha": 0.0} if "sbvh_gpu" in plan else {}
    d = Device(Wd, Hd, accel=accel)
    try:
        d.upload(sa0, from_bvh2=bvh4)
        st = d.rebuild_ranges(plan, prims[lo:hi], lo, **opt)
        assert st["blas_built"] == sum(w != "keep" for w in plan)
        want = RC.host_ranges(s, plan, prims[lo:hi], lo, bvh4=bvh4, **opt)
        _check(d, want, f"{fb} / {plan}", names, from_bvh2=bvh4, accel=accel)
    finally:
        d.close()


def test_a_frame_and_traced_rays_after_a_mixed_plan():
    s = RC.scene(first_build="sbvh")
    sa0 = s.arrays(bvh4=False)
    cam = scenes.camera_for(RC.VIEW, Wd, Hd)
    d, f = Device(Wd, Hd, **DEFAULT), Device(Wd, Hd, **DEFAULT)
    try:
        d.upload(sa0)
        d.rebuild_ranges(MIXED["sbvh"])
        want = RC.host_ranges(s, MIXED["sbvh"], bvh4=True)
        d.seed_default()
        d.render(cam, 1)
        assert_bits(d.read_accum(), Oracle(want, Wd, Hd, **DEFAULT).render(cam, 1)[0], "one frame after a mixed plan vs the oracle")
        f.upload(want)
        rng = np.random.default_rng(4)
        o = rng.uniform(-3, 3, (4096, 3)).astype(np.float32) + np.float32([0, 0, 8])
        dirs = rng.normal(size=(4096, 3)).astype(np.float32) - np.float32([0, 0, 2])
        dirs /= np.linalg.norm(dirs, axis=1, keepdims=True)
        got, ref = d.trace(o, dirs)["hit"], f.trace(o, dirs)["hit"]
        assert np.array_equal(got.view(np.uint8), ref.view(np.uint8)), "closest hits differ from a fresh context's"
        assert (ref["primIdx"] >= 0).sum() > 100
    finally:
        f.close()
        d.close()


def test_a_sharing_partner_and_a_group_render_the_new_scene():
    s = RC.scene(first_build="sbvh")
    sa0 = s.arrays(bvh4=False)
    plan = MIXED["sbvh"]
    cam = scenes.camera_for(RC.VIEW, Wd, Hd)
    a, b = Device(Wd, Hd, **DEFAULT), Device(Wd, Hd, **DEFAULT)
    g = Group(Wd, Hd, lanes=2)
    try:
        a.upload(sa0)
        b.share_scene(a)
        g.upload(sa0)
        b.seed_default()
        b.render(cam, 1)          # work in flight on a holder that is not the one rebuilding
        a.rebuild_ranges(plan)
        g.rebuild_ranges(plan)
        want = RC.host_ranges(s, plan, bvh4=True)
        ref_arrays, info = _fresh(want, **DEFAULT)
        _same(_arrays(b), ref_arrays, "the sharing partner's arrays")
        _same(_arrays(g.devs[1]), ref_arrays, "lane 1's arrays")
        assert b.kernel_info() == info
        ref = Oracle(want, Wd, Hd, **DEFAULT).render(cam, 1)[0]
        b.seed_default()
        b.reset()
        b.render(cam, 1)
        assert_bits(b.read_accum(), ref, "the sharing partner after a per-range rebuild")
        g.seed(0)
        g.reset()
        g.render(cam, 2)
        exp = sum(Oracle(want, Wd, Hd, **DEFAULT).render(cam, 1, seeds=seed_stream(m * Wd * Hd, Wd * Hd))[0] for m in range(2))
        assert_bits(g.read_accum(), exp, "2-lane group after a per-range rebuild")
    finally:
        g.close()
        b.close()
        a.close()


def test_calls_chain():
    """rebuild_ranges -> update_scene -> rebuild_scene(refit) -> rebuild_ranges keeping what the first one built."""
    s = RC.scene(first_build="sbvh")
    p1 = RC.scene(R.jitter(0.05), "sah").arrays(bvh4=False).prims
    p2 = RC.scene(R.jitter(0.03, seed=5), "sah").arrays(bvh4=False).prims
    p3 = RC.scene(RC.only(1, R.scramble()), "sah").arrays(bvh4=False).prims
    d = Device(Wd, Hd)
    try:
        d.upload(s.arrays(bvh4=False))
        d.rebuild_ranges(["keep", "keep", "lbvh"], p1[38:], 38, max_leaf=4)
        _check(d, RC.host_ranges(s, ["keep", "keep", "lbvh"], p1[38:], 38, max_leaf=4), "ranges 1")
        inst = s.arrays(bvh4=False).blas.copy()
        d.update_scene(p2, 0, inst)
        _check(d, RB.host_refit(s, p2, inst), "update")
        d.rebuild_scene(p1, 0, None, builder="refit")
        _check(d, RB.host_refit(s, p1), "refit")
        st = d.rebuild_ranges(["sah", "sbvh_gpu", "keep"], p3[:38], 0, alpha=0.0)     # BLAS 2: the linear tree of the first call, refit twice
        assert st["blas_built"] == 2
        _check(d, RC.host_ranges(s, ["sah", "sbvh_gpu", "keep"], p3[:38], 0, alpha=0.0), "ranges 2")
    finally:
        d.close()


def test_refusals_change_nothing():
    s = RC.scene(first_build="sbvh")
    sa0 = s.arrays(bvh4=False)
    p1 = RC.scene(R.jitter(0.05), "sah").arrays(bvh4=False).prims
    cam = scenes.camera_for(RC.VIEW, Wd, Hd)
    d = Device(Wd, Hd, **DEFAULT)
    try:
        d.upload(sa0)
        before = _arrays(d)
        bad_type = p1[:1].copy()
        bad_type["objType"] = W.PRIM_SPHERE
        for what, code, match, args, kw in [
            ("too few words", W.RT_E_INVALID, "3 distinct BLAS", (["keep", "sah"],), {}),
            ("no words", W.RT_E_INVALID, "null plan", ([],), {}),
            ("an unknown word", W.RT_E_INVALID, "unknown word 9", (["keep", 9, "keep"],), {}),
            ("refit in a plan", W.RT_E_INVALID, "RT_REBUILD_REFIT", (["keep", W.REBUILD_REFIT, "keep"],), {}),
            ("a window in a kept range", W.RT_E_INVALID, "intersect BLAS 2", (["keep", "sah", "keep"], p1[30:50], 30), {}),
            ("a window outside", W.RT_E_INVALID, "outside", (["sah"] * 3, p1[:10], 250), {}),
            ("a changed objType", W.RT_E_INVALID, "objType", (["sah", "keep", "keep"], bad_type, 0), {}),
            ("alpha", W.RT_E_INVALID, "alpha", (["keep", "sbvh_gpu", "keep"],), {"alpha": 2.0}),
            ("an LBVH option", W.RT_E_INVALID, "max_leaf", (["keep", "lbvh", "keep"],), {"max_leaf": 0}),
        ]:
            with pytest.raises(RtError, match=match) as e:
                d.rebuild_ranges(*args, **kw)
            assert e.value.code == code, what
            _same(_arrays(d), before, what)
        d.seed_default()
        d.render(cam, 1)
        assert_bits(d.read_accum(), Oracle(s.arrays(), Wd, Hd, **DEFAULT).render(cam, 1)[0], "the next frame after the refusals")
    finally:
        d.close()
    # what rt_rebuild_scene refuses: a BVH4 copy bound without its BVH2
    d = Device(Wd, Hd, accel=W.ACCEL_BVH4)
    try:
        d.upload(s.arrays())
        with pytest.raises(RtError, match="lost its BVH2") as e:
            d.rebuild_ranges(["keep", "sah", "keep"])
        assert e.value.code == W.RT_E_UNSUPPORTED
    finally:
        d.close()


def test_a_blas_that_is_not_compact_is_built_not_kept():
    sa, holed = CPU.with_a_hole()
    d = Device(Wd, Hd)
    try:
        d.upload(holed)
        before = _arrays(d)
        assert [k["compact"] for k in d.blas_blocks()] == [True, False, True]
        with pytest.raises(RtError, match=r"BLAS 1 \(primitives \[1, 38\)\)") as e:
            d.rebuild_ranges(["keep", "keep", "keep"])
        assert e.value.code == W.RT_E_UNSUPPORTED
        _same(_arrays(d), before, "a refused keep")
        d.rebuild_ranges(["keep", "sah", "keep"])
        _check(d, sa, "the hole closed by building BLAS 1")     # (the SAH builder's own tree is what the scene was made of)
        assert all(k["compact"] for k in d.blas_blocks())
    finally:
        d.close()


@pytest.mark.parametrize("cap", [None, "16"], ids=["default", "initial-cap-16"])
def test_alternating_plans_stop_allocating(cap, monkeypatch):
    """Two plans in turn on the SBVH-bound scene: by the third visit to each, no call allocates.  With a small initial capacity the kept
    SBVH blocks, which hold more slots than primitives, go through the growth path."""
    if cap:
        monkeypatch.setenv("RT355_REBUILD_INITIAL_CAP", cap)
    s = RC.scene(first_build="sbvh")
    d = Device(Wd, Hd)
    try:
        d.upload(s.arrays(bvh4=False))
        plans = (["keep", "keep", "lbvh"], ["sah", "keep", "keep"])
        counts = []
        for visit in range(4):
            for plan in plans:
                d.rebuild_ranges(plan)
                want = RC.host_ranges(s, plan)
                counts.append(d.rebuild_allocations())
        _check(d, want, f"after {len(counts)} alternating plans")
        assert counts[4] == counts[-1], counts
    finally:
        d.close()

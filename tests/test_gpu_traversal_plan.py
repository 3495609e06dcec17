"""A context configures itself as the device-free plan says (csrc/trav_common.h; tests/test_traversal_plan_cpu.py pins the plan's rules):
on the smallest scenes that reach each kind of traversal, traversal_plan(dev.traversal_facts()) agrees with kernel_info() and
top_levels(), for a context alone, for one that shares the GPU, and after a rebuild that changes the trees' depth."""
import pytest

import rebuild_check as RB
import refit_check as R
from magr_ray_tracer_amd import _lib as W, scenes
from magr_ray_tracer_amd.renderer import Device, traversal_plan
from test_traversal_plan_cpu import KNOBS

pytestmark = pytest.mark.gpu

Wd, Hd = 32, 32
# RtTraversalPlan.trav -> (RtKernelInfo.persist, RtKernelInfo.persist4)
REPORTED = {W.TRAV_NESTED: (0, 0), W.TRAV_BVH2: (1, 0), W.TRAV_TLAS: (2, 0), W.TRAV_TLAS_SPILL: (3, 0), W.TRAV_BVH4: (0, 1), W.TRAV_BVH4_TLAS: (0, 2),
            W.TRAV_BVH4_TLAS_SPILL: (0, 3)}
_SC = {}


def _scene(blas):
    """(arrays, arrays of the scrambled scene built from scratch: another depth, view): the one- and two-BLAS scenes of the rebuild tests."""
    if blas not in _SC:
        (_, sa0), (_, sa1), view = RB.pair(R.scramble(), "sah", "sah", blas)
        _SC[blas] = (sa0, sa1, view)
    return _SC[blas]


def _agrees(d, trav, what):
    """The plan of the context's facts is of kind `trav`, and the context reports what that plan says."""
    facts, info, top = d.traversal_facts(), d.kernel_info(), d.top_levels()
    plan = traversal_plan(facts)
    assert plan["trav"] == trav, (what, plan, facts)
    assert (info["persist"], info["persist4"]) == REPORTED[trav], (what, info, plan)
    spills = trav in (W.TRAV_TLAS_SPILL, W.TRAV_BVH4_TLAS_SPILL)
    assert info["stack_entries"] == (plan["spillCap"] if spills else facts["stackEntries"]), (what, info, plan, facts)
    assert info["layout"] == facts["layout"] and (facts["singleBlas"] == 1) == (info["n_blas"] == 1), (what, info, facts)
    limit = plan["tune"]["topLevels"], plan["tuneConnect"]["topLevels"]
    assert 0 <= top[0] <= limit[0] and 0 <= top[1] <= limit[1], (what, top, limit)       # fitted to the device: never deeper than planned
    if not plan["topAuto"]:
        assert top == limit, (what, top, limit)
    return facts, plan


# name: (BLAS, Device arguments, environment, the kind)
CASES = {
    "one BLAS, BVH2": (1, {}, {}, W.TRAV_BVH2),
    "one BLAS, BVH4": (1, dict(accel=W.ACCEL_BVH4), {}, W.TRAV_BVH4),
    "two BLAS, BVH2": (2, {}, {}, W.TRAV_TLAS),
    "two BLAS, BVH2, SPILL_CAP=6": (2, {}, {"RT355_SPILL_CAP": "6"}, W.TRAV_TLAS_SPILL),
    "two BLAS, BVH4, extend_variant 6": (2, dict(accel=W.ACCEL_BVH4, extend_variant=6), {}, W.TRAV_BVH4_TLAS),
    "layout 0": (1, dict(extend_variant=1), {}, W.TRAV_NESTED),
    "one BLAS, BVH2, TOP_LEVELS=2,1": (1, {}, {"RT355_TOP_LEVELS": "2,1"}, W.TRAV_BVH2),
}


@pytest.mark.parametrize("case", list(CASES))
def test_a_context_runs_what_the_plan_says(case, monkeypatch):
    blas, kw, env, trav = CASES[case]
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    sa, _, view = _scene(blas)
    d = Device(Wd, Hd, **kw)
    try:
        d.upload(sa)
        d.seed_default()
        d.render(scenes.camera_for(view, Wd, Hd), 1)
        d.synchronize()
        facts, plan = _agrees(d, trav, case)
        assert facts["sharedMemPerBlock"] >= 65536 and 0 <= facts["xcdFirst"] < 8, facts
        assert plan["tune"]["leafK"] == 8 and plan["tune"]["fixedChunks"] == 1, plan        # alone on the GPU
        if "RT355_TOP_LEVELS" in env:
            assert d.top_levels() == (2, 1)
        if case == "layout 0":
            assert facts["layout"] == 0
    finally:
        d.close()


def test_a_lane_that_shares_the_gpu_plans_leafk_16(monkeypatch):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    sa, _, _ = _scene(1)
    d = Device(Wd, Hd, persist_blocks_per_cu=2)
    try:
        d.upload(sa)
        facts, plan = _agrees(d, W.TRAV_BVH2, "a shared context")
        assert facts["persist_blocks_per_cu"] == 2 and plan["tune"]["leafK"] == 16 and plan["tune"]["fixedChunks"] == 0 and plan["topAuto"], (facts, plan)
    finally:
        d.close()


def test_the_facts_follow_a_rebuild(monkeypatch):
    """The scrambled two-BLAS scene builds to another depth: the facts take the new stackEntries, and plan and context still agree."""
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    sa0, sa1, _ = _scene(2)
    assert RB.depth(sa0) != RB.depth(sa1)
    d, f = Device(Wd, Hd), Device(Wd, Hd)
    try:
        d.upload(sa0)
        before, _ = _agrees(d, W.TRAV_TLAS, "before the rebuild")
        d.rebuild_scene(sa1.prims, 0, None, builder="sah")
        after, _ = _agrees(d, W.TRAV_TLAS, "after the rebuild")
        f.upload(sa1)
        fresh = f.traversal_facts()
        assert after["stackEntries"] == fresh["stackEntries"] != before["stackEntries"], (before, after, fresh)
        assert {k: v for k, v in after.items() if k != "xcdFirst"} == {k: v for k, v in fresh.items() if k != "xcdFirst"}, (after, fresh)
    finally:
        d.close()
        f.close()

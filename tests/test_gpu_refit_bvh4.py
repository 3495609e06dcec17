"""rt_rebuild_scene with RT_REBUILD_REFIT (Device.rebuild_scene(builder="refit")) on the MI355X: the refit every context takes.  A BVH4
copy bound with its BVH2 ends up, array for array and in kernel_info, as a classic upload of the scene refit and collapsed on the host,
whether the live records were rewritten in place (refit_info path 1), re-collapsed because a slot changed (2) or because the
environment forced it (3); frames and traced rays match a fresh context's; refits chain with rebuilds without allocating; a BVH2
context gets rt_update_scene's arrays; and every refusal leaves the bound scene, and the tables the next refit needs, as they were."""
import os
import subprocess
import sys

import numpy as np
import pytest

import rebuild_check as RB
import refit_bvh4_check as F
import refit_check as R
import test_gpu_rebuild_bvh4 as TB
import test_gpu_refit as RF
import test_groundtruth_cpu as C
from helpers import DEFAULT, assert_bits
from magr_ray_tracer_amd import _lib as W, scenes
from magr_ray_tracer_amd.renderer import Device, Group, RtError

pytestmark = pytest.mark.gpu

Wd, Hd, B4 = TB.Wd, TB.Hd, TB.B4
T4 = [None, RB.ROT, C.TRANSFORMS["scale"], C.TRANSFORMS["mirror"]]
# traversal path: (BLAS of `keep`, their transforms, extra BLAS of `flip`, extend_variant, what kernel_info must say)
PATHS = {"persist4": (1, None, 0, 0, dict(persist4=1)), "nested": (4, T4, 2, 0, dict(persist4=0, persist=0, layout=1)),
         "persist4-tlas": (2, [None, RB.ROT], 1, 6, dict(persist4=2))}
IN_PLACE, RECOLLAPSED, FORCED = 1, 2, 3


def _fixture(name, path):
    """(Scene, its arrays, view, [(primitives handed over, the path refit_info must report or None)])"""
    blas, T, extra, _, _ = PATHS[path]
    if name == "keep":
        s, sa, view, prims = F.keep_scene(blas, transforms=T)
        return s, sa, view, [(prims, None), (prims, IN_PLACE)]
    s = F.flip_scene(extra)
    sa = s.arrays()
    return s, sa, F.FLIP_VIEW, [(F.flip_prims(sa.prims, name[5:]), RECOLLAPSED)]


def _refit(d, prims=None, inst=None, first=0):
    return d.rebuild_scene(prims, first, inst, builder="refit")


def _frame(d, cam):
    d.seed_default()
    d.reset()
    d.render(cam, 1)
    return d.read_accum()


def _check_refit(d, st, want, path, what, **kw):
    """After a refit: stats, refit_info, arrays and kernel_info against the host-refit scene `want` (BVH4 by BuildBVH4)."""
    live, need = F.host_live(want)
    info = d.refit_info()
    assert path is None or info["path"] == path, (what, info)
    assert (info["changed_nodes"] > 0) == (info["path"] == RECOLLAPSED), (what, info)
    assert info["live_quads"] == live and info["stack_need"] == need, (what, info, live, need)
    assert st["blas_built"] == 0 and st["spatial_splits"] == 0 == st["prims_clipped"], (what, st)
    assert st["nodes"] == len(want.bvh2) and st["n_idx"] == len(want.primIdx) and st["max_depth"] == RB.depth(want), (what, st)
    return TB._check(d, want, what, **kw)


# ---- the two fixtures on the three traversal paths ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("path", list(PATHS))
@pytest.mark.parametrize("name", ["keep", "flip-swap", "flip-shrink"])
def test_keep_and_flip_give_the_arrays_and_the_frame_of_a_fresh_upload(name, path):
    s, sa0, view, steps = _fixture(name, path)
    variant, want_info = PATHS[path][3], PATHS[path][4]
    cam = scenes.camera_for(view, Wd, Hd)
    kw = dict(B4, extend_variant=variant)
    d = Device(Wd, Hd, **kw)
    try:
        d.upload(sa0, from_bvh2=True)
        assert d.refit_info()["path"] == 0
        for k, (prims, expect) in enumerate(steps):
            st = _refit(d, prims)
            want = F.host_refit(s, prims)
            info = _check_refit(d, st, want, expect, f"{name} / {path} / step {k}", **kw)
            for key, v in want_info.items():
                assert info[key] == v, (name, path, info)
        got = _frame(d, cam)
        f = Device(Wd, Hd, **kw)
        try:
            f.upload(want)
            ref = _frame(f, cam)
        finally:
            f.close()
        assert np.any(ref[..., :3] > 0), "the reference frame is black"
        assert_bits(got, ref, f"{name} / {path}: the frame after the refit against a fresh context's")
    finally:
        d.close()


# ---- the forced fallback -----------------------------------------------------------------------------------------------------------------
def keep_twice(out=None):
    """`keep` on two BLAS: the arrays and refit_info after the second refit (saved to `out` for the parent process)."""
    s, sa0, _, prims = F.keep_scene(2, transforms=[None, RB.ROT])
    d = Device(Wd, Hd, **B4)
    try:
        d.upload(sa0, from_bvh2=True)
        _refit(d, prims)
        st = _refit(d, prims)
        info = d.refit_info()
        _check_refit(d, st, F.host_refit(s, prims), None, "keep, twice", **B4)
        arrays = TB._arrays(d)
    finally:
        d.close()
    if out:
        np.savez(out, info=np.array([info[k] for k in W.RefitInfo.names]), **arrays)
    return arrays, info


_CHILD = """
import sys
sys.path.insert(0, {tests!r})
import test_gpu_refit_bvh4 as T
T.keep_twice({out!r})
"""


def test_the_forced_fallback_gives_the_bytes_of_the_in_place_path(tmp_path):
    assert "RT355_REFIT_RECOLLAPSE" not in os.environ
    arrays, info = keep_twice()
    assert info["path"] == IN_PLACE and info["changed_nodes"] == 0
    out = str(tmp_path / "forced.npz")
    here = os.path.dirname(os.path.abspath(__file__))
    subprocess.run([sys.executable, "-c", _CHILD.format(tests=here, out=out)], check=True, timeout=300, cwd=os.path.dirname(here),
                   env=dict(os.environ, RT355_REFIT_RECOLLAPSE="1"))
    other = np.load(out)
    forced = dict(zip(W.RefitInfo.names, (int(x) for x in other["info"])))
    assert forced["path"] == FORCED and forced["changed_nodes"] == 0, forced
    assert forced["live_quads"] == info["live_quads"] and forced["stack_need"] == info["stack_need"]
    for k, v in arrays.items():
        assert len(other[k]) == len(v) and np.array_equal(other[k], v), f"{k} differs between the in-place path and the forced fallback"


# ---- chains ------------------------------------------------------------------------------------------------------------------------------
def test_refits_chain_with_a_rebuild_and_a_stable_scene_stops_allocating(monkeypatch):
    monkeypatch.setenv("RT355_REBUILD_INITIAL_CAP", "8")              # every tree-sized array of both sets grows
    gt0, sa0, _ = R.build(blas=4, spheres=2, transforms=T4)
    s = gt0.s
    p1 = R.build(R.jitter(0.05, seed=4), blas=4, spheres=2)[1].prims.copy()
    p2 = R.build(R.jitter(0.3, seed=5), blas=4, spheres=2)[1].prims.copy()
    d = Device(Wd, Hd, **B4)
    try:
        d.upload(sa0, from_bvh2=True)
        st = _refit(d, p1)
        _check_refit(d, st, F.host_refit(s, p1), None, "refit 1", **B4)
        st = _refit(d, p2)
        _check_refit(d, st, F.host_refit(s, p2), None, "refit 2", **B4)
        d.rebuild_scene(p2, 0, None, builder="lbvh")
        TB._check(d, TB._host_rebuild(s, p2, "lbvh"), "the rebuild in between", **B4)
        st = _refit(d, p1)                                           # the live tables are the rebuilt set's
        _check_refit(d, st, F.host_refit(s, p1), None, "refit 3 (of a rebuilt copy)", **B4)
        inst = s.arrays(bvh4=False).blas.copy()
        inst["invT"][2] = C.invT(C.rot(0, 17.0) @ np.diag([1.2, 0.9, 1.0]), (0.1, 0.2, -0.3)).ravel()
        st = _refit(d, None, inst)
        assert st["prims"] == 0
        _check_refit(d, st, F.host_refit(s, None, inst), IN_PLACE, "refit 4 (instances only)", **B4)
        _refit(d, p1[226:448], None, first=226)
        _refit(d, p1[226:448], None, first=226)
        n = d.rebuild_allocations()
        st = _refit(d, p1[226:448], None, first=226)
        assert d.rebuild_allocations() == n, "the third refit of a stable scene allocated"
        s.SetPrimitives(226, p1[226:448])
        _check_refit(d, st, F.host_refit(s), IN_PLACE, "after the stable refits (a slice)", **B4)
    finally:
        d.close()


# ---- a BVH2 context ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", [0, 1])
def test_on_a_bvh2_context_the_refit_leaves_what_update_scene_leaves(variant):
    gt0, sa0, _ = R.build(alpha=0.0, blas=2, spheres=2, transforms=[None, RB.ROT])
    p1 = R.build(R.jitter(0.05, seed=4), alpha=0.0, blas=2, spheres=2)[1].prims.copy()
    inst = sa0.blas.copy()
    inst["invT"][1] = C.invT(C.rot(2, 31.0), (0.3, 0.1, -0.2)).ravel()
    kw = dict(DEFAULT, extend_variant=variant)
    a, b = Device(Wd, Hd, **kw), Device(Wd, Hd, **kw)
    try:
        a.upload(sa0)
        b.upload(sa0)
        for k, (prims, first, ins) in enumerate(((p1, 0, None), (p1[10:200], 10, inst), (None, 0, inst), (p1, 0, None))):
            st = _refit(a, prims, ins, first)
            b.update_scene(prims, first, ins)
            assert a.refit_info() == dict(path=IN_PLACE, live_quads=0, changed_nodes=0, stack_need=st["max_depth"])
            assert st["blas_built"] == 0 and st["nodes"] == len(sa0.bvh2) and st["n_idx"] == len(sa0.primIdx)
            for name in W.SCENE_ARRAYS:
                x, y = a.scene_array(name), b.scene_array(name)
                assert len(x) == len(y) and np.array_equal(x, y), f"step {k}: {name} differs from update_scene's"
            assert a.kernel_info() == b.kernel_info()
        a.update_scene(p1[:5], 0)                                   # (and the refit copy still updates)
    finally:
        b.close()
        a.close()


# ---- refusals ----------------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_scene_and_the_live_tables_as_they_were():
    s, _, view = RF._chain_scene(40)
    sa = s.arrays()                                                  # (with the BVH4, for the classic upload)
    cam = scenes.camera_for(view, Wd, Hd)
    d = Device(Wd, Hd, **B4)
    try:
        d.upload(sa)                                                 # the classic way: the BVH2 is gone
        with pytest.raises(RtError, match="BVH4.*rt_upload_scene_bvh2") as e:
            _refit(d)
        assert e.value.code == W.RT_E_UNSUPPORTED
        d.upload(sa, from_bvh2=True)
        moved = F.jittered(sa.prims, 0.02, seed=3)
        for rounds in range(2):                                      # the second round: the live set is a refit one
            before, info, rinfo = TB._arrays(d), d.kernel_info(), d.refit_info()
            ref = _frame(d, cam)
            bad_type = moved[:4].copy()
            bad_type["objType"][1] = W.PRIM_SPHERE
            sing = sa.blas.copy()
            sing["invT"][3] = 0
            for what, code, args in (("a changed objType", W.RT_E_INVALID, (bad_type, None)), ("a singular invT", W.RT_E_INVALID, (None, sing)),
                                     ("a TLAS 39 levels deep", W.RT_E_UNSUPPORTED, (moved, RF._chain(sa, 40)))):
                with pytest.raises(RtError) as e:
                    _refit(d, *args)
                assert e.value.code == code, (what, str(e.value))
                TB._same(TB._arrays(d), before, f"after {what} (round {rounds})")
                assert np.array_equal(TB._arrays(d)["bvh2Kept"], before["bvh2Kept"])
                assert d.kernel_info() == info and d.refit_info() == rinfo, what
                assert_bits(_frame(d, cam), ref, f"the frame after {what} (round {rounds})")
            st = _refit(d, moved)                                    # the live tables survived the refusals
            _check_refit(d, st, F.host_refit(s, moved), None, f"a refit after the refusals (round {rounds})", **B4)
            moved = F.jittered(sa.prims, 0.02, seed=4)
    finally:
        d.close()


# ---- holders -----------------------------------------------------------------------------------------------------------------------------
def test_group_lanes_a_sharing_partner_and_traced_rays_follow_the_refit():
    s, sa0, view, prims = F.keep_scene(2, transforms=[None, RB.ROT])
    cam = scenes.camera_for(view, Wd, Hd)
    rng = np.random.default_rng(12)
    origins = np.tile(np.array(view["origin"], np.float32), (4096, 1))
    dirs = rng.normal(size=(4096, 3)).astype(np.float32) * np.float32([0.5, 0.5, 0.2]) - np.float32([0, 0, 1])
    a, b, f = Device(Wd, Hd, **B4), Device(Wd, Hd, **B4), Device(Wd, Hd, **B4)
    g, gf = Group(Wd, Hd, lanes=2, **B4), Group(Wd, Hd, lanes=2, **B4)
    try:
        a.upload(sa0, from_bvh2=True)
        b.share_scene(a)
        g.upload(sa0, from_bvh2=True)
        b.seed_default()
        b.render(cam, 1)                                             # work in flight on a holder that is not the one refitting
        _refit(a, prims)
        _refit(g, prims)
        want = F.host_refit(s, prims)
        f.upload(want)
        gf.upload(want)
        want_arrays = TB._arrays(f)
        for h, fresh in ((a, f), (b, f), (g.devs[1], gf.devs[1])):   # (a lane sizes its shade grid for the group: compare lanes with lanes)
            TB._same(TB._arrays(h), want_arrays, "a holder's arrays", want.bvh2)
            assert h.kernel_info() == fresh.kernel_info()
        ref = _frame(f, cam)
        for dv in (a, b):
            assert_bits(_frame(dv, cam), ref, "the shared pair after a refit")
        for grp in (g, gf):
            grp.seed(0)
            grp.reset()
            grp.render(cam, 2)
        assert_bits(g.read_accum(), gf.read_accum(), "the 2-lane group after a refit against a fresh group")
        got, fresh = a.trace(origins, dirs), f.trace(origins, dirs)
        assert np.array_equal(got["hit"], fresh["hit"]) and int((fresh["hit"]["primIdx"] >= 0).sum()) > 400
    finally:
        gf.close()
        g.close()
        f.close()
        b.close()
        a.close()

"""The device TLAS build (k_tlas_build, csrc/refit.hip) at up to 256 instances on the MI355X: after rt_update_scene / rt_rebuild_scene
the eleven device arrays are those of a fresh upload of the scene the host built - on layouts without ties, and on layouts whose ties
only the fold across the four waves decides (tests/tlas_check.py) - up to the depth the traversal stack takes; the no-partner case is
refused and changes nothing; and the traversal kernels walk a device-built 256-instance TLAS to the oracle's frames and the float64
ground truth's hits."""
import numpy as np
import pytest

import builtins_check as B
import geom64 as G
import rebuild_check as RB
import test_gpu_groundtruth as GT
import test_gpu_refit as RF
import test_groundtruth_cpu as C
import test_tlas_cpu as TC
import tlas_check as T
from helpers import DEFAULT, assert_bits, oracle_for
from magr_ray_tracer_amd import _lib as W, scenes
from magr_ray_tracer_amd.renderer import Device, RtError, _rebuild_args, _update_args
from oracle.oracle_py import Oracle, seed_stream

pytestmark = pytest.mark.gpu

Wd, Hd = RF.Wd, RF.Hd


def _frame(d, sa, cam, what):
    """One frame of the bound scene equals the oracle's frame of `sa`, which shows the scene."""
    ref, seeds, e, c = Oracle(sa, Wd, Hd, **DEFAULT).render(cam, 1)
    print(what, "inst_visits / rays", T.assert_seen(e, c, what))
    d.seed_default()
    d.reset()
    d.render(cam, 1)
    assert_bits(d.read_accum(), ref, what)
    return ref


@pytest.mark.parametrize("n", T.NS)
def test_instance_only_updates_give_the_arrays_of_a_fresh_upload(n):
    """random -> mixed -> random by rt_update_scene(NULL, 0, 0, instances)."""
    gt, sa, _ = T.instances_scene(n, "random")
    mixed = T.instances_scene(n, "mixed")[1]
    d = Device(Wd, Hd)
    try:
        d.upload(sa)
        for inst in (mixed.blas, sa.blas):
            st = d.update_scene(None, 0, inst)
            want = RF._host_refit(gt.s, sa.prims, inst)
            assert st["tlas_nodes"] == 2 * n and st["tlas_depth"] == T.tlas_depth(want.tlas)
            RF._same_arrays(RF._arrays(d), RF._fresh(want), f"{n} instances")
    finally:
        d.close()


TIES = [(l, n) for l in ("lattice", "pairs") for n in (64, 65, 255, 256)] + [("stacked", 33)]


@pytest.mark.parametrize("layout,n", TIES, ids=[f"{l}-{n}" for l, n in TIES])
def test_primitive_only_updates_break_every_tie_as_the_host(layout, n):
    """The geometry moves from random places to the tie layouts under identity instances: the refit root boxes are the leaf boxes, and
    the device must choose as the host on every tie."""
    gt, sa, _ = T.instances_scene(n, "random", baked=True, soup=0)
    to = T.instances_scene(n, layout)[1]
    d = Device(Wd, Hd)
    try:
        d.upload(sa)
        st = d.update_scene(to.prims, 0, None)
        want = RF._host_refit(gt.s, to.prims)
        b = T.build_tlas(*T.root_leaf_boxes(want))
        assert b.tied > 0 and b.nodes.tobytes() == want.tlas.tobytes() and (n < 128 or layout == "stacked" or b.cross > 0), (b.tied, b.cross)
        assert st["tlas_nodes"] == 2 * n and st["tlas_depth"] == b.depth
        RF._same_arrays(RF._arrays(d), RF._fresh(want), f"{layout} {n}")
    finally:
        d.close()


@pytest.mark.parametrize("builder", RB.BUILDERS + ["sbvh_gpu"])
@pytest.mark.parametrize("layout,n", [(l, n) for l in ("pairs", "mixed") for n in (65, 256)])
def test_rebuild_scene_builds_the_same_tlas(layout, n, builder):
    gt, sa, _ = T.instances_scene(n, layout)
    sa = gt.s.arrays(bvh4=False)
    d = Device(Wd, Hd)
    try:
        d.upload(sa)
        st = d.rebuild_scene(builder=builder)
        want = RB.host_rebuild(gt.s, None, builder=builder)
        assert st["tlas_nodes"] == 2 * n and st["tlas_depth"] == T.tlas_depth(want.tlas)
        RF._same_arrays(RF._arrays(d), RF._fresh(want), f"{layout} {n} {builder}")
    finally:
        d.close()


def _refused(d, L, fn, args, text, before, info, cam, ref, what):
    rc = fn(d._h, *args)
    msg = L.rt_last_error().decode()
    assert rc == W.RT_E_UNSUPPORTED and text in msg, (what, rc, msg)
    RF._same_arrays(RF._arrays(d), before, f"after the refused {what}")
    assert d.kernel_info() == info, what
    d.seed_default()
    d.reset()
    d.render(cam, 1)
    assert_bits(d.read_accum(), ref, f"the frame after the refused {what}")


def test_a_tlas_of_32_levels_is_taken_and_one_of_33_refused():
    """`stacked`: n identical boxes make a chain n - 1 levels deep.  33 boxes fill the traversal stack (RT_TLAS_STACK 32) and render as
    the oracle; 34 are refused by the update and by the rebuild, and nothing changes."""
    gt, sa, _ = T.instances_scene(33, "random", baked=True, soup=0)
    gs, to, view = T.instances_scene(33, "stacked")
    cam = scenes.camera_for(view, Wd, Hd)
    d = Device(Wd, Hd, **DEFAULT)
    try:
        d.upload(sa)
        st = d.update_scene(to.prims, 0, None)
        want = RF._host_refit(gt.s, to.prims)
        assert st["tlas_depth"] == 32 == T.tlas_depth(want.tlas)
        _frame(d, want, cam, "33 stacked boxes")
    finally:
        d.close()
    gt, sa, view = T.instances_scene(34, "random", baked=True, soup=0)
    to = T.instances_scene(34, "stacked")[1]
    cam = scenes.camera_for(view, Wd, Hd)
    L = W.device_lib()
    d = Device(Wd, Hd, **DEFAULT)
    try:
        d.upload(sa)
        before, info = RF._arrays(d), d.kernel_info()
        ref = _frame(d, sa, cam, "34 boxes before the refusals")
        args, keep, _ = _update_args(to.prims, 0, None)
        _refused(d, L, L.rt_update_scene, args, "33 levels", before, info, cam, ref, "33-level update")
        for builder in RB.BUILDERS:
            args, keep, _ = _rebuild_args(to.prims, 0, None, builder, {})
            _refused(d, L, L.rt_rebuild_scene, args, "33 levels", before, info, cam, ref, f"33-level rebuild ({builder})")
    finally:
        d.close()


@pytest.mark.parametrize("n", [2, 5])
def test_no_partner_is_refused_and_changes_nothing(n):
    gt, sa, view = T.instances_scene(n, "random")
    mixed = T.instances_scene(n, "mixed")[1]
    cam = scenes.camera_for(view, Wd, Hd)
    far = TC.far_apart(sa)
    L = W.device_lib()
    d = Device(Wd, Hd, **DEFAULT)
    try:
        d.upload(sa)
        before, info = RF._arrays(d), d.kernel_info()
        ref = _frame(d, sa, cam, f"{n} instances before the refusals")
        args, keep, _ = _update_args(None, 0, far)
        _refused(d, L, L.rt_update_scene, args, "no partner", before, info, cam, ref, "no-partner update")
        for builder in RB.BUILDERS:
            args, keep, _ = _rebuild_args(None, 0, far, builder, {})
            _refused(d, L, L.rt_rebuild_scene, args, "no partner", before, info, cam, ref, f"no-partner rebuild ({builder})")
        d.update_scene(None, 0, mixed.blas)
        RF._same_arrays(RF._arrays(d), RF._fresh(RF._host_refit(gt.s, sa.prims, mixed.blas), **DEFAULT), "a valid update after the refusals")
    finally:
        d.close()


# ---- traversal of a device-built 256-instance TLAS -----------------------------------------------------------------------------------
_BIG = {}


def _big():
    """(ground truth of `mixed` at 256, the arrays of the host update random -> mixed, the uploaded random arrays, view)."""
    if not _BIG:
        gt0, sa0, view = T.instances_scene(256, "random")
        gt1, sa1, _ = T.instances_scene(256, "mixed")
        saR = RF._host_refit(gt0.s, sa0.prims, sa1.blas)
        gt1.sa = saR
        _BIG["v"] = (gt1, saR, sa0, sa1.blas, view)
    return _BIG["v"]


def _traverse(d, gt, sa, view, accel, what):
    """Two frames equal the oracle's in accumulator, seeds and work counters; camera rays, bounce-1 rays and the adversarial sets
    through stage_extend meet the float64 closest hit."""
    cam = scenes.camera_for(view, Wd, Hd)
    v = dict(DEFAULT, accel=accel)
    acc, seeds, e, c = oracle_for(sa, Wd, Hd, **v).render(cam, 2)
    T.assert_seen(e, c, what)
    d.seed_default()
    d.reset()
    d.reset_counters()
    d.render(cam, 2)
    assert_bits(d.read_accum(), acc, f"{what}: two frames vs oracle")
    assert np.array_equal(d.get_seeds(), seeds)
    B.ctr_equal(d.counters(), e, c)
    d.set_seeds(seed_stream(0, Wd * Hd))
    d.reset()
    d.stage_begin_frame()
    d.stage_generate(cam)
    for b in (0, 1):
        rays = d.get_rays(b)
        d.stage_extend(b)
        G.compare(gt, rays, d.get_rays(b), "camera" if b == 0 else "bounce", f"{what}: bounce {b} rays")
        d.stage_shade(b)
    for name, rs in C.adversarial_sets(gt, sa, accel).items():
        G.compare(gt, rs, GT._inject(d, 2, rs), "adversarial", f"{what}: {name}")


MULTI2 = [k for k, v in GT.CASES.items() if v[0] == "multi" and v[1] == W.ACCEL_BVH2]


@pytest.mark.parametrize("case", MULTI2)
def test_traversal_of_a_device_built_256_instance_tlas(case, monkeypatch):
    kind, accel, variant, env, want = GT.CASES[case]
    monkeypatch.setenv("RT355_TUNE", GT.TUNE)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    gt, saR, sa0, inst, view = _big()
    d = Device(Wd, Hd, extend_variant=variant, **dict(DEFAULT, accel=accel))
    try:
        d.upload(sa0)
        d.update_scene(None, 0, inst)
        info = d.kernel_info()
        # (a TLAS deeper than 8 levels runs the nested loops whatever the case asks for: the path the library reports is the one checked)
        fresh = Device(Wd, Hd, extend_variant=variant, **dict(DEFAULT, accel=accel))
        fresh.upload(saR)
        assert info == fresh.kernel_info()
        fresh.close()
        if T.tlas_depth(saR.tlas) <= 8:
            for k, wv in want.items():
                assert info[k] == wv, (case, info)
        _traverse(d, gt, saR, view, accel, case)
    finally:
        d.close()


def test_bvh4_nested_traversal_of_a_256_instance_tlas():
    """BVH4 contexts cannot be updated: a plain upload of the host-built scene."""
    gt, sa, view = T.instances_scene(256, "mixed")
    d = Device(Wd, Hd, **dict(DEFAULT, accel=W.ACCEL_BVH4))
    try:
        d.upload(sa)
        info = d.kernel_info()
        assert info["persist"] == 0 and info["persist4"] == 0, info
        _traverse(d, gt, sa, view, W.ACCEL_BVH4, "tlas-bvh4-nested")
    finally:
        d.close()

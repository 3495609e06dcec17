"""BVH4 contexts that were bound with their BVH2 (Device.upload(sa, from_bvh2=True): rt_upload_scene_bvh2) on the MI355X: the upload
collapses the BVH2 on the GPU and leaves the fourteen device arrays and kernel_info of a classic upload of the host's collapse; such a
copy rebuilds in place (rt_rebuild_scene with every builder) to the arrays of a classic upload of the host rebuild, frames after a
rebuild are bit-exact with the oracle on every BVH4 traversal path, sharing contexts and group lanes follow, rebuilds chain without
allocating, and every refusal leaves the bound scene rendering as before."""
import numpy as np
import pytest

import capacity_check as CC
import collapse_check as K
import rebuild_check as RB
import rebuild_sbvh_check as RS
import refit_check as R
import test_gpu_groundtruth as GT
import test_groundtruth_cpu as C
import tlas_check as TC
from helpers import DEFAULT, assert_bits
from magr_ray_tracer_amd import _lib as W, scenes
from magr_ray_tracer_amd.renderer import Device, Group, RtError
from magr_ray_tracer_amd.scenes import Scene, _std_materials
from oracle.oracle_py import Oracle, seed_stream

pytestmark = pytest.mark.gpu

Wd, Hd = 160, 120
B4 = dict(DEFAULT, accel=W.ACCEL_BVH4)
CLASSIC = list(W.SCENE_ARRAYS) + ["quads", "rootEntry"]          # what a classic upload fills; the fourteenth is the kept BVH2
assert len(CLASSIC) + 1 == len(W.SCENE_ARRAYS) + len(W.SCENE_ARRAYS_BVH4) == 14


def _arrays(d):
    return {k: d.scene_array(k) for k in CLASSIC + ["bvh2Kept"]}


def _fresh(sa, **kw):
    d = Device(Wd, Hd, **kw)
    try:
        d.upload(sa)
        return _arrays(d), d.kernel_info()
    finally:
        d.close()


def _same(got, want, what, bvh2=None):
    for k in CLASSIC:
        assert len(got[k]) == len(want[k]) and np.array_equal(got[k], want[k]), f"{what}: {k} differs ({len(got[k])} / {len(want[k])} bytes)"
    if bvh2 is not None:
        assert np.array_equal(got["bvh2Kept"], K.raw(bvh2).ravel()), f"{what}: the kept BVH2 differs"


def _check(d, sa_want, what, **kw):
    """The device's arrays and kernel_info are those of a classic upload of sa_want (whose bvh4 the host collapsed)."""
    want, info = _fresh(sa_want, **kw)
    assert len(want["bvh2Kept"]) == 0                              # a classic BVH4 copy holds no BVH2
    _same(_arrays(d), want, what, sa_want.bvh2)
    assert d.kernel_info() == info, (what, d.kernel_info(), info)
    return info


# ---- upload ----------------------------------------------------------------------------------------------------------------------------
def _need_scene(levels):
    """One BLAS whose hand-made BVH2 (collapse_check.comb2) collapses to a comb that needs 3 (levels - 1) + 4 stack entries."""
    n2, slots = K.comb2(levels)
    s = K.soup_scene([slots], seed=9)
    sa = s.arrays()
    assert len(sa.primIdx) == slots and len(sa.blas) == 1
    sa.bvh2, sa.bvh4 = n2, K.from_nodes(n2)
    sa.blas = sa.blas.copy()
    sa.blas["bvhIdx"][0] = 0
    return sa


UPLOADS = {
    "one": lambda: R.build(blas=1, spheres=2)[1],
    "two": lambda: R.build(blas=2, spheres=2, transforms=[None, RB.ROT])[1],
    "four": lambda: R.build(blas=4, spheres=2, transforms=[None, RB.ROT, C.TRANSFORMS["scale"], C.TRANSFORMS["mirror"]])[1],
    "leaf-roots": lambda: K.tiny_scene().arrays(),
    "sbvh": lambda: R.build(alpha=0.0, blas=2, spheres=2)[1],
    "need-64": lambda: _need_scene(21),
}


@pytest.mark.parametrize("variant", [0, 1])
@pytest.mark.parametrize("name", list(UPLOADS))
def test_upload_from_bvh2_gives_the_arrays_of_a_classic_upload(name, variant):
    sa = UPLOADS[name]()
    d = Device(Wd, Hd, extend_variant=variant, **B4)
    try:
        d.upload(sa, from_bvh2=True)
        info = _check(d, sa, f"{name} / variant {variant}", extend_variant=variant, **B4)
        assert info["layout"] == (0 if variant == 1 else 1)
        if name == "need-64":
            assert info["stack_entries"] == 64
    finally:
        d.close()


def test_from_bvh2_on_a_bvh2_context_is_the_classic_upload():
    sa = UPLOADS["two"]()
    d = Device(Wd, Hd, **DEFAULT)
    try:
        d.upload(sa, from_bvh2=True)
        got, info = {k: d.scene_array(k) for k in W.SCENE_ARRAYS}, d.kernel_info()
        assert len(d.scene_array("bvh2Kept")) == 0 and len(d.scene_array("quads")) == 0
    finally:
        d.close()
    d = Device(Wd, Hd, **DEFAULT)
    try:
        d.upload(sa)
        assert info == d.kernel_info()
        for k in W.SCENE_ARRAYS:
            assert np.array_equal(got[k], d.scene_array(k)), k
    finally:
        d.close()


def test_a_collapse_that_needs_67_entries_is_refused_and_the_bound_scene_stays():
    gt, sa, view = R.build(blas=2, spheres=2)
    cam = scenes.camera_for(view, Wd, Hd)
    bad = _need_scene(22)
    d = Device(Wd, Hd, **B4)
    try:
        with pytest.raises(RtError, match="needs 67 stack entries") as e:     # as rt_upload_scene refuses the host's collapse
            d.upload(bad)
        d.upload(sa, from_bvh2=True)
        before, info = _arrays(d), d.kernel_info()
        d.seed_default()
        d.render(cam, 1)
        ref = d.read_accum()
        with pytest.raises(RtError, match="needs 67 stack entries") as e:
            d.upload(bad, from_bvh2=True)
        assert e.value.code == W.RT_E_UNSUPPORTED
        broken = sa.bvh2.copy()
        broken["first"][np.where(broken["count"] == 0)[0][-1]] = 0xffffffff
        with pytest.raises(RtError) as e:
            d.upload(type(sa)(**{**sa.__dict__, "bvh2": broken}), from_bvh2=True)
        assert e.value.code == W.RT_E_INVALID
        _same(_arrays(d), before, "after the refused uploads", sa.bvh2)
        assert d.kernel_info() == info
        d.seed_default()
        d.reset()
        d.render(cam, 1)
        assert_bits(d.read_accum(), ref, "render after the refused uploads")
    finally:
        d.close()


# ---- rebuilds: array identity -------------------------------------------------------------------------------------------------------------
BUILDERS = {"sah": ("sah", None), "lbvh": ("lbvh", None), "sbvh0": ("sbvh_gpu", 0.0), "sbvh0.5": ("sbvh_gpu", 0.5)}


def _host_rebuild(s, prims, which, inst=None):
    builder, alpha = BUILDERS[which]
    if builder == "sbvh_gpu":
        return RS.host_rebuild(s, prims, alpha, inst, bvh4=True)
    return RB.host_rebuild(s, prims, inst, builder=builder, bvh4=True)


def _rebuild(d, prims, which, inst=None, first=0):
    builder, alpha = BUILDERS[which]
    return d.rebuild_scene(prims, first, inst, builder=builder, alpha=alpha)


@pytest.mark.parametrize("which", list(BUILDERS))
@pytest.mark.parametrize("blas", [1, 4])
@pytest.mark.parametrize("deform", list(RB.DEFORMS))
def test_rebuild_gives_the_arrays_of_a_classic_upload(deform, blas, which, monkeypatch):
    mk, spheres = RB.DEFORMS[deform]
    if deform == "scramble":
        monkeypatch.setenv("RT355_REBUILD_INITIAL_CAP", "8")       # bvh4 and quads grow with the node array
    T0 = None if blas < 2 else [None, RB.ROT] + [None] * (blas - 2)
    gt0, sa0, _ = R.build(alpha=1.0, blas=blas, spheres=spheres, transforms=T0)
    prims = R.build(mk(), alpha=1.0, blas=blas, spheres=spheres, transforms=T0)[1].prims
    d = Device(Wd, Hd, **B4)
    try:
        d.upload(sa0, from_bvh2=True)
        st = _rebuild(d, prims, which)
        want = _host_rebuild(gt0.s, prims, which)
        assert st["blas_built"] == blas and st["nodes"] == len(want.bvh2) and st["n_idx"] == len(want.primIdx) and st["max_depth"] == RB.depth(want)
        _check(d, want, f"{deform} / {blas} BLAS / {which}", **B4)
        _rebuild(d, prims, which)                                    # the other set of arrays: the same bytes
        _check(d, want, f"{deform} / {blas} BLAS / {which}, again", **B4)
    finally:
        d.close()


def test_leaf_roots_survive_a_rebuild():
    s = K.tiny_scene()
    sa = s.arrays()
    prims = sa.prims.copy()
    prims["v0"][:, :3] += np.float32(0.05)
    d = Device(Wd, Hd, **B4)
    try:
        d.upload(sa, from_bvh2=True)
        for which in ("sah", "lbvh"):
            _rebuild(d, prims, which)
            want = _host_rebuild(s, prims, which)
            assert want.bvh2["count"][want.blas["bvhIdx"][1]] == 1
            _check(d, want, f"leaf roots / {which}", **B4)
    finally:
        d.close()


# ---- frames ------------------------------------------------------------------------------------------------------------------------------
_SC = {}
BVH4_PATHS = ["bvh4-persist", "bvh4-layout0", "bvh4-one-ray-per-lane", "tlas-bvh4-nested"]


def _scenes(kind, which):
    if (kind, which) not in _SC:
        T = None if kind == "one" else [None, None, C.TRANSFORMS["scale"], C.TRANSFORMS["mirror"]]
        blas, tris = (1, 600) if kind == "one" else (4, 220)
        gt0, sa0, view = R.build(alpha=0.0, blas=blas, spheres=3, tris=tris, transforms=T)
        prims = R.build(R.scramble(), alpha=1.0, blas=blas, spheres=3, tris=tris, transforms=T)[1].prims
        _SC[(kind, which)] = (sa0, prims, _host_rebuild(gt0.s, prims, which), view)
    return _SC[(kind, which)]


@pytest.mark.parametrize("which", ["sah", "lbvh", "sbvh0.5"])
@pytest.mark.parametrize("case", BVH4_PATHS)
def test_frames_across_a_rebuild_match_the_oracle(case, which, monkeypatch):
    """Two frames, a rebuild, two more: accumulator, seeds and the extend work counters equal the oracle's, which renders two frames of
    the original arrays and two of the host-rebuilt, host-collapsed ones with the accumulator carried."""
    assert GT.CASES[case][1] == W.ACCEL_BVH4
    kind, accel, variant, env, want = GT.CASES[case]
    monkeypatch.setenv("RT355_TUNE", GT.TUNE)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    sa0, prims, saR, view = _scenes(kind, which)
    cam = scenes.camera_for(view, Wd, Hd)
    o0, o1 = Oracle(sa0, Wd, Hd, **B4), Oracle(saR, Wd, Hd, **B4)
    acc, seeds, ext, con = o0.render(cam, 2)
    TC.assert_seen(ext, con, f"{case}: the frames before the rebuild")
    acc, seeds, ext, con = o1.render(cam, 2, accum=acc, seeds=seeds)
    TC.assert_seen(ext, con, f"{case}: the frames after the rebuild")
    d = Device(Wd, Hd, extend_variant=variant, **B4)
    try:
        d.upload(sa0, from_bvh2=True)
        for k, wv in want.items():
            assert d.kernel_info()[k] == wv, (case, d.kernel_info())
        d.seed_default()
        d.render(cam, 2)
        _rebuild(d, prims, which)
        info = d.kernel_info()
        for k, wv in want.items():
            assert info[k] == wv, (case, info)
        d.reset_counters()
        d.render(cam, 2)
        assert_bits(d.read_accum(), acc, f"{case} / {which}: frames across a rebuild vs oracle")
        assert np.array_equal(d.get_seeds(), seeds)
        got = d.counters()
        for k in ("rays", "node_visits", "prim_tests"):
            assert got["extend_" + k] == ext[k], (case, k, got["extend_" + k], ext[k])
    finally:
        d.close()


# ---- holders and chains ------------------------------------------------------------------------------------------------------------------
def test_shared_contexts_and_group_lanes_render_the_rebuilt_scene():
    gt0, sa0, view = R.build(alpha=1.0, blas=2, spheres=2)
    prims = R.build(R.scramble(), alpha=1.0, blas=2, spheres=2)[1].prims
    cam = scenes.camera_for(view, Wd, Hd)
    a, b = Device(Wd, Hd, **B4), Device(Wd, Hd, **B4)
    g = Group(Wd, Hd, lanes=4, **B4)
    try:
        a.upload(sa0, from_bvh2=True)
        b.share_scene(a)
        g.upload(sa0, from_bvh2=True)
        g.seed(0)
        b.seed_default()
        b.render(cam, 1)                                             # work in flight on a holder that is not the one rebuilding
        _rebuild(a, prims, "sah")
        _rebuild(g, prims, "sah")
        saR = _host_rebuild(gt0.s, prims, "sah")
        want_arrays, want_info = _fresh(saR, **B4)
        for h in [a, b] + g.devs:
            assert h.kernel_info()["stack_entries"] == want_info["stack_entries"]
        assert a.kernel_info() == want_info and b.kernel_info() == want_info
        _same(_arrays(b), want_arrays, "the sharing partner's arrays", saR.bvh2)
        _same(_arrays(g.devs[3]), want_arrays, "lane 3's arrays", saR.bvh2)
        ref = Oracle(saR, Wd, Hd, **B4).render(cam, 1)[0]
        for dv in (a, b):
            dv.seed_default()
            dv.reset()
            dv.render(cam, 1)
            assert_bits(dv.read_accum(), ref, "shared pair after a rebuild")
        g.seed(0)
        g.reset()
        g.render(cam, 4)
        exp = None
        for m in range(4):
            r = Oracle(saR, Wd, Hd, **B4).render(cam, 1, seeds=seed_stream(m * Wd * Hd, Wd * Hd))[0]
            exp = r if exp is None else exp + r
        assert_bits(g.read_accum(), exp, "4-lane group after a rebuild")
    finally:
        g.close()
        b.close()
        a.close()


def test_rebuilds_chain_and_a_stable_scene_stops_allocating():
    gt0, sa0, _ = R.build(alpha=0.0, blas=4, spheres=2, transforms=[None, RB.ROT, None, None])
    p1 = R.build(R.scramble(), blas=4, spheres=2)[1].prims
    p2 = R.build(R.jitter(0.04, seed=8), blas=4, spheres=2)[1].prims
    inst = sa0.blas.copy()
    inst["invT"][2] = C.invT(C.rot(0, 17.0) @ np.diag([1.2, 0.9, 1.0]), (0.1, 0.2, -0.3)).ravel()
    s = gt0.s
    d = Device(Wd, Hd, **B4)
    try:
        d.upload(sa0, from_bvh2=True)
        _rebuild(d, p1, "sah")
        _check(d, _host_rebuild(s, p1, "sah"), "rebuild 1 (sah)", **B4)
        _rebuild(d, p2, "lbvh")
        _check(d, _host_rebuild(s, p2, "lbvh"), "rebuild 2 (lbvh)", **B4)
        inst["bvhIdx"] = s.arrays(bvh4=False).blas["bvhIdx"]
        _rebuild(d, p1[226:448], "sbvh0", inst, first=226)
        s.SetPrimitives(226, p1[226:448])
        _check(d, _host_rebuild(s, None, "sbvh0", inst), "rebuild 3 (sbvh, a slice, new transforms)", **B4)
        for which in ("sah", "lbvh"):
            _rebuild(d, p2, which)
            _rebuild(d, p2, which)
            n = d.rebuild_allocations()
            _rebuild(d, p2, which)
            assert d.rebuild_allocations() == n, f"the third {which} rebuild of a stable scene allocated"
        _check(d, _host_rebuild(s, p2, "lbvh"), "after the stable rebuilds", **B4)
    finally:
        d.close()


# ---- refusals ----------------------------------------------------------------------------------------------------------------------------
def test_updates_stay_refused_and_a_classic_copy_still_refuses_the_rebuild():
    gt, sa, _ = R.build(blas=2, spheres=2)
    d = Device(Wd, Hd, **B4)
    try:
        d.upload(sa, from_bvh2=True)
        with pytest.raises(RtError, match="BVH4") as e:
            d.update_scene(sa.prims[:2], 0)
        d.upload(sa)                                                 # the classic way: the BVH2 is gone
        with pytest.raises(RtError, match="BVH4.*rt_upload_scene_bvh2") as e:
            d.rebuild_scene()
        assert e.value.code == W.RT_E_UNSUPPORTED
        with pytest.raises(RtError, match="BVH4"):
            d.update_scene(sa.prims[:2], 0)
    finally:
        d.close()
    L = W.device_lib()
    d = Device(Wd, Hd, **B4)
    try:
        d.upload(sa, from_bvh2=True)
        st = np.zeros((), W.UpdateStats)
        assert L.rt_update_scene(d._h, W.ptr(sa.prims[:2].copy()), 0, 2, None, 0, W.ptr(st)) == W.RT_E_UNSUPPORTED
        assert b"BVH4" in L.rt_last_error()
    finally:
        d.close()


def test_refused_rebuilds_leave_the_scene_as_it_was():
    """A layout change (128 coincident triangles make a leaf that no packed entry holds) and an alpha of 2."""
    s = Scene()
    _std_materials(s)
    rng = np.random.default_rng(6)
    s.AddTriangles(C._soup(rng, 40, -1.0, 1.0, 0.3), "white-light")
    s.BuildBLAS(0)
    tri = np.array([[(2, 0, 0), (3, 0, 0), (2, 1, 0)]], np.float32)
    s.AddTriangles(np.repeat(tri, 128, axis=0) + rng.normal(scale=0.2, size=(128, 3, 3)).astype(np.float32), "green")
    s.BuildBLAS(40)
    sa = s.arrays()
    s2 = Scene()
    _std_materials(s2)
    s2.AddTriangles(np.repeat(tri, 128, axis=0), "green")
    s2.BuildBLAS(0)
    prims = sa.prims.copy()
    prims[40:168] = s2.arrays(bvh4=False).prims
    prims["matIdx"][40:168] = sa.prims["matIdx"][40:168]
    cam = scenes.camera_for(dict(origin=(0.5, 0.5, 8.0), forward=(0.0, 0.0, 1.0), fov=64.0, aperture=0.01), Wd, Hd)
    d = Device(Wd, Hd, **B4)
    try:
        d.upload(sa, from_bvh2=True)
        assert d.kernel_info()["layout"] == 1
        d.rebuild_scene(builder="sah")                               # (both sets exist, the live one is a rebuilt one)
        before, info = _arrays(d), d.kernel_info()
        d.seed_default()
        d.render(cam, 1)
        ref = d.read_accum()
        for what, code, args, kw in (("layout-changing", W.RT_E_UNSUPPORTED, (prims, 0, None), dict(builder="sah")),
                                     ("alpha 2", W.RT_E_INVALID, (), dict(builder="sbvh_gpu", alpha=2.0))):
            with pytest.raises(RtError) as e:
                d.rebuild_scene(*args, **kw)
            assert e.value.code == code, (what, e.value.code, str(e.value))
            _same(_arrays(d), before, f"after the refused {what} rebuild")
            assert np.array_equal(_arrays(d)["bvh2Kept"], before["bvh2Kept"])
            assert d.kernel_info() == info, what
            d.seed_default()
            d.reset()
            d.render(cam, 1)
            assert_bits(d.read_accum(), ref, f"render after the refused {what} rebuild")
        d.rebuild_scene(prims, 0, None, builder="lbvh")              # the linear builder's leaves hold at most max_leaf: fine
        assert d.kernel_info()["layout"] == 1
    finally:
        d.close()

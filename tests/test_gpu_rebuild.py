"""In-place BLAS rebuilds on the MI355X (rt_rebuild_scene / rt_group_rebuild_scene): after a rebuild the eleven device arrays and
kernel_info are those of a fresh upload of the scene built from scratch on the host with the same builder, two runs give the same
arrays, frames are bit-exact with the oracle on every BVH2 traversal path, sharing contexts and group lanes render the new scene with
its stack size, rebuilds and updates chain, and every refusal leaves the bound scene rendering as before."""
import subprocess
import sys

import numpy as np
import pytest

import ranges_check as RC
import rebuild_check as RB
import refit_check as R
import test_gpu_groundtruth as GT
import test_gpu_refit as RF
import test_groundtruth_cpu as C
from helpers import DEFAULT, assert_bits
from magr_ray_tracer_amd import _lib as W, scenes
from magr_ray_tracer_amd.renderer import Device, Group, RtError
from magr_ray_tracer_amd.scene import build_sah_gpu
from magr_ray_tracer_amd.scenes import Scene, _std_materials
from oracle.oracle_py import Oracle, seed_stream

pytestmark = pytest.mark.gpu

Wd, Hd = 160, 120
ARRAYS = list(W.SCENE_ARRAYS)


def _arrays(d):
    return {k: d.scene_array(k) for k in ARRAYS}


def _fresh(sa, **kw):
    d = Device(Wd, Hd, **kw)
    d.upload(sa)
    a, info = _arrays(d), d.kernel_info()
    d.close()
    return a, info


def _same(got, want, what):
    for k in ARRAYS:
        assert len(got[k]) == len(want[k]) and np.array_equal(got[k], want[k]), f"{what}: {k} differs ({len(got[k])} / {len(want[k])} bytes)"


def _check(d, sa_want, what, **kw):
    want, info = _fresh(sa_want, **kw)
    _same(_arrays(d), want, what)
    assert d.kernel_info() == info, (what, d.kernel_info(), info)


def _scrambled(sa, seed=2):
    """Every triangle's vertices scrambled across the triangles of the scene (objType / matIdx kept; normals and areas stay the old
    records' - the builders and the refit only read the vertices)."""
    rng = np.random.default_rng(seed)
    p = sa.prims.copy()
    tri = np.where(p["objType"] == W.PRIM_TRIANGLE)[0]
    v = np.stack([p["v0"][tri], p["v1"][tri], p["v2"][tri]], axis=1).reshape(-1, 4)
    v = v[rng.permutation(len(v))].reshape(-1, 3, 4)
    p["v0"][tri], p["v1"][tri], p["v2"][tri] = v[:, 0], v[:, 1], v[:, 2]
    return p


# ---- array identity --------------------------------------------------------------------------------------------------------------------
CASES = [(dname, fb, blas) for dname in RB.DEFORMS for fb, blas in (("sah", 1), ("sbvh", 2), ("lbvh", 4))] + [("scramble", "sbvh", 4)]


@pytest.mark.parametrize("builder", RB.BUILDERS)
@pytest.mark.parametrize("deform,first_build,blas", CASES, ids=[f"{a}-{b}-{c}" for a, b, c in CASES])
def test_rebuild_gives_the_arrays_of_a_fresh_upload(deform, first_build, blas, builder):
    mk, spheres = RB.DEFORMS[deform]
    T0 = None if blas < 2 else [None, RB.ROT] + [None] * (blas - 2)
    (gt0, sa0), (gt1, sa1), _ = RB.pair(mk(), first_build, builder, blas, spheres=spheres, transforms=T0)
    d = Device(Wd, Hd)
    try:
        d.upload(sa0)
        st = d.rebuild_scene(sa1.prims, 0, None, builder=builder)
        assert st["blas_built"] == blas and st["nodes"] == len(sa1.bvh2) and st["n_idx"] == len(sa1.primIdx) and st["max_depth"] == RB.depth(sa1)
        _check(d, sa1, f"{deform} / {first_build} / {blas} BLAS / {builder}")
        # the host restatement says the same
        RB.same_wire_arrays(RB.host_rebuild(gt0.s, sa1.prims, builder=builder), sa1, "host restatement")
    finally:
        d.close()


@pytest.mark.parametrize("builder", RB.BUILDERS)
@pytest.mark.parametrize("name", ["sponza_class", "config5"])
def test_rebuild_of_the_bench_scenes(name, builder):
    """sponza_class with every vertex scrambled, config 5's two-BLAS scene (its second BLAS an SBVH 63 levels deep) jittered."""
    s = scenes.sponza_class(1.0)[0] if name == "sponza_class" else scenes.config5_scene(0.0)[0]
    sa = s.arrays(bvh4=False)
    prims = _scrambled(sa) if name == "sponza_class" else sa.prims.copy()
    if name == "config5":
        prims["v0"][:, :3] += np.random.default_rng(3).normal(scale=1e-3, size=(len(prims), 3)).astype(np.float32)
    d = Device(Wd, Hd)
    try:
        d.upload(sa)
        d.rebuild_scene(prims, 0, None, builder=builder)
        _check(d, RB.host_rebuild(s, prims, builder=builder), f"{name} / {builder}")
    finally:
        d.close()


def _tiny_scene(builder="sah"):
    """Three BLAS: a soup, one triangle (its root is a leaf) and two triangles (a leaf root as well)."""
    s = Scene()
    _std_materials(s)
    rng = np.random.default_rng(5)
    s.AddTriangles(C._soup(rng, 60, -1.0, 1.0, 0.3), "sand")
    y = 3.0
    for v in ([(-1, y, -1), (1, y, -1), (1, y, 1)], [(1, y, 1), (-1, y, 1), (-1, y, -1)]):
        s.AddTriangle(*[np.array(p, np.float32) for p in v], "white-light")
    s.BuildBLAS(0, builder=builder, device=None) if builder == "lbvh" else s.BuildBLAS(0)
    s.AddTriangles(C._soup(rng, 1, 1.5, 2.0, 0.3), "green")
    s.BuildBLAS(62, builder=builder, device=None) if builder == "lbvh" else s.BuildBLAS(62)
    s.AddTriangles(C._soup(rng, 2, -2.0, -1.5, 0.3), "red")
    s.BuildBLAS(63, builder=builder, device=None) if builder == "lbvh" else s.BuildBLAS(63)
    return s


@pytest.mark.parametrize("builder", RB.BUILDERS)
def test_a_blas_whose_root_is_a_leaf(builder):
    s = _tiny_scene()
    sa = s.arrays(bvh4=False)
    assert sa.bvh2["count"][sa.blas["bvhIdx"][1]] == 1 and sa.bvh2["count"][sa.blas["bvhIdx"][2]] == 2
    prims = sa.prims.copy()
    prims["v0"][:, :3] += np.float32(0.05)
    d = Device(Wd, Hd)
    try:
        d.upload(sa)
        d.rebuild_scene(prims, 0, None, builder=builder)
        want = RB.host_rebuild(s, prims, builder=builder)
        assert want.bvh2["count"][want.blas["bvhIdx"][1]] == 1
        _check(d, want, f"leaf roots / {builder}")
    finally:
        d.close()


# ---- determinism ------------------------------------------------------------------------------------------------------------------------
_CHILD = """
import sys, numpy as np
sys.path.insert(0, {tests!r})
import rebuild_check as RB, refit_check as R
from magr_ray_tracer_amd import _lib as W
from magr_ray_tracer_amd.renderer import Device
(gt0, sa0), (gt1, sa1), _ = RB.pair(R.scramble(), "sbvh", {builder!r}, 4)
d = Device(160, 120)
d.upload(sa0)
d.rebuild_scene(sa1.prims, 0, None, builder={builder!r})
np.savez({out!r}, **{{k: d.scene_array(k) for k in W.SCENE_ARRAYS}})
d.close()
"""


@pytest.mark.parametrize("builder", RB.BUILDERS)
def test_two_rebuilds_give_identical_arrays(builder, tmp_path):
    """The same rebuild twice in one context (the second writes the other set of arrays), and once from a fresh process."""
    import os
    (gt0, sa0), (gt1, sa1), _ = RB.pair(R.scramble(), "sbvh", builder, 4)
    d = Device(Wd, Hd)
    try:
        d.upload(sa0)
        d.rebuild_scene(sa1.prims, 0, None, builder=builder)
        first = _arrays(d)
        for k in range(3):
            d.rebuild_scene(sa1.prims, 0, None, builder=builder)
            _same(_arrays(d), first, f"rebuild {k + 2}")
    finally:
        d.close()
    out = str(tmp_path / "child.npz")
    code = _CHILD.format(tests=os.path.dirname(os.path.abspath(__file__)), builder=builder, out=out)
    subprocess.run([sys.executable, "-c", code], check=True, timeout=300, cwd=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    other = np.load(out)
    _same({k: other[k] for k in ARRAYS}, first, "a second process")


# ---- frames ----------------------------------------------------------------------------------------------------------------------------
_SC = {}


def _scenes(kind, builder):
    """(original arrays, deformed records, arrays of the host rebuild, view): one SBVH BLAS, or four under transforms."""
    if (kind, builder) not in _SC:
        T = None if kind == "one" else [None, None, C.TRANSFORMS["scale"], C.TRANSFORMS["mirror"]]
        blas, tris = (1, 600) if kind == "one" else (4, 220)
        (gt0, sa0), (gt1, sa1), view = RB.pair(R.scramble(), "sbvh", builder, blas, spheres=3, tris=tris, transforms=T)
        _SC[(kind, builder)] = (sa0, sa1.prims, RB.host_rebuild(gt0.s, sa1.prims, builder=builder, bvh4=True), view)
    return _SC[(kind, builder)]


BVH2_PATHS = [k for k, v in GT.CASES.items() if v[1] == W.ACCEL_BVH2]


@pytest.mark.parametrize("builder", RB.BUILDERS)
@pytest.mark.parametrize("case", BVH2_PATHS)
def test_frames_across_a_rebuild_match_the_oracle(case, builder, monkeypatch):
    """Two frames, a rebuild, two more: accumulator, seeds and the extend work counters equal the oracle rendering the same sequence
    (two frames of the original arrays, then two of the host-rebuilt ones, accumulator carried); the traversal path is confirmed by
    kernel_info before and after (the spill cases force the spill kernel through RT355_SPILL_CAP, whatever the depth)."""
    kind, accel, variant, env, want = GT.CASES[case]
    monkeypatch.setenv("RT355_TUNE", GT.TUNE)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    sa0, prims, saR, view = _scenes(kind, builder)
    cam = scenes.camera_for(view, Wd, Hd)
    v = dict(DEFAULT, accel=accel)
    o0, o1 = Oracle(sa0, Wd, Hd, **v), Oracle(saR, Wd, Hd, **v)
    acc, seeds, _, _ = o0.render(cam, 2)
    acc, seeds, _, _ = o1.render(cam, 2, accum=acc, seeds=seeds)
    d = Device(Wd, Hd, extend_variant=variant, **v)
    try:
        d.upload(sa0)
        for k, wv in want.items():
            assert d.kernel_info()[k] == wv, (case, d.kernel_info())
        d.seed_default()
        d.render(cam, 2)
        d.rebuild_scene(prims, 0, None, builder=builder)
        info = d.kernel_info()
        for k, wv in want.items():
            assert info[k] == wv, (case, info)
        d.reset_counters()
        d.render(cam, 2)
        assert_bits(d.read_accum(), acc, f"{case} / {builder}: frames across a rebuild vs oracle")
        assert np.array_equal(d.get_seeds(), seeds)
        # the work counters of the two frames after the rebuild: those of a fresh context rendering the same two frames of the new scene
        got = d.counters()
        f = Device(Wd, Hd, extend_variant=variant, **v)
        try:
            f.upload(saR)
            f.set_seeds(Oracle(sa0, Wd, Hd, **v).render(cam, 2)[1])
            f.render(cam, 2)
            ref = f.counters()
        finally:
            f.close()
        for k in ("extend_rays", "extend_node_visits", "extend_prim_tests", "connect_rays", "connect_node_visits", "connect_prim_tests"):
            assert got[k] == ref[k], (case, k, got[k], ref[k])
    finally:
        d.close()


# ---- holders ---------------------------------------------------------------------------------------------------------------------------
def _oracle_frames(sa, cam, frames, acc=None, seeds=None):
    return Oracle(sa, Wd, Hd, **DEFAULT).render(cam, frames, accum=acc, seeds=seeds)


@pytest.mark.parametrize("builder", RB.BUILDERS)
def test_shared_contexts_and_group_lanes_render_the_rebuilt_scene(builder):
    """An rt_share_scene pair and a 4-lane group: after a rebuild that changes the trees' depth every holder reports the new stack size
    (that of a fresh upload) and renders the new scene."""
    (gt0, sa0), (gt1, sa1), view = RB.pair(R.scramble(), builder, builder, 2)
    d0, d1 = RB.depth(sa0), RB.depth(sa1)
    assert d0 != d1 and max(d0, d1) + 1 > 6, (d0, d1)      # the host builds differ in depth: the stack size must follow
    cam = scenes.camera_for(view, Wd, Hd)
    a, b = Device(Wd, Hd, **DEFAULT), Device(Wd, Hd, **DEFAULT)
    g = Group(Wd, Hd, lanes=4)
    try:
        a.upload(sa0)
        b.share_scene(a)
        g.upload(sa0)
        g.seed(0)
        holders = [a, b] + g.devs
        before = [h.kernel_info()["stack_entries"] for h in holders]
        b.seed_default()          # (a context renders only once it is seeded: xorshift32 never leaves 0, and sample_ball rejects forever)
        b.render(cam, 1)          # work in flight on a holder that is not the one rebuilding
        st = a.rebuild_scene(sa1.prims, 0, None, builder=builder)
        st2 = g.rebuild_scene(sa1.prims, 0, None, builder=builder)
        assert st["max_depth"] == d1 == st2["max_depth"] and st["reconfigured"] and st2["reconfigured"]
        want_arrays, want_info = _fresh(sa1, **DEFAULT)
        for h, was in zip(holders, before):
            info = h.kernel_info()
            assert info["stack_entries"] == want_info["stack_entries"] != was, (info, want_info, was)
        assert a.kernel_info() == want_info and b.kernel_info() == want_info
        _same(_arrays(b), want_arrays, "the sharing partner's arrays")
        _same(_arrays(g.devs[3]), want_arrays, "lane 3's arrays")
        ref = _oracle_frames(sa1, cam, 1)[0]
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
            r = _oracle_frames(sa1, cam, 1, seeds=seed_stream(m * Wd * Hd, Wd * Hd))[0]
            exp = r if exp is None else exp + r
        assert_bits(g.read_accum(), exp, "4-lane group after a rebuild")
    finally:
        g.close()
        b.close()
        a.close()


# ---- chaining --------------------------------------------------------------------------------------------------------------------------
def test_rebuilds_and_updates_chain():
    """rebuild -> update -> rebuild -> update, the device arrays equal the host restatement chain at every step."""
    gt0, sa0, _ = R.build(alpha=0.0, blas=4, spheres=2, transforms=[None, RB.ROT, None, None])
    p1 = R.build(R.scramble(), blas=4, spheres=2)[1].prims
    p2 = R.build(R.jitter(0.04, seed=8), blas=4, spheres=2)[1].prims
    p3 = R.build(R.rigid_blas(2), blas=4, spheres=2)[1].prims
    p4 = R.build(R.spheres_moved(), blas=4, spheres=2)[1].prims
    inst = sa0.blas.copy()
    inst["invT"][2] = C.invT(C.rot(0, 17.0) @ np.diag([1.2, 0.9, 1.0]), (0.1, 0.2, -0.3)).ravel()
    s = gt0.s
    d = Device(Wd, Hd)
    try:
        d.upload(sa0)
        d.rebuild_scene(p1, 0, None, builder="sah")
        _check(d, RB.host_rebuild(s, p1, builder="sah"), "rebuild 1 (sah)")
        with pytest.raises(RtError, match="bvhIdx"):
            d.update_scene(p2, 0, inst)            # the roots have moved: instance records carry the bound scene's bvhIdx
        inst["bvhIdx"] = s.arrays(bvh4=False).blas["bvhIdx"]
        assert np.array_equal(np.frombuffer(d.scene_array("instances").tobytes(), W.BVHInstance)["bvhIdx"], inst["bvhIdx"])
        st = d.update_scene(p2, 0, inst)
        assert st["nodes"] == len(s.arrays(bvh4=False).bvh2)
        _check(d, RB.host_refit(s, p2, inst), "update 1")
        d.rebuild_scene(p3, 0, None, builder="lbvh", max_leaf=4)
        _check(d, RB.host_rebuild(s, p3, builder="lbvh", max_leaf=4), "rebuild 2 (lbvh)")
        d.update_scene(p4[100:400], 100, None)
        _check(d, _refit_slice(s, p4, 100, 400), "update 2 (a slice)")
        inst["bvhIdx"] = s.arrays(bvh4=False).blas["bvhIdx"]
        d.rebuild_scene(p1[226:448], 226, inst, builder="sah")
        s.SetPrimitives(226, p1[226:448])
        _check(d, RB.host_rebuild(s, None, inst, builder="sah"), "rebuild 3 (a slice, new transforms)")
    finally:
        d.close()


def _refit_slice(s, prims, a, b):
    s.SetPrimitives(a, prims[a:b])
    s.Refit()
    return s.arrays(bvh4=False)


def test_rebuild_without_new_primitives_changes_the_builder():
    gt, sa, _ = R.build(blas=2, spheres=2, builder="lbvh")
    _, sa_s, _ = R.build(blas=2, spheres=2, builder="sah")
    d = Device(Wd, Hd)
    try:
        d.upload(sa)
        st = d.rebuild_scene(builder="sah")
        assert st["prims"] == 0
        _check(d, sa_s, "lbvh scene rebuilt with sah")
        d.rebuild_scene(builder="lbvh")
        _check(d, sa, "and back")
    finally:
        d.close()


# ---- refusals ----------------------------------------------------------------------------------------------------------------------------
def _coincident(n=128):
    """n coincident triangles in a BLAS of their own behind a soup: the SAH builder makes one leaf of n primitives out of them."""
    s = Scene()
    _std_materials(s)
    rng = np.random.default_rng(6)
    s.AddTriangles(C._soup(rng, 40, -1.0, 1.0, 0.3), "sand")
    s.BuildBLAS(0)
    tri = np.array([[(2, 0, 0), (3, 0, 0), (2, 1, 0)]], np.float32)
    s.AddTriangles(np.repeat(tri, n, axis=0) + rng.normal(scale=0.2, size=(n, 3, 3)).astype(np.float32), "green")
    s.BuildBLAS(40)
    return s, np.repeat(tri, n, axis=0)


def _refused(d, code, before, info, cam, ref, what, *args, **kw):
    with pytest.raises(RtError) as e:
        d.rebuild_scene(*args, **kw)
    assert e.value.code == code, (what, e.value.code, str(e.value))
    _same(_arrays(d), before, f"after the refused {what} rebuild")
    assert d.kernel_info() == info, what
    d.seed_default()
    d.reset()
    d.render(cam, 1)
    assert_bits(d.read_accum(), ref, f"render after the refused {what} rebuild")


def test_refusals_return_their_code_and_change_nothing():
    gt, sa, view = R.build(blas=4, spheres=2)
    cam = scenes.camera_for(view, Wd, Hd)
    d = Device(Wd, Hd, **DEFAULT)
    try:
        d.upload(sa)
        d.rebuild_scene(builder="sah")          # (so that both sets of arrays exist and the live one is a rebuilt one)
        before, info = _arrays(d), d.kernel_info()
        d.seed_default()
        d.render(cam, 1)
        ref = d.read_accum()
        bad_type = sa.prims[:4].copy()
        bad_type["objType"][1] = W.PRIM_SPHERE
        bad_mat = sa.prims[:4].copy()
        bad_mat["matIdx"][0] += 1
        live = np.frombuffer(before["instances"].tobytes(), W.BVHInstance).copy()
        bad_idx = live.copy()
        bad_idx["bvhIdx"][2] = live["bvhIdx"][3]
        sing = live.copy()
        sing["invT"][1] = np.diag([1.0, 1.0, 0.0, 1.0]).astype(np.float32).ravel()
        nan = sa.prims.copy()
        nan["v1"][500, 1] = np.inf
        huge = sa.prims.copy()
        huge["v0"][230:440, :3] *= np.float32(1e20)
        I, U = W.RT_E_INVALID, W.RT_E_UNSUPPORTED
        for what, code, args, kw in (
                ("objType", I, (bad_type, 0, None), {}), ("matIdx", I, (bad_mat, 0, None), {}), ("bvhIdx", I, (None, 0, bad_idx), {}),
                ("range", I, (sa.prims[:4], len(sa.prims) - 2, None), {}), ("instance count", I, (None, 0, live[:3]), {}),
                ("singular", I, (None, 0, sing), {}), ("max_leaf", I, (), dict(builder="lbvh", max_leaf=1000)),
                ("cost", I, (), dict(builder="lbvh", cost_intersect=-1.0)),
                ("non-finite", U, (nan, 0, None), {}), ("areas beyond 1e30", U, (huge, 0, None), {})):
            _refused(d, code, before, info, cam, ref, what, *args, **kw)
        L = W.device_lib()
        st = np.zeros((), W.RebuildStats)
        assert L.rt_rebuild_scene(d._h, None, 0, 0, None, 0, 7, None, W.ptr(st)) == I      # an unknown builder
        _same(_arrays(d), before, "after the unknown builder")
        d.rebuild_scene(sa.prims, 0, None, builder="lbvh")                                # and it still rebuilds
        _check(d, R.build(blas=4, spheres=2, builder="lbvh")[1], "a rebuild after the refusals", **DEFAULT)
    finally:
        d.close()


def test_a_rebuild_that_would_change_the_layout_is_refused():
    """128 coincident triangles: one leaf of 128 primitives, which rt_upload_scene answers with layout 0."""
    s, coincident = _coincident()
    sa = s.arrays(bvh4=False)
    view = dict(origin=(0.5, 0.5, 8.0), forward=(0.0, 0.0, 1.0), fov=64.0, aperture=0.01)
    cam = scenes.camera_for(view, Wd, Hd)
    s2 = Scene()
    _std_materials(s2)
    s2.AddTriangles(coincident, "green")
    s2.BuildBLAS(0)
    same = s2.arrays(bvh4=False).prims
    n1, _, _ = build_sah_gpu(same, device=None)
    assert len(n1) == 1 and n1["count"][0] == 128                    # the host restatement: the input does make that leaf
    prims = sa.prims.copy()
    prims[40:168] = same
    prims["matIdx"][40:168] = sa.prims["matIdx"][40:168]
    d = Device(Wd, Hd, **DEFAULT)
    try:
        d.upload(sa)
        assert d.kernel_info()["layout"] == 1
        before, info = _arrays(d), d.kernel_info()
        d.seed_default()
        d.render(cam, 1)
        ref = d.read_accum()
        _refused(d, W.RT_E_UNSUPPORTED, before, info, cam, ref, "layout-changing", prims, 0, None)
        d.rebuild_scene(prims, 0, None, builder="lbvh")              # the linear builder's leaves hold at most max_leaf: fine
        assert d.kernel_info()["layout"] == 1
    finally:
        d.close()


def test_bvh4_contexts_and_unrebuildable_scenes_are_refused():
    gt, sa, _ = R.build(blas=2, spheres=2)
    d4 = Device(Wd, Hd, **dict(DEFAULT, accel=W.ACCEL_BVH4))
    try:
        d4.upload(gt.s.arrays())
        with pytest.raises(RtError, match="BVH4") as e:
            d4.rebuild_scene()
        assert e.value.code == W.RT_E_UNSUPPORTED
    finally:
        d4.close()
    # two BLAS whose roots come in the other order than their primitive ranges: every array is valid, upload takes it, rebuild does not
    n0 = int(sa.blas["bvhIdx"][1])
    nodes = np.concatenate([sa.bvh2[n0:], sa.bvh2[:n0]])
    inner = nodes["count"] == 0
    nodes["first"][inner] = np.where(np.arange(len(nodes))[inner] < len(sa.bvh2) - n0, nodes["first"][inner] - n0, nodes["first"][inner] + len(sa.bvh2) - n0)
    sw = type(sa)(prims=sa.prims, mats=sa.mats, tex=sa.tex, lights=sa.lights, bvh2=nodes, bvh4=sa.bvh4, primIdx=sa.primIdx, tlas=sa.tlas,
                  blas=sa.blas.copy())
    sw.blas["bvhIdx"] = [len(sa.bvh2) - n0, 0]
    RB.validate(sw)
    d = Device(Wd, Hd, **DEFAULT)
    try:
        d.upload(sw)
        before = _arrays(d)
        with pytest.raises(RtError, match="order of the BLAS roots") as e:
            d.rebuild_scene()
        assert e.value.code == W.RT_E_UNSUPPORTED
        _same(_arrays(d), before, "after the refusal")
        d.update_scene(sa.prims[:10], 0)          # (it can still be refit)
    finally:
        d.close()


def test_a_rebuilt_tlas_deeper_than_the_stack_is_refused_late_and_changes_nothing():
    """40 instances moved into a chain: TLAS::Build's clustering gives a TLAS 39 levels deep.  This is the latest refusal of the call:
    every BLAS has been built, every record derived and the TLAS built into the set that is not live.  That set must stay not live:
    arrays, kernel_info and the next frame of the rebuilding context and of a sharing partner stay as they were, and the next rebuild
    (into the same set) succeeds."""
    s, sa, view = RF._chain_scene(40)
    cam = scenes.camera_for(view, Wd, Hd)
    deep = RF._chain(sa, 40)
    d, b = Device(Wd, Hd, **DEFAULT), Device(Wd, Hd, **DEFAULT)
    try:
        d.upload(sa)
        b.share_scene(d)
        for rounds in range(2):               # the second round: the live set is a rebuilt one, the refused work goes into the other
            before, info, info_b = _arrays(d), d.kernel_info(), b.kernel_info()
            d.seed_default()
            d.reset()
            d.render(cam, 1)
            ref = d.read_accum()
            if rounds == 0:   # the frame every refusal is compared with is the oracle's frame of the grid, and shows the grid
                assert_bits(ref, RF._oracle_frames(sa, cam, 1)[0], "the frame before the refusals")
            live = np.frombuffer(before["instances"].tobytes(), W.BVHInstance).copy()
            deep["bvhIdx"] = live["bvhIdx"]
            for builder in RB.BUILDERS:
                _refused(d, W.RT_E_UNSUPPORTED, before, info, cam, ref, f"deep-TLAS ({builder}, round {rounds})", None, 0, deep, builder=builder)
                assert b.kernel_info() == info_b
                _same(_arrays(b), before, "the sharing partner after the refusal")
                b.seed_default()
                b.reset()
                b.render(cam, 1)
                assert_bits(b.read_accum(), ref, "the sharing partner's frame after the refusal")
            st = d.rebuild_scene(builder="sah")
            assert st["tlas_depth"] == RF._tlas_depth(sa.tlas)
            sa_new = RB.host_rebuild(s, None, builder="sah")
            _check(d, sa_new, f"a rebuild after the refusals (round {rounds})", **DEFAULT)
            assert b.kernel_info() == d.kernel_info()
            for dv in (d, b):
                dv.seed_default()
                dv.reset()
                dv.render(cam, 1)
                assert_bits(dv.read_accum(), RF._oracle_frames(sa_new, cam, 1)[0], f"the frame after the rebuild (round {rounds})")
    finally:
        b.close()
        d.close()


def test_a_blas_deeper_than_the_stack_is_refused_at_65_levels():
    """The ladder of rebuild_check: bound with a tree 64 levels deep (the most a context takes: 64 stack entries), a rebuild to 65
    levels is refused and changes nothing, one to another 64-level tree is taken."""
    s = RB.ladder_scene(-90)
    sa = s.arrays(bvh4=False)
    p65 = RB.ladder_scene(-93).arrays(bvh4=False).prims
    view = dict(origin=(0.0, 0.0, 3.0), forward=(0.0, 0.0, 1.0), fov=64.0, aperture=0.01)
    cam = scenes.camera_for(view, Wd, Hd)
    d = Device(Wd, Hd, **DEFAULT)
    try:
        d.upload(sa)
        before, info = _arrays(d), d.kernel_info()
        assert info["stack_entries"] == 64
        d.seed_default()
        d.render(cam, 1)
        ref = d.read_accum()
        _refused(d, W.RT_E_UNSUPPORTED, before, info, cam, ref, "65-level", p65, 0, None)
        other = RB.ladder_scene(-88).arrays(bvh4=False)
        st = d.rebuild_scene(other.prims, 0, None)
        assert st["max_depth"] == 64
        _check(d, other, "a 64-level rebuild", **DEFAULT)
        d.rebuild_scene(p65, 0, None, builder="lbvh")
        _check(d, RB.host_rebuild(s, p65, builder="lbvh"), "the 65-level ladder by the linear builder", **DEFAULT)
    finally:
        d.close()


def _balanced_tlas(n, mn, mx):
    """A TLAS over n identity instances of one BLAS (box mn, mx): leaves at 1 .. n, joins pairwise level by level behind them, node 0 a
    copy of the root - valid for rt_upload_scene, not what TLAS::Build makes beyond 256 instances."""
    t = np.zeros(2 * n, W.TLASNode)
    t["aabbMin"], t["aabbMax"] = mn, mx
    t["BLASidx"][1:n + 1] = np.arange(n)
    cur, nxt = list(range(1, n + 1)), n + 1
    while len(cur) > 1:
        up = []
        for k in range(0, len(cur) - 1, 2):
            t["leftRight"][nxt] = cur[k] + (cur[k + 1] << 16)
            up.append(nxt)
            nxt += 1
        if len(cur) % 2:
            up.append(cur[-1])
        cur = up
    t[0] = t[cur[0]]
    return t


def test_scenes_without_a_context_scene_or_of_another_tlas_shape_are_refused():
    empty = Device(Wd, Hd, **DEFAULT)
    try:
        with pytest.raises(RtError, match="no scene") as e:
            empty.rebuild_scene()
        assert e.value.code == W.RT_E_INVALID
    finally:
        empty.close()
    gt, sa, _ = R.build(blas=1, spheres=2)
    many = type(sa)(prims=sa.prims, mats=sa.mats, tex=sa.tex, lights=sa.lights, bvh2=sa.bvh2, bvh4=sa.bvh4, primIdx=sa.primIdx,
                    tlas=_balanced_tlas(257, sa.bvh2["aabbMin"][0], sa.bvh2["aabbMax"][0]), blas=np.repeat(sa.blas[:1], 257))
    gt2, sa2, _ = R.build(blas=2, spheres=2)
    extra = type(sa2)(prims=sa2.prims, mats=sa2.mats, tex=sa2.tex, lights=sa2.lights, bvh2=sa2.bvh2, bvh4=sa2.bvh4, primIdx=sa2.primIdx,
                      tlas=np.concatenate([sa2.tlas, sa2.tlas[1:2]]), blas=sa2.blas)
    for what, sw, frag in (("257 instances", many, "256 instances"), ("a TLAS of 2 x instances + 1 nodes", extra, "TLAS")):
        RB.validate(sw)
        d = Device(Wd, Hd, **DEFAULT)
        try:
            d.upload(sw)
            before, info = _arrays(d), d.kernel_info()
            for builder in RB.BUILDERS:
                with pytest.raises(RtError, match=frag) as e:
                    d.rebuild_scene(sw.prims, 0, None, builder=builder)
                assert e.value.code == W.RT_E_UNSUPPORTED, what
            _same(_arrays(d), before, f"after the refused rebuild of {what}")
            assert d.kernel_info() == info
        finally:
            d.close()


# ---- the preamble of every entry point that changes or inspects a bound copy -------------------------------------------------------------
def _calls(sa):
    """name -> the call on a Device, with arguments that pass every check before the one the table is about."""
    return {
        "rt_update_scene": lambda d: d.update_scene(),
        "rt_rebuild_scene": lambda d: d.rebuild_scene(),
        "rt_rebuild_ranges": lambda d: d.rebuild_ranges(["sah", "keep", "keep"]),
        "rt_resize_scene": lambda d: d.resize_scene(sa.prims, list(RC.COUNTS)),
        "rt_update_materials": lambda d: d.update_materials(mats=sa.mats),
        "rt_scene_blas_blocks": lambda d: d.blas_blocks(),
        "rt_refit_info": lambda d: d.refit_info(),
        "rt_debug_rebuild_allocations": lambda d: d.rebuild_allocations(),
        "rt_debug_get_scene_array": lambda d: d.scene_array("prims"),
    }


def _refusal(d, call):
    d._chk = d._chk_code            # (every wrapper then reports the code)
    with pytest.raises(RtError) as e:
        call(d)
    return e.value.code, str(e.value)


def test_the_preamble_of_every_entry_point_on_a_bound_copy():
    """A 16 x 16 context, no frame.  Without a scene each entry point answers RT_E_INVALID '<entry point>: no scene uploaded'; on a BVH4
    context bound through plain rt_upload_scene those that need the BVH2 answer RT_E_UNSUPPORTED 'lost its BVH2', rt_update_scene 'BVH4
    contexts cannot refit', and every array stays byte for byte what it was."""
    sa = RC.scene().arrays()
    assert len(sa.prims) == sum(RC.COUNTS)
    calls = _calls(sa)
    empty = Device(16, 16, **DEFAULT)
    try:
        for name, call in calls.items():
            assert _refusal(empty, call) == (W.RT_E_INVALID, f"{name}: no scene uploaded"), name
    finally:
        empty.close()
    every = [*W.SCENE_ARRAYS, *W.SCENE_ARRAYS_BVH4, *W.SCENE_ARRAYS_RESIZE, *W.SCENE_ARRAYS_MATERIALS]
    d4 = Device(16, 16, **dict(DEFAULT, accel=W.ACCEL_BVH4))
    try:
        d4.upload(sa)
        before, info = {k: d4.scene_array(k) for k in every}, d4.kernel_info()
        table = [(name, "lost its BVH2") for name in ("rt_rebuild_scene", "rt_rebuild_ranges", "rt_resize_scene", "rt_scene_blas_blocks")]
        for name, frag in table + [("rt_update_scene", "BVH4 contexts cannot refit")]:
            code, text = _refusal(d4, calls[name])
            assert code == W.RT_E_UNSUPPORTED and text.startswith(name + ": ") and frag in text, (name, code, text)
            for k in every:
                assert np.array_equal(d4.scene_array(k), before[k]), (name, k)
            assert d4.kernel_info() == info, name
    finally:
        d4.close()

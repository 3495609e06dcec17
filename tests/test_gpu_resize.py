"""In-place resizes on the MI355X (rt_resize_scene / rt_group_resize_scene): after a resize every device array (the light list included),
kernel_info and rt_shade_tables are those of a fresh upload of the new scene built from scratch on the host with the builder's host
form; the scan's edges, growth of the array sets, chains with updates and rebuilds, determinism, frames against the oracle on every
traversal path, queries against the float64 ground truth, holders and their queues, and every refusal leaving the scene as it was."""
import numpy as np
import pytest
import torch

import geom64 as G
import rebuild_check as RB
import refit_check as R
import resize_check as Z
import test_gpu_groundtruth as GT
import test_groundtruth_cpu as C
from helpers import DEFAULT, assert_bits
from magr_ray_tracer_amd import _lib as W, scenes
from magr_ray_tracer_amd.renderer import Device, Group, RtError
from oracle.oracle_py import Oracle, seed_stream

pytestmark = pytest.mark.gpu

Wd, Hd = Z.Wd, Z.Hd
DEV = torch.device("cuda", 0)
T4 = [None, RB.ROT, C.TRANSFORMS["scale"], C.TRANSFORMS["mirror"]]
TA, TB = C.invT(C.rot(1, 31.0), (0.8, 0.1, -3.0)), C.invT(np.diag([1.3, 0.8, 1.1]), (-0.6, 0.4, 2.5))
# the scenes (keywords of resize_check.build), each built once per builder and shared
SCENES = {
    "one220": dict(tris=(220,)), "one57": dict(tris=(57,)),
    "two220": dict(tris=(220, 220), spheres=(1, 1)), "two9-301": dict(tris=(9, 301), spheres=(2, 0)),
    "four-a": dict(tris=(60, 60, 60, 60), spheres=(1, 1), transforms=T4), "four-b": dict(tris=(80, 30, 45, 70), spheres=(0, 2), transforms=T4),
    "three": dict(tris=(50, 40, 30), spheres=(1,)),
    "two-inst2": dict(tris=(100, 80)), "two-inst5": dict(tris=(100, 80), extra=[(0, TA), (1, TB), (0, RB.ROT)]),
    "leaf-roots": dict(tris=(60, 1, 2)),
    "lights0": dict(tris=(40,), lights=0), "lights1": dict(tris=(33,), lights=1), "lights2": dict(tris=(25,), lights=2),
    "small": dict(tris=(20,), lights=1), "large": dict(tris=(300, 200), spheres=(2, 1), lights=3, extra=[(1, TA)]),
}
PAIRS = [("one220", "one57"), ("two220", "two9-301"), ("four-a", "four-b"), ("one220", "three"), ("three", "one57"),
         ("two-inst2", "two-inst5"), ("two-inst5", "two-inst2"), ("one220", "leaf-roots"), ("lights0", "lights1"), ("lights1", "lights0")]
_BUILT = {}


def scene(name, builder="sah"):
    if (name, builder) not in _BUILT:
        _BUILT[(name, builder)] = Z.build(builder=builder, **SCENES[name])
    return _BUILT[(name, builder)]


def _lights_n():
    """The first light count that no longer fits k_shade's staged tables beside the standard materials (queried, not assumed)."""
    if "n" not in _BUILT:
        _, sa, _ = scene("lights2")
        d = Device(Wd, Hd)
        try:
            d.upload(sa)
            cap, staged = d.shade_tables()
        finally:
            d.close()
        assert staged
        _BUILT["n"] = Z.first_light_count_that_does_not_fit(cap, len(sa.mats))
        SCENES["lightsN"] = dict(tris=(30,), lights=_BUILT["n"])
    return _BUILT["n"]


def _resized(a, b, builder, **kw):
    """A context bound to scene `a` (built with the SAH builder) and resized to `b`; returns (device, arrays of b, stats)."""
    _, sa0, _ = scene(a)
    _, sa1, counts = scene(b, builder)
    d = Device(Wd, Hd, **kw)
    try:
        d.upload(sa0, from_bvh2=kw.get("accel") == W.ACCEL_BVH4)
        st = Z.resize(d, sa1, counts, builder)
    except BaseException:
        d.close()
        raise
    return d, sa1, st


# ---- 1. array identity ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("builder", list(Z.BUILDERS))
@pytest.mark.parametrize("a,b", PAIRS, ids=[f"{a}->{b}" for a, b in PAIRS])
def test_resize_gives_the_arrays_of_a_fresh_upload(a, b, builder):
    d, sa1, st = _resized(a, b, builder)
    try:
        assert st["prims"] == len(sa1.prims) and st["nodes"] == len(sa1.bvh2) and st["n_idx"] == len(sa1.primIdx)
        assert st["blas_built"] == len(SCENES[b]["tris"]) and st["tlas_nodes"] == len(sa1.tlas) and st["max_depth"] == RB.depth(sa1)
        assert np.array_equal(np.frombuffer(d.scene_array("lights").tobytes(), np.uint32), sa1.lights)
        Z.check(d, sa1, f"{a} -> {b} / {builder}", key=(b, builder))
        single = len(sa1.blas) == 1
        assert d.kernel_info()["n_blas"] == len(sa1.blas) and (d.kernel_info()["persist"] == 1) == single
    finally:
        d.close()


@pytest.mark.parametrize("builder", list(Z.BUILDERS))
@pytest.mark.parametrize("to_many", [True, False])
def test_light_count_across_the_staged_tables_capacity(to_many, builder):
    n = _lights_n()
    assert n > 2
    a, b = ("lights2", "lightsN") if to_many else ("lightsN", "lights2")
    d, sa1, _ = _resized(a, b, builder)
    try:
        assert len(sa1.lights) == (n if to_many else 2)
        Z.check(d, sa1, f"{a} -> {b}", key=(b, builder))
        assert d.shade_tables()[1] == (not to_many)
    finally:
        d.close()


@pytest.mark.parametrize("builder", ["sah", "lbvh"])
@pytest.mark.parametrize("a,b", [("two220", "two9-301"), ("three", "one57"), ("two-inst2", "two-inst5")])
def test_resize_of_a_bvh4_copy_that_keeps_its_bvh2(a, b, builder):
    d, sa1, _ = _resized(a, b, builder, accel=W.ACCEL_BVH4)
    try:
        Z.check(d, sa1, f"BVH4 {a} -> {b} / {builder}", key=(b, builder), names=Z.ARRAYS_BVH4, from_bvh2=True, accel=W.ACCEL_BVH4)
        assert len(d.scene_array("bvh2Kept")) == len(sa1.bvh2) * W.BVHNode2.itemsize
    finally:
        d.close()


@pytest.mark.parametrize("builder", ["sah", "sbvh05"])
def test_primitives_in_a_torch_tensor_give_the_same_bytes(builder):
    _, sa0, _ = scene("two220")
    _, sa1, counts = scene("two9-301", builder)
    t = torch.from_numpy(np.ascontiguousarray(sa1.prims).view(np.uint8).copy()).to(DEV)
    d = Device(Wd, Hd)
    try:
        d.upload(sa0)
        Z.resize(d, sa1, counts, builder, prims=t)
        Z.check(d, sa1, "device-resident primitives", key=("two9-301", builder))
    finally:
        d.close()


# ---- 2. scan edges -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [255, 256, 257])
def test_light_scan_at_the_block_edges(n):
    _, sa0, _ = scene("small")
    d = Device(Wd, Hd)
    try:
        d.upload(sa0)
        patterns = {"first": [(1, "white-light"), (n - 1, "sand")], "last": [(n - 1, "sand"), (1, "red-light")],
                    "both-ends": [(1, "green-light"), (n - 2, "sand"), (1, "white-light")], "everywhere": [(n, "white-light")], "nowhere": [(n, "sand")]}
        for name, runs in patterns.items():
            sa, counts = Z.build_runs(runs)
            assert len(sa.prims) == n
            Z.resize(d, sa, counts, "sah")
            Z.check(d, sa, f"{n} primitives, lights {name}")
            want = {"first": [0], "last": [n - 1], "both-ends": [0, n - 1], "everywhere": list(range(n)), "nowhere": []}[name]
            assert list(np.frombuffer(d.scene_array("lights").tobytes(), np.uint32)) == want
    finally:
        d.close()


# ---- 3. growth -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("builder", ["sah", "lbvh", "sbvh0"])
def test_alternating_shapes_stop_allocating(builder, monkeypatch):
    monkeypatch.setenv("RT355_REBUILD_INITIAL_CAP", "64")
    _, small, cs = scene("small", builder)
    _, large, cl = scene("large", builder)
    d = Device(Wd, Hd)
    try:
        d.upload(small)
        allocs = []
        for visit in range(3):
            for name, sa, counts in (("large", large, cl), ("small", small, cs)):
                Z.resize(d, sa, counts, builder)
                Z.check(d, sa, f"visit {visit + 1} to {name} / {builder}", key=(name, builder))
                allocs.append(d.rebuild_allocations())
        assert allocs[0] > 0
        assert allocs[4] == allocs[3] and allocs[5] == allocs[4], f"the third visits allocated: {allocs}"
        d.update_scene(small.prims, 0, None)                              # the update's staging follows the shape
        Z.check(d, small, "an update after the resizes", key=("small", builder))
    finally:
        d.close()


# ---- 4. chains -----------------------------------------------------------------------------------------------------------------------
def _jittered(prims, seed, scale=0.04):
    p = prims.copy()
    rng = np.random.default_rng(seed)
    tri = p["objType"] == W.PRIM_TRIANGLE
    for f in ("v0", "v1", "v2"):
        p[f][tri, :3] += rng.normal(scale=scale, size=(int(tri.sum()), 3)).astype(np.float32)
    return p


@pytest.mark.parametrize("accel", [W.ACCEL_BVH2, W.ACCEL_BVH4])
def test_resizes_updates_and_rebuilds_chain(accel):
    """resize -> update_scene -> rebuild_scene("refit") -> rebuild_scene("lbvh") -> resize; after each step the arrays equal the host
    restatement's on a Scene built from scratch (SetPrimitives / Refit / Rebuild).  A BVH4 copy has no update_scene: it refits twice."""
    bvh4 = accel == W.ACCEL_BVH4
    names = Z.ARRAYS_BVH4 if bvh4 else Z.ARRAYS
    kw = dict(names=names, from_bvh2=bvh4, accel=accel)
    _, sa0, _ = scene("two220")
    gt, sa1, counts = Z.build(**SCENES["four-b"])                        # (a Scene of its own: the chain changes it)
    s = gt.s
    p2, p3, p4 = _jittered(sa1.prims, 1), _jittered(sa1.prims, 2), _jittered(sa1.prims, 3, 0.2)
    inst = sa1.blas.copy()
    inst["invT"][1] = TA.ravel()
    d = Device(Wd, Hd, accel=accel)
    try:
        d.upload(sa0, from_bvh2=bvh4)
        Z.resize(d, sa1, counts, "sah")
        Z.check(d, sa1, "resize", **kw)
        if bvh4:
            d.rebuild_scene(p2, 0, inst, builder="refit")
        else:
            d.update_scene(p2, 0, inst)
        s.SetPrimitives(0, p2)
        s.SetInstanceTransform(1, TA)
        s.Refit()
        Z.check(d, s.arrays(), "update", **kw)
        d.rebuild_scene(p3[80:110], 80, None, builder="refit")
        s.SetPrimitives(80, p3[80:110])
        s.Refit()
        Z.check(d, s.arrays(), "refit of a slice", **kw)
        d.rebuild_scene(p4, 0, None, builder="lbvh")
        Z.check(d, RB.host_rebuild(s, p4, builder="lbvh", bvh4=True), "rebuild (lbvh)", **kw)
        _, sa5, c5 = scene("two-inst5", "sbvh0")
        Z.resize(d, sa5, c5, "sbvh0")
        Z.check(d, sa5, "second resize", key=("two-inst5", "sbvh0"), **kw)
        d.rebuild_scene(None, 0, None, builder="sah")                     # ... and the bookkeeping is the new shape's: two BLAS, five instances
        _, sa6, _ = scene("two-inst5", "sah")
        Z.check(d, sa6, "rebuild after the second resize", key=("two-inst5", "sah"), **kw)
    finally:
        d.close()


# ---- 5. determinism ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("builder", list(Z.BUILDERS))
def test_the_same_resize_twice_gives_identical_arrays(builder):
    d, sa1, _ = _resized("four-a", "four-b", builder)
    try:
        first = Z.arrays(d)
        _, _, counts = scene("four-b", builder)
        for k in range(2):                                                # (each call writes the set the one before did not)
            Z.resize(d, sa1, counts, builder)
            Z.same(Z.arrays(d), first, f"resize {k + 2}")
    finally:
        d.close()


# ---- 6. frames -----------------------------------------------------------------------------------------------------------------------
FRAME_CASES = [k for k, v in GT.CASES.items() if v[1] == W.ACCEL_BVH2] + ["bvh4-persist", "bvh4-tlas-persist"]
_ROOM = {}


def _frame_scenes(kind):
    """(arrays bound, arrays resized to, counts): one BLAS 220 -> 57 triangles, or four BLAS -> four BLAS of other sizes under transforms."""
    if kind not in _ROOM:
        a, b = ("one220", "one57") if kind == "one" else ("four-a", "four-b")
        _ROOM[kind] = (scene(a)[1], scene(b)[1], scene(b)[2])
    return _ROOM[kind]


@pytest.mark.parametrize("case", FRAME_CASES)
def test_frames_across_a_resize_match_the_oracle(case, monkeypatch):
    """Two frames, a resize, two more: accumulator, seeds and the extend counters equal the oracle rendering two frames of the first
    scene's arrays and then two of the second's, accumulator carried; kernel_info confirms the traversal path before and after."""
    if case == "bvh4-tlas-persist":
        kind, accel, variant, env = "multi", W.ACCEL_BVH4, 6, {}
        want = None
    else:
        kind, accel, variant, env, want = GT.CASES[case]
    monkeypatch.setenv("RT355_TUNE", GT.TUNE)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    sa0, sa1, counts = _frame_scenes(kind)
    bvh4 = accel == W.ACCEL_BVH4
    cam = scenes.camera_for(Z.VIEW, Wd, Hd)
    v = dict(DEFAULT, accel=accel)
    acc, seeds, _, _ = Oracle(sa0, Wd, Hd, **v).render(cam, 2)
    seeds2 = seeds.copy()
    acc, seeds, _, _ = Oracle(sa1, Wd, Hd, **v).render(cam, 2, accum=acc, seeds=seeds)

    def path(info):
        if want is None:
            assert info["persist4"] in (2, 3) and info["persist"] == 0, (case, info)
        else:
            for k, wv in want.items():
                assert info[k] == wv, (case, info)
    d = Device(Wd, Hd, extend_variant=variant, **v)
    try:
        d.upload(sa0, from_bvh2=bvh4)
        path(d.kernel_info())
        d.seed_default()
        d.render(cam, 2)
        Z.resize(d, sa1, counts, "sah")
        path(d.kernel_info())
        d.reset_counters()
        d.render(cam, 2)
        assert_bits(d.read_accum(), acc, f"{case}: frames across a resize vs oracle")
        assert np.array_equal(d.get_seeds(), seeds)
        got = d.counters()
        f = Device(Wd, Hd, extend_variant=variant, **v)
        try:
            f.upload(sa1, from_bvh2=bvh4)
            f.set_seeds(seeds2)
            f.render(cam, 2)
            ref = f.counters()
        finally:
            f.close()
        for k in ("extend_rays", "extend_node_visits", "extend_prim_tests", "connect_rays", "connect_node_visits", "connect_prim_tests"):
            assert got[k] == ref[k], (case, k, got[k], ref[k])
    finally:
        d.close()


# ---- 7. queries ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("a,b", [("one220", "two9-301"), ("four-a", "one57")])
def test_queries_after_a_resize_against_the_float64_ground_truth(a, b):
    d, sa1, _ = _resized(a, b, "sah")
    try:
        gt = scene(b)[0]
        rng = np.random.default_rng(9)
        n = 3000
        O = np.tile(np.array(Z.VIEW["origin"], np.float32), (n, 1)) + rng.normal(scale=0.3, size=(n, 3)).astype(np.float32)
        target = rng.uniform(-3.5, 3.5, (n, 3))
        D = G._unit32(target - O)
        rays = G.make_rays(O, D)
        r = d.trace(np.ascontiguousarray(rays["O"][:, :3]), np.ascontiguousarray(rays["D"][:, :3]), point=True)
        got = rays.copy()
        for f in ("t", "primIdx", "u", "v"):
            got[f] = r["hit"][f]
        got["I"] = r["point"]
        assert G.compare(gt, rays, got, "camera", f"{a} -> {b}: closest") > 0.9
        assert (got["primIdx"] >= 0).sum() > n // 4 and got["primIdx"].max() < len(sa1.prims)
        tmax = rng.uniform(6.0, 14.0, n).astype(np.float32)
        occ = d.trace(np.ascontiguousarray(rays["O"][:, :3]), np.ascontiguousarray(rays["D"][:, :3]), tmax=tmax, mode="any")
        want, dec = G.any_hit(gt, rays["O"], rays["D"], tmax)
        assert dec.mean() > 0.9 and np.array_equal(occ.astype(bool)[dec], want[dec])
    finally:
        d.close()


# ---- 8. holders ----------------------------------------------------------------------------------------------------------------------
def _oracle_frame(sa, cam, seeds=None):
    return Oracle(sa, Wd, Hd, **DEFAULT).render(cam, 1, seeds=seeds)[0]


def test_group_lanes_and_sharing_contexts_render_the_resized_scene():
    _, sa0, _ = scene("four-a")
    _, sa1, counts = scene("one57")
    cam = scenes.camera_for(Z.VIEW, Wd, Hd)
    a, b = Device(Wd, Hd, **DEFAULT), Device(Wd, Hd, **DEFAULT)
    g = Group(Wd, Hd, lanes=3)
    try:
        a.upload(sa0)
        b.share_scene(a)
        g.upload(sa0)
        g.seed(0)
        b.seed_default()
        b.render(cam, 1)                                                  # work in flight on a holder that is not the one resizing
        g.render(cam, 3)
        Z.resize(a, sa1, counts, "sah")
        Z.resize(g, sa1, counts, "sah")
        want, info, tables = Z.fresh(sa1, key=("one57", "sah"), **DEFAULT)
        for h in [a, b] + g.devs[:1]:
            Z.same(Z.arrays(h), want, "a holder's arrays")
        for h in (a, b):
            assert h.kernel_info() == info and h.shade_tables() == tables
        lanes = [h.kernel_info() for h in g.devs]
        assert all(k == lanes[0] for k in lanes) and lanes[0]["n_blas"] == 1 and lanes[0]["persist"] == 1, lanes
        ref = _oracle_frame(sa1, cam)
        for dv in (a, b):
            dv.seed_default()
            dv.reset()
            dv.render(cam, 1)
            assert_bits(dv.read_accum(), ref, "shared pair after a resize")
        g.seed(0)
        g.reset()
        g.render(cam, 3)
        exp = None
        for m in range(3):
            r = _oracle_frame(sa1, cam, seeds=seed_stream(m * Wd * Hd, Wd * Hd))
            exp = r if exp is None else exp + r
        assert_bits(g.read_accum(), exp, "3-lane group after a resize")
    finally:
        g.close()
        b.close()
        a.close()


def test_a_holders_queues_are_emptied_and_set_rays_checks_the_new_count():
    """Three holders of one copy.  b has rays, hits and shadow rays of the old array queued when a resizes: whichever call comes first
    afterwards (here rt_debug_get_shadow) finds the queues empty.  c has not launched since the resize when rays are injected into it:
    it takes the copy over first, so the injected rays are checked against the new count and are still there afterwards."""
    _, sa0, _ = scene("one220")
    _, sa1, counts = scene("one57")
    n1 = len(sa1.prims)
    cam = scenes.camera_for(Z.VIEW, Wd, Hd)
    a, b, c = Device(Wd, Hd, **DEFAULT), Device(Wd, Hd, **DEFAULT), Device(Wd, Hd, **DEFAULT)
    try:
        a.upload(sa0)
        for x in (b, c):
            x.share_scene(a)
            x.seed_default()
            x.stage_begin_frame()
            x.stage_generate(cam)
            x.stage_extend(0)
        b.stage_shade(0)
        old = b.get_rays(0)
        assert len(old) == Wd * Hd and old["primIdx"].max() >= n1          # the queue names primitives the new array lacks
        assert len(b.get_shadow(0, 0)) > 0 and len(b.get_rays(1)) > 0
        Z.resize(a, sa1, counts, "sah")
        assert len(b.get_shadow(0, 0)) == 0                                # (the first call on b since the resize)
        assert len(b.get_rays(0)) == 0 and len(b.get_rays(1)) == 0
        rays = old[:4].copy()
        rays["primIdx"] = [0, n1 - 1, -1, n1]
        # c, which has not taken the copy over yet: the refusal, then good rays, which must survive the takeover
        with pytest.raises(RtError, match=rf"primIdx {n1} outside \[-1, {n1}\)"):
            c.set_rays(0, rays)
        c.set_rays(0, rays[:3])
        got = c.get_rays(0)
        assert len(got) == 3 and list(got["primIdx"]) == [0, n1 - 1, -1] and np.array_equal(got["pixelIdx"], rays["pixelIdx"][:3])
        c.stage_extend(0)                                                  # a stage on the injected queue: three rays traced in the new scene
        after = c.get_rays(0)
        assert len(after) == 3 and after["primIdx"].max() < n1
        # a itself, whose first call since its resize is an injection
        a.set_rays(0, rays[:2])
        assert len(a.get_rays(0)) == 2
        with pytest.raises(RtError, match="primIdx"):
            b.set_rays(0, rays)
        b.set_rays(0, rays[:3])
        assert len(b.get_rays(0)) == 3
    finally:
        c.close()
        b.close()
        a.close()


# ---- 9. refusals ---------------------------------------------------------------------------------------------------------------------
def _unchanged(d, twin, before, cam, what, names=Z.ARRAYS):
    Z.same(Z.arrays(d, names), before, what)
    for x in (d, twin):
        x.render(cam, 1)
    assert_bits(d.read_accum(), twin.read_accum(), f"{what}: the next frame")
    assert np.array_equal(d.get_seeds(), twin.get_seeds())


class _Claims:
    """Device memory at `ptr` handed over as n primitive records (what Device.resize_scene reads of a tensor)."""

    def __init__(self, ptr, n):
        self.ptr, self.n = ptr, n

    def is_contiguous(self):
        return True

    def numel(self):
        return self.n * W.Primitive.itemsize

    def element_size(self):
        return 1

    def data_ptr(self):
        return self.ptr


def test_refusals_leave_the_scene_and_its_next_frame_as_they_were():
    _, sa0, _ = scene("two220")
    _, sa1, counts = scene("two9-301")
    cam = scenes.camera_for(Z.VIEW, Wd, Hd)
    n, nm = len(sa1.prims), len(sa1.mats)
    rc, ir, inst = Z.shape_of(sa1, counts)
    sing = inst.copy()
    sing["invT"][1] = np.diag([1.0, 0.0, 1.0, 1.0]).astype(np.float32).ravel()
    bad_mat, bad_type = sa1.prims.copy(), sa1.prims.copy()
    bad_mat["matIdx"][n - 1] = nm
    bad_type["objType"][n - 1] = 3
    both = bad_type.copy()
    both["matIdx"][7] = -1                                                # two bad records: the lowest index is named
    coincident = np.repeat(sa1.prims[:1], 128)
    t_bad = torch.from_numpy(np.ascontiguousarray(bad_mat).view(np.uint8).copy()).to(DEV)
    t_bad_type = torch.from_numpy(np.ascontiguousarray(bad_type).view(np.uint8).copy()).to(DEV)
    # 20 MiB: a block of its own in torch's allocator, so the allocation the runtime knows ends where the tensor ends
    big = torch.zeros(163840 * W.Primitive.itemsize, dtype=torch.uint8, device=DEV)
    d, twin = Device(Wd, Hd, **DEFAULT), Device(Wd, Hd, **DEFAULT)
    try:
        for x in (d, twin):
            x.upload(sa0)
            x.seed_default()
            x.render(cam, 1)
        before = Z.arrays(d)
        cases = [
            ("count sum off by one", lambda: d.resize_scene(sa1.prims, [counts[0], counts[1] - 1], ir, inst), W.RT_E_INVALID, "primitives in all"),
            ("a zero count", lambda: d.resize_scene(sa1.prims, [n, 0], ir, inst), W.RT_E_INVALID, "holds 0 primitives"),
            ("an unnamed range", lambda: d.resize_scene(sa1.prims, rc, [0, 0], inst), W.RT_E_INVALID, "named by no instance"),
            ("instRange out of range", lambda: d.resize_scene(sa1.prims, rc, [0, 2], inst), W.RT_E_INVALID, "instRange 2 outside"),
            ("257 instances", lambda: d.resize_scene(sa1.prims, rc, [0, 1] + [0] * 255), W.RT_E_INVALID, "257 instances"),
            ("a singular invT", lambda: d.resize_scene(sa1.prims, rc, ir, sing), W.RT_E_INVALID, "instance 1: the transform is singular"),
            ("matIdx == nMats at the last primitive", lambda: d.resize_scene(bad_mat, rc, ir, inst), W.RT_E_INVALID, f"primitive {n - 1}: objType 2 / matIdx {nm} out of range"),
            ("objType == 3 at the last primitive", lambda: d.resize_scene(bad_type, rc, ir, inst), W.RT_E_INVALID, f"primitive {n - 1}: objType 3 "),
            ("the lowest bad index is named", lambda: d.resize_scene(both, rc, ir, inst), W.RT_E_INVALID, "primitive 7: objType 2 / matIdx -1"),
            ("matIdx == nMats in a torch tensor", lambda: d.resize_scene(t_bad, rc, ir, inst), W.RT_E_INVALID, f"primitive {n - 1}: "),
            ("objType == 3 in a torch tensor", lambda: d.resize_scene(t_bad_type, rc, ir, inst), W.RT_E_INVALID, f"primitive {n - 1}: objType 3 "),
            ("a device pointer whose allocation ends one record early", lambda: d.resize_scene(_Claims(big.data_ptr() + W.Primitive.itemsize, 163840), [163840], [0]),
             W.RT_E_INVALID, "prims needs 20971520 bytes .* its allocation ends 128 bytes earlier"),
            ("RT_REBUILD_REFIT", lambda: d.resize_scene(sa1.prims, rc, ir, inst, builder="refit"), W.RT_E_INVALID, "no tree to refit"),
            ("no primitives", lambda: d.resize_scene(sa1.prims[:0], rc, ir, inst), W.RT_E_INVALID, "null argument"),
            ("128 coincident triangles", lambda: d.resize_scene(coincident, [128], [0]), W.RT_E_UNSUPPORTED, "derived layout"),
            ("a 65-level tree", lambda: d.resize_scene(RB.ladder_scene(-93).arrays(bvh4=False).prims, [192], [0]), W.RT_E_UNSUPPORTED, "stack entries"),
        ]
        for what, call, code, pattern in cases:
            with pytest.raises(RtError, match=pattern) as e:
                call()
            assert e.value.code == code, (what, e.value)
            _unchanged(d, twin, before, cam, what)
        Z.resize(d, sa1, counts, "sah")                                   # ... and the context still takes a good one
        Z.check(d, sa1, "after the refusals", key=("two9-301", "sah"), **DEFAULT)
    finally:
        twin.close()
        d.close()


def _refused_with_a_twin(sa_bound, names, pattern, **kw):
    """Two contexts bound alike render a frame; one is asked for a resize that must be refused as RT_E_UNSUPPORTED: its arrays stay and its
    next frame equals that of the twin that was never asked."""
    _, sa1, counts = scene("one57")
    cam = scenes.camera_for(Z.VIEW, Wd, Hd)
    d, twin = Device(Wd, Hd, **kw), Device(Wd, Hd, **kw)
    try:
        for x in (d, twin):
            x.upload(sa_bound)
            x.seed_default()
            x.render(cam, 1)
        before = Z.arrays(d, names)
        with pytest.raises(RtError, match=pattern) as e:
            Z.resize(d, sa1, counts, "sah")
        assert e.value.code == W.RT_E_UNSUPPORTED
        _unchanged(d, twin, before, cam, pattern, names)
    finally:
        twin.close()
        d.close()


def test_a_classic_bvh4_copy_is_refused():
    _, sa0, _ = scene("two220")
    _refused_with_a_twin(sa0, Z.ARRAYS_BVH4, "lost its BVH2", **dict(DEFAULT, accel=W.ACCEL_BVH4))   # rt_upload_scene on a BVH4 context: the BVH2 is gone


def test_a_bound_scene_with_a_gap_between_its_ranges_is_refused():
    # the second BLAS starts two primitives after the first ends: two lights that belong to no BLAS
    s2 = scenes.Scene()
    scenes._std_materials(s2)
    rng = np.random.default_rng(4)
    soup, lights = C._soup(rng, 30, -1.0, 1.0, 0.3), C._soup(rng, 2, 3.0, 3.5, 0.3)
    s2.AddTriangles(soup, "sand")
    s2.BuildBLAS(0)
    s2.AddTriangles(lights, "white-light")
    s2.AddTriangles(C._soup(rng, 20, -1.0, 1.0, 0.3), "green")
    s2.BuildBLAS(32)
    sg = s2.arrays()
    assert len(sg.prims) == 52 and s2.blas_ranges() == [(0, 30), (32, 20)]
    _refused_with_a_twin(sg, Z.ARRAYS, r"leave a gap: primitives \[30, 32\)", **DEFAULT)

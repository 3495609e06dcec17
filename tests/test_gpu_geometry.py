"""Replacement geometry that lies on the MI355X (rt_update_geometry, rt_rebuild_geometry, rt_rebuild_geometry_ranges and their group
forms): each call leaves the scene copy as its counterpart - update_scene, rebuild_scene, rebuild_ranges - leaves it for host records
over the same window, bit for bit in every array; the vertex form's records are Scene::AddTriangle's for the same vertices; refusals
found on the device change nothing; a stable caller stops allocating."""
import numpy as np
import pytest
import torch

import geometry_check as GC
import refit_check as R
from helpers import DEFAULT, assert_bits
from tlas_check import assert_seen
from magr_ray_tracer_amd import _lib as W, scenes
from magr_ray_tracer_amd.renderer import Device, Group, RtError
from oracle.oracle_py import Oracle, seed_stream

pytestmark = pytest.mark.gpu

Wd, Hd = 160, 120
ARRAYS = list(W.SCENE_ARRAYS)
N = GC.NB0 + 220 + GC.N_FLIP
# (1, 63) and (7, 65) sit on either side of a wavefront, (219, 2) reaches from the soup into the lights, (223, 2) crosses into BLAS 1,
# (444, 2) are the triangles added with flipNormal=True
WINDOWS = [(0, 1), (1, 63), (7, 65), (219, 2), (223, 2), (444, 2), (0, N)]
_S = {}


def _scene(alpha=0.0, which="bound"):
    """The arrays of geometry_check.build: as bound, or built through AddTriangle from the moved vertices (the lights move too)."""
    key = (alpha, which)
    if key not in _S:
        _S[key] = GC.build(R.identity if which == "bound" else GC.moved(), alpha=alpha)[1]
        assert len(_S[key].prims) == N
    return _S[key]


def _arrays(d, names=ARRAYS):
    return {k: d.scene_array(k) for k in names}


def _same_arrays(got, want, what):
    for k in want:
        assert len(got[k]) == len(want[k]) and np.array_equal(got[k], want[k]), f"{what}: {k} differs ({len(got[k])} / {len(want[k])} bytes)"


def _device(sa, **kw):
    d = Device(Wd, Hd, **kw)
    d.upload(sa, from_bvh2=kw.get("accel") == W.ACCEL_BVH4)
    return d


def _gpu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _gpu_records(prims):
    return _gpu(np.ascontiguousarray(prims).view(np.uint8).reshape(-1, 128))


def _sources(v, where, stride, index):
    """positions (and indices) of the (count, 3, 3) vertices v as the call takes them."""
    p, idx = GC.indexed(v) if index else (v.reshape(-1, 3), None)
    if where == "numpy":
        return dict(positions=GC.strided(p, stride), indices=idx)
    wide = np.full((len(p), stride // 4), np.nan, np.float32)
    wide[:, :3] = p
    t = _gpu(wide)[:, :3]
    assert (stride == 12) == t.is_contiguous()
    return dict(positions=t, indices=None if idx is None else _gpu(idx.astype(np.int32)))


# ---- 4. the kernel against the host rule ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("first,count", WINDOWS)
def test_vertices_give_the_arrays_of_the_host_records(first, count):
    sa0, sa1 = _scene(), _scene(which="moved")
    v = GC.verts(sa1.prims[first:first + count])
    s = GC.build()[0].s
    s.SetVertices(first, v)
    mirror = s.arrays(bvh4=False).prims
    GC.same_records(mirror[first:first + count], sa1.prims[first:first + count], "the host mirror against AddTriangle")
    if first == 0 and count == N:
        assert GC.is_flipped(sa0.prims).sum() == GC.N_FLIP
    ref = _device(sa0)
    try:
        ref.update_scene(mirror[first:first + count], first)
        want = _arrays(ref)
    finally:
        ref.close()
    fresh = GC.build()[0].s                                                       # test_gpu_refit's _fresh(_host_refit(...))
    p = sa0.prims.copy()
    p[first:first + count] = sa1.prims[first:first + count]
    fresh.SetPrimitives(0, p)
    fresh.Refit()
    ref = _device(fresh.arrays(bvh4=False))
    try:
        _same_arrays(_arrays(ref), want, "the two references")
    finally:
        ref.close()
    d = _device(sa0)
    try:
        for where in ("torch", "numpy"):
            for stride in (12, 16, 32):
                for index in (False, True):
                    what = f"[{first}, +{count}) {where} stride {stride} {'indexed' if index else 'packed'}"
                    d.update_scene(sa0.prims, 0)                                  # the bound records again
                    assert not np.array_equal(d.scene_array("prims"), want["prims"])
                    st = d.update_geometry(first, **_sources(v, where, stride, index))
                    assert st["prims"] == count and st["gpu_ms"] > 0, (what, st)
                    GC.same_records(d.scene_array("prims").view(W.Primitive), mirror, what)
                    _same_arrays(_arrays(d), want, what)
    finally:
        d.close()


# ---- 5. records form from the GPU -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("first,count", WINDOWS)
def test_records_on_the_gpu_give_the_arrays_of_records_on_the_host(first, count):
    sa0, sa1 = _scene(), _scene(which="moved")
    recs = sa1.prims[first:first + count]
    a, b = _device(sa0), _device(sa0)
    try:
        st = a.update_geometry(first, prims=_gpu_records(recs))
        st2 = b.update_scene(recs, first)
        assert {k: v for k, v in st.items() if k != "gpu_ms"} == {k: v for k, v in st2.items() if k != "gpu_ms"}
        _same_arrays(_arrays(a), _arrays(b), f"[{first}, +{count}) records on the GPU")
        b.update_geometry(first, prims=recs)                                      # host records through the new door
        _same_arrays(_arrays(b), _arrays(a), f"[{first}, +{count}) records on the host")
    finally:
        a.close()
        b.close()


def _frame(d, cam):
    d.seed_default()
    d.reset()
    d.render(cam, 1)
    return d.read_accum()


def _refused(d, cam, before, ref, what, match, call):
    with pytest.raises(RtError, match=match) as e:
        call()
    assert e.value.code == W.RT_E_INVALID, (what, e.value.code)
    _same_arrays(_arrays(d), before, f"after the refusal: {what}")
    assert_bits(_frame(d, cam), ref, f"the frame after the refusal: {what}")
    return str(e.value)


def test_a_changed_matidx_on_the_gpu_is_refused_with_the_hosts_message():
    sa0, sa1 = _scene(), _scene(which="moved")
    cam = scenes.camera_for(GC.build()[2], Wd, Hd)
    first, count = 7, 65
    d = _device(sa0, **DEFAULT)
    try:
        before, ref = _arrays(d), _frame(d, cam)
        for at in ([0], [count - 1], [count - 1, 0]):
            bad = sa1.prims[first:first + count].copy()
            bad["matIdx"][at] += 1
            with pytest.raises(RtError) as host:
                d.update_scene(bad, first)
            want = str(host.value).replace("rt_update_scene", "rt_update_geometry")
            assert f"primitive {first + min(at)} changes its objType / matIdx" in want
            got = _refused(d, cam, before, ref, f"matIdx at {at}", "changes its objType / matIdx", lambda: d.update_geometry(first, prims=_gpu_records(bad)))
            assert got == want
        bad["objType"][3] = W.PRIM_SPHERE
        _refused(d, cam, before, ref, "objType through the rebuild", f"rt_rebuild_geometry: primitive {first} changes",
                 lambda: d.rebuild_geometry(first, prims=_gpu_records(bad), builder="lbvh"))
    finally:
        d.close()


# ---- 6. through the rebuild and the range plans ----------------------------------------------------------------------------------------
NAMES = {**W.SCENE_ARRAYS, "rootEntry": W.SCENE_ARRAYS_BVH4["rootEntry"]}
INSIDE = (GC.NB0 + 3, 130)                                                         # a window inside BLAS 1


def _pair_check(sa0, new, old, what, names=NAMES, **kw):
    """`new` on one device, `old` (the counterpart with host records) on another: arrays, ranges_info and kernel_info must agree."""
    a, b = _device(sa0, **kw), _device(sa0, **kw)
    try:
        sa_, sb_ = new(a), old(b)
        for k in ("prims", "blas_built", "nodes", "n_idx", "max_depth", "tlas_nodes", "tlas_depth", "reconfigured"):
            assert sa_[k] == sb_[k], (what, k, sa_[k], sb_[k])
        _same_arrays(_arrays(a, names), _arrays(b, names), what)
        assert a.ranges_info() == b.ranges_info() and a.kernel_info() == b.kernel_info(), what
        assert not np.array_equal(a.scene_array("prims"), sa0.prims.view(np.uint8))
        return a.ranges_info()
    finally:
        a.close()
        b.close()


@pytest.mark.parametrize("builder", ["lbvh", "sah"])
def test_rebuild_geometry_is_rebuild_scene(builder):
    sa0, sa1 = _scene(1.0), _scene(1.0, "moved")
    first, count = GC.NB0 - 3, 100                                                # across the BLAS boundary
    recs = sa1.prims[first:first + count]
    src = _sources(GC.verts(recs), "torch", 16, True)
    _pair_check(sa0, lambda d: d.rebuild_geometry(first, builder=builder, **src), lambda d: d.rebuild_scene(recs, first, builder=builder),
                f"rebuild_geometry({builder})")


@pytest.mark.parametrize("alpha,plan", [(1.0, ["keep", "refit"]), (1.0, ["keep", "lbvh"]), (0.0, ["keep", "refit"])])
def test_rebuild_geometry_ranges_is_rebuild_ranges(alpha, plan):
    sa0, sa1 = _scene(alpha), _scene(alpha, "moved")
    first, count = INSIDE
    recs = sa1.prims[first:first + count]
    for form, src in (("vertices", _sources(GC.verts(recs), "torch", 12, False)), ("records", dict(prims=_gpu_records(recs)))):
        info = _pair_check(sa0, lambda d: d.rebuild_geometry_ranges(plan, first, **src), lambda d: d.rebuild_ranges(plan, recs, first),
                           f"rebuild_geometry_ranges({plan}, alpha {alpha}, {form})")
        assert info["kept"] == 1 and info["refit"] + info["built"] == 1, info


def test_a_window_that_touches_the_kept_blas_is_refused_as_today():
    sa0, sa1 = _scene(1.0), _scene(1.0, "moved")
    cam = scenes.camera_for(GC.build()[2], Wd, Hd)
    first, count = GC.NB0 - 1, 20
    recs = sa1.prims[first:first + count]
    d = _device(sa0, **DEFAULT)
    try:
        before, ref = _arrays(d), _frame(d, cam)
        with pytest.raises(RtError) as host:
            d.rebuild_ranges(["keep", "refit"], recs, first)
        got = _refused(d, cam, before, ref, "a kept BLAS in the window", "rt_rebuild_geometry_ranges",
                       lambda: d.rebuild_geometry_ranges(["keep", "refit"], first, positions=_gpu(GC.verts(recs))))
        assert got == str(host.value).replace("rt_rebuild_ranges", "rt_rebuild_geometry_ranges")
    finally:
        d.close()


def test_a_bvh4_copy_that_keeps_its_bvh2_refits_from_vertices():
    sa0, sa1 = _scene(1.0), _scene(1.0, "moved")
    kw = dict(accel=W.ACCEL_BVH4)
    names = {**W.SCENE_ARRAYS, **W.SCENE_ARRAYS_BVH4}
    src = _sources(GC.verts(sa1.prims), "torch", 12, True)
    _pair_check(sa0, lambda d: d.rebuild_geometry(0, builder="refit", **src), lambda d: d.rebuild_scene(sa1.prims, 0, builder="refit"),
                "a BVH4 copy: rebuild_geometry(refit)", names, **kw)
    d = _device(sa0, **kw)
    try:
        with pytest.raises(RtError, match="rt_update_geometry: BVH4"):
            d.update_geometry(0, **src)
    finally:
        d.close()


# ---- 7. frames ------------------------------------------------------------------------------------------------------------------------
def test_frames_across_update_geometry_match_the_oracle():
    """Two frames, every vertex moved on the GPU (the lights among them), two more: accumulator and seeds equal the oracle rendering
    the same sequence on the host-updated scene, the counters those of a fresh context on it; a group of 2 lanes sees the update."""
    gt0, sa0, view = GC.build()
    gt1, sa1, _ = GC.build(GC.moved())
    saR = R.host_update(GC.build()[0], gt1, sa1)
    cam = scenes.camera_for(view, Wd, Hd)
    lights = list(GC.LIGHTS)
    assert np.array_equal(sa0.lights, lights) and not np.array_equal(sa0.prims["v0"][lights], sa1.prims["v0"][lights])
    pos, idx = GC.indexed(GC.verts(sa1.prims))
    src = dict(positions=_gpu(pos), indices=_gpu(idx.astype(np.int32)))
    acc, seeds, _, _ = Oracle(sa0, Wd, Hd, **DEFAULT).render(cam, 2)
    seeds2 = seeds.copy()
    acc, seeds, e, c = Oracle(saR, Wd, Hd, **DEFAULT).render(cam, 2, accum=acc, seeds=seeds)
    print("inst_visits / rays", assert_seen(e, c, "the oracle's frames after the update"))
    d = _device(sa0, **DEFAULT)
    try:
        d.seed_default()
        d.render(cam, 2)
        d.update_geometry(0, **src)
        d.reset_counters()
        d.render(cam, 2)
        assert_bits(d.read_accum(), acc, "frames across update_geometry vs the oracle")
        assert np.array_equal(d.get_seeds(), seeds)
        got = d.counters()
        f = _device(saR, **DEFAULT)
        try:
            f.set_seeds(seeds2)
            f.render(cam, 2)
            ref = f.counters()
            _same_arrays(_arrays(d), _arrays(f), "the arrays after update_geometry / a fresh upload of the host update")
        finally:
            f.close()
        for k in ("extend_rays", "extend_node_visits", "extend_prim_tests", "connect_rays", "connect_node_visits", "connect_prim_tests"):
            assert got[k] == ref[k], (k, got[k], ref[k])
    finally:
        d.close()
    g = Group(Wd, Hd, lanes=2)
    try:
        g.upload(sa0)
        g.update_geometry(0, **src)
        g.seed(0)
        g.reset()
        g.render(cam, 2)
        exp = None
        for m in range(2):
            r = Oracle(saR, Wd, Hd, **DEFAULT).render(cam, 1, seeds=seed_stream(m * Wd * Hd, Wd * Hd))[0]
            exp = r if exp is None else exp + r
        assert_bits(g.read_accum(), exp, "a 2-lane group after update_geometry")
    finally:
        g.close()


# ---- 8. refusals found on the device, and by the pointer rule -------------------------------------------------------------------------
def test_refusals_name_the_argument_and_change_nothing():
    sa0, sa1 = _scene(), _scene(which="moved")
    cam = scenes.camera_for(GC.build()[2], Wd, Hd)
    first, count = 7, 65
    pos, idx = GC.indexed(GC.verts(sa1.prims[first:first + count]))
    nv = len(pos)
    d = _device(sa0, **DEFAULT)
    L = W.device_lib()
    try:
        before, ref = _arrays(d), _frame(d, cam)
        tpos = _gpu(pos)
        for tri in (0, count - 1):
            for where in (_gpu, np.asarray):
                bad = idx.astype(np.int32)
                bad[3 * tri + 2] = nv                                             # equal to nVertices: the first index that is no vertex
                _refused(d, cam, before, ref, f"index {nv} at triangle {tri}",
                         f"rt_update_geometry: indices: triangle {tri} of the window: index {nv} \\(corner 2\\) is no vertex, nVertices is {nv}",
                         lambda: d.update_geometry(first, positions=tpos, indices=where(bad)))
        both = idx.astype(np.int32)
        both[3 * (count - 1)] = both[3 * 5 + 1] = -1                              # (0xffffffff; the lowest triangle is reported)
        _refused(d, cam, before, ref, "two indices out of range", "triangle 5 of the window: index 4294967295 \\(corner 1\\)",
                 lambda: d.rebuild_geometry(first, positions=tpos, indices=_gpu(both), builder="lbvh"))

        def raw(g):
            rc = L.rt_update_geometry(d._h, W.ptr(g), None, 0, None)
            if rc != 0:
                err = RtError(L.rt_last_error().decode())
                err.code = rc
                raise err
        tidx = _gpu(idx.astype(np.int32))
        # 20 MiB: a block of its own in torch's allocator, so the allocation the runtime knows ends where the tensor ends
        V = (20 << 20) // 16
        big = torch.full((V, 4), float("nan"), dtype=torch.float32, device="cuda")
        big[:nv, :3] = tpos
        torch.cuda.synchronize()
        fits = GC.geometry(first, count, positions=big.data_ptr(), stride=16, n_vertices=V, indices=tidx.data_ptr())
        short = fits.copy()
        short["nVertices"] = V + 1
        _refused(d, cam, before, ref, "positions one vertex short", f"rt_update_geometry: positions needs {16 * V + 12} bytes .* its allocation ends 12 bytes earlier",
                 lambda: raw(short))
        odd = fits.copy()
        odd["positions"] += 2
        _refused(d, cam, before, ref, "misaligned positions", "rt_update_geometry: positions .* is not aligned to 4 bytes", lambda: raw(odd))
        odd = fits.copy()
        odd["indices"] += 1
        _refused(d, cam, before, ref, "misaligned indices", "rt_update_geometry: indices .* is not aligned to 4 bytes", lambda: raw(odd))
        raw(fits)                                                                 # ... and what fits is taken
        b = _device(sa0)
        try:
            b.update_scene(sa1.prims[first:first + count], first)
            _same_arrays(_arrays(d), _arrays(b), "after the refusals the same call with good data")
        finally:
            b.close()
    finally:
        d.close()


# ---- 9. a stable caller stops allocating ----------------------------------------------------------------------------------------------
def test_a_stable_caller_stops_allocating():
    sa0, sa1 = _scene(1.0), _scene(1.0, "moved")
    first, count = INSIDE
    v = GC.verts(sa1.prims[first:first + count])
    pos, idx = GC.indexed(v)
    sources = [dict(positions=_gpu(pos), indices=_gpu(idx.astype(np.int32))), dict(positions=pos, indices=idx), dict(positions=v),
               dict(prims=_gpu_records(sa1.prims[first:first + count]))]
    for src in sources:
        d = _device(sa0)
        try:
            n = []
            for _ in range(3):
                d.update_geometry(first, **src)
                n.append(d.rebuild_allocations())
            assert n[0] > 0 and n[2] == n[1], n
            n = []
            for _ in range(3):
                d.rebuild_geometry_ranges(["keep", "refit"], first, **src)
                n.append(d.rebuild_allocations())
            assert n[2] == n[1], n
        finally:
            d.close()

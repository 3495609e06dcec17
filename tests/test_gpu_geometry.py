"""Replacement geometry that lies on the MI355X (rt_update_geometry, rt_rebuild_geometry, rt_rebuild_geometry_ranges and their group
forms): each call leaves the scene copy as its counterpart - update_scene, rebuild_scene, rebuild_ranges - leaves it for host records
over the same window, bit for bit in every array; the vertex form's records are Scene::AddTriangle's for the same vertices; refusals
found on the device change nothing; a stable caller stops allocating.  From section 10 on the vertex kernel runs on geometry_check's
hard classes: its records are AddTriangle's and the host mirror's up to the sign of a NaN, and everything derived from them is what
update_scene derives from those very records."""
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


# ---- 10. the vertex kernel at the floats' edges (geometry_check's hard classes) --------------------------------------------------------
# One BLAS, one instance: k_tlas_build has nothing to cluster and the refit takes any values, so update_geometry commits NaN and
# infinite vertices too and the records can be read back.
_H = {}
UNTOUCHED = np.array([w for w in range(32) if w >= 20 and w != 30])               # uv0, uv1, uv2, the pad words, objType, matIdx


def _hard():
    """geometry_check.hard_scene, made once: (Scene arrays, flips, the bound records)."""
    if not _H:
        _, sa, flips = GC.hard_scene()
        assert len(sa.blas) == 1 and len(sa.prims) == GC.N_HARD and np.array_equal(GC.is_flipped(sa.prims), flips)
        assert flips.reshape(-1, 64).any(axis=1).all() and not flips.reshape(-1, 64).all(axis=1).any()      # both kinds in every wavefront
        _H.update(sa=sa, flips=flips)
    return _H["sa"], _H["flips"]


def _host(v, flips, first=0, bound=None):
    """(AddTriangle's records of the vertices v with those flips, the host mirror's: the bound benign records moved by SetVertices)."""
    want = GC.records(GC.added(v, flips))
    m = GC.added(GC.benign(GC.N_HARD), GC.flip_pattern(GC.N_HARD))
    if bound is not None:
        m.SetPrimitives(0, bound)
    m.SetVertices(first, v)
    return want, GC.records(m)


def _records(d):
    return d.scene_array("prims").view(W.Primitive)


def _check_records(got, want, mirror, bound, what):
    GC.same_records_nan(got, want, f"{what}: the GPU against AddTriangle")
    GC.same_records_nan(got, mirror, f"{what}: the GPU against the host mirror")
    a, b = got.view(np.uint32).reshape(-1, 32)[:, UNTOUCHED], bound.view(np.uint32).reshape(-1, 32)[:, UNTOUCHED]
    assert np.array_equal(a, b), f"{what}: a word beside the rows and the area changed"


def _fed_back(d, fb, sa, what):
    """Every scene array of d against a second device that took d's own read-back records through update_scene."""
    fb.update_scene(sa.prims, 0)
    fb.update_scene(_records(d), 0)
    _same_arrays(_arrays(d), _arrays(fb), f"{what}: the arrays against update_scene of the read-back records")


@pytest.mark.parametrize("name", list(GC.CLASSES))
def test_hard_vertices_give_add_triangles_records(name):
    sa, flips = _hard()
    v = GC.tiled(GC.hard(name))
    want, mirror = _host(v, flips)
    GC.same_records_nan(mirror, want, "the host mirror against AddTriangle")
    print(name, GC.census(want))
    pos, idx = GC.indexed(v)
    d, fb = _device(sa), _device(sa)
    try:
        for what, src in (("torch, packed", dict(positions=_gpu(v.reshape(-1, 3)))), ("numpy, packed", dict(positions=v)),
                          ("torch, indexed", dict(positions=_gpu(pos), indices=_gpu(idx.astype(np.int32))))):
            what = f"{name}, {what}"
            d.update_scene(sa.prims, 0)                                           # the bound records again
            GC.same_records(_records(d), sa.prims, "bound")
            st = d.update_geometry(0, **src)
            assert st["prims"] == GC.N_HARD, (what, st)
            _check_records(_records(d), want, mirror, sa.prims, what)
            _fed_back(d, fb, sa, what)
    finally:
        d.close()
        fb.close()


def test_well_conditioned_vertices_on_the_gpu_against_float64():
    sa, flips = _hard()
    v = GC.well_conditioned()[:GC.N_HARD]
    assert GC.min_angle(v).min() >= GC.MIN_ANGLE
    want, mirror = _host(v, flips)
    d = _device(sa)
    try:
        d.update_geometry(0, positions=_gpu(v.reshape(-1, 3)))
        got = _records(d).copy()
    finally:
        d.close()
    err = GC.errors64(got)
    print("the GPU's records against float64:", err, "bounds:", GC.BOUNDS)
    for k, bound in GC.BOUNDS.items():
        assert err[k] <= bound, (k, err[k], bound)
    GC.same_records(got, want, "well-conditioned triangles: no NaN, so byte for byte")
    GC.same_records(got, mirror, "... and the mirror")


@pytest.mark.parametrize("through", ["points", "non_finite"])
def test_a_flip_is_lost_through_a_degenerate_state_on_the_gpu_too(through):
    """Flipped bound -> `through` -> back: after each step the device equals the host mirror and AddTriangle with the documented flip
    (false once the bound N is NaN or zero)."""
    sa, flips = _hard()
    first, mid = GC.verts(sa.prims), GC.tiled(GC.hard(through))
    m = GC.added(GC.benign(GC.N_HARD), flips)
    d, fb = _device(sa), _device(sa)
    try:
        for i, (v, fl) in enumerate([(first, flips), (mid, flips), (first, np.zeros(GC.N_HARD, bool))]):
            what = f"through {through}, step {i}"
            m.SetVertices(0, v)
            d.update_geometry(0, positions=_gpu(v.reshape(-1, 3)))
            _check_records(_records(d), GC.records(GC.added(v, fl)), GC.records(m), sa.prims, what)
            _fed_back(d, fb, sa, what)
        assert flips.sum() == GC.N_HARD // 4 and not GC.is_flipped(_records(d)).any()
    finally:
        d.close()
        fb.close()


@pytest.mark.parametrize("first,count", [(255, 2), (0, 256), (0, 257), (4095, 1)])
def test_a_window_of_needles_leaves_the_records_outside(first, count):
    sa, flips = _hard()
    v = GC.tiled(GC.hard("needles"))[first:first + count]
    want = GC.records(GC.added(v, flips[first:first + count]))
    _, mirror = _host(v, None, first)
    d = _device(sa)
    try:
        st = d.update_geometry(first, positions=_gpu(v.reshape(-1, 3)))
        assert st["prims"] == count
        got = _records(d)
        _check_records(got[first:first + count], want, mirror[first:first + count], sa.prims[first:first + count], f"needles [{first}, +{count})")
        GC.same_records(got[:first], sa.prims[:first], "the records before the window")
        GC.same_records(got[first + count:], sa.prims[first + count:], "the records behind the window")
    finally:
        d.close()


def test_a_group_moves_hard_vertices_as_a_device_does():
    sa, flips = _hard()
    v = GC.tiled(np.concatenate([GC.hard(k) for k in ("non_finite", "signed_zero", "points", "collinear_rounded", "needles")]))
    want, mirror = _host(v, flips)
    g = Group(Wd, Hd, lanes=2)
    d = _device(sa)
    try:
        g.upload(sa)
        g.update_geometry(0, positions=_gpu(v.reshape(-1, 3)))
        d.update_geometry(0, positions=_gpu(v.reshape(-1, 3)))
        for lane in g.devs:
            _check_records(_records(lane), want, mirror, sa.prims, "a 2-lane group")
            _same_arrays(_arrays(lane), _arrays(d), "a lane of the group against a device")
    finally:
        d.close()
        g.close()


# ---- 11. refusals after the vertex kernel has run ---------------------------------------------------------------------------------------
def _bad_blas1(kind):
    """(first, vertices of BLAS 1 of geometry_check.build with one vertex made bad, the host mirror's records of that window)."""
    sa0 = _scene(1.0)
    first, count = GC.NB0, N - GC.NB0
    v = GC.verts(sa0.prims[first:])
    if kind == "huge":
        v = (v * np.float32(1e20)).astype(np.float32)
    else:
        v[57, 2] = dict(nan=np.nan, inf=np.inf)[kind]                             # the last corner: the box rule folds it in last
    s = GC.build(alpha=1.0)[0].s
    s.SetVertices(first, v)
    return first, v, GC.records(s)[first:first + count]                           # (no TLAS: the host would refuse to build it)


# (the LBVH builder refuses no NaN vertex - its unions ignore a NaN operand, lbvh_common.h - so that case is held to its counterpart's
# arrays below, not to a message)
REFUSALS = {
    "rebuild sah, a NaN vertex": ("nan", "rt_rebuild_scene", "rt_rebuild_geometry",
                                  lambda d, first, recs: d.rebuild_scene(recs, first, builder="sah"),
                                  lambda d, first, src: d.rebuild_geometry(first, builder="sah", **src)),
    "ranges keep / lbvh, an inf vertex": ("inf", "rt_rebuild_ranges", "rt_rebuild_geometry_ranges",
                                          lambda d, first, recs: d.rebuild_ranges(["keep", "lbvh"], recs, first),
                                          lambda d, first, src: d.rebuild_geometry_ranges(["keep", "lbvh"], first, **src)),
    "update, BLAS 1 times 1e20": ("huge", "rt_update_scene", "rt_update_geometry",
                                  lambda d, first, recs: d.update_scene(recs, first),
                                  lambda d, first, src: d.update_geometry(first, **src)),
}


@pytest.mark.parametrize("case", list(REFUSALS))
def test_bad_vertices_are_refused_as_the_host_records_are(case):
    kind, old_name, new_name, old, new = REFUSALS[case]
    sa0, sa1 = _scene(1.0), _scene(1.0, "moved")
    cam = scenes.camera_for(GC.build()[2], Wd, Hd)
    first, v, recs = _bad_blas1(kind)
    d = _device(sa0, **DEFAULT)
    try:
        before, ref = _arrays(d), _frame(d, cam)
        with pytest.raises(RtError) as host:
            old(d, first, recs)
        print(case, "->", host.value)
        assert old_name in str(host.value)
        _same_arrays(_arrays(d), before, f"after the host-records refusal: {case}")
        for where, src in (("torch", dict(positions=_gpu(v.reshape(-1, 3)))), ("numpy", dict(positions=v))):
            with pytest.raises(RtError) as e:
                new(d, first, src)
            assert str(e.value) == str(host.value).replace(old_name, new_name), (case, where)
            assert e.value.code in (W.RT_E_INVALID, W.RT_E_UNSUPPORTED) and getattr(host.value, "code", None) in (None, e.value.code), (case, where)
            _same_arrays(_arrays(d), before, f"after the refusal: {case}, {where}")
            assert_bits(_frame(d, cam), ref, f"the frame after the refusal: {case}, {where}")
        good = GC.verts(sa1.prims[first:])
        new(d, first, dict(positions=_gpu(good.reshape(-1, 3))))                  # ... and a good call is taken
        b = _device(sa0, **DEFAULT)
        try:
            old(b, first, sa1.prims[first:])
            _same_arrays(_arrays(d), _arrays(b), f"after the refusals a good call: {case}")
        finally:
            b.close()
    finally:
        d.close()


def test_a_nan_vertex_goes_through_the_lbvh_rebuild_as_host_records_do():
    """rebuild_scene(builder="lbvh") takes host records with a NaN vertex (the box rule and the unions drop the NaN), so
    rebuild_geometry(builder="lbvh") takes the vertices: its records are the mirror's, and every array is what rebuild_scene makes of
    the GPU's own read-back records."""
    sa0 = _scene(1.0)
    first, v, recs = _bad_blas1("nan")
    count = len(v)
    a, b, c = _device(sa0), _device(sa0), _device(sa0)
    try:
        sb = b.rebuild_scene(recs, first, builder="lbvh")                         # not refused: the premise
        sa_ = a.rebuild_geometry(first, builder="lbvh", positions=_gpu(v.reshape(-1, 3)))
        got = _records(a)
        GC.same_records_nan(got[first:first + count], recs, "rebuild_geometry(lbvh) with a NaN vertex against the host mirror")
        GC.same_records(got[:first], sa0.prims[:first], "the records before the window")
        assert np.isnan(got["v2"][first + 57, :3]).all() and np.isnan(got["N"][first + 57, :3]).all()
        sc = c.rebuild_scene(got[first:first + count], first, builder="lbvh")
        for k in ("prims", "blas_built", "nodes", "n_idx", "max_depth", "tlas_nodes", "tlas_depth", "reconfigured"):
            assert sa_[k] == sc[k] == sb[k], (k, sa_[k], sc[k], sb[k])
        _same_arrays(_arrays(a, NAMES), _arrays(c, NAMES), "rebuild_geometry(lbvh) / rebuild_scene(lbvh) of the read-back records")
        skip = ("prims", "shadeRecs")                                             # (they carry N: the host's NaN has another sign)
        _same_arrays(_arrays(a, [k for k in NAMES if k not in skip]), _arrays(b, [k for k in NAMES if k not in skip]), "... and of the host mirror's records")
    finally:
        a.close()
        b.close()
        c.close()


# ---- 12. frames with degenerate triangles -----------------------------------------------------------------------------------------------
def test_frames_with_points_collinears_and_needles_match_the_oracle():
    """40 soup triangles of BLAS 0 (no light among them) become points, exact collinears and needles on the GPU: two frames equal the
    oracle's on the host-updated scene, seeds and traversal counters those of a fresh context on it."""
    gt0, sa0, view = GC.build()
    cam = scenes.camera_for(view, Wd, Hd)
    first, count = 90, 40
    assert not set(range(first, first + count)) & set(GC.LIGHTS) and first + count <= 220
    c = GC.verts(sa0.prims[first:first + count]).mean(axis=1, keepdims=True)      # where the triangles were
    shape = np.concatenate([GC.hard("points")[:14], GC.hard("collinear_exact")[:13], GC.hard("needles")[:13]])
    v = (np.round(c * 8) / 8 + (shape - shape[:, :1]) / 8).astype(np.float32)     # points and collinears stay exact: small integers over 64
    ab = v[27:, :2].astype(np.float64)                                            # ... and the needles' third vertex is made anew
    v[27:, 2] = (ab[:, 0] + (ab[:, 1] - ab[:, 0]) * np.random.default_rng(31).uniform(0, 1, (13, 1))).astype(np.float32)
    s = GC.build()[0].s
    s.SetVertices(first, v)
    p = GC.records(s)[first:first + count]
    assert np.isnan(p["N"][:27, :3]).all() and (p["area"][27:] == 0).sum() >= 6 and np.isfinite(v).all()
    s.Refit()
    saR = s.arrays()
    acc, seeds, e, c_ = Oracle(saR, Wd, Hd, **DEFAULT).render(cam, 2)
    print("inst_visits / rays", assert_seen(e, c_, "the oracle's frames on the degenerate triangles"))
    d = _device(sa0, **DEFAULT)
    try:
        d.update_geometry(first, positions=_gpu(v.reshape(-1, 3)))
        GC.same_records_nan(_records(d), saR.prims, "the records after update_geometry")
        d.seed_default()
        d.reset()
        d.reset_counters()
        d.render(cam, 2)
        assert_bits(d.read_accum(), acc, "frames with degenerate triangles vs the oracle")
        assert np.array_equal(d.get_seeds(), seeds)
        got = d.counters()
        f = _device(saR, **DEFAULT)
        try:
            f.seed_default()
            f.render(cam, 2)
            ref = f.counters()
        finally:
            f.close()
        for k in ("extend_rays", "extend_node_visits", "extend_prim_tests", "connect_rays", "connect_node_visits", "connect_prim_tests"):
            assert got[k] == ref[k], (k, got[k], ref[k])
    finally:
        d.close()

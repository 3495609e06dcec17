"""In-place scene updates on the MI355X (rt_update_scene / rt_group_update_scene): after an update the device arrays are bit for bit
those of a fresh upload of the host-refit scene, frames are bit-exact with the oracle on every BVH2 traversal path, sharing contexts
and group lanes see the update and reconfigure, and every refusal leaves the bound scene rendering as before."""
import numpy as np
import pytest

import refit_check as R
import test_gpu_groundtruth as GT
import test_groundtruth_cpu as C
from helpers import DEFAULT, assert_bits
from tlas_check import assert_seen
from magr_ray_tracer_amd import _lib as W, scenes
from magr_ray_tracer_amd.renderer import Device, Group, RtError, _update_args
from magr_ray_tracer_amd.scenes import Scene, _std_materials, box_tris
from oracle.oracle_py import Oracle, seed_stream

pytestmark = pytest.mark.gpu

Wd, Hd = 160, 120
ARRAYS = list(W.SCENE_ARRAYS)


def _arrays(d):
    return {k: d.scene_array(k) for k in ARRAYS}


def _fresh(sa, **kw):
    d = Device(Wd, Hd, **kw)
    d.upload(sa)
    a = _arrays(d)
    d.close()
    return a


def _same_arrays(got, want, what):
    for k in ARRAYS:
        assert len(got[k]) == len(want[k]) and np.array_equal(got[k], want[k]), f"{what}: {k} differs ({len(got[k])} / {len(want[k])} bytes)"


def _jittered(sa, seed=5, scale=1e-3):
    """The same records with their triangle vertices and sphere centres moved (objType / matIdx kept)."""
    rng = np.random.default_rng(seed)
    p = sa.prims.copy()
    for f in ("v0", "v1", "v2"):
        p[f][:, :3] += rng.normal(scale=scale, size=(len(p), 3)).astype(np.float32)
    return p


def _host_refit(s, prims, inst=None):
    s.SetPrimitives(0, prims)
    if inst is not None:
        for b, r in enumerate(inst):
            s.SetInstanceTransform(b, r["invT"].reshape(4, 4))
    s.Refit()
    return s.arrays(bvh4=False)


def _big(name):
    if name == "sponza_class":
        return scenes.sponza_class(1.0)[0]
    if name == "config5":
        return scenes.config5_scene(0.0)[0]
    if name == "lbvh":
        return scenes.sponza_class(0.5, builder="lbvh", device=None)[0]
    if name == "spheres-lights":
        return R.build(alpha=0.0, blas=2, spheres=4)[0].s
    return R.build(blas=4, spheres=2, transforms=[None, C.invT(C.rot(1, 23.0), (0.3, -0.2, 0.4)), None, None])[0].s


@pytest.mark.parametrize("name", ["sponza_class", "config5", "lbvh", "spheres-lights", "instances"])
def test_update_gives_the_arrays_of_a_fresh_upload(name):
    """All eleven device arrays after rt_update_scene equal those of rt_upload_scene of the scene refit on the host; ten repeated
    updates give the same arrays."""
    s = _big(name)
    sa = s.arrays(bvh4=False)
    prims = _jittered(sa)
    inst = None
    if len(sa.blas) > 1:
        inst = sa.blas.copy()
        inst["invT"][1] = C.invT(C.rot(0, 17.0) @ np.diag([1.2, 0.9, 1.0]), (0.1, 0.2, -0.3)).ravel()
    d = Device(Wd, Hd)
    try:
        d.upload(sa)
        st = d.update_scene(prims, 0, inst)
        assert st["prims"] == len(prims) and st["nodes"] > 0 and st["gpu_ms"] > 0
        got = _arrays(d)
        want = _fresh(_host_refit(s, prims, inst))
        _same_arrays(got, want, name)
        for k in range(10):
            d.update_scene(prims, 0, inst)
            _same_arrays(_arrays(d), got, f"{name}: update {k + 2}")
    finally:
        d.close()


# ---- frames --------------------------------------------------------------------------------------------------------------------------
_SC = {}


def _scenes(kind):
    """(original arrays, its Scene, deformed records, deformed instances, arrays of the host update, view)."""
    if kind not in _SC:
        if kind == "one":
            gt0, sa0, view = R.build(alpha=0.0, blas=1, spheres=3, tris=600)
            gt1, sa1, _ = R.build(R.jitter(0.05), alpha=0.0, blas=1, spheres=3, tris=600)
        else:
            T = [None, None, C.TRANSFORMS["scale"], C.TRANSFORMS["mirror"]]
            gt0, sa0, view = R.build(alpha=0.0, blas=4, spheres=3, transforms=T)
            T1 = [None, C.TRANSFORMS["rigid"], C.TRANSFORMS["mirror"], C.TRANSFORMS["scale"]]
            gt1, sa1, _ = R.build(R.rigid_blas(0), alpha=0.0, blas=4, spheres=3, transforms=T1)
        saR = R.host_update(R.build(alpha=0.0, blas=len(sa0.blas), spheres=3, tris=600 if kind == "one" else 220,
                                    transforms=None if kind == "one" else [None, None, C.TRANSFORMS["scale"], C.TRANSFORMS["mirror"]])[0],
                            gt1, sa1)
        _SC[kind] = (sa0, sa1.prims, sa1.blas if kind != "one" else None, saR, view)
    return _SC[kind]


BVH2_PATHS = [k for k, v in GT.CASES.items() if v[1] == W.ACCEL_BVH2]


@pytest.mark.parametrize("case", BVH2_PATHS)
def test_frames_across_an_update_match_the_oracle(case, monkeypatch):
    """Two frames, an update, two more: the accumulator and seeds equal the oracle rendering the same sequence (two frames of the
    original arrays, then two of the host-updated ones), path confirmed by kernel_info before and after the update."""
    kind, accel, variant, env, want = GT.CASES[case]
    monkeypatch.setenv("RT355_TUNE", GT.TUNE)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    sa0, prims, inst, saR, view = _scenes(kind)
    cam = scenes.camera_for(view, Wd, Hd)
    v = dict(DEFAULT, accel=accel)
    acc, seeds, _, _ = Oracle(sa0, Wd, Hd, **v).render(cam, 2)
    acc, seeds, _, _ = Oracle(saR, Wd, Hd, **v).render(cam, 2, accum=acc, seeds=seeds)
    d = Device(Wd, Hd, extend_variant=variant, **v)
    try:
        d.upload(sa0)
        d.seed_default()
        d.render(cam, 2)
        d.update_scene(prims, 0, inst)
        info = d.kernel_info()
        for k, wv in want.items():
            assert info[k] == wv, (case, info)
        d.render(cam, 2)
        assert_bits(d.read_accum(), acc, f"{case}: frames across an update vs oracle")
        assert np.array_equal(d.get_seeds(), seeds)
    finally:
        d.close()


# ---- sharing and reconfiguration ---------------------------------------------------------------------------------------------------
def _chain_scene(n):
    """n small BLAS (a box and a few triangles each) under a TLAS, laid out on a grid: a shallow TLAS."""
    s = Scene()
    _std_materials(s)
    rng = np.random.default_rng(9)
    for b in range(n):
        s.AddTriangles(np.asarray(box_tris((-0.4, -0.4, -0.4), (0.4, 0.4, 0.4)), np.float32), ["sand", "green", "red", "white"][b % 4])
        s.AddTriangles(C._soup(rng, 6, -0.4, 0.4, 0.2), "grey")
        if b == 0:   # an emissive quad above the grid and a floor under it (in the coordinates of BLAS 0, which sits at (-2, -1.5, 0))
            s.AddQuad((1.5, 5.5, -1), (3.5, 5.5, -1), (3.5, 5.5, 1), (1.5, 5.5, 1), "white-light")
            s.AddQuad((-1, -1.0, -2), (-1, -1.0, 2), (6, -1.0, 2), (6, -1.0, -2), "grey")
        s.BuildBLAS(s.num_prims - (22 if b == 0 else 18))
    grid = [C.invT(np.eye(3), (-(b % 4) * 1.5 + 2.0, -(b // 4) * 1.5 + 1.5, 0.0)) for b in range(n)]
    for b in range(n):
        s.SetInstanceTransform(b, grid[b])
    s.Refit()   # (the device refits on every update: equal values, and with this the same bits on +-0 too)
    sa = s.arrays(bvh4=False)
    view = dict(origin=(0.0, 0.0, 12.0), forward=(0.0, 0.0, 1.0), fov=60.0, aperture=0.01)   # (the camera looks along -forward)
    return s, sa, view


def _chain(sa, n):
    """Instances moved to x = 4 * 3^k: TLAS::Build's clustering makes a chain, n - 1 levels deep."""
    inst = sa.blas.copy()
    for b in range(len(inst)):
        inst["invT"][b] = C.invT(np.eye(3), (-4.0 * 3.0 ** b if b < n else -3.0, 0.0, 0.0)).ravel()
    return inst


def _tlas_depth(t):
    d, st = 0, [(0, 0)]
    while st:
        i, k = st.pop()
        d = max(d, k)
        lr = int(t["leftRight"][i])
        if lr:
            st += [(lr & 0xffff, k + 1), (lr >> 16, k + 1)]
    return d


def _oracle_frames(sa, cam, frames, acc=None, seeds=None):
    """The oracle's frames, which must show the scene (tlas_check.assert_seen): a camera that faces away renders the sky bit-exactly."""
    r = Oracle(sa, Wd, Hd, **DEFAULT).render(cam, frames, accum=acc, seeds=seeds)
    print("inst_visits / rays", assert_seen(r[2], r[3], "the oracle's frame"))
    return r


def test_shared_contexts_and_group_lanes_see_the_update_and_reconfigure(monkeypatch):
    """A 4-lane group and an rt_share_scene pair hold one scene each.  Updating the instances into a chain 11 levels deep switches
    every holder from k_trace_persist_tlas (persist 2 / 3) to the nested loops (persist 0) and back; frames stay bit-exact."""
    s, sa, view = _chain_scene(12)
    cam = scenes.camera_for(view, Wd, Hd)
    deep = _chain(sa, 12)
    s2 = _chain_scene(12)[0]
    for b in range(12):
        s2.SetInstanceTransform(b, deep["invT"][b].reshape(4, 4))
    s2.Refit()
    sa_deep = s2.arrays(bvh4=False)
    assert _tlas_depth(sa.tlas) <= 8 < _tlas_depth(sa_deep.tlas) <= 32
    a, b = Device(Wd, Hd, **DEFAULT), Device(Wd, Hd, **DEFAULT)
    g = Group(Wd, Hd, lanes=4)
    try:
        a.upload(sa)
        b.share_scene(a)
        g.upload(sa)
        g.seed(0)
        holders = [a, b] + g.devs
        assert all(h.kernel_info()["persist"] in (2, 3) for h in holders)
        for upd, sa_now, want in ((a, sa_deep, lambda p: p == 0), (a, sa, lambda p: p in (2, 3))):
            st = upd.update_scene(None, 0, sa_now.blas)
            st2 = g.update_scene(None, 0, sa_now.blas)
            assert st["reconfigured"] and st2["reconfigured"] and st["tlas_depth"] == _tlas_depth(sa_now.tlas)
            assert all(want(h.kernel_info()["persist"]) for h in holders), [h.kernel_info() for h in holders]
            ref, seeds, _, _ = _oracle_frames(sa_now, cam, 1)
            for dv in (a, b):
                dv.seed_default()
                dv.reset()
                dv.render(cam, 1)
                assert_bits(dv.read_accum(), ref, "shared pair after an update")
            _same_arrays(_arrays(a), _fresh(sa_now), "shared pair: arrays")
            g.seed(0)
            g.reset()
            g.render(cam, 4)
            acc = g.read_accum()
            exp = None
            for m in range(4):
                r = _oracle_frames(sa_now, cam, 1, seeds=seed_stream(m * Wd * Hd, Wd * Hd))[0]
                exp = r if exp is None else exp + r
            assert_bits(acc, exp, "4-lane group after an update")
    finally:
        g.close()
        b.close()
        a.close()


# ---- refusals -----------------------------------------------------------------------------------------------------------------------
def test_refusals_return_their_code_and_change_nothing():
    s, sa, view = _chain_scene(40)
    cam = scenes.camera_for(view, Wd, Hd)
    d = Device(Wd, Hd, **DEFAULT)
    try:
        d.upload(sa)
        before = _arrays(d)
        d.seed_default()
        d.render(cam, 1)
        ref = d.read_accum()
        assert_bits(ref, _oracle_frames(sa, cam, 1)[0], "the frame before the refusals")
        L = W.device_lib()
        bad_type = sa.prims[:4].copy()
        bad_type["objType"][1] = W.PRIM_SPHERE
        bad_mat = sa.prims[:4].copy()
        bad_mat["matIdx"][0] += 1
        bad_idx = sa.blas.copy()
        bad_idx["bvhIdx"][2] = sa.blas["bvhIdx"][3]
        sing = sa.blas.copy()
        sing["invT"][5] = np.diag([1.0, 1.0, 0.0, 1.0]).astype(np.float32).ravel()
        cases = [("objType", (bad_type, 0, None), W.RT_E_INVALID), ("matIdx", (bad_mat, 0, None), W.RT_E_INVALID),
                 ("bvhIdx", (None, 0, bad_idx), W.RT_E_INVALID), ("range", (sa.prims[:4], len(sa.prims) - 2, None), W.RT_E_INVALID),
                 ("singular", (None, 0, sing), W.RT_E_INVALID), ("too deep", (None, 0, _chain(sa, 40)), W.RT_E_UNSUPPORTED)]
        for what, (p, first, inst), code in cases:
            args, keep, st = _update_args(p, first, inst)
            rc = L.rt_update_scene(d._h, *args)
            assert rc == code, (what, rc, L.rt_last_error())
            _same_arrays(_arrays(d), before, f"after the refused {what} update")
            d.seed_default()
            d.reset()
            d.render(cam, 1)
            assert_bits(d.read_accum(), ref, f"render after the refused {what} update")
        d4 = Device(Wd, Hd, **dict(DEFAULT, accel=W.ACCEL_BVH4))
        try:
            d4.upload(s.arrays())
            with pytest.raises(RtError, match="BVH4"):
                d4.update_scene(sa.prims[:2], 0)
        finally:
            d4.close()
    finally:
        d.close()

"""In-place material updates on the MI355X (rt_update_materials / rt_group_update_materials): after an update every device array - the
table and the atlas with its pad included - kernel_info and rt_shade_tables are those of a fresh upload of the numpy truth
(materials_check.truth: matIdx patched, table and atlas replaced, the light list by the Scene rule, trees untouched); the scan's edges,
zero lights, both crossings of k_shade's staged-table capacity, the atlas's growth, shrinkage and pad, torch tensors, frames against the
oracle, queries, chains with rebuilds, updates and resizes, holders, allocations, and every refusal leaving the scene as it was."""
import dataclasses

import numpy as np
import pytest
import torch

import materials_check as M
import rebuild_check as RB
import resize_check as Z
import test_groundtruth_cpu as C
from helpers import DEFAULT, assert_bits, oracle_for
from magr_ray_tracer_amd import _lib as W, scenes
from magr_ray_tracer_amd.renderer import Device, Group, RtError
from oracle.oracle_py import seed_stream

pytestmark = pytest.mark.gpu

Wd, Hd = Z.Wd, Z.Hd
DEV = torch.device("cuda", 0)
T4 = [None, RB.ROT, C.TRANSFORMS["scale"], C.TRANSFORMS["mirror"]]
SCENES = {"one": dict(tris=(220,)), "four": dict(tris=(50, 50, 50, 50), spheres=(1, 1), transforms=T4)}
# how a context is bound: (Device keywords, from_bvh2, the arrays compared)
CONTEXTS = {"bvh2": (dict(accel=W.ACCEL_BVH2), False, M.ARRAYS), "bvh4-kept": (dict(accel=W.ACCEL_BVH4), True, M.ARRAYS_BVH4),
            "bvh4-classic": (dict(accel=W.ACCEL_BVH4), False, M.ARRAYS_BVH4)}
_BUILT = {}


def scene(name):
    if name not in _BUILT:
        _BUILT[name] = Z.build(**SCENES[name])[1]
    return _BUILT[name]


def _bound(sa, ctx="bvh2", **more):
    kw, from_bvh2, names = CONTEXTS[ctx]
    d = Device(Wd, Hd, **dict(DEFAULT, **kw, **more))
    try:
        d.upload(sa, from_bvh2=from_bvh2)
    except BaseException:
        d.close()
        raise
    return d, dict(names=names, from_bvh2=from_bvh2, **dict(DEFAULT, **kw, **more))


def _texels(n, seed=21):
    return np.random.default_rng(seed).uniform(0.05, 1.0, (n, 4)).astype(np.float32)


def case(name, sa):
    """The keywords of one update of a scene of resize_check.build (ten standard materials, no texture bound)."""
    m, n, rng = sa.mats.copy(), len(sa.prims), np.random.default_rng(17)
    if name == "table":                                                   # colours and emittance changed, flags kept
        m["color"][M.SAND], m["specular"][M.GREEN], m["emittance"][M.WHITE_LIGHT] = (0.1, 0.8, 0.4, 0.0), 0.3, (3.0, 40.0, 5.0, 0.0)
        return dict(mats=m)
    if name == "flags":                                                   # a flag switched on (the floor) and another off
        m["isLight"][M.GREY], m["emittance"][M.GREY], m["isLight"][M.WHITE_LIGHT] = 1, (7.0, 7.0, 9.0, 0.0), 0
        return dict(mats=m)
    if name == "primMat":                                                 # (every material, the three lights among them)
        return dict(prim_mat=rng.integers(0, len(m), 37).astype(np.int32), prim_first=n // 3)
    if name == "texels":
        return dict(texels=_texels(12), tex_first=5, n_texels=20)
    assert name == "all"
    m = M.textured(M.textured(m, M.SAND, 8, 4, 3), M.RED, 0, 1, 1)
    m["isLight"][M.GREEN_LIGHT], m["emittance"][M.RED_LIGHT] = 0, (1.0, 2.0, 30.0, 0.0)
    return dict(mats=m, texels=_texels(17), tex_first=3, n_texels=20, prim_mat=rng.integers(0, len(m), 61).astype(np.int32), prim_first=n - 61)


CASES = ["table", "flags", "primMat", "texels", "all"]


# ---- 1. array identity ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(SCENES))
@pytest.mark.parametrize("ctx", list(CONTEXTS))
def test_an_update_gives_the_arrays_of_a_fresh_upload(ctx, name):
    sa = scene(name)
    d, kw = _bound(sa, ctx)
    try:
        for c in CASES:
            if c != CASES[0]:
                d.upload(sa, from_bvh2=kw["from_bvh2"])
            args = case(c, sa)
            want, st = M.update(d, sa, **args)
            M.check(d, want, f"{ctx} / {name} / {c}", key=(name, c), **kw)
            assert st["mats"] == (len(args["mats"]) if "mats" in args else 0) and st["texels"] == len(args.get("texels", ()))
            assert st["prims"] == len(args.get("prim_mat", ())) and st["lights"] == len(want.lights)
            assert st["atlas_reallocated"] == ("n_texels" in args)      # (the upload's array holds the two texels of an empty atlas's pad)
        before, allocs = Z.arrays(d, kw["names"]), d.rebuild_allocations()
        st = d.update_materials()                                         # all three parts absent: nothing is touched
        assert st["mats"] == st["texels"] == st["prims"] == 0 and st["lights"] == len(want.lights)
        Z.same(Z.arrays(d, kw["names"]), before, "an empty update")
        assert d.rebuild_allocations() == allocs
    finally:
        d.close()


def test_texels_alone_keep_a_callers_odd_light_list():
    sa = scene("one")
    n = len(sa.prims)
    odd = dataclasses.replace(sa, lights=np.array([n - 3, n - 4, 3], np.uint32))   # legal (every index is a primitive), not the Scene rule's
    d, kw = _bound(odd)
    try:
        want, st = M.update(d, odd, texels=_texels(6), tex_first=1, n_texels=9)
        assert list(want.lights) == [n - 3, n - 4, 3] and st["lights"] == 3
        M.check(d, want, "texels only, an odd list", **kw)
        want, _ = M.update(d, want, mats=want.mats)                       # the same table again: now the Scene rule
        assert list(want.lights) == list(sa.lights)
        M.check(d, want, "the table given: the Scene rule", **kw)
    finally:
        d.close()


# ---- 2. scan edges -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [255, 256, 257, 513])
def test_light_scan_at_the_block_edges(n):
    at = sorted({i for i in (0, 255, 256, n - 1) if i < n})
    runs, i = [], 0
    for a in at:                                                          # "red" exactly at those indices, "sand" between them
        if a > i:
            runs.append((a - i, "sand"))
        runs.append((1, "red"))
        i = a + 1
    if i < n:
        runs.append((n - i, "sand"))
    sa, _ = Z.build_runs(runs)
    assert len(sa.prims) == n and len(sa.lights) == 0 and list(np.flatnonzero(sa.prims["matIdx"] == M.RED)) == at
    d, kw = _bound(sa)
    try:
        m = sa.mats.copy()
        m["isLight"][M.RED], m["emittance"][M.RED] = 1, (4.0, 5.0, 6.0, 0.0)
        want, st = M.update(d, sa, mats=m)
        assert list(want.lights) == at and st["lights"] == len(at)
        M.check(d, want, f"{n} primitives, lights at {at}", **kw)
        pm = np.full(n, M.SAND, np.int32)                                 # ... and the same through the assignment: every primitive named
        pm[at] = M.WHITE_LIGHT
        want, _ = M.update(d, sa, mats=sa.mats, prim_mat=pm)
        assert list(want.lights) == at
        M.check(d, want, f"{n} primitives, a whole assignment", **kw)
    finally:
        d.close()


# ---- 3. zero lights ------------------------------------------------------------------------------------------------------------------
def test_all_lights_off_and_on_again():
    sa = scene("one")
    d, kw = _bound(sa)
    try:
        off = sa.mats.copy()
        off["isLight"][:] = 0
        want, st = M.update(d, sa, mats=off)
        assert st["lights"] == 0 and len(want.lights) == 0 and len(d.scene_array("lights")) == 0 and len(d.scene_array("lightRecs")) == 0
        M.check(d, want, "no light", **kw)
        want, st = M.update(d, want, mats=sa.mats)
        assert st["lights"] == len(sa.lights) and np.array_equal(want.lights, sa.lights)
        M.check(d, want, "the lights back on", key=("one", "as built"), **kw)
    finally:
        d.close()


# ---- 4. the staged tables' capacity, both directions ---------------------------------------------------------------------------------
def _frame_matches(d, sa, cam, what):
    d.seed_default()
    d.reset()
    d.render(cam, 1)
    assert_bits(d.read_accum(), oracle_for(sa, Wd, Hd, **DEFAULT).render(cam, 1)[0], what)


def test_the_staged_tables_follow_the_light_and_material_counts():
    """Ten materials: two lights fit k_shade's 42 rows (12 + 30), a third does not (18 + 30); at two lights an eleventh material does not
    either (12 + 33)."""
    sa = scene("one")
    cam = scenes.camera_for(Z.VIEW, Wd, Hd)
    d, kw = _bound(sa)
    try:
        cap, staged = d.shade_tables()
        assert cap == 42 and staged and len(sa.lights) == 2 and len(sa.mats) == 10
        want, st = M.update(d, sa, prim_mat=[M.RED_LIGHT], prim_first=5)  # a third light
        assert st["lights"] == 3 and st["tables_staged_changed"] and d.shade_tables() == (42, False)
        M.check(d, want, "three lights", **kw)
        _frame_matches(d, want, cam, "three lights: tables in global memory")
        want, st = M.update(d, want, prim_mat=[M.SAND], prim_first=5)     # ... and two again
        assert st["lights"] == 2 and st["tables_staged_changed"] and d.shade_tables() == (42, True)
        M.check(d, want, "two lights again", key=("one", "as built"), **kw)
        _frame_matches(d, want, cam, "two lights: tables staged")
        eleven = np.concatenate([sa.mats, sa.mats[M.MIRROR:M.MIRROR + 1]])
        want, st = M.update(d, want, mats=eleven)                         # an eleventh material
        assert st["mats"] == 11 and st["tables_staged_changed"] and d.shade_tables() == (42, False)
        M.check(d, want, "eleven materials", **kw)
        _frame_matches(d, want, cam, "eleven materials: tables in global memory")
        want, st = M.update(d, want, mats=sa.mats)
        assert st["tables_staged_changed"] and d.shade_tables() == (42, True)
        M.check(d, want, "ten materials again", key=("one", "as built"), **kw)
        want, st = M.update(d, want, mats=case("table", sa)["mats"])      # no crossing
        assert not st["tables_staged_changed"] and d.shade_tables() == (42, True)
    finally:
        d.close()


# ---- 5. the atlas --------------------------------------------------------------------------------------------------------------------
def test_the_atlas_grows_shrinks_and_keeps_its_pad_zero():
    sa = scene("one")
    assert len(sa.tex) == 0
    d, kw = _bound(sa)
    try:
        m1 = M.textured(sa.mats, M.SAND, 0, 1, 1)
        want, st = M.update(d, sa, mats=m1, texels=_texels(1), n_texels=1)            # a 1 x 1 texture: pad 3
        assert st["atlas_reallocated"] and st["texels"] == 1
        M.check(d, want, "a 1 x 1 texture", **kw)
        m2 = M.textured(m1, M.GREEN, 8, 4, 3)
        want, st = M.update(d, want, mats=m2, texels=_texels(12, 5), tex_first=8, n_texels=20)   # a 4 x 3 window ending at nTexels: pad 6
        assert st["atlas_reallocated"] and not want.tex[1:8].any() and want.tex[8:].all()
        M.check(d, want, "a 4 x 3 window ending at the atlas end", **kw)
        at20 = want
        want, st = M.update(d, want, texels=_texels(4, 6), tex_first=30, n_texels=40)  # growth: zero but the range
        assert st["atlas_reallocated"] and not want.tex[20:30].any() and not want.tex[34:].any() and want.tex[30:34].all()
        M.check(d, want, "growth", **kw)
        want, st = M.update(d, want, n_texels=20)                                      # shrinkage, in place
        assert not st["atlas_reallocated"] and st["texels"] == 0
        M.check(d, want, "shrinkage", **kw)
        want, st = M.update(d, want, n_texels=36, texels=_texels(2, 7), tex_first=33)  # in-place growth over what the shrinkage left behind
        assert not st["atlas_reallocated"] and not want.tex[20:33].any() and not want.tex[35:].any()
        M.check(d, want, "growth in place", **kw)
        want, _ = M.update(d, want, n_texels=20)
        m3 = M.textured(m1, M.GREEN, 2, 9, 2)                                          # texW 4 -> 9: pad 6 -> 11, in the room the growth left
        want, st = M.update(d, want, mats=m3)
        assert not st["atlas_reallocated"] and M.tex_pad(m2) == 6 and M.tex_pad(m3) == 11
        M.check(d, want, "pad 6 -> 11 in place", **kw)
        d.upload(at20)                                                                 # ... and in an array that fits 20 + 6 exactly
        want, st = M.update(d, at20, mats=m3)
        assert st["atlas_reallocated"]
        M.check(d, want, "pad 6 -> 11 in a new array", **kw)
        want, st = M.update(d, want, mats=m2)                                          # ... and back: the pad shrinks with the texture
        assert not st["atlas_reallocated"]
        M.check(d, want, "pad 11 -> 6", **kw)
    finally:
        d.close()


# ---- 6. torch tensors ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ctx", ["bvh2", "bvh4-kept"])
def test_torch_tensors_give_the_same_bytes(ctx):
    sa = scene("four")
    args = case("all", sa)
    want = M.truth(sa, **args)
    d, kw = _bound(sa, ctx)
    try:
        t = torch.from_numpy(args["texels"]).to(DEV)
        pm = torch.from_numpy(args["prim_mat"]).to(DEV)
        st = d.update_materials(**dict(args, texels=t, prim_mat=pm))
        assert st["texels"] == len(args["texels"]) and st["prims"] == len(args["prim_mat"])
        M.check(d, want, f"{ctx}: device-resident texels and matIdx values", key=("four", "all"), **kw)
        # the host's shadow of matIdx came back from the device: a refit checks its primitives against it
        with pytest.raises(RtError, match="changes its objType / matIdx"):
            d.rebuild_scene(sa.prims, 0, None, builder="refit")
        d.rebuild_scene(want.prims, 0, None, builder="refit")
    finally:
        d.close()


# ---- 7. frames -----------------------------------------------------------------------------------------------------------------------
def _room():
    """A textured soup, a textured sphere, a glass sphere, plain triangles, a light and a floor in one BLAS; the 6 x 5 texture's material
    is the eleventh."""
    if "room" not in _BUILT:
        rng = np.random.default_rng(12)
        s = scenes.Scene()
        scenes._std_materials(s)
        assert s.AddTexture("cloth", rng.uniform(0.1, 1.0, (5, 6, 4)).astype(np.float32)) == 10
        s.AddTriangles(C._soup(rng, 120, -1.6, 1.6, 0.5), "cloth", uvs=rng.uniform(0.0, 1.0, (120, 3, 2)).astype(np.float32))
        s.AddSphere((0.9, -0.2, 0.6), 0.7, "cloth")
        s.AddSphere((-1.0, 0.1, 0.9), 0.6, "white-glass")
        s.AddTriangles(C._soup(rng, 60, -1.6, 1.6, 0.4), "sand")
        s.AddTriangles(np.array([[(-1.5, 4.2, -1), (1.5, 4.2, -1), (1.5, 4.2, 1.5)]], np.float32), "white-light")
        s.AddTriangles(np.array([[(-4, -2.6, -4), (4, -2.6, -4), (4, -2.6, 4)], [(4, -2.6, 4), (-4, -2.6, 4), (-4, -2.6, -4)]], np.float32), "grey")
        s.BuildBLAS(0, **Z.BUILDERS["sah"][1])
        _BUILT["room"] = s.arrays()
    return _BUILT["room"]


def _room_update(sa):
    m = sa.mats.copy()
    m["emittance"][M.WHITE_LIGHT], m["color"][M.GREY] = (30.0, 60.0, 120.0, 0.0), (0.6, 0.3, 0.3, 0.0)
    m = M.textured(m, 10, 34, 4, 7)                                        # the texture moves to a 4 x 7 window of a longer atlas
    pm = np.full(30, M.MIRROR, np.int32)
    pm[::7] = M.GREEN_LIGHT                                                # part of the sand repainted: mirrors and five new lights
    return dict(mats=m, texels=_texels(28, 3), tex_first=34, n_texels=62, prim_mat=pm, prim_first=130)


@pytest.mark.parametrize("ctx", ["bvh2", "bvh4-kept", "bvh4-classic"])
def test_frames_after_an_update_match_the_oracle(ctx):
    """A frame, an update, two more: accumulator, seeds and extend's counters equal the oracle rendering one frame of the bound arrays
    and two of the truth, accumulator and seeds carried."""
    sa = _room()
    args = _room_update(sa)
    cam = scenes.camera_for(Z.VIEW, Wd, Hd)
    d, kw = _bound(sa, ctx)
    v = {k: kw[k] for k in DEFAULT}
    try:
        acc, seeds, _, _ = oracle_for(sa, Wd, Hd, **v).render(cam, 1)
        d.seed_default()
        d.render(cam, 1)
        want, st = M.update(d, sa, **args)
        assert st["lights"] == 6 and len(want.lights) == 6
        acc, seeds, e, _ = oracle_for(want, Wd, Hd, **v).render(cam, 2, accum=acc, seeds=seeds)
        d.reset_counters()
        d.render(cam, 2)
        assert_bits(d.read_accum(), acc, f"{ctx}: frames across an update vs oracle")
        assert np.array_equal(d.get_seeds(), seeds)
        got = d.counters()
        for k in ("rays", "tlas_visits", "inst_visits", "node_visits", "prim_tests"):
            assert got["extend_" + k] == e[k], (ctx, k, got["extend_" + k], e[k])
        M.check(d, want, f"{ctx}: the room after its update", **kw)
    finally:
        d.close()


# ---- 8. queries ----------------------------------------------------------------------------------------------------------------------
def test_closest_hits_are_unchanged_by_an_update():
    sa = scene("four")
    rng = np.random.default_rng(9)
    n = 2000
    O = (np.tile(np.array(Z.VIEW["origin"], np.float32), (n, 1)) + rng.normal(scale=0.3, size=(n, 3))).astype(np.float32)
    D = rng.uniform(-3.5, 3.5, (n, 3)).astype(np.float32) - O
    D /= np.linalg.norm(D, axis=1, keepdims=True).astype(np.float32)
    d, kw = _bound(sa)
    try:
        before = d.trace(O, D, point=True, normal=True)
        assert (before["hit"]["primIdx"] >= 0).sum() > n // 4
        M.update(d, sa, **case("all", sa))
        after = d.trace(O, D, point=True, normal=True)
        for k in before:
            assert before[k].tobytes() == after[k].tobytes(), k
    finally:
        d.close()


# ---- 9. chains -----------------------------------------------------------------------------------------------------------------------
def _jittered(prims, seed, scale=0.04):
    p = prims.copy()
    rng = np.random.default_rng(seed)
    tri = p["objType"] == W.PRIM_TRIANGLE
    for f in ("v0", "v1", "v2"):
        p[f][tri, :3] += rng.normal(scale=scale, size=(int(tri.sum()), 3)).astype(np.float32)
    return p


def _host_update(s, mats=None, texels=None, tex_first=0, n_texels=None, prim_mat=None, prim_first=0):
    """The update on the host's Scene, the atlas first (the table is checked against it)."""
    if texels is not None or n_texels is not None:
        s.SetTexels(texels, tex_first, n_texels)
    if mats is not None:
        s.SetMaterials(mats)
    if prim_mat is not None:
        s.SetPrimMaterials(prim_first, prim_mat)


@pytest.mark.parametrize("ctx", ["bvh2", "bvh4-kept"])
def test_updates_rebuilds_and_refits_chain(ctx):
    """update_materials -> rebuild_scene with every builder, the refit included -> update_scene (a BVH4 copy: a second refit) -> another
    update_materials -> a rebuild that carries its light list; after each step the arrays equal a fresh upload of the host's Scene, which
    follows with SetMaterials / SetTexels / SetPrimMaterials, Rebuild and Refit (the first step also against the numpy truth)."""
    gt, sa, _ = Z.build(**SCENES["four"])                                 # (a Scene of its own: the chain changes it)
    s = gt.s
    bvh4 = ctx != "bvh2"
    d, kw = _bound(sa, ctx)
    try:
        args = case("all", sa)
        want, _ = M.update(d, sa, **args)
        _host_update(s, **args)
        host = s.arrays()
        for f in ("prims", "mats", "lights"):
            assert np.array_equal(getattr(host, f), getattr(want, f)), f
        M.check(d, host, "update_materials", **kw)
        for k, (builder, opts) in enumerate([("sah", {}), ("lbvh", {}), ("sbvh_gpu", dict(alpha=0.0)), ("refit", {})]):
            p = _jittered(host.prims, k + 1)
            d.rebuild_scene(p, 0, None, builder=builder, **opts)
            if builder == "refit":
                s.SetPrimitives(0, p)
                s.Refit()
                host = s.arrays()
            else:
                host = RB.host_rebuild(s, p, builder=builder, bvh4=True, **opts)
            M.check(d, host, f"rebuild ({builder}) after update_materials", **kw)
        p = _jittered(host.prims, 9)
        if bvh4:
            d.rebuild_scene(p, 0, None, builder="refit")
        else:
            d.update_scene(p, 0, None)
        s.SetPrimitives(0, p)
        s.Refit()
        host = s.arrays()
        M.check(d, host, "update_scene after the rebuilds", **kw)
        again = dict(prim_mat=np.array([M.RED_LIGHT, M.GLASS, M.GREEN_LIGHT], np.int32), prim_first=7, mats=case("flags", sa)["mats"], n_texels=0)
        d.update_materials(**again)                                       # the bound lists live in a rebuild's set by now
        _host_update(s, mats=again["mats"])                               # (the table first: its windows go before the atlas does)
        _host_update(s, n_texels=0, prim_mat=again["prim_mat"], prim_first=7)
        host = s.arrays()
        M.check(d, host, "a second update_materials", **kw)
        d.rebuild_scene(None, 0, None, builder="sah")                     # ... and a rebuild carries the new list on
        M.check(d, RB.host_rebuild(s, None, builder="sah", bvh4=True), "a rebuild after the second update", **kw)
    finally:
        d.close()


@pytest.mark.parametrize("ctx", ["bvh2", "bvh4-kept"])
def test_a_resize_checks_against_the_new_table(ctx):
    sa0 = scene("one")
    _, sa1, counts = Z.build(tris=(40, 30), spheres=(1, 0), seed=4)
    eleven = np.concatenate([sa0.mats, sa0.mats[M.WHITE_LIGHT:M.WHITE_LIGHT + 1]])
    eleven["emittance"][10] = (2.0, 3.0, 4.0, 0.0)
    p = sa1.prims.copy()
    p["matIdx"][[3, 50]] = 10                                             # legal under the new table only; material 10 is a light
    d, kw = _bound(sa0, ctx)
    try:
        with pytest.raises(RtError, match="primitive 3: objType 2 / matIdx 10 out of range"):
            Z.resize(d, dataclasses.replace(sa1, prims=p), counts, "sah")
        M.update(d, sa0, mats=eleven)
        Z.resize(d, dataclasses.replace(sa1, prims=p), counts, "sah")
        want = dataclasses.replace(sa1, prims=p, mats=eleven, lights=M.scene_light_list(p, eleven))
        assert 3 in want.lights and 50 in want.lights
        M.check(d, want, "a resize under the new table", **kw)
        with pytest.raises(RtError, match=r"primitive 3: matIdx 10 outside the new table \(nMats 10\); the scene is unchanged") as e:
            d.update_materials(mats=sa0.mats)                             # the shorter table no longer serves the resized primitives
        assert e.value.code == W.RT_E_INVALID
        M.check(d, want, "the refused shorter table", **kw)
        want, _ = M.update(d, want, mats=sa0.mats, prim_mat=np.full(48, M.SAND, np.int32), prim_first=3)   # ... unless they leave it in the same call
        M.check(d, want, "a shorter table with a new assignment", **kw)
    finally:
        d.close()


# ---- 10. holders ---------------------------------------------------------------------------------------------------------------------
def test_group_lanes_and_sharing_contexts_render_the_updated_scene():
    sa = _room()
    args = _room_update(sa)
    want = M.truth(sa, **args)
    cam = scenes.camera_for(Z.VIEW, Wd, Hd)
    a, b = Device(Wd, Hd, **DEFAULT), Device(Wd, Hd, **DEFAULT)
    g = Group(Wd, Hd, lanes=2)
    try:
        a.upload(sa)
        b.share_scene(a)
        g.upload(sa)
        g.seed(0)
        b.seed_default()
        b.render(cam, 1)                                                  # work in flight on a holder that is not the one updating
        g.render(cam, 2)
        a.update_materials(**args)
        st = g.update_materials(**args)
        assert st["lights"] == len(want.lights)
        fresh, info, tables = Z.fresh(want, key=("room", "updated"), names=M.ARRAYS, **DEFAULT)
        for h in [a, b] + g.devs:
            Z.same(Z.arrays(h, M.ARRAYS), fresh, "a holder's arrays")
            assert h.shade_tables() == tables
        for h in (a, b):
            assert h.kernel_info() == info
        ref = oracle_for(want, Wd, Hd, **DEFAULT).render(cam, 1)[0]
        for dv in (a, b):
            dv.seed_default()
            dv.reset()
            dv.render(cam, 1)
            assert_bits(dv.read_accum(), ref, "shared pair after an update")
        g.seed(0)
        g.reset()
        g.render(cam, 2)
        exp = None
        for m in range(2):
            r = oracle_for(want, Wd, Hd, **DEFAULT).render(cam, 1, seeds=seed_stream(m * Wd * Hd, Wd * Hd))[0]
            exp = r if exp is None else exp + r
        assert_bits(g.read_accum(), exp, "2-lane group after an update")
    finally:
        g.close()
        b.close()
        a.close()


# ---- 11. allocations -----------------------------------------------------------------------------------------------------------------
def test_alternating_material_states_stop_allocating():
    sa = scene("one")
    n = len(sa.prims)
    rng = np.random.default_rng(2)
    big = M.textured(np.concatenate([sa.mats, sa.mats[:2]]), 11, 0, 8, 8)
    pm = rng.integers(0, 12, n).astype(np.int32)
    state_b = dict(mats=big, texels=_texels(64), n_texels=64, prim_mat=pm)
    state_a = dict(mats=sa.mats, n_texels=0, prim_mat=sa.prims["matIdx"].copy())
    d, kw = _bound(sa)
    try:
        want, allocs = sa, []
        for visit in range(3):
            for name, args in (("B", state_b), ("A", state_a)):
                want, _ = M.update(d, want, **args)
                M.check(d, want, f"visit {visit + 1} to {name}", key=("one", "state", name), **kw)
                allocs.append(d.rebuild_allocations())
        assert allocs[0] > 0 and len(M.truth(sa, **state_b).lights) > 40
        assert allocs[4] == allocs[3] and allocs[5] == allocs[4], f"the third visits allocated: {allocs}"
    finally:
        d.close()


# ---- 12. refusals --------------------------------------------------------------------------------------------------------------------
def _unchanged(d, twin, before, cam, what, names=M.ARRAYS):
    Z.same(Z.arrays(d, names), before, what)
    for x in (d, twin):
        x.render(cam, 1)
    assert_bits(d.read_accum(), twin.read_accum(), f"{what}: the next frame")
    assert np.array_equal(d.get_seeds(), twin.get_seeds())


class _Claims:
    """Device memory at `ptr` handed over as n elements of `dtype` (what Device.update_materials reads of a tensor)."""

    def __init__(self, ptr, n, dtype, size):
        self.ptr, self.n, self.dtype, self.size, self.is_cuda = ptr, n, dtype, size, False

    def is_contiguous(self):
        return True

    def numel(self):
        return self.n * self.size // 4

    def element_size(self):
        return 4

    def data_ptr(self):
        return self.ptr


def _raw(d, **fields):
    """rt_update_materials with the struct filled by hand (a count without a pointer cannot be said through Device.update_materials)."""
    u = np.zeros((), W.MaterialUpdate)
    u["nTexels"] = -1
    for k, v in fields.items():
        u[k] = v
    rc = d._lib.rt_update_materials(d._h, W.ptr(u), None)
    return rc, d._lib.rt_last_error().decode()


def test_refusals_leave_the_scene_and_its_next_frame_as_they_were():
    sa = scene("one")
    n, nm = len(sa.prims), len(sa.mats)
    cam = scenes.camera_for(Z.VIEW, Wd, Hd)
    bound = dict(mats=M.textured(sa.mats, M.SAND, 0, 4, 4), texels=_texels(16), n_texels=16)   # a 4 x 4 texture that fills the atlas
    # 32 MiB: a block of its own in torch's allocator, so the allocation the runtime knows ends where the tensor ends
    big = torch.zeros(1 << 25, dtype=torch.uint8, device=DEV)
    short_tex = _Claims(big.data_ptr() + 16, (1 << 25) // 16, torch.float32, 16)
    short_mat = _Claims(big.data_ptr() + (1 << 25) - 4 * (n - 1), n, torch.int32, 4)
    d, twin = Device(Wd, Hd, **DEFAULT), Device(Wd, Hd, **DEFAULT)
    try:
        with pytest.raises(RtError, match="no scene uploaded") as e:
            d.update_materials(mats=sa.mats)
        assert e.value.code == W.RT_E_INVALID
        for x in (d, twin):
            x.upload(sa)
            x.update_materials(**bound)
            x.seed_default()
            x.render(cam, 1)
        have = M.truth(sa, **bound)
        before = Z.arrays(d, M.ARRAYS)
        cases = [
            ("a table the lights no longer fit: the lowest index is named", lambda: d.update_materials(mats=have.mats[:M.WHITE_LIGHT]),
             rf"primitive {n - 4}: matIdx {M.WHITE_LIGHT} outside the new table \(nMats {M.WHITE_LIGHT}\); the scene is unchanged"),
            ("a new matIdx == nMats", lambda: d.update_materials(prim_mat=[0, nm, -1], prim_first=5), rf"primitive 6: matIdx {nm} outside the new table \(nMats {nm}\)"),
            ("a new matIdx == -1 at the last primitive", lambda: d.update_materials(prim_mat=[-1], prim_first=n - 1), rf"primitive {n - 1}: matIdx -1 "),
            ("a new matIdx in a torch tensor", lambda: d.update_materials(prim_mat=torch.tensor([1, 2, nm + 5], dtype=torch.int32, device=DEV), prim_first=0),
             rf"primitive 2: matIdx {nm + 5} "),
            ("a window outside the new atlas", lambda: d.update_materials(mats=M.textured(have.mats, M.RED, 13, 2, 2)), f"material {M.RED}: texture window exceeds the atlas"),
            ("a window outside a grown atlas", lambda: d.update_materials(mats=M.textured(have.mats, M.RED, 16, 4, 2), n_texels=23), f"material {M.RED}: texture window"),
            ("an atlas shrunk under a bound window", lambda: d.update_materials(n_texels=15), f"material {M.SAND}: texture window exceeds the atlas"),
            ("a texel range past the atlas", lambda: d.update_materials(texels=_texels(3), tex_first=14), r"texel range \[14, 17\) outside the new atlas of 16"),
            ("a negative first texel", lambda: d.update_materials(texels=_texels(3), tex_first=-1), "negative texel range"),
            ("a primitive range past the scene", lambda: d.update_materials(prim_mat=[0, 0], prim_first=n - 1), rf"primitive range \[{n - 1}, {n + 1}\) outside the {n} bound"),
            ("a negative first primitive", lambda: d.update_materials(prim_mat=[0], prim_first=-3), "negative primitive range"),
            ("nTexels = -2", lambda: d.update_materials(n_texels=-2), "nTexels -2"),
            ("an empty table", lambda: d.update_materials(mats=have.mats[:0]), "at least one material"),
            ("texels whose allocation ends a texel early", lambda: d.update_materials(texels=short_tex, n_texels=1 << 21),
             "texels needs 33554432 bytes .* its allocation ends 16 bytes earlier"),
            ("matIdx values whose allocation ends a value early", lambda: d.update_materials(prim_mat=short_mat), f"primMat needs {4 * n} bytes .* its allocation ends 4 bytes earlier"),
        ]
        for what, call, pattern in cases:
            with pytest.raises(RtError, match=pattern) as e:
                call()
            assert e.value.code == W.RT_E_INVALID, (what, e.value)
            _unchanged(d, twin, before, cam, what)
        for what, fields, pattern in [("a texel count without texels", dict(texCount=3), "texCount 3 but texels == NULL"),
                                      ("a primitive count without values", dict(primCount=2), "primCount 2 but primMat == NULL"),
                                      ("a negative count", dict(primCount=-1), "negative primitive range")]:
            rc, msg = _raw(d, **fields)
            assert rc == W.RT_E_INVALID and pattern in msg, (what, rc, msg)
            _unchanged(d, twin, before, cam, what)
        assert d._lib.rt_update_materials(d._h, None, None) == W.RT_E_INVALID and d._lib.rt_update_materials(None, None, None) == W.RT_E_INVALID
        args = case("flags", have)                                        # ... and the context still takes a good one
        want, _ = M.update(d, have, **args)
        M.check(d, want, "after the refusals", **DEFAULT)
    finally:
        twin.close()
        d.close()


def test_scenes_that_cannot_be_refit_or_rebuilt_take_an_update():
    """A bound scene with a gap between its BLAS ranges (rt_resize_scene refuses it) and a classic BVH4 copy without
    its BVH2 (everything else refuses it): materials, texels and matIdx change all the same."""
    s2 = scenes.Scene()
    scenes._std_materials(s2)
    rng = np.random.default_rng(4)
    s2.AddTriangles(C._soup(rng, 30, -1.0, 1.0, 0.3), "sand")
    s2.BuildBLAS(0)
    s2.AddTriangles(C._soup(rng, 2, 3.0, 3.5, 0.3), "white-light")
    s2.AddTriangles(C._soup(rng, 20, -1.0, 1.0, 0.3), "green")
    s2.BuildBLAS(32)
    sg = s2.arrays()
    assert s2.blas_ranges() == [(0, 30), (32, 20)]
    for ctx in ("bvh2", "bvh4-classic"):
        d, kw = _bound(sg, ctx)
        try:
            with pytest.raises(RtError, match="leave a gap" if ctx == "bvh2" else "lost its BVH2") as e:
                d.resize_scene(sg.prims, [len(sg.prims)])
            assert e.value.code == W.RT_E_UNSUPPORTED
            m = M.textured(sg.mats, M.GREEN, 0, 3, 2)
            m["isLight"][M.SAND] = 1
            want, st = M.update(d, sg, mats=m, texels=_texels(6), n_texels=6, prim_mat=[M.RED_LIGHT, M.MIRROR], prim_first=30)
            assert st["lights"] == 31
            M.check(d, want, f"{ctx}: a scene with a gap", **kw)
        finally:
            d.close()

"""The device-free side of in-place material updates: rt_materials_check, the checks rt_update_materials runs on a table before any device
work, and the host restatement Scene.SetMaterials / SetTexels / SetPrimMaterials (rth_set_*), whose arrays() must equal the numpy truth
of materials_check.truth - light list included - and whose refusals must change nothing."""
import numpy as np
import pytest

import materials_check as M
import resize_check as Z
import test_groundtruth_cpu as C
from magr_ray_tracer_amd import _lib as W
from magr_ray_tracer_amd.scene import BuildError
from magr_ray_tracer_amd.scenes import Scene, _std_materials


def _std():
    s = Scene()
    _std_materials(s)
    return s.material_array()


# ---- rt_materials_check ----------------------------------------------------------------------------------------------------------------
def test_a_window_ending_exactly_at_the_atlas_end_is_accepted_and_one_texel_past_is_refused():
    m = M.textured(_std(), M.SAND, 8, 4, 3)                               # texels [8, 20)
    assert M.materials_check(m, 20) == (W.RT_OK, "")
    rc, msg = M.materials_check(m, 19)
    assert rc == W.RT_E_INVALID and msg == f"material {M.SAND}: texture window exceeds the atlas"
    assert M.materials_check(M.textured(_std(), M.RED, 19, 1, 1), 20)[0] == W.RT_OK      # a 1 x 1 texture in the last texel


@pytest.mark.parametrize("tex_idx,w,h", [(0, 0, 3), (0, 3, 0), (-2, 2, 2), (0, -1, 2)])
def test_a_malformed_window_is_refused(tex_idx, w, h):
    rc, msg = M.materials_check(M.textured(_std(), M.GREEN, tex_idx, w, h), 64)
    assert rc == W.RT_E_INVALID and msg == f"material {M.GREEN}: texture window exceeds the atlas"


def test_an_empty_table_and_a_negative_atlas_are_refused():
    rc, msg = M.materials_check(_std()[:0], 16)
    assert rc == W.RT_E_INVALID and "at least one material" in msg
    assert M.materials_check(_std(), -1)[0] == W.RT_E_INVALID
    assert M.materials_check(_std(), 0) == (W.RT_OK, "")                   # no texture, no atlas
    assert W.device_lib().rt_materials_check(None, 3, 16) == W.RT_E_INVALID


def test_the_new_structs_have_the_sizes_of_the_header():
    assert W.MaterialUpdate.itemsize == 56 and W.MaterialStats.itemsize == 48
    assert W.MaterialUpdate.fields["texels"][1] == 16 and W.MaterialUpdate.fields["primMat"][1] == 40 and W.MaterialUpdate.fields["primCount"][1] == 52
    assert W.SCENE_ARRAYS_MATERIALS == {"materials": 15, "textures": 16}


# ---- the host restatement --------------------------------------------------------------------------------------------------------------
def _scene(n=60, tex=True):
    """A Scene of n soup triangles in runs of four materials, two lights and (tex) a 4 x 3 and a 2 x 2 texture; not built: arrays are read one by one."""
    rng = np.random.default_rng(3)
    s = Scene()
    _std_materials(s)
    if tex:
        s.AddTexture("t43", rng.uniform(0, 1, (3, 4, 4)).astype(np.float32))
        s.AddTexture("t22", rng.uniform(0, 1, (2, 2, 4)).astype(np.float32))
    for k, mat in enumerate(["sand", "white-light", "green", "red-light", "t43" if tex else "white"]):
        s.AddTriangles(C._soup(rng, n // 5, -1.5, 1.5, 0.3), mat)
    s.BuildBLAS(0, **Z.BUILDERS["sah"][1])
    return s


def _same(s, want, what):
    got = s.arrays()
    for f in ("prims", "mats", "lights", "bvh2", "bvh4", "primIdx", "tlas", "blas"):
        assert np.array_equal(getattr(got, f), getattr(want, f)), f"{what}: {f}"
    assert np.array_equal(np.asarray(got.tex).reshape(-1, 4), np.asarray(want.tex).reshape(-1, 4)), f"{what}: tex"


def test_set_materials_gives_the_numpy_truth():
    s = _scene()
    sa = s.arrays()
    m = sa.mats.copy()
    m["color"][M.SAND] = (0.1, 0.9, 0.3, 0.0)
    m["emittance"][M.WHITE_LIGHT] = (5, 6, 7, 0)                          # flags kept: the list stays
    s.SetMaterials(m)
    t1 = M.truth(sa, mats=m)
    assert np.array_equal(t1.lights, sa.lights)
    _same(s, t1, "colours and emittance")
    m2 = m.copy()
    m2["isLight"][M.WHITE_LIGHT], m2["isLight"][M.GREEN] = 0, 1           # one flag off, another on
    s.SetMaterials(m2)
    t2 = M.truth(t1, mats=m2)
    assert len(t2.lights) == len(sa.lights) and not np.array_equal(t2.lights, sa.lights)
    _same(s, t2, "flags moved")
    s.SetMaterials(np.concatenate([m2, m2[:3]]))                          # a longer table
    _same(s, M.truth(t2, mats=np.concatenate([m2, m2[:3]])), "a longer table")
    off = m2.copy()
    off["isLight"][:] = 0
    s.SetMaterials(off)
    assert len(s.arrays().lights) == 0
    _same(s, M.truth(t2, mats=off), "no light left")


def test_set_texels_gives_the_numpy_truth():
    s = _scene()
    sa = s.arrays()
    n = len(sa.tex)
    assert n == 16
    rng = np.random.default_rng(8)
    t = rng.uniform(0, 1, (5, 4)).astype(np.float32)
    s.SetTexels(t, first=11)                                              # the range ends at the atlas end
    t1 = M.truth(sa, texels=t, tex_first=11)
    _same(s, t1, "a range ending at the atlas end")
    s.SetTexels(t[:2], first=20, n_texels=24)                             # growth: zeros but the range
    t2 = M.truth(t1, texels=t[:2], tex_first=20, n_texels=24)
    assert not t2.tex[16:20].any() and not t2.tex[22:].any() and t2.tex[20:22].all()
    _same(s, t2, "growth")
    s.SetTexels(n_texels=16)                                              # shrinkage to exactly what the windows need
    _same(s, M.truth(t2, n_texels=16), "shrinkage")
    assert np.array_equal(s.arrays().lights, sa.lights)


def test_set_prim_materials_gives_the_numpy_truth():
    s = _scene()
    sa = s.arrays()
    pm = np.array([M.RED_LIGHT, M.SAND, M.GREEN_LIGHT, M.MIRROR, M.SAND, M.WHITE_LIGHT], np.int32)
    s.SetPrimMaterials(9, pm)                                             # across the end of the first run and into the lights' run
    t1 = M.truth(sa, prim_mat=pm, prim_first=9)
    assert not np.array_equal(t1.lights, sa.lights)
    _same(s, t1, "a range across two runs")
    s.SetPrimMaterials(len(sa.prims) - 1, [M.GREEN_LIGHT])                # the last primitive becomes a light
    t2 = M.truth(t1, prim_mat=[M.GREEN_LIGHT], prim_first=len(sa.prims) - 1)
    assert t2.lights[-1] == len(sa.prims) - 1
    _same(s, t2, "the last primitive")
    s.SetPrimMaterials(0, [])                                             # nothing
    _same(s, t2, "an empty range")


def test_refusals_leave_the_arrays_unchanged():
    s = _scene()
    sa = s.arrays()
    n, nm = len(sa.prims), len(sa.mats)
    t43 = int(np.flatnonzero(sa.mats["texW"] == 4)[0])
    cases = [
        ("a table the last run no longer fits", lambda: s.SetMaterials(sa.mats[:t43]), rf"primitive {n - n // 5}: matIdx {t43} outside the new table \(nMats {t43}\)"),
        ("an empty table", lambda: s.SetMaterials(sa.mats[:0]), "at least one material"),
        ("a window past the atlas", lambda: s.SetMaterials(M.textured(sa.mats, M.RED, 13, 2, 2)), f"material {M.RED}: texture window exceeds the atlas"),
        ("texW = 0", lambda: s.SetMaterials(M.textured(sa.mats, M.RED, 0, 0, 2)), f"material {M.RED}: texture window exceeds the atlas"),
        ("an atlas shrunk under a window", lambda: s.SetTexels(n_texels=15), f"material {t43 + 1}: texture window exceeds the atlas"),
        ("a range past the atlas", lambda: s.SetTexels(np.ones((3, 4), np.float32), first=14), r"texel range \[14, 17\) outside the new atlas of 16"),
        ("a negative first texel", lambda: s.SetTexels(np.ones((1, 4), np.float32), first=-1), "bad texel range"),
        ("nTexels = -2", lambda: s.SetTexels(n_texels=-2), "nTexels -2"),
        ("matIdx == nMats", lambda: s.SetPrimMaterials(3, [M.SAND, nm]), rf"primitive 4: matIdx {nm} outside the table \(nMats {nm}\)"),
        ("matIdx == -1", lambda: s.SetPrimMaterials(0, [-1]), "primitive 0: matIdx -1"),
        ("a range past the primitives", lambda: s.SetPrimMaterials(n - 1, [0, 0]), rf"primitive range \[{n - 1}, {n + 1}\) outside the {n}"),
        ("a negative first primitive", lambda: s.SetPrimMaterials(-1, [0]), "bad primitive range"),
    ]
    for what, call, pattern in cases:
        with pytest.raises(BuildError, match=pattern) as e:
            call()
        assert e.value.code == W.RT_E_INVALID, what
        _same(s, sa, what)
    L = W.host_lib()
    assert L.rth_set_materials(None, W.ptr(sa.mats), nm) == W.RT_E_INVALID and L.rth_set_texels(s._h, None, 0, 3, -1) == W.RT_E_INVALID
    assert L.rth_set_prim_materials(s._h, 0, 2, None) == W.RT_E_INVALID
    _same(s, sa, "null arguments")


def test_names_keep_their_materials_and_dropped_names_are_forgotten():
    s = Scene()
    _std_materials(s)
    m = s.material_array()
    s.SetMaterials(m[:8])                                                 # green-light and red-light are gone
    rng = np.random.default_rng(1)
    s.AddTriangles(C._soup(rng, 2, -1, 1, 0.3), "white-light")
    s.AddTriangles(C._soup(rng, 2, -1, 1, 0.3), "red-light")              # an unknown name now: material 0, as for any unknown name
    s.AddMaterial("blue", m[M.MIRROR])
    s.AddTriangles(C._soup(rng, 1, -1, 1, 0.3), "blue")
    s.BuildBLAS(0)
    sa = s.arrays()
    assert list(sa.prims["matIdx"]) == [M.WHITE_LIGHT] * 2 + [0] * 2 + [8] and list(sa.lights) == [0, 1] and len(sa.mats) == 9

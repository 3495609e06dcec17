"""Shared pieces of the in-place material update's tests (test_materials_cpu.py, test_gpu_materials.py): the truth an update must
reproduce, made in numpy from scenes of resize_check.build / build_runs - a copy of the arrays with prims["matIdx"] patched, the table
and the atlas replaced and the light list by the Scene rule - which shares no code with the device path or the host restatement, and
what compares a context with a fresh upload of it (resize_check.fresh / same, with the two arrays rt_update_materials adds)."""
import dataclasses

import numpy as np

import resize_check as Z
from magr_ray_tracer_amd import _lib as W

ARRAYS = Z.ARRAYS + list(W.SCENE_ARRAYS_MATERIALS)
ARRAYS_BVH4 = Z.ARRAYS_BVH4 + list(W.SCENE_ARRAYS_MATERIALS)
GREY, WHITE, RED, GREEN, SAND, MIRROR, GLASS, WHITE_LIGHT, GREEN_LIGHT, RED_LIGHT = range(10)   # scenes._std_materials, in its order


def scene_light_list(prims, mats):
    """The Scene rule: the indices, in increasing order, of the primitives whose material is a light."""
    return np.flatnonzero(mats["isLight"][prims["matIdx"]] != 0).astype(np.uint32)


def truth(sa, mats=None, texels=None, tex_first=0, n_texels=None, prim_mat=None, prim_first=0):
    """The arrays after Device.update_materials(...) with the same keywords on a context bound to `sa`: the trees, the TLAS and the
    instances as they are; with only texels given the light list stays as it is, otherwise it follows the Scene rule."""
    prims = sa.prims.copy()
    m = sa.mats.copy() if mats is None else np.ascontiguousarray(mats, dtype=W.Material).copy()
    old = np.asarray(sa.tex, np.float32).reshape(-1, 4)
    n = len(old) if n_texels is None else int(n_texels)
    tex = np.zeros((n, 4), np.float32)
    keep = min(n, len(old))
    tex[:keep] = old[:keep]
    if texels is not None:
        t = np.asarray(texels, np.float32).reshape(-1, 4)
        assert tex_first >= 0 and tex_first + len(t) <= n
        tex[tex_first:tex_first + len(t)] = t
    if prim_mat is not None:
        pm = np.asarray(prim_mat, np.int32).ravel()
        assert prim_first >= 0 and prim_first + len(pm) <= len(prims)
        prims["matIdx"][prim_first:prim_first + len(pm)] = pm
    lights = sa.lights.copy() if mats is None and prim_mat is None else scene_light_list(prims, m)
    return dataclasses.replace(sa, prims=prims, mats=m, tex=tex, lights=lights)


def update(d, sa, **kw):
    """Device.update_materials (or Group's) with the keywords of truth(); returns (the truth afterwards, the stats)."""
    return truth(sa, **kw), d.update_materials(**kw)


def tex_pad(mats):
    """validate_scene's pad behind the atlas: two texels, or the widest texture's width plus two."""
    t = mats[mats["texIdx"] != -1]
    return max(2, int(t["texW"].max()) + 2) if len(t) else 2


def check(d, sa, what, key=None, names=ARRAYS, from_bvh2=False, **kw):
    """resize_check.check over the arrays of this module, and the two new arrays against numpy directly: the table, and the atlas with
    its zero pad."""
    Z.check(d, sa, what, key=key, names=names, from_bvh2=from_bvh2, **kw)
    assert np.array_equal(np.frombuffer(d.scene_array("materials").tobytes(), W.Material), sa.mats), f"{what}: the table"
    tex = np.frombuffer(d.scene_array("textures").tobytes(), np.float32).reshape(-1, 4)
    n = len(sa.tex)
    assert len(tex) == n + tex_pad(sa.mats), f"{what}: {len(tex)} texels with the pad, {n} + {tex_pad(sa.mats)} expected"
    assert np.array_equal(tex[:n].view(np.uint32), np.asarray(sa.tex, np.float32).reshape(-1, 4).view(np.uint32)), f"{what}: the atlas"
    assert not tex[n:].view(np.uint32).any(), f"{what}: the pad is not zero"
    assert np.array_equal(np.frombuffer(d.scene_array("lights").tobytes(), np.uint32), sa.lights), f"{what}: the light list"


def materials_check(mats, n_texels):
    """rt_materials_check, the device-free checks of a material table: (return code, message)."""
    L = W.device_lib()
    m = np.ascontiguousarray(mats, dtype=W.Material).ravel()
    rc = L.rt_materials_check(W.ptr(m) if len(m) else None, len(m), int(n_texels))
    return rc, (L.rt_last_error().decode() if rc else "")


def textured(mats, idx, tex_idx, w, h):
    """A copy of the table whose material `idx` shows the w x h window at texel tex_idx."""
    m = np.ascontiguousarray(mats, dtype=W.Material).copy()
    m["texIdx"][idx], m["texW"][idx], m["texH"][idx] = tex_idx, w, h
    return m

"""Replacement geometry from vertex positions on the host (Scene.SetVertices / rth_set_vertices, rt_geometry_check): the one rule of
csrc/geometry_common.h held to Scene::AddTriangle - a scene built from moved vertices through AddTriangle gives the records that
SetVertices must produce from those vertices, byte for byte - and every refusal, after which nothing has changed."""
import ctypes as C

import numpy as np
import pytest

import geometry_check as GC
import refit_check as R
from magr_ray_tracer_amd import _lib as W
from magr_ray_tracer_amd.renderer import RtError, geometry_check
from magr_ray_tracer_amd.scene import BuildError

FLIP_V = np.array([(0.3, 0.1, -0.2), (1.1, 0.4, 0.3), (0.2, 1.3, 0.6)], np.float32)


def _pair(deform):
    """R.build(alpha=0.0, blas=2, spheres=0) and one more triangle added with flipNormal=True (R.build has none), as bound and from the
    deformed vertices: (Scene, its records) twice."""
    out = []
    for d in (R.identity, deform):
        gt, _, _ = R.build(d, alpha=0.0, blas=2, spheres=0)
        gt.s.AddTriangle(*d("tris", 1, FLIP_V.reshape(1, 3, 3))[0], "red", flipNormal=True)
        out.append((gt.s, gt.s.arrays(bvh4=False).prims))
    return out


def test_set_vertices_gives_add_triangles_records():
    (s, p0), (_, p1) = _pair(R.jitter())
    n = len(p0)
    assert n == 2 * 220 + 4 + 1 and np.all(p0["objType"] == W.PRIM_TRIANGLE)
    flipped = GC.is_flipped(p0)
    assert flipped.any() and not flipped.all() and np.array_equal(flipped, GC.is_flipped(p1))
    mats = s.material_array()
    assert (mats["isLight"][p0["matIdx"]] != 0).sum() >= 1                       # a light triangle is among them
    assert not np.array_equal(p0["v0"], p1["v0"])
    v1 = GC.verts(p1)
    # the identity first: the scene's own vertices, packed and indexed
    s.SetVertices(0, GC.verts(p0))
    GC.same_records(s.arrays(bvh4=False).prims, p0, "the scene's own vertices, packed")
    s.SetVertices(0, *GC.indexed(GC.verts(p0)))
    GC.same_records(s.arrays(bvh4=False).prims, p0, "the scene's own vertices, indexed")
    # the moved vertices, packed
    s.SetVertices(0, v1)
    GC.same_records(s.arrays(bvh4=False).prims, p1, "packed")
    # back, then indexed through a vertex buffer without duplicates
    s.SetVertices(0, GC.verts(p0))
    vb, idx = GC.indexed(v1)
    assert len(vb) <= 3 * n and idx.max() == len(vb) - 1
    s.SetVertices(0, vb, idx)
    GC.same_records(s.arrays(bvh4=False).prims, p1, "indexed")
    # ... and through rows of a wider row, a window in the middle
    s.SetVertices(0, GC.verts(p0))
    s.SetVertices(7, GC.strided(v1[7:72].reshape(-1, 3), 32))
    want = p0.copy()
    want[7:72] = p1[7:72]
    GC.same_records(s.arrays(bvh4=False).prims, want, "a window at stride 32")


def _raw(s, first, count, positions, stride, n_vertices, indices=None):
    L = W.host_lib()
    rc = L.rth_set_vertices(s._h, first, count, None if positions is None else C.c_void_p(positions.ctypes.data), stride, n_vertices,
                            None if indices is None else C.c_void_p(indices.ctypes.data))
    return rc, L.rth_last_error().decode()


def test_every_refusal_changes_nothing():
    gt, sa, _ = R.build(alpha=0.0, blas=2, spheres=4)
    s = gt.s
    before = sa.prims.copy()
    types = before["objType"].astype(np.int32)
    sph = int(np.nonzero(types == W.PRIM_SPHERE)[0][0])
    n = len(before)
    pos = np.zeros((30, 3), np.float32) + np.arange(30, dtype=np.float32)[:, None]
    idx = np.arange(30, dtype=np.uint32)
    at = pos.ctypes.data
    rec = before[:4].ctypes.data
    G = GC.geometry
    L = W.device_lib()
    # rt_geometry_check, one case each: (geometry, objType, a word of the message)
    cases = [
        (None, types, "null geometry"),
        (G(0, -1, positions=at, n_vertices=30), types, "bad primitive count -1"),
        (G(-1, 0), types, "starts at primitive -1"),
        (G(-1, 4, positions=at, n_vertices=30), types, "primitive range [-1, 3)"),
        (G(n - 2, 4, positions=at, n_vertices=30), types, f"outside the {n} uploaded"),
        (G(0, 4, prims=rec, positions=at, n_vertices=30), types, "both prims and positions"),
        (G(0, 4), types, "NULL records"),
        (G(0, 4, positions=at, stride=8, n_vertices=30), types, "positionStride 8"),
        (G(0, 4, positions=at, stride=14, n_vertices=30), types, "positionStride 14"),
        (G(0, 4, positions=at, n_vertices=-1, indices=idx.ctypes.data), types, "nVertices -1"),
        (G(0, 4, positions=at, n_vertices=11), types, "11 vertices for 4 triangles"),
        (G(sph - 2, 4, positions=at, n_vertices=30), types, f"primitive {sph} is no triangle"),
    ]
    for g, t, word in cases:
        rc = L.rt_geometry_check(None if g is None else W.ptr(g), n, W.ptr(t))
        assert rc == W.RT_E_INVALID and word in L.rt_last_error().decode(), (word, rc, L.rt_last_error())
    assert L.rt_geometry_check(W.ptr(G(sph - 2, 4, positions=at, n_vertices=30)), n, None) == W.RT_OK      # objType NULL: all triangles
    assert L.rt_geometry_check(W.ptr(G(sph - 2, 4, prims=rec)), n, W.ptr(types)) == W.RT_OK                # records form: any type
    assert L.rt_geometry_check(W.ptr(G(0, 4, positions=at, n_vertices=12)), n, W.ptr(types)) == W.RT_OK
    assert L.rt_geometry_check(W.ptr(G(0, 0)), n, W.ptr(types)) == W.RT_OK
    with pytest.raises(RtError, match="no triangle") as e:                        # the Python face of the same check
        geometry_check(n, sph, positions=pos[:3], obj_types=types)
    assert e.value.code == W.RT_E_INVALID
    with pytest.raises(ValueError):
        geometry_check(n, 0, positions=pos[:4])
    # rth_set_vertices: the same refusals with the same words, and an index that is no vertex
    bad_first, bad_last = idx[:12].copy(), idx[:12].copy()
    bad_first[1], bad_last[11] = 30, 30                                          # equal to nVertices
    host = [
        ((0, -1, pos, 12, 30), "bad primitive count -1"),
        ((-1, 4, pos, 12, 30), "primitive range [-1, 3)"),
        ((n - 2, 4, pos, 12, 30), f"outside the {n} uploaded"),
        ((0, 4, None, 12, 30), "NULL records"),
        ((0, 4, pos, 8, 30), "positionStride 8"),
        ((0, 4, pos, 14, 30), "positionStride 14"),
        ((0, 4, pos, 12, -1, idx), "nVertices -1"),
        ((0, 4, pos, 12, 11), "11 vertices for 4 triangles"),
        ((sph - 2, 4, pos, 12, 30), f"primitive {sph} is no triangle"),
        ((0, 4, pos, 12, 30, bad_first), "triangle 0 of the window: index 30 (corner 1) is no vertex, nVertices is 30"),
        ((0, 4, pos, 12, 30, bad_last), "triangle 3 of the window: index 30 (corner 2) is no vertex, nVertices is 30"),
    ]
    for args, word in host:
        rc, msg = _raw(s, *args)
        assert rc == W.RT_E_INVALID and word in msg, (word, rc, msg)
        GC.same_records(s.arrays(bvh4=False).prims, before, f"after the refusal '{word}'")
    with pytest.raises(BuildError, match="no triangle") as e:
        s.SetVertices(sph, pos[:3])
    assert e.value.code == W.RT_E_INVALID
    assert W.host_lib().rth_set_vertices(None, 0, 0, None, 12, 0, None) == W.RT_E_INVALID
    GC.same_records(s.arrays(bvh4=False).prims, before, "after all refusals")


def test_a_zero_area_triangle_has_nan_where_add_triangle_has():
    """Three equal vertices: N is NaN (in x, y and z) as AddTriangle's is, every other word is AddTriangle's, the neighbours stay."""
    p = np.array([1.5, -0.25, 3.0], np.float32)

    def degenerate(kind, b, x):
        if kind == "tris" and b == 1:
            x = x.copy()
            x[5] = p
        return x
    (s, p0), (_, p1) = [(gt.s, gt.s.arrays(bvh4=False).prims) for gt in (R.build(d, alpha=0.0, blas=2, spheres=0)[0] for d in (R.identity, degenerate))]
    k = 224 + 5
    assert np.isnan(p1["N"][k][:3]).all() and p1["N"][k][3] == 0 and p1["area"][k] == 0
    s.SetVertices(k, np.tile(p, (3, 1)))
    got = s.arrays(bvh4=False).prims
    assert np.isnan(got["N"][k][:3]).all()
    a, b = got[k:k + 1].copy(), p1[k:k + 1].copy()
    a["N"][:, :3] = b["N"][:, :3] = 0
    GC.same_records(a, b, "the words beside N")
    GC.same_records(got[:k], p0[:k], "the records before")
    GC.same_records(got[k + 1:], p0[k + 1:], "the records behind")

"""Shared pieces of the tests of replacement geometry from vertex positions (test_geometry_cpu.py, test_gpu_geometry.py).  Expected
records never come from the rule under test alone: a scene is built twice by the same calls, once as bound and once from moved
vertices, so the moved scene's records are Scene::AddTriangle's; the vertices go in, and those records must come out."""
import numpy as np

import geom64 as G
import refit_check as R
import test_groundtruth_cpu as C
from magr_ray_tracer_amd import _lib as W
from magr_ray_tracer_amd.scenes import Scene, _std_materials

NB0 = 224          # BLAS 0 of build(): 220 soup triangles, 2 light triangles (220, 221), 2 floor triangles
N_FLIP = 2         # BLAS 1 of build() ends with this many triangles added with flipNormal=True
LIGHTS = (220, 221)


def build(deform=R.identity, alpha=0.0):
    """refit_check.build(blas=2, spheres=0) with two more triangles at the end of BLAS 1, added with flipNormal=True: 224 + 222
    triangles.  Returns (ground truth, arrays, view) as it does."""
    rng = np.random.default_rng(11)
    gt = G.GTScene(Scene())
    _std_materials(gt.s)
    for b in range(2):
        c = np.array(R.CENTRES[b])
        gt.triangles(deform("tris", b, C._soup(rng, 220, c - 1.6, c + 1.6, 0.3)), R.MATS[b])
        if b == 0:
            y = 4.2
            for v in ([(-1, y, -1), (1, y, -1), (1, y, 1)], [(1, y, 1), (-1, y, 1), (-1, y, -1)]):
                gt.light(deform("light", b, np.array(v, np.float32)), "white-light")
            gt.triangles(deform("tris", b, np.array([[(-4, -2.6, -4), (4, -2.6, -4), (4, -2.6, 4)],
                                                     [(4, -2.6, 4), (-4, -2.6, 4), (-4, -2.6, -4)]], np.float32)), "grey")
        else:
            v = np.ascontiguousarray(deform("tris", b, C._soup(rng, N_FLIP, c - 1.6, c + 1.6, 0.5)), np.float32)
            gt.blas[-1]["tri"].append(v.astype(np.float64))
            gt.blas[-1]["tri_idx"].append(np.arange(gt.s.num_prims, gt.s.num_prims + len(v)))
            gt.s.AddTriangles(v, "red", flipNormal=True)
        gt.build_blas(alpha)
    sa = gt.finish()
    view = dict(origin=(0.1, 0.6, 10.0), forward=(0.0, 0.05, 1.0), fov=64.0, aperture=0.01)
    return gt, sa, view


def moved(scale=0.08, seed=1):
    """refit_check.jitter that moves the lights too (a window that holds a light changes light records and NEE)."""
    rng = np.random.default_rng(seed)

    def d(kind, b, x):
        if kind in ("tris", "light"):
            return (x + rng.normal(scale=scale, size=x.shape)).astype(np.float32)
        return x
    return d


def verts(prims):
    """(n, 3, 3) float32: the vertices of triangle records."""
    return np.ascontiguousarray(np.stack([prims["v0"][:, :3], prims["v1"][:, :3], prims["v2"][:, :3]], axis=1), np.float32)


def is_flipped(prims):
    """AddTriangle's flip, told from a record in float64 (the tests' own statement, not the library's)."""
    v = verts(prims).astype(np.float64)
    n = np.cross(v[:, 1] - v[:, 0], v[:, 2] - v[:, 0])
    return np.einsum("ij,ij->i", n, prims["N"][:, :3].astype(np.float64)) < 0


def indexed(v):
    """(vertex buffer (m, 3) float32 without duplicates, indices (3n,) uint32) of (n, 3, 3) vertices: np.unique over the words, so that
    +0 and -0 stay two vertices."""
    words = np.ascontiguousarray(v, np.float32).reshape(-1, 3).view(np.uint32)
    uniq, inv = np.unique(words, axis=0, return_inverse=True)
    return np.ascontiguousarray(uniq).view(np.float32), np.ascontiguousarray(inv.ravel(), np.uint32)


def strided(p, stride):
    """The (n, 3) positions as rows of a wider row of `stride` bytes whose other words are NaN: a view, not contiguous for stride > 12."""
    wide = np.full((len(p), stride // 4), np.nan, np.float32)
    wide[:, :3] = p
    return wide[:, :3]


def same_records(got, want, what):
    """Byte for byte, record by record."""
    a, b = np.ascontiguousarray(got).view(np.uint8).reshape(-1, 128), np.ascontiguousarray(want).view(np.uint8).reshape(-1, 128)
    assert a.shape == b.shape, (what, a.shape, b.shape)
    bad = np.nonzero((a != b).any(axis=1))[0]
    assert len(bad) == 0, f"{what}: {len(bad)} records differ, first {bad[0]}: {got[bad[0]]} / {want[bad[0]]}"


def geometry(first, count, prims=0, positions=0, stride=12, n_vertices=0, indices=0):
    """A raw RtGeometry record (addresses as integers)."""
    g = np.zeros((), W.Geometry)
    g["first"], g["count"], g["prims"], g["positions"], g["positionStride"], g["nVertices"], g["indices"] = first, count, prims, positions, stride, n_vertices, indices
    return g

"""Shared pieces of the tests of replacement geometry from vertex positions (test_geometry_cpu.py, test_gpu_geometry.py).  Expected
records never come from the rule under test alone: a scene is built twice by the same calls, once as bound and once from moved
vertices, so the moved scene's records are Scene::AddTriangle's; the vertices go in, and those records must come out.  The second half
holds the hard inputs - points, collinear vertices, needles, a ladder of scales through every float32 exponent, large offsets,
non-finite values, signed zeros -, a comparison that lets a NaN match any NaN in the computed words and nothing else, and a float64
ground truth for well-conditioned triangles."""
import numpy as np

import geom64 as G
import refit_check as R
import test_groundtruth_cpu as C
from magr_ray_tracer_amd import _lib as W
from magr_ray_tracer_amd.scene import _view
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


# ---- hard inputs: where the rule of geometry_common.h leaves the well-behaved floats ------------------------------------------------
# Every generator is seeded and returns (n, 3, 3) float32 vertices.
LADDER_K = range(-149, 128)       # the ladder's scales 2^k: the smallest subnormal to the largest power of two
LADDER_M = 8                      # ... of this many triangles each
N_HARD = 4096                     # the one-BLAS scene of the GPU tests (hard_scene)
MIN_ANGLE = 10.0                  # degrees: the smallest angle of a "well-shaped" triangle


def min_angle(v):
    """The smallest angle of each triangle, degrees, in float64."""
    v = np.asarray(v, np.float64)
    out = np.full(len(v), 180.0)
    for i in range(3):
        a, b = v[:, (i + 1) % 3] - v[:, i], v[:, (i + 2) % 3] - v[:, i]
        c = np.einsum("ij,ij->i", a, b) / (np.linalg.norm(a, axis=1) * np.linalg.norm(b, axis=1))
        out = np.minimum(out, np.degrees(np.arccos(np.clip(c, -1.0, 1.0))))
    return out


def well_shaped(n, seed=21, origin=False, lo=-2.0, hi=2.0):
    """n random triangles with edges around 1 and smallest angle >= MIN_ANGLE; origin: v0 is (0, 0, 0)."""
    rng = np.random.default_rng(seed)
    out = np.zeros((0, 3, 3), np.float32)
    while len(out) < n:
        v = rng.normal(size=(4 * n, 3, 3)) * 0.6
        v = (v - v[:, :1] if origin else v + rng.uniform(lo, hi, (4 * n, 1, 3))).astype(np.float32)
        out = np.concatenate([out, v[min_angle(v) >= MIN_ANGLE]])
    return np.ascontiguousarray(out[:n])


def points(n=256, seed=22):
    """Three equal vertices."""
    p = np.random.default_rng(seed).uniform(-2, 2, (n, 1, 3)).astype(np.float32)
    return np.ascontiguousarray(np.repeat(p, 3, axis=1))


def collinear_exact(n=256, seed=23):
    """Three multiples of one step from one base, all small integers over 8: every difference and product is exact, the cross product
    is exactly zero."""
    rng = np.random.default_rng(seed)
    base, step = rng.integers(-64, 65, (n, 1, 3)), rng.integers(-8, 9, (n, 1, 3))
    step[(step == 0).all(axis=2)[:, 0]] = (1, -2, 3)
    m = np.stack([rng.permutation(np.arange(-3, 4))[:3] for _ in range(n)]).reshape(n, 3, 1)
    return np.ascontiguousarray(((base + m * step) / 8.0).astype(np.float32))


def collinear_rounded(n=256, seed=24):
    """Ramps in steps of 0.1 along one direction, rounded to float32: collinear up to the rounding of 0.1 * i."""
    rng = np.random.default_rng(seed)
    d = rng.integers(-3, 4, (n, 1, 3)).astype(np.float64)
    d[(d == 0).all(axis=2)[:, 0]] = (1, 2, 3)
    i = rng.integers(0, 40, (n, 1, 1)) + np.array([0, 1, 2]).reshape(1, 3, 1) * rng.integers(1, 4, (n, 1, 1))
    return np.ascontiguousarray((0.1 * i * d).astype(np.float32))


def needles(n=N_HARD, seed=25):
    """Two random vertices a, b in [-2, 2]^3 and a third on the segment between them, a + (b - a) * s rounded to float32."""
    rng = np.random.default_rng(seed)
    a, b = rng.uniform(-2, 2, (2, n, 3)).astype(np.float32).astype(np.float64)
    c = a + (b - a) * rng.uniform(0, 1, (n, 1))
    return np.ascontiguousarray(np.stack([a, b, c], axis=1).astype(np.float32))


def ladder_base():
    return well_shaped(LADDER_M, seed=26, origin=True)


def ladder():
    """ladder_base() times 2^k for every k of LADDER_K, k-major: triangle j at scale k is row (k - LADDER_K[0]) * LADDER_M + j.  The
    scaling is exact where nothing becomes subnormal."""
    base = ladder_base()
    with np.errstate(over="ignore"):                                              # (a coordinate above 1 times 2^127 is inf)
        return np.ascontiguousarray(np.concatenate([np.ldexp(base, k).astype(np.float32) for k in LADDER_K]))


def offset(n=128, seed=27):
    """Well-shaped triangles with edges around 2^-4, first at coordinates around 1e6 (one ulp there is 2^-4: the edges keep a bit or
    two), then the same triangles with x around 3e38 (one ulp is 2^101: every x is the same number, the triangle lies in a plane of
    constant x and keeps its normal and area, and the centroid's sum of three x overflows)."""
    rng = np.random.default_rng(seed)
    t = well_shaped(n, seed=seed, origin=True).astype(np.float64) / 16.0
    far = t + rng.uniform(-1, 1, (n, 1, 3)) * 1e6
    high = t + rng.uniform(-100, 100, (n, 1, 3))
    high[:, :, 0] = 3e38 * np.where(np.arange(n) % 2, -1.0, 1.0)[:, None]
    return np.ascontiguousarray(np.concatenate([far, high]).astype(np.float32))


NAN_A, NAN_B = 0x7FC00123, 0xFFC04567     # two quiet NaNs of different sign and payload


def non_finite():
    """One NaN, +inf or -inf in each of the nine coordinate slots of one benign triangle (27), then two triangles with two NaN vertices
    of different payloads."""
    base = np.array([(0.3, 0.1, -0.2), (1.1, 0.4, 0.3), (0.2, 1.3, 0.6)], np.float32)
    out = []
    for bad in (np.nan, np.inf, -np.inf):
        for slot in range(9):
            v = base.copy()
            v.reshape(-1)[slot] = bad
            out.append(v)
    for i, j in ((0, 1), (2, 0)):
        w = base.copy().view(np.uint32)
        w[i], w[j] = NAN_A, NAN_B
        out.append(w.view(np.float32))
    return np.ascontiguousarray(np.stack(out), np.float32)


def signed_zero():
    """Triangles in the three coordinate planes: the coordinate that is zero carries every pattern of +0 / -0 over the three vertices,
    the zeros inside the plane are +0 or -0, and both windings appear (96 triangles)."""
    out = []
    for axis in range(3):
        u, w = (axis + 1) % 3, (axis + 2) % 3
        for signs in range(8):
            for inner in (0.0, -0.0):
                for swap in (False, True):
                    v = np.zeros((3, 3), np.float32)
                    v[:, u], v[:, w] = (inner, 1.0, inner), (inner, inner, 1.0)
                    v[:, axis] = [-0.0 if signs >> k & 1 else 0.0 for k in range(3)]
                    out.append(v[[0, 2, 1]] if swap else v)
    return np.ascontiguousarray(np.stack(out), np.float32)


CLASSES = dict(points=points, collinear_exact=collinear_exact, collinear_rounded=collinear_rounded, needles=needles, ladder=ladder,
               offset=offset, non_finite=non_finite, signed_zero=signed_zero)
_HARD = {}


def hard(name):
    """The vertices of one class, made once (read only)."""
    if name not in _HARD:
        _HARD[name] = CLASSES[name]()
        _HARD[name].setflags(write=False)
    return _HARD[name]


def tiled(v, n=N_HARD):
    """(n, 3, 3): the class repeated until it fills n triangles."""
    return np.ascontiguousarray(np.resize(v, (n, 3, 3)))


# ---- records without a tree ---------------------------------------------------------------------------------------------------------
def records(s):
    """A Scene's primitive records as they are (no BLAS or TLAS is built: none is defined over non-finite vertices)."""
    return _view(s._lib.rth_primitives, s._h, W.Primitive)


def flip_pattern(n, every=4):
    """Every `every`-th triangle flipped: each wavefront of the vertex kernel holds both kinds."""
    return np.arange(n) % every == every - 1


def added(v, flips, material="red"):
    """A fresh Scene whose triangles are AddTriangle's of the vertices v; flips: one flipNormal for all, or one per triangle."""
    s = Scene()
    _std_materials(s)
    add(s, v, flips, material)
    return s


def add(s, v, flips, material="red"):
    v = np.ascontiguousarray(v, np.float32)
    flips = np.broadcast_to(np.asarray(flips, bool), (len(v),))
    cut = np.concatenate([[0], np.nonzero(flips[1:] != flips[:-1])[0] + 1, [len(v)]])
    for a, b in zip(cut[:-1], cut[1:]):
        s.AddTriangles(v[a:b], material, flipNormal=bool(flips[a]))


def benign(n, seed=28):
    """n well-behaved triangles (the soup of build()), the records a hard class is moved from."""
    return C._soup(np.random.default_rng(seed), n, np.full(3, -1.6), np.full(3, 1.6), 0.3)


def hard_scene(n=N_HARD):
    """One BLAS of n benign triangles, a quarter of them added with flipNormal=True: (Scene, arrays, flips)."""
    flips = flip_pattern(n)
    s = added(benign(n), flips)
    s.BuildBLAS(0)
    return s, s.arrays(bvh4=False), flips


# ---- the comparison that knows about NaN --------------------------------------------------------------------------------------------
# words of a 128-byte record that the rule computes: N.xyz, centroid.xyz, area.  v0, v1, v2 are copies; every w word is a constant 0
# (N.w: -0 after a flip) and is compared as bits with everything else.
COMPUTED = np.array([12, 13, 14, 16, 17, 18, 30])


def _words(p):
    return np.ascontiguousarray(p).view(np.uint32).reshape(-1, 32)


def same_records_nan(got, want, what):
    """same_records, but in the computed words (N.xyz, centroid.xyz, area) a NaN matches any NaN: x86 and the GPU make NaNs of different
    sign.  Everything else - the copied rows v0, v1, v2 with their NaN payloads, every w word, uv, objType, matIdx, padding - is bytes."""
    a, b = _words(got), _words(want)
    assert a.shape == b.shape, (what, a.shape, b.shape)
    ok = a == b
    fa, fb = a[:, COMPUTED].view(np.float32), b[:, COMPUTED].view(np.float32)
    ok[:, COMPUTED] |= np.isnan(fa) & np.isnan(fb)
    bad = np.nonzero(~ok.all(axis=1))[0]
    assert len(bad) == 0, (f"{what}: {len(bad)} records differ, first {bad[0]} in words {np.nonzero(~ok[bad[0]])[0].tolist()}: "
                           f"{got[bad[0]]} / {want[bad[0]]}")


def census(p):
    """How many triangle records have: a NaN in N, NaN area, area exactly 0, N exactly (+-0, +-0, +-0), an infinite computed word."""
    n, c, a = p["N"][:, :3], p["centroid"][:, :3], p["area"]
    return dict(n=len(p), nan_N=int(np.isnan(n).any(axis=1).sum()), nan_area=int(np.isnan(a).sum()), zero_area=int((a == 0).sum()),
                zero_N=int((n == 0).all(axis=1).sum()), inf_words=int((np.isinf(n).any(axis=1) | np.isinf(c).any(axis=1) | np.isinf(a)).sum()))


# ---- float64 ground truth for the well-conditioned range ----------------------------------------------------------------------------
# Measured on Scene::AddTriangle's records (the reference, g++ -O2 -ffp-contract=off) over the ladder steps 2^-20 .. 2^20 and 4,096
# triangles of well_shaped(seed=29), flipped and unflipped alike; each bound is twice the worst value seen.  The float32 evaluation
# error grows with 1 / sin of the smallest angle, which MIN_ANGLE caps.
#   | |N| - 1 |                                   1.570e-07   ->  3.14e-07
#   angle between N and the float64 normal        2.912e-07   ->  5.83e-07 rad
#   centroid, ulps of the largest coordinate      1.667       ->  3.34
#   relative area error (Heron)                   4.913e-06   ->  9.83e-06
BOUNDS = dict(unit=3.14e-07, angle=5.83e-07, centroid_ulps=3.34, area_rel=9.83e-06)
# the ladder's scales 2^k at which every triangle (edges around 2^k, smallest angle >= MIN_ANGLE) has a unit N and a finite positive area
LADDER_UNIT = (-32, 31)


def well_conditioned():
    """The triangles the float64 bounds are stated for: the ladder's steps 2^-20 .. 2^20, then 4,096 triangles of well_shaped."""
    lad = hard("ladder").reshape(len(LADDER_K), LADDER_M, 3, 3)
    zero = -LADDER_K[0]
    return np.ascontiguousarray(np.concatenate([lad[zero - 20:zero + 21].reshape(-1, 3, 3), well_shaped(4096, seed=29)]))


def truth64(v):
    """(unit normal, centroid, area) of (n, 3, 3) vertices in float64."""
    v = np.asarray(v, np.float64)
    c = np.cross(v[:, 1] - v[:, 0], v[:, 2] - v[:, 0])
    l = np.linalg.norm(c, axis=1)
    return c / l[:, None], v.mean(axis=1), 0.5 * l


def errors64(p):
    """The worst errors of triangle records against truth64 of their own vertices: | |N| - 1 |, the angle between N and the float64
    normal (radians; the flip is taken out), the centroid's error in ulps of the triangle's largest coordinate, the relative area error."""
    v = verts(p)
    n64, c64, a64 = truth64(v)
    n = p["N"][:, :3].astype(np.float64)
    n = n * np.where(is_flipped(p), -1.0, 1.0)[:, None]
    unit = np.abs(np.linalg.norm(n, axis=1) - 1.0)
    angle = np.arctan2(np.linalg.norm(np.cross(n, n64), axis=1), np.einsum("ij,ij->i", n, n64))
    big = np.abs(v).max(axis=(1, 2))
    cen = np.abs(p["centroid"][:, :3].astype(np.float64) - c64).max(axis=1) / np.spacing(big).astype(np.float64)
    area = np.abs(p["area"].astype(np.float64) - a64) / a64
    return dict(unit=float(unit.max()), angle=float(angle.max()), centroid_ulps=float(cen.max()), area_rel=float(area.max()))

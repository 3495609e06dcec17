"""Replacement geometry from vertex positions on the host (Scene.SetVertices / rth_set_vertices, rt_geometry_check): the one rule of
csrc/geometry_common.h held to Scene::AddTriangle - a scene built from moved vertices through AddTriangle gives the records that
SetVertices must produce from those vertices, byte for byte - and every refusal, after which nothing has changed; then the same
mirror at the floats' edges (geometry_check's hard classes: NaN where AddTriangle has NaN, every other word bit for bit), the
conditions that keep those classes hard, the flip that a degenerate state loses, and AddTriangle's records against float64."""
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


# ---- the rule at the floats' edges: geometry_check's hard classes ---------------------------------------------------------------------
_E = {}


def _expected(name, flip):
    """AddTriangle's records of a class (flip: one flipNormal for all), made once."""
    if (name, flip) not in _E:
        _E[name, flip] = GC.records(GC.added(GC.hard(name), flip))
        _E[name, flip].setflags(write=False)
    return _E[name, flip]


@pytest.mark.parametrize("flip", [False, True])
@pytest.mark.parametrize("name", list(GC.CLASSES))
def test_set_vertices_is_add_triangle_on_hard_inputs(name, flip):
    v, want = GC.hard(name), _expected(name, flip)
    s = GC.added(GC.benign(len(v)), flip)
    bound = GC.records(s)
    assert np.array_equal(GC.is_flipped(bound), np.full(len(v), flip))
    s.SetVertices(0, v)
    GC.same_records_nan(GC.records(s), want, f"{name}, packed")
    s.SetPrimitives(0, bound)
    s.SetVertices(0, *GC.indexed(v))                                              # indexed by bit pattern: NaNs and +-0 survive
    GC.same_records_nan(GC.records(s), want, f"{name}, indexed")
    assert np.array_equal(GC.verts(want).view(np.uint32), v.view(np.uint32))      # AddTriangle copies the vertices bit for bit
    assert np.array_equal(np.signbit(want["N"][:, 3]), np.full(len(v), flip)) and np.all(want["N"][:, 3] == 0)   # N.w: -0 after a flip
    print(name, "flipped" if flip else "unflipped", GC.census(want))


def test_the_comparison_takes_any_nan_for_a_nan_and_nothing_else():
    want = _expected("non_finite", True).copy()
    got = want.copy()
    w = got.view(np.uint32).reshape(-1, 32)
    nan = np.isnan(w[:, GC.COMPUTED].view(np.float32))
    assert nan.any(axis=0).all()                                                  # every computed word is NaN in some record
    w[:, GC.COMPUTED] = np.where(nan, w[:, GC.COMPUTED] ^ 0x80000001, w[:, GC.COMPUTED])      # other sign, other payload
    GC.same_records_nan(got, want, "NaNs of another sign and payload")
    with pytest.raises(AssertionError):
        GC.same_records(got, want, "bytes")
    for word in (0, 3, 15, 19, 20, 28, 29, 31):                                   # a copied word, w words, uv, objType, matIdx, padding
        bad = want.copy()
        bad.view(np.uint32).reshape(-1, 32)[5, word] ^= 1
        with pytest.raises(AssertionError, match=f"first 5 in words \\[{word}\\]"):
            GC.same_records_nan(bad, want, "one bit")
    k = len(want) - 1                                                             # v0 of the last record is NaN: its payload counts
    bad = want.copy()
    bad.view(np.uint32).reshape(-1, 32)[k, 0] = 0x7FC00000
    assert np.isnan(bad["v0"][k, 0]) and np.isnan(want["v0"][k, 0])
    with pytest.raises(AssertionError):
        GC.same_records_nan(bad, want, "a copied NaN")
    fin = np.nonzero(np.isfinite(want["N"][:, :3]).all(axis=1))[0]
    assert len(fin) == 0                                                          # (non_finite has no finite N; take one from the needles)
    want = _expected("needles", False)
    bad = want.copy()
    i = int(np.nonzero(np.isfinite(want["N"][:, 0]))[0][0])
    bad["N"][i, 0] = np.nan
    with pytest.raises(AssertionError):
        GC.same_records_nan(bad, want, "NaN for a number")


def test_the_classes_hit_what_they_are_there_for():
    """Conditions on AddTriangle's records, not on SetVertices': they keep the tests above from becoming vacuous."""
    def N(p):
        return p["N"][:, :3]
    p = _expected("points", False)
    assert np.isnan(N(p)).all() and np.all(p["area"] == 0)
    p = _expected("collinear_exact", False)
    assert np.isnan(N(p)).all() and (p["area"] == 0).sum() >= len(p) // 2      # (Heron's lengths are rounded: some areas are NaN or tiny)
    p = _expected("collinear_rounded", False)
    finite = np.isfinite(N(p)).all(axis=1)
    assert (finite & (p["area"] == 0)).sum() >= len(p) // 8 and np.isnan(N(p)).all(axis=1).sum() >= len(p) // 8
    p = _expected("needles", False)
    n = len(p)
    nz = np.isfinite(N(p)).all(axis=1) & (N(p) != 0).any(axis=1)
    share = dict(nan_area=np.isnan(p["area"]).sum() / n, nan_N=np.isnan(N(p)).any(axis=1).sum() / n, zero_area=(p["area"] == 0).sum() / n,
                 finite_N_zero_area=(nz & (p["area"] == 0)).sum() / n)
    print("needles", share)
    assert share["nan_area"] >= 0.05 and share["nan_N"] >= 0.05 and share["zero_area"] >= 0.5 and share["finite_N_zero_area"] >= 0.05, share
    p = _expected("offset", False)
    far, high = p[:len(p) // 2], p[len(p) // 2:]
    assert np.all(np.abs(GC.verts(far)).max(axis=(1, 2)) > 1e4) and 0 < (far["area"] == 0).sum() < len(far) // 2
    assert np.isinf(high["centroid"][:, 0]).all() and np.isfinite(N(high)).all() and np.all(np.isfinite(high["area"]) & (high["area"] > 0))
    p = _expected("non_finite", False)
    assert len(p) == 29 and np.isnan(N(p)).any(axis=1).all() and np.isnan(p["area"]).all()       # (so none of them reads as flipped)
    assert np.isinf(p["centroid"][:, :3]).any() and np.isnan(p["centroid"][:, :3]).any()
    assert {int(w) for w in p[27:].view(np.uint32).reshape(-1, 32)[:, :12].ravel()} >= {GC.NAN_A, GC.NAN_B}
    for flip in (False, True):
        p = _expected("signed_zero", flip)
        assert np.isfinite(N(p)).all() and np.all(np.abs(p["area"] - 0.5) < 1e-6)
        for rows in (N(p), p["centroid"][:, :3]):
            zero = rows == 0
            assert (zero & np.signbit(rows)).any() and (flip or (zero & ~np.signbit(rows)).any())


def _ladder_rows(p):
    return p.reshape(len(GC.LADDER_K), GC.LADDER_M)


def test_the_ladder_passes_every_regime_and_is_scale_free_between():
    p = _ladder_rows(_expected("ladder", False))
    ks = np.array(GC.LADDER_K)
    v, N, area, cen = GC.verts(p.ravel()).reshape(len(ks), GC.LADDER_M, 9), p["N"][:, :, :3], p["area"], p["centroid"][:, :, :3]
    tiny = np.float32(2.0 ** -126)
    unit = np.isfinite(N).all(axis=2) & (np.abs(np.linalg.norm(N.astype(np.float64), axis=2) - 1) < 1e-6)
    regimes = {
        "subnormal vertices and centroid": ((np.abs(v) < tiny) & (v != 0)).any(axis=2) & ((np.abs(cen) < tiny) & (cen != 0)).any(axis=2),
        "the cross product underflows: N NaN, area 0": np.isnan(N).all(axis=2) & (area == 0) & (v != 0).any(axis=2),
        "dot(cross, cross) underflows: 1 / sqrt is inf": np.isinf(N).any(axis=2) & (area == 0),
        "dot(cross, cross) is subnormal: N finite, not unit": np.isfinite(N).all(axis=2) & (N != 0).any(axis=2) & ~unit,
        "normal": unit & np.isfinite(area) & (area > 0),
        "dot(cross, cross) overflows: N 0, area inf": (N == 0).all(axis=2) & np.isinf(area),
        "the cross product overflows: N NaN": np.isnan(N).any(axis=2) & np.isfinite(v).all(axis=2) & (ks > 0)[:, None],
        "a length overflows: area NaN": np.isnan(area) & np.isfinite(v).all(axis=2),
    }
    for what, hit in regimes.items():
        k = ks[hit.any(axis=1)]
        assert len(k), what
        print(f"{what}: k = {k.min()} .. {k.max()} (all {GC.LADDER_M} triangles: {[int(x) for x in ks[hit.all(axis=1)][[0, -1]]] if hit.all(axis=1).any() else 'never'})")
    k_unit = ks[(unit & np.isfinite(area) & (area > 0)).all(axis=1)]
    assert np.array_equal(k_unit, np.arange(k_unit.min(), k_unit.max() + 1))
    print(f"a finite unit N and a finite positive area for every triangle of the ladder: k = {k_unit.min()} .. {k_unit.max()}")
    assert (k_unit.min(), k_unit.max()) == GC.LADDER_UNIT
    # between: nothing depends on the scale
    base = GC.ladder_base().astype(np.float64)
    c2 = (np.cross(base[:, 1] - base[:, 0], base[:, 2] - base[:, 0]) ** 2).sum(axis=1)        # at k = 0; times 2^4k at scale k
    zero = int(np.nonzero(ks == 0)[0][0])
    checked = 0
    for i, k in enumerate(ks):
        scale_free = (c2 * 2.0 ** (4 * int(k)) >= 2.0 ** -100) & (c2 * 2.0 ** (4 * int(k)) <= 2.0 ** 100)
        if not scale_free.any():
            continue
        checked += 1
        assert np.array_equal(N[i][scale_free].view(np.uint32), N[zero][scale_free].view(np.uint32)), k
        assert np.array_equal(np.ldexp(cen[i][scale_free], -int(k)).view(np.uint32), cen[zero][scale_free].view(np.uint32)), k
    assert checked >= 49                                                          # k = -24 .. 24 at the least


def test_records_of_well_conditioned_triangles_against_float64():
    """The constants of geometry_check.BOUNDS are twice what this test measures on AddTriangle's records; SetVertices' are held to them."""
    v = GC.well_conditioned()
    assert GC.min_angle(v).min() >= GC.MIN_ANGLE
    for flip in (False, True):
        ref = GC.errors64(GC.records(GC.added(v, flip)))
        print("AddTriangle", flip, ref)
        for k, bound in GC.BOUNDS.items():
            assert bound / 4 <= ref[k] <= bound / 2 * 1.001, (k, ref[k], bound)                 # the comment beside BOUNDS is still true
        s = GC.added(GC.benign(len(v)), flip)
        s.SetVertices(0, v)
        got = GC.errors64(GC.records(s))
        for k, bound in GC.BOUNDS.items():
            assert got[k] <= bound, (k, got[k], bound)


def _flip_sequence(through):
    """[(vertices, AddTriangle's flipNormal per triangle)] of: bound with every flip_pattern triangle flipped -> `through` -> back.  The
    documented rule: the flip is read from the bound record and is false once its N is NaN or zero, as it is after `through`."""
    n = 64
    first, flips = GC.benign(n), GC.flip_pattern(n)
    mid = GC.tiled(GC.hard(through), n)
    want_mid = GC.records(GC.added(mid, flips))
    assert (np.isnan(want_mid["N"][:, :3]).any(axis=1) | (want_mid["N"][:, :3] == 0).all(axis=1)).all() and flips.any()
    return [(first, flips), (mid, flips), (first, np.zeros(n, bool))]


@pytest.mark.parametrize("through", ["points", "non_finite"])
def test_a_flip_is_lost_through_a_degenerate_state(through):
    steps = _flip_sequence(through)
    s = GC.added(*steps[0])
    for i, (v, flips) in enumerate(steps):
        s.SetVertices(0, v)
        GC.same_records_nan(GC.records(s), GC.records(GC.added(v, flips)), f"through {through}, step {i}")
    assert not GC.is_flipped(GC.records(s)).any()


def test_a_bound_triangle_whose_cross_product_underflows_counts_as_not_flipped():
    """Edges around 1e-25: the bound cross product is (0, 0, 0) in float32, so the dot product with any N is no negative number."""
    tiny = (GC.benign(16) * np.float32(1e-25)).astype(np.float32)
    s = GC.added(tiny, True)
    bound = GC.records(s)
    assert np.isnan(bound["N"][:, :3]).all()
    n64 = GC.truth64(tiny)[0]
    assert np.isfinite(n64).all()
    bound["N"][:, :3] = -n64                                                      # a flipped unit normal, as a caller might have written it
    s.SetPrimitives(0, bound)
    assert GC.is_flipped(GC.records(s)).all()                                     # float64 calls it flipped; the rule's float32 cannot
    v = GC.benign(16, seed=30)
    s.SetVertices(0, v)
    GC.same_records_nan(GC.records(s), GC.records(GC.added(v, False)), "from a bound triangle without a cross product")

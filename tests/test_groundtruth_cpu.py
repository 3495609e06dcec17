"""The host builder and the oracle's traversal against a float64 brute-force ground truth (tests/geom64.py).

The other traversal tests compare HIP, oracle and reference with each other; all of them walk the node arrays of the same builder,
so a hit the tree loses is lost everywhere.  Here the answer comes from the primitives the test added: camera rays, bounce rays
of real frames, and adversarial sets (axis-parallel rays with signed-zero components whose origins lie exactly on box faces and
SBVH split planes, origins inside boxes / spheres / instances, far rays, directions whose reciprocal overflows) through
`Oracle.extend`; the shadow rays of real frames through `Oracle.connect`.  The HIP kernels are bit-exact with the oracle
(test_gpu_parity.py) and are checked against the same ground truth directly in test_gpu_groundtruth.py."""
import numpy as np
import pytest

import geom64 as G
from magr_ray_tracer_amd import _lib as W, scenes
from magr_ray_tracer_amd.scenes import Scene, _std_materials, box_tris, param_surface
from oracle.oracle_py import Oracle, seed_stream

WD, HD = 64, 48
FRAME = dict(shading=1, sampling=1, russian_roulette=False, filter_fireflies=True)


def _soup(rng, n, lo, hi, size):
    c = rng.uniform(lo, hi, (n, 1, 3))
    return (c + size * rng.normal(size=(n, 3, 3))).astype(np.float32)


def _lights_and_walls(gt, y):
    """A light quad (two triangles) facing down at height y, a thin wall standing right beside it and a small occluder hanging
    just below it: shadow rays that end near tmax, and walls a shadow ray grazes on its way to the light."""
    gt.light([(-1, y, -1), (1, y, -1), (1, y, 1)], "white-light")
    gt.light([(1, y, 1), (-1, y, 1), (-1, y, -1)], "white-light")
    gt.triangles(np.array([[(1.05, y - 1.5, -1), (1.05, y + 0.2, -1), (1.05, y + 0.2, 1)],
                           [(1.05, y + 0.2, 1), (1.05, y - 1.5, 1), (1.05, y - 1.5, -1)]], np.float32), "white")
    gt.triangles(np.array([[(-0.3, y - 0.02, -0.3), (0.3, y - 0.02, -0.3), (0.0, y - 0.02, 0.3)]], np.float32), "red")


def soup_scene(alpha, seed=7, spheres=0, room=False):
    """A 600-triangle random soup (extent 8), a mesh patch with shared vertices and edges, exact duplicates, lights; optional spheres,
    optionally a closed room around it all (so that nearly every ray hits: long bounce queues)."""
    rng = np.random.default_rng(seed)
    gt = G.GTScene(Scene())
    _std_materials(gt.s)
    tris = _soup(rng, 600, -4, 4, 0.45)
    gt.triangles(tris, "sand")
    gt.triangles(tris[:6], "green")              # exact duplicates: ties
    gt.triangles(param_surface(lambda U, V: (-3 + 6 * U, -3.6 + 0.3 * np.sin(5 * U) * np.cos(4 * V), -3 + 6 * V), 10, 10), "grey")
    for k in range(spheres):
        gt.sphere(rng.uniform(-3.5, 3.5, 3), rng.uniform(0.15, 0.6), ["mirror", "white-glass", "red"][k % 3])
    _lights_and_walls(gt, 4.6)
    if room:
        gt.triangles(box_tris((-7, -5, -7), (7, 7, 13)), "white")
    gt.build_blas(alpha)
    sa = gt.finish()
    view = dict(origin=(0.2, 0.3, 11.0), forward=(0.0, 0.0, 1.0), fov=62.0, aperture=0.01)
    return gt, sa, view


def rot(axis, deg):
    a = np.deg2rad(deg)
    c, s = np.cos(a), np.sin(a)
    i, j = [k for k in (0, 1, 2) if k != axis]
    R = np.eye(3)
    R[i, i], R[i, j], R[j, i], R[j, j] = c, -s, s, c
    return R


def invT(A, t):
    T = np.eye(4, dtype=np.float32)
    T[:3, :3], T[:3, 3] = A, t
    return T


TRANSFORMS = {
    "identity": None,
    "rigid": invT(rot(1, 23.0) @ rot(0, -11.0), (0.31, -0.17, 0.45)),
    "scale": invT(np.diag([1.7, 0.6, 1.15]), (0.2, 0.1, -0.3)),                    # non-uniform scale: triangles only
    "mirror": invT(rot(2, 9.0) @ np.diag([-1.0, 1.0, 1.0]), (-0.25, 0.05, 0.1)),  # negative determinant: triangles only
}


def tlas_scene(alpha=0.0, seed=11, room=False):
    """Four BLAS under a TLAS, one per kind of instance transform; spheres only under identity and rigid transforms (the kernels'
    sphere test assumes a unit D, which only those keep)."""
    rng = np.random.default_rng(seed)
    gt = G.GTScene(Scene())
    _std_materials(gt.s)
    centres = {"identity": (-2.2, 0, -1.5), "rigid": (2.0, 0.3, -1.2), "scale": (-1.8, 0.2, 2.0), "mirror": (2.1, -0.2, 1.9)}
    for b, (name, T) in enumerate(TRANSFORMS.items()):
        c = np.array(centres[name])
        gt.triangles(_soup(rng, 220, c - 1.6, c + 1.6, 0.3), ["sand", "green", "red", "white"][b])
        if name in ("identity", "rigid"):
            for k in range(4):
                gt.sphere(c + rng.uniform(-1.3, 1.3, 3), rng.uniform(0.15, 0.45), "mirror" if k % 2 else "red")
        if name == "identity":
            _lights_and_walls(gt, 4.2)
            gt.triangles(param_surface(lambda U, V: (-4 + 8 * U, -2.6 + 0.2 * np.sin(3 * U + 2 * V), -4 + 8 * V), 8, 8), "grey")
            if room:
                gt.triangles(box_tris((-7, -5, -7), (7, 7, 12)), "white")
        gt.build_blas(alpha)
    for b, (name, T) in enumerate(TRANSFORMS.items()):
        if T is not None:
            gt.s.SetInstanceTransform(b, T)
    sa = gt.finish()
    assert len(sa.blas) == 4 and np.linalg.det(sa.blas["invT"][3].reshape(4, 4)[:3, :3]) < 0
    view = dict(origin=(0.1, 0.6, 10.0), forward=(0.0, 0.05, 1.0), fov=64.0, aperture=0.01)
    return gt, sa, view


def adversarial_sets(gt, sa, accel, seed=3, n=1500):
    """The adversarial ray sets of geom64 for one scene and accel."""
    rng = np.random.default_rng(seed)
    out = {}
    sp = G.split_planes(sa)
    if sp:
        out["split planes"] = G.axis_rays_on_planes(rng, sa, sp, n)
    out["box planes"] = G.axis_rays_on_planes(rng, sa, G.box_planes(sa, accel), n)
    out["axis"] = G.axis_rays(rng, sa, n)
    out["inside boxes"] = G.inside_box_rays(rng, G.node_boxes(sa, accel), n)
    if len(sa.blas) > 1:
        out["inside instances"] = G.inside_box_rays(rng, G.tlas_leaf_boxes(sa), n)
    if any(len(st["sph_r"]) for st in gt.sets):
        out["inside spheres"] = G.inside_sphere_rays(rng, gt, n // 2)
    if not any(len(st["sph_r"]) for st in gt.sets):
        out["far"] = G.far_rays(rng, gt, n)
    out["tiny components"] = G.tiny_component_rays(rng, gt, n)
    return out


def camera_rays(o, sa, view):
    cam = scenes.camera_for(view, WD, HD)
    seeds = seed_stream(0, WD * HD)
    return o.generate(cam, 0, WD * HD, seeds), cam, seeds


def _extend(o, rays):
    r = rays.copy()
    o.extend(r)
    return r


_CACHE = {}


def _scene(key):
    if key not in _CACHE:
        kind, a = key
        _CACHE[key] = (soup_scene(a) if kind == "soup" else soup_scene(a, seed=5, spheres=18) if kind == "spheres" else
                       soup_scene(a, seed=5, spheres=4) if kind == "few spheres" else tlas_scene(a))
    return _CACHE[key]


CASES = [("soup", 0.0), ("soup", 1e-5), ("soup", 1.0), ("spheres", 0.0), ("spheres", 1.0), ("tlas", 0.0), ("tlas", 1.0)]


@pytest.mark.parametrize("accel", [W.ACCEL_BVH2, W.ACCEL_BVH4], ids=["bvh2", "bvh4"])
@pytest.mark.parametrize("case", CASES, ids=[f"{k}-alpha{a:g}" for k, a in CASES])
def test_extend_matches_float64_closest_hit(case, accel):
    """Oracle.extend over the builder's arrays returns the true closest hit on every decidable ray: hit / miss and the primitive
    exactly (a duplicate of it counts), t, u, v and the hit point within their float32 conditioning bounds."""
    gt, sa, view = _scene(case)
    o = Oracle(sa, WD, HD, accel=accel, **FRAME)
    rays, _, _ = camera_rays(o, sa, view)
    fr = {"camera": G.compare(gt, rays, _extend(o, rays), "camera", f"{case} accel {accel}: camera rays")}
    for name, rs in adversarial_sets(gt, sa, accel).items():
        fr[name] = G.compare(gt, rs, _extend(o, rs), "adversarial", f"{case} accel {accel}: {name}")
    print(case, accel, {k: round(v, 4) for k, v in fr.items()})


# (four spheres in the sphere scene of the frames: a sphere an extension ray with a non-unit D passes through is undecidable, and
# eighteen of them leave too few bounce rays decidable)
@pytest.mark.parametrize("case", [("soup", 0.0), ("few spheres", 0.0), ("tlas", 0.0)], ids=["soup-sbvh", "spheres", "tlas"])
def test_frames_bounces_and_connect_match_float64(case):
    """Real frames through the oracle (NEE, no Russian roulette, so connect runs after every bounce): the extension rays of
    bounces 1-6 as shade leaves them against the float64 closest hit, and every shadow ray's occlusion, as connect decides it,
    against the float64 any-hit (occluded iff a primitive is hit with 0 <= t < tmax)."""
    gt, sa, view = _scene(case)
    for accel in (W.ACCEL_BVH2, W.ACCEL_BVH4):
        o = Oracle(sa, WD, HD, accel=accel, **FRAME)
        rays, cam, seeds = camera_rays(o, sa, view)
        acc = np.zeros((WD * HD, 4), np.float32)
        n_shadow = n_dec = 0
        for b in range(W.MAX_BOUNCES - 1):
            got = _extend(o, rays)
            G.compare(gt, rays, got, "camera" if b == 0 else "bounce", f"{case} accel {accel}: bounce {b} rays")
            nxt, sh = o.shade(got, acc, seeds)
            if len(sh):
                eps = np.float32(W_EPS)
                org = (sh["I"] + sh["L"] * eps)[:, :3]
                tmax = sh["dist"] - np.float32(2) * eps
                occ, dec = G.any_hit(gt, org, sh["L"][:, :3], tmax)
                a = np.zeros((WD * HD, 4), np.float32)
                o.connect(sh, a)
                lit = np.any(a[sh["pixelIdx"]] != 0, axis=1)          # one shadow ray per pixel per bounce
                # a record whose radiance is zero cannot show that it was unoccluded
                pos = (sh["dotNL"] > 0) & np.all(sh["intensity"][:, :3] > 0, axis=1) & np.all(sh["BRDF"][:, :3] > 0, axis=1)
                chk = dec & pos
                bad = np.where(chk & (lit == occ))[0]
                assert len(bad) == 0, (f"{case} accel {accel} bounce {b}: {len(bad)} of {int(chk.sum())} decidable shadow rays wrong, "
                                       f"e.g. origin {org[bad[0]].tolist()} dir {sh['L'][bad[0]][:3].tolist()} tmax {tmax[bad[0]]} "
                                       f"truth occluded={occ[bad[0]]}")
                n_shadow += len(sh)
                n_dec += int(dec.sum())
                assert occ[chk].any() and (~occ[chk]).any() or len(sh) < 50
            if not len(nxt):
                break
            rays = nxt
        assert n_shadow > 500 and n_dec >= G.MIN_DECIDABLE["shadow"] * n_shadow, (n_shadow, n_dec)
        print(case, accel, "shadow rays", n_shadow, "decidable", n_dec / n_shadow)


W_EPS = 1e-4   # RT_EPSILON: a shadow ray starts at I + L * eps and ends at dist - 2 * eps (wavefront.cl:144-201)


def test_vertex_and_edge_rays_are_classified_undecidable():
    """Rays aimed at the shared vertices and edge midpoints of a mesh touch an edge: the classifier must call them undecidable
    (it is what keeps the other assertions from depending on a tie-break)."""
    gt = G.GTScene(Scene())
    _std_materials(gt.s)
    mesh = param_surface(lambda U, V: (-3 + 6 * U, 0.4 * np.sin(5 * U) * np.cos(4 * V), -3 + 6 * V), 12, 12)
    gt.triangles(mesh, "grey")
    gt.build_blas(1.0)
    gt.finish()
    rng = np.random.default_rng(1)
    rs = G.vertex_edge_rays(rng, gt, 2000, V=mesh.astype(np.float64), box=((-4, 2, -4), (4, 6, 4)))
    r = G.closest_hit(gt, rs["O"], rs["D"])
    assert (~r["decidable"]).mean() > 0.9, (~r["decidable"]).mean()


def test_sbvh_fragments_never_share_a_split_plane():
    """The builder pads the bounds of every clipped fragment outward by one ulp (accel_build.cpp, BVH2::SpatialSplit): an SBVH's
    sibling boxes never meet exactly at the split plane, where a ray with a zero direction component in that axis and its origin on the
    plane gets NaN from its slab test and is rejected by both (the reference's builder and kernels lose such hits).  Sequential and
    parallel builds produce the same arrays."""
    # a soup large enough for the parallel build (> 2048 references)
    rng = np.random.default_rng(2)
    tris = _soup(rng, 2600, -4, 4, 0.45)
    arrays = []
    for threads in (1, 4):
        s = Scene()
        _std_materials(s)
        s.AddTriangles(tris, "sand")
        s.BuildBLAS(0, 0.0, threads=threads)
        st = s.stats()
        arrays.append(s.arrays())
        assert st["spatial_splits"] > 0 and st["prims_clipped"] > 0
    assert not G.split_planes(arrays[0])
    for k in ("bvh2", "primIdx"):
        assert np.array_equal(getattr(arrays[0], k).view(np.uint8), getattr(arrays[1], k).view(np.uint8)), k

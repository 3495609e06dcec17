"""Shared pieces of the in-place resize's tests (test_resize_cpu.py, test_gpu_resize.py): scenes in the manner of refit_check.build whose
BLAS differ in their triangle, sphere and light counts and whose instances may share BLAS (Scene.AddInstance), each built from scratch on
the host with the host form of the builder a resize names - the truth a resize must reproduce, which shares no code with the device
path - and what compares a context with a fresh upload of such a scene."""
import numpy as np

import geom64 as G
import refit_check as R
import test_groundtruth_cpu as C
from magr_ray_tracer_amd import _lib as W
from magr_ray_tracer_amd.renderer import Device
from magr_ray_tracer_amd.scenes import Scene, _std_materials

Wd, Hd = 160, 120
ARRAYS = list(W.SCENE_ARRAYS) + list(W.SCENE_ARRAYS_RESIZE)
ARRAYS_BVH4 = ARRAYS + list(W.SCENE_ARRAYS_BVH4)
# name -> (Device.resize_scene keywords, Scene.BuildBLAS keywords of the builder's host form)
BUILDERS = {
    "sah": (dict(builder="sah"), dict(builder="sah_gpu", device=None)),
    "lbvh": (dict(builder="lbvh"), dict(builder="lbvh", device=None)),
    "sbvh0": (dict(builder="sbvh_gpu", alpha=0.0), dict(builder="sbvh_gpu", alpha=0.0, device=None)),
    "sbvh05": (dict(builder="sbvh_gpu", alpha=0.5), dict(builder="sbvh_gpu", alpha=0.5, device=None)),
}
VIEW = dict(origin=(0.1, 0.6, 10.0), forward=(0.0, 0.05, 1.0), fov=64.0, aperture=0.01)
LIGHT_MATS = ["white-light", "green-light", "red-light"]


def build(tris=(220,), spheres=(0,), lights=2, builder="sah", transforms=None, extra=(), floor=True, seed=11, light_blas=0):
    """One BLAS per entry of `tris`: a soup of tris[b] triangles around refit_check's b-th centre and spheres[b] spheres; BLAS
    `light_blas` also gets `lights` emissive triangles (behind its soup) and BLAS 0 the floor.  Every BLAS is built by the host form of
    `builder` (a BUILDERS name).  transforms[b]: invT of instance b (None: identity); extra: (b, invT) pairs, each a further instance
    of BLAS b (Scene.AddInstance).  Returns (gt, arrays, counts): geom64's description (it describes the scene only while `extra` is
    empty), the arrays with BVH4 and TLAS built, and the primitive count of every BLAS."""
    rng = np.random.default_rng(seed)
    gt = G.GTScene(Scene())
    _std_materials(gt.s)
    spheres = tuple(spheres) + (0,) * (len(tris) - len(spheres))
    host = BUILDERS[builder][1]
    counts = []
    for b, n in enumerate(tris):
        start = gt.s.num_prims
        c = np.array(R.CENTRES[b % len(R.CENTRES)]) + np.array([0.0, 0.0, -4.0]) * (b // len(R.CENTRES))
        if n:
            gt.triangles(C._soup(rng, n, c - 1.6, c + 1.6, 0.3), R.MATS[b % len(R.MATS)])
        for k in range(spheres[b]):
            gt.sphere(c + rng.uniform(-1.3, 1.3, 3), float(rng.uniform(0.15, 0.45)), "mirror" if k % 2 else "red")
        if b == light_blas:
            for k in range(lights):
                y, x = 4.2, -1.0 + 2.2 * k
                gt.light(np.array([(x, y, -1), (x + 2, y, -1), (x + 2, y, 1)], np.float32), LIGHT_MATS[k % len(LIGHT_MATS)])
        if b == 0 and floor:
            gt.triangles(np.array([[(-4, -2.6, -4), (4, -2.6, -4), (4, -2.6, 4)], [(4, -2.6, 4), (-4, -2.6, 4), (-4, -2.6, -4)]], np.float32), "grey")
        gt.s.BuildBLAS(start, **host)
        gt.blas.append(gt._new())
        counts.append(gt.s.num_prims - start)
    for b, T in enumerate(transforms or ()):
        if T is not None:
            gt.s.SetInstanceTransform(b, T)
    sa = gt.finish()
    if extra:
        for b, T in extra:
            gt.s.AddInstance(b, T)
        sa = gt.s.arrays()
    return gt, sa, counts


def build_runs(runs, builder="sah", seed=5):
    """One BLAS of sum(n) soup triangles, added as runs of (n, material): the lights sit exactly where the runs put them.  Returns
    (arrays, counts)."""
    rng = np.random.default_rng(seed)
    s = Scene()
    _std_materials(s)
    for n, mat in runs:
        s.AddTriangles(C._soup(rng, n, -1.5, 1.5, 0.3), mat)
    s.BuildBLAS(0, **BUILDERS[builder][1])
    return s.arrays(), [s.num_prims]


def shape_of(sa, counts):
    """(range_counts, inst_range, instances) of arrays built by build(): the ranges in the order of the roots, every instance's range."""
    roots = sorted({int(r) for r in sa.blas["bvhIdx"]})
    assert len(roots) == len(counts)
    inst_range = np.array([roots.index(int(r)) for r in sa.blas["bvhIdx"]], np.int32)
    return np.array(counts, np.int32), inst_range, sa.blas.copy()


def check_args(n_prims, counts, inst_range, instances=None, builder=W.REBUILD_SAH, opts=None):
    """rt_resize_check, the device-free argument checks of rt_resize_scene: (return code, message)."""
    L = W.device_lib()
    c = np.ascontiguousarray(counts, np.int32)
    ir = np.ascontiguousarray(inst_range, np.int32)
    b = None if instances is None else np.ascontiguousarray(instances, W.BVHInstance)
    shape = np.zeros((), W.SceneShape)
    shape["nRanges"], shape["rangeCount"] = len(c), c.ctypes.data if len(c) else 0
    shape["nBlas"], shape["instRange"] = len(ir), ir.ctypes.data if len(ir) else 0
    shape["blas"] = 0 if b is None else b.ctypes.data
    rc = L.rt_resize_check(int(n_prims), W.ptr(shape), int(builder), None if opts is None else W.ptr(opts))
    return rc, (L.rt_last_error().decode() if rc else "")


def resize(d, sa, counts, builder, prims=None, **kw):
    """Device.resize_scene (or Group's) to the scene `sa` of build(); prims: other storage of the same records (a torch tensor)."""
    rc, ir, inst = shape_of(sa, counts)
    return d.resize_scene(sa.prims if prims is None else prims, rc, ir, inst, **BUILDERS[builder][0], **kw)


def arrays(d, names=ARRAYS):
    return {k: d.scene_array(k) for k in names}


_FRESH = {}


def fresh(sa, key=None, names=ARRAYS, from_bvh2=False, **kw):
    """(arrays, kernel_info, shade_tables) of a fresh context that uploaded `sa`; key: computed once per key and shared."""
    k = None if key is None else (key, tuple(names), from_bvh2, tuple(sorted(kw.items())))
    if k is None or k not in _FRESH:
        d = Device(Wd, Hd, **kw)
        try:
            d.upload(sa, from_bvh2=from_bvh2)
            out = (arrays(d, names), d.kernel_info(), d.shade_tables())
        finally:
            d.close()
        if k is None:
            return out
        _FRESH[k] = out
    return _FRESH[k]


def same(got, want, what):
    for k in want:
        assert len(got[k]) == len(want[k]) and np.array_equal(got[k], want[k]), f"{what}: {k} differs ({len(got[k])} / {len(want[k])} bytes)"


def check(d, sa, what, key=None, names=ARRAYS, from_bvh2=False, **kw):
    """Every array, kernel_info and rt_shade_tables of `d` equal those of a fresh upload of `sa`."""
    want, info, tables = fresh(sa, key, names, from_bvh2, **kw)
    same(arrays(d, names), want, what)
    assert d.kernel_info() == info, (what, d.kernel_info(), info)
    assert d.shade_tables() == tables, (what, d.shade_tables(), tables)


def first_light_count_that_does_not_fit(capacity_rows, n_mats):
    """k_shade stages six rows per light and three per material (include/rt355.h, rt_shade_tables)."""
    return max((capacity_rows - 3 * n_mats) // 6 + 1, 0)

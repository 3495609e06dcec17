"""Shared pieces of the GPU SBVH builder's tests (test_sbvh_gpu_cpu.py, test_gpu_sbvh_build.py): the inputs, the host builder's own
figures at alpha 0 (which show that the inputs reach the spatial-split code), and the references - BVH2::BuildBLAS at 1 and 16 host
threads - each computed once per process and left unchanged."""
import functools

import numpy as np

import lbvh_check as K
import test_sah_gpu_cpu as S
from magr_ray_tracer_amd import _lib as W, scenes

ALPHAS = (0.0, 1e-5, 0.5, 1.0)
STAT_KEYS = ("depth", "sah_cost", "spatial_splits", "prims_clipped")


def mixed_no_plane():
    """lbvh_check.mixed without its plane: triangles and spheres, every ref box finite."""
    rng = np.random.default_rng(2)
    s = K._scene()
    s.AddTriangles(K._soup(rng, 300), "sand")
    for _ in range(40):
        s.AddSphere(rng.uniform(-4, 4, 3), rng.uniform(0.1, 0.7), "red")
    s.AddTriangles(K._soup(rng, 100), "green")
    return s


def spheres_300():
    """300 overlapping spheres: at alpha 0 a sphere fragment's clip comes out inverted (ClipSphereToAABB's Intersection) and the
    next spatial search computes a bin index below -1."""
    rng = np.random.default_rng(21)
    s = K._scene()
    for _ in range(300):
        s.AddSphere(rng.uniform(-4, 4, 3), rng.uniform(0.05, 0.9), "red")
    return s


# unbuilt scenes: test_sah_gpu_cpu.CASES minus mixed (its plane is refused at alpha 0), plus
INPUTS = {k: v for k, v in S.CASES.items() if k != "mixed"}
INPUTS.update({"mixed_no_plane": mixed_no_plane, "soup-5000-seed9": lambda: K.soup(5000, seed=9)})

# The host builder's own figures at alpha 0: prims, primIdx, nodes, depth, spatial splits, clipped
FIGURES = {
    "soup-600": (600, 638, 765, 12, 52, 38), "soup-5000-seed9": (5000, 9591, 11507, 20, 667, 4591),
    "wide-range": (3000, 5598, 6935, 47, 710, 2598), "signed-zero": (600, 842, 1063, 15, 82, 282), "geometric": (160, 160, 197, 21, 98, 0),
    "mixed_no_plane": (440, 457, 545, 10, 27, 17), "duplicates": (1500, 1500, 9, 3, 3, 0), "one-centroid": (4097, 4097, 1, 0, 0, 0),
}
TWO_BLAS_FIGURES = (1733, 1928, 2106, 74, 286)      # two_blas_scene(0.0): prims, primIdx, nodes, spatial splits, clipped (both BLAS)
NO_SPATIAL = ("flat-patch", "ladder")               # no spatial split at any alpha: the arrays are build_sah_gpu's


@functools.lru_cache(maxsize=None)
def prims(name):
    p = K.prims_of(INPUTS[name]())
    p.setflags(write=False)
    return p


@functools.lru_cache(maxsize=None)
def reference(name, alpha, threads):
    """(nodes, primIdx, stats) of BVH2::BuildBLAS over INPUTS[name] with bvh2->alpha = alpha."""
    s = INPUTS[name]()
    s.BuildBLAS(0, alpha=alpha, threads=threads)
    nodes, idx, _ = S.raw(s)
    for a in (nodes, idx):
        a.setflags(write=False)
    return nodes, idx, s.stats()


@functools.lru_cache(maxsize=None)
def sponza_blocks(alpha):
    """sponza_class(0.2): the factory's BLAS (one thread), then the same primitives appended as a second BLAS at 16 threads.
    Returns (prims, [(node_base, idx_base, nodes, primIdx, stats of that BLAS alone or None)])."""
    s, _ = scenes.sponza_class(0.2, alpha=alpha)
    p = K.prims_of(s)
    n1, i1, _ = S.raw(s)
    st = s.stats()
    s.BuildBLAS(0, alpha=alpha, threads=16)
    nodes, idx, blas = S.raw(s)
    assert blas["bvhIdx"][1] == len(n1)
    return p, [(0, 0, n1, i1, st), (len(n1), len(i1), nodes[len(n1):], idx[len(i1):], None)]


def _factory_at(threads, factory):
    """A scene factory's scene with every BuildBLAS it makes run at `threads` host threads (the factories take no such argument)."""
    orig = scenes.Scene.BuildBLAS

    def at_threads(self, *a, **kw):
        kw.setdefault("threads", threads)
        return orig(self, *a, **kw)
    scenes.Scene.BuildBLAS = at_threads
    try:
        return factory()
    finally:
        scenes.Scene.BuildBLAS = orig


@functools.lru_cache(maxsize=None)
def two_blas_blocks(alpha, threads=1):
    """scenes.two_blas_scene(alpha): (prims, [(first, count, node_base, idx_base, nodes, primIdx)] per BLAS, scene stats)."""
    s, _ = _factory_at(threads, lambda: scenes.two_blas_scene(alpha))
    p = K.prims_of(s)
    nodes, idx, blas = S.raw(s)
    r1 = int(blas["bvhIdx"][1])
    i1 = int(nodes["count"][:r1].sum())                       # primIdx entries of the first BLAS
    f1 = int(idx[i1:].min())                                  # first primitive of the second
    return p, [(0, f1, 0, 0, nodes[:r1], idx[:i1]), (f1, len(p) - f1, r1, i1, nodes[r1:], idx[i1:])], s.stats()


@functools.lru_cache(maxsize=None)
def config5_blocks(decimate):
    """config5_scene(0.0, decimate), built by the host at 16 threads per BLAS: (prims, blocks as two_blas_blocks, stats)."""
    s, _ = _factory_at(16, lambda: scenes.config5_scene(0.0, decimate=decimate))
    p = K.prims_of(s)
    nodes, idx, blas = S.raw(s)
    r1 = int(blas["bvhIdx"][1])
    i1 = int(nodes["count"][:r1].sum())
    f1 = int(idx[i1:].min())
    return p, [(0, f1, 0, 0, nodes[:r1], idx[:i1]), (f1, len(p) - f1, r1, i1, nodes[r1:], idx[i1:])], s.stats()


def build(p, alpha, first=0, count=None, **kw):
    """build_sbvh_gpu; for the large inputs into arrays that are large enough at once (soup-50k's tree has 15.7 nodes and 12.6 primIdx
    entries per primitive), so that the slow host restatement is not run twice by the capacity protocol, which the small inputs exercise."""
    from magr_ray_tracer_amd.scene import build_sbvh_gpu
    n = len(p) - first if count is None else count
    if n >= 20000 and alpha < 0.5:
        kw = dict(kw, nodes=np.zeros(32 * n, W.BVHNode2), idx=np.zeros(16 * n, np.uint32))
    return build_sbvh_gpu(p, alpha, first, count, **kw)


def same(got, nodes, idx, what):
    """The arrays byte for byte (w lanes and the sign of every zero included) and the counts in the stats."""
    gn, gi, st = got
    assert len(gn) == len(nodes) and np.array_equal(gn.view(np.uint8), nodes.view(np.uint8)), f"{what}: node arrays differ"
    assert np.array_equal(gi, idx), f"{what}: primIdx differs"
    assert st["nodes"] == len(nodes) and st["n_idx"] == len(idx) and st["leaves"] == int((nodes["count"] > 0).sum()), (what, st)


def same_stats(st, scene_stats, what):
    for k in STAT_KEYS:
        assert st[k] == scene_stats[k], (what, k, st[k], scene_stats[k])


def refused_call(build, p, alpha, code, frag, device=None, **kw):
    """build_sbvh_gpu raises BuildError(code) and leaves the caller's arrays (pre-filled with a sentinel) untouched."""
    from magr_ray_tracer_amd.scene import BuildError
    import pytest
    n = max(kw.get("count") or len(p), 1)
    nodes = np.zeros(2 * n + 64, W.BVHNode2)
    nodes.view(np.uint8)[:] = 0xA5
    idx = np.full(n + 64, 0xDEADBEEF, np.uint32)
    with pytest.raises(BuildError) as e:
        build(p, alpha, device=device, nodes=nodes, idx=idx, **kw)
    assert e.value.code == code and frag in str(e.value), (kw, e.value.code, str(e.value))
    assert (nodes.view(np.uint8) == 0xA5).all() and (idx == 0xDEADBEEF).all()
    return e.value


def capacity_protocol(build, p, alpha, device=None):
    """One short in either capacity: RT_E_INVALID with "capacity", the needed sizes reported, sentinel-filled arrays untouched; the
    retry with those sizes succeeds and gives the tree."""
    from magr_ray_tracer_amd.scene import BuildError
    import pytest
    ref = build(p, alpha, device=device)
    nn, ni = len(ref[0]), len(ref[1])
    for dn, di in ((1, 0), (0, 1)):
        nodes = np.zeros(nn - dn, W.BVHNode2)
        nodes.view(np.uint8)[:] = 0xA5
        idx = np.full(ni - di, 0xDEADBEEF, np.uint32)
        with pytest.raises(BuildError) as e:
            build(p, alpha, device=device, nodes=nodes, idx=idx)
        assert e.value.code == W.RT_E_INVALID and "capacity" in str(e.value) and e.value.needed == (nn, ni), (str(e.value), e.value.needed)
        assert (nodes.view(np.uint8) == 0xA5).all() and (idx == 0xDEADBEEF).all()
        nodes, idx = np.zeros(e.value.needed[0], W.BVHNode2), np.zeros(e.value.needed[1], np.uint32)
        same(build(p, alpha, device=device, nodes=nodes, idx=idx), ref[0], ref[1], "retry with the reported sizes")
    return ref

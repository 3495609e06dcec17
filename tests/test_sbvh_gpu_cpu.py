"""The GPU build of SBVH BLAS trees (rt_build_bvh2_sbvh, Scene.BuildBLAS(builder="sbvh_gpu")) through its host restatement, without a
GPU.  Its node and primIdx arrays equal what BVH2::BuildBLAS appends with alpha in {0, 1e-5, 0.5, 1} byte for byte (w lanes and the
sign of every zero included), at 1 and 16 host threads, with equal statistics (depth, cost, spatial splits, clipped primitives); the
inputs reach the spatial-split code (the host builder's own figures at alpha 0); alpha 1 is the GPU SAH builder's tree; the capacity
protocol; refusals - the new spatial bin-index rule among them, on the restatement and on the host builder - leave the caller's
arrays and the scene alone; it mixes BLAS by BLAS with the other builders."""
import numpy as np
import pytest

import lbvh_check as K
import sbvh_check as C
import test_sah_gpu_cpu as S
from magr_ray_tracer_amd import _lib as W, scenes
from magr_ray_tracer_amd.scene import build_sah_gpu, build_sbvh_gpu


@pytest.mark.parametrize("alpha", C.ALPHAS)
@pytest.mark.parametrize("name", list(C.INPUTS))
def test_restatement_equals_buildblas(name, alpha):
    p = C.prims(name)
    got = C.build(p, alpha)
    for threads in (1, 16):
        nodes, idx, st = C.reference(name, alpha, threads)
        C.same(got, nodes, idx, f"{name}, alpha {alpha}, {threads} threads")
        C.same_stats(got[2], st, f"{name}, alpha {alpha}, {threads} threads")
    s = C.INPUTS[name]()
    s.BuildBLAS(0, alpha=alpha, builder="sbvh_gpu", device=None)
    for a, b in zip(S.raw(s), (nodes, idx)):
        assert np.array_equal(a.view(np.uint8), b.view(np.uint8)), (name, alpha)
    sst = s.stats()
    assert {k: v for k, v in sst.items() if k != "build_ms"} == {k: v for k, v in st.items() if k != "build_ms"}, (name, alpha, sst, st)
    print(name, alpha, len(p), {k: got[2][k] for k in ("nodes", "n_idx", "depth", "spatial_splits", "prims_clipped", "levels", "peak_refs")})
    if alpha == 0.0 and name in C.FIGURES:
        n, n_idx, n_nodes, depth, splits, clipped = C.FIGURES[name]
        assert (len(p), len(idx), len(nodes), st["depth"], st["spatial_splits"], st["prims_clipped"]) == (n, n_idx, n_nodes, depth, splits, clipped)
        if name == "duplicates":
            assert nodes["count"].max() == 300
    if alpha == 1.0 or name in C.NO_SPATIAL:
        sah = build_sah_gpu(p)
        assert got[2]["spatial_splits"] == 0
        assert np.array_equal(got[0].view(np.uint8), sah[0].view(np.uint8)) and np.array_equal(got[1], sah[1]), (name, alpha)


@pytest.mark.parametrize("alpha", C.ALPHAS)
def test_sponza_class_and_an_appended_blas(alpha):
    """sponza_class(0.2) (the factory's BuildBLAS, one thread), then the same primitives again as a second BLAS at 16 threads: the
    restatement gives both blocks at their node and primIdx offsets."""
    p, blocks = C.sponza_blocks(alpha)
    for nb, ib, nodes, idx, st in blocks:
        got = build_sbvh_gpu(p, alpha, node_base=nb, idx_base=ib)
        C.same(got, nodes, idx, f"sponza_class(0.2), alpha {alpha}, node base {nb}")
        if st is not None:
            C.same_stats(got[2], st, f"sponza_class(0.2), alpha {alpha}")
    if alpha == 1.0:
        sah = build_sah_gpu(p)
        first = build_sbvh_gpu(p, alpha)
        assert np.array_equal(first[0].view(np.uint8), sah[0].view(np.uint8)) and np.array_equal(first[1], sah[1])
    print(alpha, len(p), {k: got[2][k] for k in ("nodes", "n_idx", "depth", "spatial_splits", "prims_clipped", "levels", "peak_refs")})


@pytest.mark.parametrize("threads", (1, 16))
@pytest.mark.parametrize("alpha", C.ALPHAS)
def test_two_blas_scene_both_blas_at_their_offsets(alpha, threads):
    p, blocks, st = C.two_blas_blocks(alpha, threads)
    got = [build_sbvh_gpu(p, alpha, first, count, node_base=nb, idx_base=ib) for first, count, nb, ib, _, _ in blocks]
    for g, (first, count, nb, ib, nodes, idx) in zip(got, blocks):
        C.same(g, nodes, idx, f"two_blas_scene({alpha}) [{first}, +{count})")
    assert sum(g[2]["spatial_splits"] for g in got) == st["spatial_splits"] and sum(g[2]["prims_clipped"] for g in got) == st["prims_clipped"]
    assert max(g[2]["depth"] for g in got) == st["depth"]
    if alpha == 0.0:
        assert (len(p), sum(len(g[1]) for g in got), sum(len(g[0]) for g in got), st["spatial_splits"], st["prims_clipped"]) == C.TWO_BLAS_FIGURES
    # the scene path: both BLAS appended by builder="sbvh_gpu" equal the factory's arrays and statistics
    r = C._factory_at(1, lambda: _two_blas_by(alpha, "sbvh_gpu"))
    h = C._factory_at(threads, lambda: _two_blas_by(alpha, "sah"))
    for a, b in zip(S.raw(r), S.raw(h)):
        assert np.array_equal(a.view(np.uint8), b.view(np.uint8))
    assert {k: v for k, v in r.stats().items() if k != "build_ms"} == {k: v for k, v in h.stats().items() if k != "build_ms"}


def _two_blas_by(alpha, builder):
    """two_blas_scene's two BuildBLAS calls made with `builder`."""
    orig = scenes.Scene.BuildBLAS

    def by(self, start, a, **kw):
        kw = dict(kw, builder=builder, device=None) if builder != "sah" else kw
        return orig(self, start, a, **kw)
    scenes.Scene.BuildBLAS = by
    try:
        return scenes.two_blas_scene(alpha)[0]
    finally:
        scenes.Scene.BuildBLAS = orig


def test_capacity_protocol():
    C.capacity_protocol(build_sbvh_gpu, C.prims("soup-600"), 0.0)
    # without arrays of its own the wrapper asks twice: the tree of soup-5000-seed9 has 9,591 primIdx entries for 5,000 primitives
    nodes, idx, st = build_sbvh_gpu(C.prims("soup-5000-seed9"), 0.0)
    assert (len(nodes), len(idx)) == (11507, 9591) and st["peak_refs"] > 5000


def _scene_unchanged(make, start_alpha, **kw):
    """A refused BuildBLAS appended to a scene that already holds a BLAS: RuntimeError, arrays and statistics as before."""
    s = K.soup(300)
    s.BuildBLAS(0, alpha=0.0)
    before, st = S.raw(s), s.stats()
    src = K.prims_of(make())
    # the refused range: the same primitives appended behind the first BLAS
    for q in src:
        if q["objType"] == W.PRIM_TRIANGLE:
            s.AddTriangle(q["v0"][:3], q["v1"][:3], q["v2"][:3], "sand")
        elif q["objType"] == W.PRIM_SPHERE:
            s.AddSphere(q["v0"][:3], q["v1"][0], "red")
        else:
            s.AddPlane((0, 1, 0), 3.0, "grey")
    with pytest.raises(RuntimeError) as e:
        s.BuildBLAS(300, alpha=start_alpha, **kw)
    for a, b in zip(S.raw(s), before):
        assert np.array_equal(a.view(np.uint8), b.view(np.uint8))
    assert s.stats() == st
    return str(e.value)


@pytest.mark.parametrize("name", ("mixed", "spheres_300"))
def test_spatial_bin_index_rule(name):
    """A ref with an empty box (mixed's plane) or an inverted one (a sphere fragment) makes scale * (x - bmin) leave what (int) and bins[]
    define as soon as a spatial split is evaluated: RT_E_UNSUPPORTED on the restatement, RuntimeError on the host builder (sequential and
    task-parallel), nothing written, the scene unchanged."""
    make = K.mixed if name == "mixed" else C.spheres_300
    p = K.prims_of(make())
    C.refused_call(build_sbvh_gpu, p, 0.0, W.RT_E_UNSUPPORTED, "bin index")
    assert "bin index" in _scene_unchanged(make, 0.0, builder="sbvh_gpu", device=None)
    for threads in (1, 16):
        assert "bin index" in _scene_unchanged(make, 0.0, threads=threads)
        s = make()
        with pytest.raises(RuntimeError):
            s.BuildBLAS(0, alpha=0.0, threads=threads)
        assert all(len(a) == 0 for a in S.raw(s))


def test_the_rule_is_lazy():
    """mixed() at alpha 0.5 never evaluates a spatial split: it builds, and equals BuildBLAS."""
    p = K.prims_of(K.mixed())
    got = build_sbvh_gpu(p, 0.5)
    for threads in (1, 16):
        s = K.mixed()
        s.BuildBLAS(0, alpha=0.5, threads=threads)
        nodes, idx, _ = S.raw(s)
        C.same(got, nodes, idx, f"mixed, alpha 0.5, {threads} threads")
        C.same_stats(got[2], s.stats(), "mixed, alpha 0.5")
    assert got[2]["spatial_splits"] == 0


def test_refusals_leave_the_arrays_and_the_scene_unchanged():
    for alpha in (0.0, 1.0):
        for name, (make, frag) in S.REFUSED.items():
            C.refused_call(build_sbvh_gpu, K.prims_of(make()), alpha, W.RT_E_UNSUPPORTED, frag)
    p = K.prims_of(K.soup(50))
    for kw, frag in S.BAD_ARGS:
        if "node_cap" not in kw:           # (the capacities have their own protocol)
            C.refused_call(build_sbvh_gpu, p, 0.0, W.RT_E_INVALID, frag, **kw)
    for alpha in (float("nan"), -0.1, 1.5):
        C.refused_call(build_sbvh_gpu, p, alpha, W.RT_E_INVALID, "alpha")
    s = K.soup(600)
    s.BuildBLAS(0)
    before, st = S.raw(s), s.stats()
    with pytest.raises(ValueError):
        s.BuildBLAS(0, alpha=0.0, threads=4, builder="sbvh_gpu", device=None)
    with pytest.raises(ValueError):
        s.BuildBLAS(0, alpha=0.0, max_leaf=4, builder="sbvh_gpu", device=None)
    with pytest.raises(RuntimeError):
        s.BuildBLAS(0, alpha=1.5, builder="sbvh_gpu", device=None)
    with pytest.raises(ValueError):
        s.BuildBLAS(0, alpha=0.5, builder="sah_gpu", device=None)          # still refused: no spatial splits there
    s.AddTriangles(K._soup(np.random.default_rng(4), 200) * np.float32(1e16), "sand")
    with pytest.raises(RuntimeError):
        s.BuildBLAS(600, alpha=0.0, builder="sbvh_gpu", device=None)
    with pytest.raises(RuntimeError):
        s.BuildBLAS(800, alpha=0.0, builder="sbvh_gpu", device=None)       # empty range
    for a, b in zip(S.raw(s), before):
        assert np.array_equal(a.view(np.uint8), b.view(np.uint8))
    assert s.stats() == st


def _three_blas(last):
    """Three BLAS over three soups: SAH, LBVH, then `last` at alpha 0, appended in turn."""
    rng = np.random.default_rng(11)
    s = scenes.Scene()
    scenes._std_materials(s)
    for k, builder in enumerate(("sah", "lbvh", last)):
        start = s.num_prims
        s.AddTriangles(K._soup(rng, 700 + 300 * k, -4 + 9 * k, 4 + 9 * k), "sand")
        if k < 2:
            s.BuildBLAS(start, builder=builder, device=None)
        else:
            s.BuildBLAS(start, alpha=0.0, builder=builder, device=None)
    return s


def test_builders_mix_blas_by_blas():
    s, r = _three_blas("sbvh_gpu"), _three_blas("sah")
    for a, b in zip(S.raw(s), S.raw(r)):
        assert np.array_equal(a.view(np.uint8), b.view(np.uint8))
    assert s.stats()["spatial_splits"] > 0 and {k: v for k, v in s.stats().items() if k != "build_ms"} == {k: v for k, v in r.stats().items() if k != "build_ms"}
    sa, ra = s.arrays(), r.arrays()
    for k in ("bvh2", "primIdx", "blas", "bvh4", "tlas"):
        assert np.array_equal(getattr(sa, k).view(np.uint8), getattr(ra, k).view(np.uint8)), k
    for accel in (W.ACCEL_BVH2, W.ACCEL_BVH4):
        assert K.validate(sa, accel) == 0, W.device_lib().rt_last_error()
        assert K.validate(ra, accel) == 0, W.device_lib().rt_last_error()


def test_factories_take_the_builder():
    s, _ = scenes.config5_scene(0.0, decimate=16, builder="sbvh_gpu", device=None)
    h, _ = scenes.config5_scene(0.0, decimate=16)
    for a, b in zip(S.raw(s), S.raw(h)):
        assert np.array_equal(a.view(np.uint8), b.view(np.uint8))
    assert s.stats()["spatial_splits"] == h.stats()["spatial_splits"] > 0
    g, _ = scenes.sponza_class(0.05, alpha=1e-5, builder="sbvh_gpu", device=None)
    h, _ = scenes.sponza_class(0.05, alpha=1e-5)
    for a, b in zip(S.raw(g), S.raw(h)):
        assert np.array_equal(a.view(np.uint8), b.view(np.uint8))

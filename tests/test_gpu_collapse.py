"""The BVH2 -> BVH4 collapse on the MI355X (rt_build_bvh4): the RtBVHNode4 array equals the host restatement's and the reference-exact
sequential collapse's (Scene.BuildBVH4, rth_bvh4_from_nodes) byte for byte, its statistics equal a numpy walk of the collapsed tree, two
runs give identical bytes, and a refusal writes nothing."""
import numpy as np
import pytest

import collapse_check as K
from magr_ray_tracer_amd import _lib as W, scenes
from magr_ray_tracer_amd.scene import BuildError, build_bvh4_gpu

pytestmark = pytest.mark.gpu

STATS = ("live_nodes", "levels", "stack_need", "largest_leaf")


def _check(n2, roots, n_idx, want, what):
    got, st = build_bvh4_gpu(n2, roots, n_idx, device=0)
    K.same_bytes(got, want, f"{what}: device")
    host, sh = build_bvh4_gpu(n2, roots, n_idx, device=None)
    K.same_bytes(host, want, f"{what}: host restatement")
    walk = K.walk(want, roots, n_idx)
    assert {k: st[k] for k in STATS} == {k: sh[k] for k in STATS} == {k: walk[k] for k in STATS}, (what, st, sh)
    again, _ = build_bvh4_gpu(n2, roots, n_idx, device=0)
    assert np.array_equal(K.raw(again), K.raw(got)), f"{what}: two runs differ"
    return st


@pytest.mark.parametrize("name", list(K.SCENES))
def test_device_collapse_equals_the_sequential_one_on_scenes(name):
    s = K.SCENES[name]()
    n2, roots, n_idx, want = K.inputs(s)
    _check(n2, roots, n_idx, want, name)
    s.BuildBVH4(builder="gpu", device=0)
    K.same_bytes(K.scene_bvh4(s), want, f"{name}: Scene.BuildBVH4('gpu')")


def test_two_instances_naming_one_root():
    n2, roots, n_idx, want = K.inputs(K.SCENES["four-blas"]())
    shared = np.array([roots[0], roots[1], roots[1], roots[2], roots[3], roots[0]], np.uint32)
    _check(n2, shared, n_idx, want, "shared root")


@pytest.mark.parametrize("name", list(K.HAND) + ["comb2(22)"])
def test_device_collapse_equals_the_sequential_one_on_hand_made_arrays(name):
    n2, n_idx = K.comb2(22) if name == "comb2(22)" else K.HAND[name]()
    st = _check(n2, [0], n_idx, K.from_nodes(n2), name)
    if name.startswith("comb2"):
        levels = int(name[6:-1])
        assert st["stack_need"] == 3 * (levels - 1) + 4          # 64 and 67: returned with the figure, it is the upload that refuses


def test_random_soups():
    rng = np.random.default_rng(11)
    for k in range(40):
        n = int(rng.integers(1, 301))
        s = K.soup_scene([n], seed=100 + k, alpha=float(rng.choice([1.0, 0.0])) if n > 8 else 1.0)
        n2, roots, n_idx, want = K.inputs(s)
        got, _ = build_bvh4_gpu(n2, roots, n_idx, device=0)
        K.same_bytes(got, want, f"soup {k} ({n} triangles)")
        s.close()


@pytest.mark.parametrize("name", ["sponza_class", "config5"])
def test_the_bench_scenes(name):
    s = scenes.sponza_class(1.0)[0] if name == "sponza_class" else scenes.config5_scene(0.0)[0]
    n2, roots, n_idx, want = K.inputs(s)
    got, st = build_bvh4_gpu(n2, roots, n_idx, device=0)
    K.same_bytes(got, want, name)
    host, sh = build_bvh4_gpu(n2, roots, n_idx, device=None)
    K.same_bytes(host, want, f"{name}: host restatement")
    assert {k: st[k] for k in STATS} == {k: sh[k] for k in STATS}
    print(f"{name}: {len(n2)} BVH2 nodes -> {st['live_nodes']} live, {st['levels']} levels, need {st['stack_need']}, device {st['device_ms']:.3f} ms")


def test_refusals_write_nothing():
    n2, n_idx = K.fixture13()
    out = np.full(len(n2) * W.BVHNode4.itemsize, 0xAB, np.uint8).view(W.BVHNode4)
    before = out.copy()
    bad = n2.copy()
    bad["first"][9] = 0xffffffff
    deep, slots = K.deep_chain(65)
    big = np.full(len(deep) * W.BVHNode4.itemsize, 0xAB, np.uint8).view(W.BVHNode4)
    for code, fragment, nodes, roots, idx, dev, o in (
            (W.RT_E_INVALID, "node 9: child index 4294967295 out of range", bad, [0], n_idx, 0, out),
            (W.RT_E_INVALID, "root 1: node 13 is out of range", n2, [0, 13], n_idx, 0, out),
            (W.RT_E_INVALID, "leaf range exceeds nIdx", n2, [0], 21, 0, out),
            (W.RT_E_INVALID, "node 1 is reachable twice", n2, [0, 1], n_idx, 0, out),
            (W.RT_E_INVALID, "count <= 0", n2, [0], 0, 0, out),
            (W.RT_E_INVALID, "device 99 out of range", n2, [0], n_idx, 99, out),
            (W.RT_E_UNSUPPORTED, "65 levels deep, at most 64", deep, [0], slots, 0, big)):
        with pytest.raises(BuildError, match=fragment) as e:
            build_bvh4_gpu(nodes, roots, idx, device=dev, out=o)
        assert e.value.code == code, (fragment, e.value.code)
        assert np.array_equal(K.raw(o[:len(before)]), K.raw(before)), f"{fragment}: the refusal wrote to out4"
    got, _ = build_bvh4_gpu(n2, [0], n_idx, device=0, out=out)       # and the same array takes a good call
    K.same_bytes(got, K.from_nodes(n2), "after the refusals")

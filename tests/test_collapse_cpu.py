"""The BVH2 -> BVH4 collapse as the GPU runs it, checked without one: the level-wise host restatement (rth_build_bvh4_levels, the rules
of csrc/collapse_common.h) against the reference-exact sequential collapse (BVH4::Convert / Collapse: Scene.BuildBVH4 and
rth_bvh4_from_nodes), RtBVHNode4 arrays byte for byte; what the upload derives from the collapsed tree (live ids, quad records, root
entries, stack need, largest leaf) against a numpy breadth-first walk; every refusal by code and message."""
import numpy as np
import pytest

import capacity_check as CC
import collapse_check as K
from magr_ray_tracer_amd import _lib as W
from magr_ray_tracer_amd.scene import BuildError, build_bvh4_gpu

_SC = {}


def _scene(name):
    if name not in _SC:
        s = K.SCENES[name]()
        _SC[name] = (s,) + K.inputs(s)
    return _SC[name]


@pytest.mark.parametrize("name", list(K.SCENES))
def test_levels_equal_the_sequential_collapse_on_scenes(name):
    s, n2, roots, n_idx, want = _scene(name)
    got, st, quads, entry, qnode = build_bvh4_gpu(n2, roots, n_idx, device=None, derived=True)
    K.same_bytes(got, want, name)
    K.check_derived(st, quads, entry, qnode, K.walk(want, roots, n_idx), name)
    # Scene.BuildBVH4(builder="gpu") with the host restatement leaves the same array in the scene
    s.BuildBVH4(builder="gpu", device=None)
    K.same_bytes(K.scene_bvh4(s), want, f"{name}: Scene.BuildBVH4('gpu')")
    s.BuildBVH4()


def test_two_instances_naming_one_root():
    """Four BLAS, five instances: the second Collapse of an already collapsed root changes nothing (the Python restatement collapses it
    twice), so the array is that of the four instances, and the live ids skip the root seen before."""
    s, n2, roots, n_idx, want = _scene("four-blas")
    shared = np.array([roots[0], roots[1], roots[1], roots[2], roots[3], roots[0]], np.uint32)
    K.same_bytes(K.recursive_collapse(n2, shared), want, "recursive restatement, a root named twice")
    got, st, quads, entry, qnode = build_bvh4_gpu(n2, shared, n_idx, device=None, derived=True)
    K.same_bytes(got, want, "shared root")
    K.check_derived(st, quads, entry, qnode, K.walk(want, shared, n_idx), "shared root")
    assert entry[1] == entry[2] and entry[0] == entry[5] == 0


def test_forty_random_soups():
    rng = np.random.default_rng(11)
    for k in range(40):
        n = int(rng.integers(1, 301))
        s = K.soup_scene([n], seed=100 + k, alpha=float(rng.choice([1.0, 0.0])) if n > 8 else 1.0)
        n2, roots, n_idx, want = K.inputs(s)
        got, st, quads, entry, qnode = build_bvh4_gpu(n2, roots, n_idx, device=None, derived=True)
        K.same_bytes(got, want, f"soup {k} ({n} triangles)")
        K.check_derived(st, quads, entry, qnode, K.walk(want, roots, n_idx), f"soup {k}")
        s.close()


@pytest.mark.parametrize("name", list(K.HAND))
def test_levels_equal_the_sequential_collapse_on_hand_made_arrays(name):
    n2, n_idx = K.HAND[name]()
    want = K.from_nodes(n2)
    K.same_bytes(K.recursive_collapse(n2, [0]), want, f"{name}: the Python restatement")
    got, st, quads, entry, qnode = build_bvh4_gpu(n2, [0], n_idx, device=None, derived=True)
    K.same_bytes(got, want, name)
    K.check_derived(st, quads, entry, qnode, K.walk(want, [0], n_idx), name)
    if name == "lattice":        # the first of equal areas: the root absorbs node 1, then node 3 (now in slot 0) before node 2
        assert got["first"][0].tolist() == [7, 2, 4, 8]
    if name == "nan-child":      # never absorbed: node 1 survives as a child of the root
        assert 1 in got["first"][0].tolist() and got["count"][0][got["first"][0].tolist().index(1)] == 0
    if name == "unreachable":    # converted like every interior record
        assert got["first"][13].tolist() == [1, 3, -1, -1] and got["count"][13].tolist() == [2, 4, -1, -1]


@pytest.mark.parametrize("levels,need", [(21, 64), (22, 67)])
def test_stack_need_on_either_side_of_the_limit(levels, need):
    """capacity_check's BVH4 comb is a collapse result: comb2(L) is a BVH2 that collapses to it.  The collapse itself returns both needs
    (it is the upload that refuses 67)."""
    n2, n_idx = K.comb2(levels)
    assert need == 3 * (levels - 1) + 4 == CC.comb(levels).need[W.ACCEL_BVH4]
    got, st = build_bvh4_gpu(n2, [0], n_idx, device=None)
    K.same_bytes(got, K.from_nodes(n2), f"comb2({levels})")
    assert st["stack_need"] == need == K.walk(got, [0], n_idx)["stack_need"]
    assert got["first"][0].tolist()[3] != -1 and (got["count"][0] == 0).all()   # four surviving children; the next level in the last slot


def _refused(code, fragment, n2, roots, n_idx, **kw):
    out = np.full(max(len(n2) if n2 is not None else 1, 1), 0xAB, np.uint8).repeat(W.BVHNode4.itemsize).view(W.BVHNode4)
    before = out.copy()
    with pytest.raises(BuildError, match=fragment) as e:
        build_bvh4_gpu(n2 if n2 is not None else np.zeros(0, W.BVHNode2), roots, n_idx, device=None, out=out, **kw)
    assert e.value.code == code, (e.value.code, str(e.value))
    assert np.array_equal(K.raw(out), K.raw(before)), "a refusal wrote to out4"


def test_refusals():
    n2, n_idx = K.fixture13()
    INVALID, UNSUP = W.RT_E_INVALID, W.RT_E_UNSUPPORTED
    _refused(INVALID, "missing array", None, [0], n_idx)
    _refused(INVALID, "missing array", n2, [], n_idx)
    _refused(INVALID, "count <= 0", n2, [0], 0)
    _refused(INVALID, "root 1: node 13 is out of range", n2, [0, 13], n_idx)
    bad = n2.copy()
    bad["first"][9] = 12                                     # first + 1 = 13 is outside
    _refused(INVALID, "node 9: child index 12 out of range", bad, [0], n_idx)
    bad = n2.copy()
    bad["first"][9] = 0xffffffff                             # first + 1 wraps to 0
    _refused(INVALID, "node 9: child index 4294967295 out of range", bad, [0], n_idx)
    more, _ = K.unreachable()
    more["first"][13] = 15                                   # an unreachable interior record is read too
    _refused(INVALID, "node 13: child index 15 out of range", more, [0], n_idx)
    _refused(INVALID, "node 11: leaf range exceeds nIdx", n2, [0], 21)
    _refused(INVALID, "node 1 is reachable twice", n2, [0, 1], n_idx)          # a root inside another BLAS
    bad = n2.copy()
    bad["first"][6] = 7                                      # node 6 names the children of node 3
    _refused(INVALID, "reachable twice", bad, [0], n_idx)
    deep, slots = K.deep_chain(65)
    _refused(UNSUP, "65 levels deep, at most 64", deep, [0], slots)
    ok, slots = K.deep_chain(64)
    got, st = build_bvh4_gpu(ok, [0], slots, device=None)
    K.same_bytes(got, K.from_nodes(ok), "a chain 64 levels deep")
    assert st["levels"] == K.walk(got, [0], slots)["levels"] == 22   # a full node of a caterpillar takes three BVH2 levels: ceil(64 / 3)

"""The in-place collapse of a refit BVH2 on the host (rth_bvh4_refit, Scene.RefitBVH4: the sequential restatement of what
rt_rebuild_scene does with RT_REBUILD_REFIT on a BVH4 copy that keeps its BVH2).  Whatever the boxes did, its array equals the
level-wise collapse of the refit BVH2 byte for byte; it reports a change exactly when the slots of a live record changed; and the two
named fixtures the GPU tests render (refit_bvh4_check.py) behave as their names say.  No GPU needed."""
import numpy as np
import pytest

import collapse_check as K
import refit_bvh4_check as F
import refit_check as R
from magr_ray_tracer_amd import _lib as W
from magr_ray_tracer_amd.scene import BuildError

BUILDERS = {"sah": ("sah", 1.0), "sbvh": ("sah", 0.0), "lbvh": ("lbvh", 1.0)}
# triangles per BLAS: a single-leaf root, a root over two leaves, small trees, about 240 leaves (400 triangles), 2 to 4 BLAS
COUNTS = ([1], [2], [3], [7], [40], [150], [400], [40, 9], [60, 1, 2, 30], [200, 50, 5])
# Vertex jitter, as a length (the triangles are about 0.3 long, a soup 2 wide).  The greedy step compares box areas, so a slot changes
# where a jitter reorders two areas: the two smaller amplitudes leave nearly every tree in place, the larger ones re-collapse about
# every other tree of a hundred leaves and more.  Tuned on the host restatement alone; the counts are asserted below.
AMPLITUDES = (1e-4, 1e-3, 1e-2, 0.05)
MIN_EACH = 20

_CASES = {}


def _fuzz():
    """Every (builder, counts, amplitude): the bound collapse, the refit BVH2, what rth_bvh4_refit made of them, the fresh collapse."""
    if not _CASES:
        k = 0
        for name, (builder, alpha) in BUILDERS.items():
            for counts in COUNTS:
                for amp in AMPLITUDES:
                    s = K.soup_scene(counts, seed=k, alpha=alpha, builder=builder)
                    n2, roots, n_idx = F.wire(s)
                    n4, _, qnode = F.collapse(n2, roots, n_idx)
                    s.SetPrimitives(0, F.jittered(s.arrays(bvh4=False).prims, amp, seed=1000 + k))
                    s.Refit()
                    n2r = F.wire(s)[0]
                    got, changed = F.bvh4_refit(n2r, roots, n_idx, n4, qnode)
                    want, _, qnode_r = F.collapse(n2r, roots, n_idx)
                    _CASES[(name, tuple(counts), amp)] = dict(n2=n2, n2r=n2r, roots=roots, n_idx=n_idx, n4=n4, qnode=qnode, got=got,
                                                               changed=changed, want=want, qnode_r=qnode_r)
                    k += 1
    return _CASES


def test_the_refit_collapse_equals_the_level_wise_collapse_byte_for_byte():
    """Live, absorbed and unreachable records alike (an absorbed node keeps Convert's record of the refit boxes)."""
    for key, c in _fuzz().items():
        assert np.array_equal(c["n2"]["first"], c["n2r"]["first"]) and np.array_equal(c["n2"]["count"], c["n2r"]["count"]), key
        K.same_bytes(c["got"], c["want"], f"{key}")


def test_a_change_is_reported_exactly_when_a_live_slot_changed():
    for key, c in _fuzz().items():
        agree = F.slots_agree(c["n4"], c["qnode"], c["want"], c["qnode_r"])
        assert (c["changed"] == 0) == agree, (key, c["changed"], agree)


def test_both_outcomes_occur_often_and_the_shapes_are_covered():
    cases = _fuzz()
    in_place = sum(1 for c in cases.values() if c["changed"] == 0 and len(c["qnode"]) > 1)
    again = sum(1 for c in cases.values() if c["changed"] > 0)
    print(f"{len(cases)} cases: {in_place} in place (more than one live node), {again} re-collapsed")
    assert in_place >= MIN_EACH and again >= MIN_EACH
    leaves = [int((c["n2"]["count"] > 0).sum()) for c in cases.values()]
    assert min(leaves) == 1 and max(leaves) >= 200
    roots = [(c["n2"], int(r)) for c in cases.values() for r in c["roots"]]
    assert any(n["count"][r] > 0 for n, r in roots), "no single-leaf root"
    assert any(n["count"][r] == 0 and n["count"][n["first"][r]] > 0 and n["count"][n["first"][r] + 1] > 0 for n, r in roots), "no root over two leaves"
    assert {len(c["roots"]) for c in cases.values()} >= {1, 2, 3, 4}
    for name in BUILDERS:
        assert any(k[0] == name and c["changed"] for k, c in cases.items()) and any(k[0] == name and not c["changed"] for k, c in cases.items()), name


def test_the_same_records_twice_stay_in_place():
    """An identical BVH2 has identical slots: the second pass changes nothing, whatever the first did."""
    for key, c in _fuzz().items():
        got, changed = F.bvh4_refit(c["n2r"], c["roots"], c["n_idx"], c["want"], c["qnode_r"])
        assert changed == 0, key
        K.same_bytes(got, c["want"], f"{key}, again")


def test_scene_refit_bvh4_follows_the_scene():
    for counts, amp in (([150], 1e-4), ([150], 0.05), ([60, 1, 2, 30], 0.05), ([1], 0.05)):
        s = K.soup_scene(counts, seed=5)
        sa = s.arrays(bvh4=True)
        n2, roots, n_idx = sa.bvh2.copy(), sa.blas["bvhIdx"].astype(np.uint32), len(sa.primIdx)
        n4, _, qnode = F.collapse(n2, roots, n_idx)
        s.SetPrimitives(0, F.jittered(sa.prims, amp, seed=6))
        s.Refit()
        in_place = s.RefitBVH4()
        n2r = F.wire(s)[0]
        got = K.scene_bvh4(s).copy()
        assert in_place == (F.bvh4_refit(n2r, roots, n_idx, n4, qnode)[1] == 0)
        K.same_bytes(got, s.arrays(bvh4=True).bvh4, f"{counts} / {amp}: Scene.RefitBVH4 against BuildBVH4")
        assert s.RefitBVH4() is True


def test_keep_is_in_place_and_flip_changes_slots_and_the_live_count():
    s, sa, _, prims = F.keep_scene(blas=2)
    roots, n_idx = sa.blas["bvhIdx"].astype(np.uint32), len(sa.primIdx)
    n4, _, qnode = F.collapse(sa.bvh2, roots, n_idx)
    first = F.host_refit(s, prims)
    n2a = first.bvh2.copy()
    n4a, _ = F.bvh4_refit(n2a, roots, n_idx, n4, qnode)
    qa = F.collapse(n2a, roots, n_idx)[2]
    second = F.host_refit(s, prims)
    assert np.array_equal(K.raw(second.bvh2), K.raw(n2a))
    got, changed = F.bvh4_refit(second.bvh2, roots, n_idx, n4a, qa)
    assert changed == 0
    K.same_bytes(got, second.bvh4, "keep")
    live = {}
    for extra in (0, 2):
        for variant in F.FLIP_VARIANTS:
            s = F.flip_scene(extra)
            n2, roots, n_idx = F.wire(s)
            root = int(roots[0])
            assert n2["count"][root] == 0 and n2["count"][n2["first"][root]] == 0 and n2["count"][n2["first"][root] + 1] == 0
            n4, st0, qnode = F.collapse(n2, roots, n_idx)
            want = F.host_refit(s, F.flip_prims(s.arrays(bvh4=False).prims, variant))
            got, changed = F.bvh4_refit(want.bvh2, roots, n_idx, n4, qnode)
            assert changed > 0, (variant, extra)
            K.same_bytes(got, want.bvh4, f"flip / {variant} / {extra} more BLAS")
            assert not np.array_equal(F.slots(n4, [root]), F.slots(got, [root])), "the root's slots stayed"
            live[(variant, extra)] = (len(qnode), F.host_live(want)[0])
    assert any(a != b for a, b in live.values()), live
    assert live[("swap", 0)][0] == live[("swap", 0)][1]            # only the order of two slots: the same live nodes


def test_refusals_leave_the_array_alone():
    s = K.soup_scene([40])
    n2, roots, n_idx = F.wire(s)
    n4, _, qnode = F.collapse(n2, roots, n_idx)
    for what, args in (("a live node out of range", (n2, roots, n_idx, n4, np.array([len(n2)], np.uint32))),
                       ("no live node", (n2, roots, n_idx, n4, np.zeros(0, np.uint32))),
                       ("a root out of range", (n2, np.array([len(n2)], np.uint32), n_idx, n4, qnode))):
        with pytest.raises(BuildError) as e:
            F.bvh4_refit(*args)
        assert e.value.code == W.RT_E_INVALID, what
    L = W.host_lib()
    assert L.rth_bvh4_refit(None, 0, 0, None, 0, None, None, 0, None) == W.RT_E_INVALID


def test_the_names_the_constants_and_the_struct_sizes():
    gt, _, _ = R.build(blas=1, spheres=2)
    L = W.host_lib()
    assert L.rth_rebuild(gt.s._h, 3, None) == W.RT_E_INVALID        # the host's refit is rth_refit
    with pytest.raises(ValueError, match="Scene.Refit"):
        gt.s.Rebuild("refit")
    from magr_ray_tracer_amd.scene import rebuild_builder
    assert rebuild_builder("refit") == W.REBUILD_REFIT == 3
    with pytest.raises(ValueError, match="alpha"):
        rebuild_builder("refit", alpha=0.5)
    with pytest.raises(ValueError, match="max_leaf"):
        rebuild_builder("refit", dict(max_leaf=4))
    assert W.RefitInfo.itemsize == 16 and W.RefitInfo.names == ("path", "live_quads", "changed_nodes", "stack_need")
    assert W.RebuildStats.itemsize == 96 and W.BVHNode4.itemsize == 160
    D = W.device_lib()
    info = np.zeros((), W.RefitInfo)
    assert D.rt_refit_info(None, W.ptr(info)) == W.RT_E_INVALID
    assert b"null argument" in D.rt_last_error()

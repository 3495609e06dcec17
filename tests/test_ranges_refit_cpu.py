"""The per-range refit (plan word "refit", RT_REBUILD_REFIT_RANGE) and the relocation rule of derived pair records on the host (no GPU):
the plan rules, the host mirror against Scene.Refit() - which the new host code does not share -, what a neighbour's refit leaves alone
on an SBVH-bound scene, and rebuild::relocated_entry against the upload's own derivation of the fully rebuilt scene.  All comparisons
are byte for byte."""
import numpy as np
import pytest

import ranges_check as RC
import ranges_refit_check as RR
import rebuild_check as RB
import refit_check as R
import test_ranges_cpu as CPU
from magr_ray_tracer_amd import _lib as W
from magr_ray_tracer_amd import scene as SC
from magr_ray_tracer_amd.scene import BuildError, blas_blocks


def test_the_word():
    assert W.REBUILD_REFIT_RANGE == 5 and SC.PLAN_WORDS["refit"] == 5
    assert list(SC.plan_words(["keep", "refit", 3, 5])) == [W.REBUILD_KEEP, 5, 3, 5]          # integers pass through unchanged


def test_the_plan_rules_take_the_refit_word():
    check = lambda *a, **kw: RC.ranges_check(258, RR.RANGES, *a, **kw)
    assert check(["keep", "refit", "keep"])[0] == 0
    assert check(["refit", 5, "refit"])[0] == 0
    assert check(["keep", "refit", "keep"], first=5, count=3)[0] == 0                          # a window inside a refit range
    assert check(["sah", "refit", "keep"], first=0, count=38)[0] == 0                          # ... across a built and a refit one
    rc, msg = check(["keep", "refit", "keep"], first=40, count=3)                              # ... in a kept one, beside a refit one
    assert rc == W.RT_E_INVALID and "intersect BLAS 2" in msg, (rc, msg)
    rc, msg = check(["refit", "refit", "keep"], first=30, count=20)
    assert rc == W.RT_E_INVALID and "intersect BLAS 2" in msg, (rc, msg)
    rc, msg = check(["keep", W.REBUILD_REFIT, "refit"])                                        # word 3 stays refused
    assert rc == W.RT_E_INVALID and "RT_REBUILD_REFIT" in msg and "plan[1]" in msg, (rc, msg)
    rc, msg = check(["keep", 6, "refit"])
    assert rc == W.RT_E_INVALID and "unknown word 6" in msg, (rc, msg)


def test_a_blas_that_is_not_compact_cannot_be_refit():
    _, holed = CPU.with_a_hole()
    flags = [int(b["compact"]) for b in blas_blocks(holed)]
    assert flags == [1, 0, 1]
    rc, msg = RC.ranges_check(258, RR.RANGES, ["keep", "refit", "keep"], compact=flags)
    assert rc == W.RT_E_UNSUPPORTED and "BLAS 1 (primitives [1, 38))" in msg and "RT_REBUILD_REFIT_RANGE" in msg, (rc, msg)
    assert RC.ranges_check(258, RR.RANGES, ["refit", "sah", "refit"], compact=flags)[0] == 0


def test_the_host_mirror_takes_the_word_and_its_refusals_change_nothing():
    s = RC.scene(first_build="sbvh")
    before = RR.snap(s.arrays(bvh4=False))
    for plan, match in ((["keep", W.REBUILD_REFIT, "refit"], "RT_REBUILD_REFIT"), (["refit", "refit"], "3 distinct BLAS"), (["refit", 6, "keep"], "unknown word 6")):
        with pytest.raises(BuildError, match=match) as e:
            s.RebuildRanges(plan)
        assert e.value.code == W.RT_E_INVALID
        RB.same_wire_arrays(s.arrays(bvh4=False), before, f"after the refused {plan}")
    s.RebuildRanges(["keep", "refit", 5])
    RC.check_wire(s.arrays(bvh4=False))


@pytest.mark.parametrize("fb", CPU.XS)
def test_refitting_every_range_is_a_refit_of_the_scene(fb):
    prims = RR.prims_of(R.jitter(0.05))
    got = RC.host_ranges(RC.scene(first_build=fb), ["refit"] * 3, prims, 0)
    RB.same_wire_arrays(got, RB.host_refit(RC.scene(first_build=fb), prims), f"{fb}: three refits")
    R.check_bounds(got, f"{fb}: three refits")


def _fixed_point(fb):
    """The trees of the SAH and the linear builder are fixed points of the refit: their boxes are the unions the refit computes."""
    s = RC.scene(first_build=fb)
    before = RR.snap(s.arrays(bvh4=False))
    s.Refit()
    RB.same_wire_arrays(s.arrays(bvh4=False), before, f"{fb}: a refit of the scene as built")


@pytest.mark.parametrize("fb", ["sah", "lbvh"])
def test_refitting_one_range_beside_kept_ones(fb):
    """Independent of the new host code: where every tree is a fixed point of the refit, a refit of the whole scene changes exactly the
    BLAS whose primitives moved."""
    _fixed_point(fb)
    prims = RR.prims_of(RC.only(1, R.jitter(0.05)))
    assert not np.array_equal(prims[1:38], RR.prims_of(R.identity)[1:38])
    got = RC.host_ranges(RC.scene(first_build=fb), ["keep", "refit", "keep"], prims[1:38], 1)
    RB.same_wire_arrays(got, RB.host_refit(RC.scene(first_build=fb), prims), f"{fb}: keep, refit, keep")


@pytest.mark.parametrize("move", list(CPU.MOVES))
@pytest.mark.parametrize("fb", ["sah", "lbvh"])
def test_a_refit_range_behind_a_rebuilt_one_moves_and_is_refit(fb, move):
    """["keep", X, "refit"] is ["keep", X, "keep"], which the builders alone pin, followed by a refit of the scene: BLAS 2 moves down in
    one case and up in the other, and the other two trees are fixed points."""
    _fixed_point(fb)
    d0, d1 = (f() for f in CPU.MOVES[move])
    x = RC.X_OF[fb]
    prims = RR.prims_of(RR.per_blas(None, d1, R.jitter(0.05)))
    s = RC.scene(RC.only(1, d0), fb)
    root0 = RC.blocks(s.arrays(bvh4=False))[2][0]
    got = RR.snap(RC.host_ranges(s, ["keep", x, "refit"], prims[1:], 1, **CPU.OPT[fb]))
    root1 = RC.blocks(got)[2][0]
    assert (root1 < root0) if move == "shrink" else (root1 > root0), (root0, root1)
    w = RC.scene(RC.only(1, d0), fb)
    w.SetPrimitives(1, prims[1:38])
    w.RebuildRanges(["keep", x, "keep"], **CPU.OPT[fb])
    w.SetPrimitives(38, prims[38:])
    w.Refit()
    RB.same_wire_arrays(got, w.arrays(bvh4=False), f"{fb} / {move}: keep, {x}, refit")
    RC.check_wire(got)


def test_a_neighbours_refit_leaves_the_clipped_boxes_of_an_sbvh_tree():
    s = RC.scene(first_build="sbvh")
    sa0 = RR.snap(s.arrays(bvh4=False))
    got = RR.snap(RC.host_ranges(s, ["keep", "refit", "keep"]))
    w = RC.scene(first_build="sbvh")
    w.Refit()
    ref = RR.snap(w.arrays(bvh4=False))
    assert np.array_equal(RR.node_bytes(got, 2), RR.node_bytes(sa0, 2)), "BLAS 2 is kept: its nodes are the bound bytes"
    assert np.array_equal(RR.node_bytes(got, 0), RR.node_bytes(sa0, 0))
    changed = (RR.node_bytes(ref, 2) != RR.node_bytes(sa0, 2)).any(axis=1).sum()
    assert changed > 0, "a refit of the whole scene was expected to replace clipped boxes of BLAS 2"
    assert np.array_equal(RR.node_bytes(got, 1), RR.node_bytes(ref, 1)), "BLAS 1 is refit: Scene.Refit()'s nodes"
    assert (RR.node_bytes(got, 1) != RR.node_bytes(sa0, 1)).any(axis=1).sum() > 0
    for k in ("prims", "primIdx"):
        assert np.array_equal(getattr(got, k), getattr(sa0, k))


LAST = [(fb, 2, m) for fb in CPU.XS for m in CPU.MOVES]   # BLAS 2 rebuilt: the only way BLAS 1's pair ids move (see keep_and_build_last)
SEEN = []


@pytest.mark.parametrize("fb,r,move", CPU.CASES + LAST, ids=[f"{a}-r{b}-{c}" for a, b, c in CPU.CASES + LAST])
def test_relocated_pair_records_are_the_derivation_of_the_rebuilt_scene(fb, r, move):
    """The block of every kept BLAS in the upload's derivation of the bound arrays, pushed through relocated_entry with the offsets of
    that BLAS, is its block in the derivation of the fully rebuilt arrays; pairNode moves by the node offset, and the root entries
    follow the same rule."""
    _, sa0, _, plan, want = CPU.keep_and_build(fb, r, move) if r < 2 else RR.keep_and_build_last(fb, move)
    sa0 = RR.snap(sa0)
    p0, n0, e0 = RR.derive_pairs(sa0)
    p1, n1, e1 = RR.derive_pairs(want)
    inst_blas = [2, 1, 0, 0]                                              # ranges_check.scene's instances
    for k in range(3):
        if plan[k] != "keep":
            continue
        (root0, m, lo0, slots), (root1, m1, lo1, slots1) = RC.blocks(sa0)[k], RC.blocks(want)[k]
        assert (m, slots) == (m1, slots1)
        (a0, cnt), (a1, cnt1) = RR.pair_run(n0, root0, m), RR.pair_run(n1, root1, m)
        assert cnt == cnt1
        pair_delta, idx_delta, node_delta = a1 - a0, lo1 - lo0, root1 - root0
        SEEN.append((pair_delta, node_delta))
        assert np.array_equal(RR.relocate_pairs(p0[a0:a0 + cnt], pair_delta, idx_delta), p1[a1:a1 + cnt]), f"pair records of BLAS {k}"
        assert np.array_equal((n0[a0:a0 + cnt].astype(np.int64) + node_delta).astype(np.uint32), n1[a1:a1 + cnt]), f"pairNode of BLAS {k}"
        for i in (i for i, b in enumerate(inst_blas) if b == k):
            rec = np.zeros((1, 4, 4), np.uint32)
            rec[0, 3, :2] = e0[i]
            assert RR.relocate_pairs(rec, pair_delta, idx_delta)[0, 3, 0] == e1[i], f"root entry of instance {i}"
            assert (e1[i] >> 31) == (1 if m == 1 else 0) and (m == 1 or e1[i] == a1)   # a leaf root's entry, or the start of the run


def test_the_cases_move_pair_ids_by_another_offset_than_nodes():
    """(after the cases above) at least one kept BLAS had a non-zero pair offset that differs from its node offset."""
    if not SEEN:
        for fb, r, move in LAST[:2]:
            test_relocated_pair_records_are_the_derivation_of_the_rebuilt_scene(fb, r, move)
    assert any(p != 0 and p != n for p, n in SEEN), SEEN

"""Per-range rebuild plans on the host (rth_rebuild_ranges, rt_rebuild_ranges_check; no GPU): a plan that builds every range is a rebuild, a
plan that keeps every range changes nothing, and - the independent oracle - keeping the BLAS that did not change and building the one
that did equals building everything, which rests on the builders alone.  All comparisons are byte for byte."""
import numpy as np
import pytest

import ranges_check as RC
import rebuild_check as RB
import refit_check as R
from magr_ray_tracer_amd import _lib as W
from magr_ray_tracer_amd.scene import BuildError, SceneArrays, blas_blocks


def test_the_host_mirror_refuses_what_the_device_refuses():
    """rth_rebuild_ranges throws under the plan rules and changes nothing."""
    s = RC.scene(first_build="sbvh")
    before = s.arrays(bvh4=False)
    for plan, code, match in ((["keep", "sah"], W.RT_E_INVALID, "3 distinct BLAS"), (["keep", 9, "keep"], W.RT_E_INVALID, "unknown word 9"),
                              (["keep", W.REBUILD_REFIT, "keep"], W.RT_E_INVALID, "RT_REBUILD_REFIT"), ([], W.RT_E_INVALID, "null plan")):
        with pytest.raises(BuildError, match=match) as e:
            s.RebuildRanges(plan)
        assert e.value.code == code
    with pytest.raises(BuildError, match="alpha") as e:
        s.RebuildRanges(["keep", "sbvh_gpu", "keep"], alpha=1.5)
    assert e.value.code == W.RT_E_INVALID
    RB.same_wire_arrays(s.arrays(bvh4=False), before, "after the refusals")

XS = list(RC.X_OF)                       # first builds, each with the plan word that builds the same trees
OPT = {"sah": {}, "lbvh": {}, "sbvh": {"alpha": 0.0}}


def _rebuilt(s, fb):
    s.Rebuild(RC.X_OF[fb], **OPT[fb])
    return s.arrays(bvh4=False)


@pytest.mark.parametrize("fb", XS)
def test_the_test_scene(fb):
    sa = RC.scene(first_build=fb).arrays(bvh4=False)
    assert RC.ranges(sa) == list(zip(RC.FIRST, RC.COUNTS))
    blk = RC.blocks(sa)
    assert blk[0][1] == 1 and sa.bvh2["count"][blk[0][0]] == 1            # BLAS 0: a leaf root, no interior node
    assert [int(r) for r in sa.blas["bvhIdx"]] == [blk[2][0], blk[1][0], blk[0][0], blk[0][0]]   # the instances name BLAS 2 first
    if fb == "sbvh":
        assert len(sa.primIdx) > len(sa.prims)                             # spatial splits: more slots than primitives
        assert blk[1][3] > RC.COUNTS[1] and blk[2][3] > RC.COUNTS[2]
    RC.check_wire(sa)


@pytest.mark.parametrize("fb", XS)
@pytest.mark.parametrize("x", XS)
def test_a_plan_that_builds_every_range_is_a_rebuild(fb, x):
    a = RC.host_ranges(RC.scene(first_build=fb), [RC.X_OF[x]] * 3, **OPT[x])
    b = _rebuilt(RC.scene(first_build=fb), x)
    RB.same_wire_arrays(a, b, f"{fb} -> all {x}")


@pytest.mark.parametrize("fb", XS)
def test_keeping_every_range_changes_nothing(fb):
    s = RC.scene(first_build=fb)
    before = s.arrays(bvh4=False)
    RB.same_wire_arrays(RC.host_ranges(s, ["keep"] * 3), before, f"{fb}: all kept")


# (bound deformation of BLAS 1, new deformation of BLAS 1): scrambled vertices make larger leaves, so the rebuilt BLAS 1 has fewer nodes
# going one way and more going the other, and BLAS 2 behind it shifts down or up
MOVES = {"shrink": (lambda: R.identity, lambda: R.scramble()), "grow": (lambda: R.scramble(), lambda: R.identity)}


def keep_and_build(fb, r, move):
    """(bound Scene, its arrays, the new primitives of range r, the plan, the arrays of a full rebuild of the deformed scene)."""
    if r == 1:
        d0, d1 = (RC.only(1, f()) for f in MOVES[move])
    else:
        d0, d1 = R.identity, RC.only(0, R.lights_moved())
    s = RC.scene(d0, fb)
    sa0 = s.arrays(bvh4=False)
    prims = RC.scene(d1, "sah").arrays(bvh4=False).prims
    full = RC.scene(d0, fb)
    full.SetPrimitives(0, prims)
    want = _rebuilt(full, fb)
    plan = ["keep"] * 3
    plan[r] = RC.X_OF[fb]
    a, n = RC.FIRST[r], RC.COUNTS[r]
    outside = np.ones(len(prims), bool)
    outside[a:a + n] = False
    assert np.array_equal(prims[outside].view(np.uint8), sa0.prims[outside].view(np.uint8)) and not np.array_equal(prims[a:a + n], sa0.prims[a:a + n])
    return s, sa0, prims[a:a + n], plan, want


CASES = [(fb, 0, "moved") for fb in XS] + [(fb, 1, m) for fb in XS for m in MOVES]


@pytest.mark.parametrize("fb,r,move", CASES, ids=[f"{a}-r{b}-{c}" for a, b, c in CASES])
def test_keeping_the_unchanged_blas_equals_rebuilding_everything(fb, r, move):
    s, sa0, window, plan, want = keep_and_build(fb, r, move)
    if r == 1:   # the rebuilt BLAS changes its node count, so BLAS 2 moves: down in one case, up in the other
        m0, m1 = RC.blocks(sa0)[1][1], RC.blocks(want)[1][1]
        assert (m1 < m0) if move == "shrink" else (m1 > m0), (m0, m1)
        assert RC.blocks(want)[2][0] != RC.blocks(sa0)[2][0]
    got = RC.host_ranges(s, plan, window, RC.FIRST[r], **OPT[fb])
    RB.same_wire_arrays(got, want, f"{fb}: keep all but range {r} ({move})")


def test_a_mixed_plan_on_the_sbvh_scene_is_a_valid_scene():
    s = RC.scene(first_build="sbvh")
    kept = RC.blocks(s.arrays(bvh4=False))[1]
    sa = RC.host_ranges(s, ["lbvh", "keep", "sah"])
    RC.check_wire(sa)
    blk = RC.blocks(sa)
    assert blk[1][1:] == (kept[1], blk[0][3], kept[3]) and kept[3] > RC.COUNTS[1]   # the kept SBVH tree: its nodes and slots, at the new bases
    assert blk[2][3] == RC.COUNTS[2]


RANGES = list(zip(RC.FIRST, RC.COUNTS))


@pytest.mark.parametrize("what,kw,match", [
    ("a null plan", dict(plan=None, n_ranges=3), "null plan"),
    ("too few words", dict(plan=["sah", "keep"]), "3 distinct BLAS"),
    ("too many words", dict(plan=["sah", "keep", "keep", "keep"]), "3 distinct BLAS"),
    ("an unknown word", dict(plan=["sah", 7, "keep"]), "unknown word 7"),
    ("a negative word", dict(plan=[-1, "keep", "keep"]), "unknown word -1"),
    ("refit in a plan", dict(plan=["keep", W.REBUILD_REFIT, "keep"]), "RT_REBUILD_REFIT"),
    ("a window inside a kept range", dict(plan=["keep", "sah", "keep"], first=40, count=3), "intersect BLAS 2"),
    ("a window that reaches into a kept range", dict(plan=["keep", "sah", "keep"], first=1, count=38), "intersect BLAS 2"),
    ("a window that starts in a kept range", dict(plan=["keep", "sah", "sah"], first=0, count=5), "intersect BLAS 0"),
    ("a window outside the primitives", dict(plan=["sah"] * 3, first=250, count=9), "outside"),
    ("a negative count", dict(plan=["sah"] * 3, first=0, count=-1), "outside"),
    ("alpha out of range", dict(plan=["keep", "sbvh_gpu", "keep"], alpha=1.5), "alpha"),
    ("alpha NaN", dict(plan=["keep", "sbvh_gpu", "keep"], alpha=float("nan")), "alpha"),
    ("a bad LBVH option", dict(plan=["keep", "lbvh", "keep"], max_leaf=0), "max_leaf"),
])
def test_ranges_check_refuses(what, kw, match):
    rc, msg = RC.ranges_check(258, RANGES, **kw)
    assert rc == W.RT_E_INVALID and match in msg, (what, rc, msg)


def test_ranges_check_accepts_and_names_a_range_that_is_not_compact():
    assert RC.ranges_check(258, RANGES, ["keep", "lbvh", "sbvh_gpu"], first=1, count=257, alpha=0.5)[0] == 0
    assert RC.ranges_check(258, RANGES, ["keep", "sah", "keep"], first=1, count=37)[0] == 0     # a window that touches only the built range
    assert RC.ranges_check(258, RANGES, ["sah", "keep", "keep"], alpha=7.0)[0] == 0             # no SBVH range: alpha is not read
    rc, msg = RC.ranges_check(258, RANGES, ["keep", "keep", "sah"], compact=[1, 0, 1])
    assert rc == W.RT_E_UNSUPPORTED and "BLAS 1 (primitives [1, 38))" in msg and "not compact" in msg, (rc, msg)
    assert RC.ranges_check(258, RANGES, ["keep", "sah", "sah"], compact=[1, 0, 1])[0] == 0


def with_a_hole(fb="sah"):
    """The test scene's arrays with an unreachable node inside BLAS 1's id interval: every node from the second node of BLAS 1 on moves
    up by one and a copy of a leaf nobody names takes the place.  A valid scene; BLAS 1 is no longer a block."""
    sa = RC.scene(first_build=fb).arrays(bvh4=False)
    root = RC.blocks(sa)[1][0]
    at = root + 1
    n = np.insert(sa.bvh2, at, sa.bvh2[RC.blocks(sa)[0][0]])
    interior = n["count"] == 0
    n["first"][interior & (n["first"] >= at)] += 1
    blas = sa.blas.copy()
    blas["bvhIdx"][blas["bvhIdx"] >= at] += 1
    return sa, SceneArrays(prims=sa.prims, mats=sa.mats, tex=sa.tex, lights=sa.lights, bvh2=n, bvh4=sa.bvh4, primIdx=sa.primIdx, tlas=sa.tlas, blas=blas)


def test_a_blas_with_an_unreachable_node_in_its_interval_cannot_be_kept():
    sa, holed = with_a_hole()
    RB.validate(holed)
    with pytest.raises(AssertionError, match="not one block"):
        RC.blocks(holed)
    assert [b["compact"] for b in blas_blocks(sa)] == [True, True, True]
    found = blas_blocks(holed)
    assert [b["compact"] for b in found] == [True, False, True]
    assert [(b["prim_first"], b["prim_count"]) for b in found] == RANGES
    assert [b["nodes"] for b in found] == [b["nodes"] for b in blas_blocks(sa)]     # the nodes it reaches, not the interval's
    flags = [int(b["compact"]) for b in found]
    rc, msg = RC.ranges_check(258, RANGES, ["keep", "keep", "keep"], compact=flags)
    assert rc == W.RT_E_UNSUPPORTED and "BLAS 1 (primitives [1, 38))" in msg, (rc, msg)
    for word in ("sah", "lbvh", "sbvh_gpu"):                                        # ... and builds fine with a builder there
        assert RC.ranges_check(258, RANGES, ["keep", word, "keep"], compact=flags)[0] == 0

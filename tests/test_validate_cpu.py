"""rt_validate_scene held to every index the kernels follow (no GPU needed).

The property: whatever rt_validate_scene accepts can be walked by every kernel and by the upload-time derivations without leaving the
arrays, without exceeding a stack and in finite time - for the reference arrays (layout 0) and for the derived records (layout 1),
since extend_variant picks the layout after validation.  wire_audit.py says what "can be walked" means, from the kernels' code alone;
validate_sweep.py mutates valid scenes one, two and three fields at a time and puts every mutant to both.

The sweep runs in a child process that logs each mutant before the library sees it: a crash of the library is a finding that names
its mutant (the first run of this module found one: rth_bvh4_from_nodes converted unreachable interior records unchecked)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import geom64 as G
import test_groundtruth_cpu as C
import validate_catalogue as K
import validate_sweep as S
import wire_audit as A
from magr_ray_tracer_amd import _lib as W, scenes
from oracle.oracle_py import Oracle

HERE = os.path.dirname(os.path.abspath(__file__))
# The sweep's size: 7 base scenes x 2 accels; per scene and accel the unmutated arrays, 8 shortened counts, every field of the sampled
# records (every record of the smallest scene) x the boundary values, and per fuzz seed (2) FUZZ_PER_PAIR = 6 draws for each of the 28
# field pairs of a BVH4 node / the 1 + 3 + 1 + 3 pairs of a BVH2, TLAS, primitive and material record plus FUZZ_TRIPLES = 150 triples;
# then the 10 scenes at and beyond the limits.  27,430 mutants when this was written; the floor below catches a sweep that lost a loop.
MIN_MUTANTS = 25000
SWEEP_TIMEOUT = 1500             # seconds; the sweep takes about 35 (a validation that walks a cycle for ever must end the test, not hang it)
# every refusal of validate_scene must be exercised (so that deleting any one check lets a mutant through to the audit)
REFUSALS = ("primIdx[", "lights[", "texture window", "tlas node : child out of range", "BLASidx out of range", "reachable twice",
            "tlas: depth", "bvhIdx out of range", "malformed BVH", "leaf range exceeds primIdx", "stack entries", "exceed the", "matIdx",
            "objType", "negative count", "bvh node  slot")


def _two_blas():
    return scenes.two_blas_scene(0.0, 8)[0].arrays()


# ---- the audit itself ---------------------------------------------------------------------------------------------------------------------
def test_audit_flags_each_access_class_it_claims_to_follow():
    """One hand-made mutant per access class, each of which the audit must name (an audit that missed a class would make the sweep's
    property vacuous for it), on arrays the audit otherwise passes."""
    sa = _two_blas()
    for accel in (0, 1):
        assert A.audit_both(sa, accel) == []
    leaf2 = int(np.where(sa.bvh2["count"] > 0)[0][0])
    inner2 = int(sa.blas["bvhIdx"][0])
    node4, slot4 = [(i, k) for i in range(len(sa.bvh4)) for k in range(4) if sa.bvh4["count"][i][k] > 0 and sa.bvh4["first"][i][k] != -1][0]
    tl = int(np.where(sa.tlas["leftRight"] != 0)[0][0])
    cases = [
        (0, [("bvh2", leaf2, "first", None, len(sa.primIdx))], "primIdx"),
        (0, [("bvh2", inner2, "first", None, len(sa.bvh2) - 1)], "nodes"),
        (0, [("bvh2", inner2, "first", None, inner2)], "termination"),
        (1, [("bvh4", node4, "first", slot4, -5)], "primIdx"),
        (1, [("bvh4", node4, "first", slot4, S.I32_MIN)], "primIdx"),
        (1, [("bvh4", node4, "count", slot4, -3), ("bvh4", node4, "first", slot4, 7000000)], "nodes"),
        (1, [("bvh4", node4, "count", slot4, 0), ("bvh4", node4, "first", slot4, int(sa.blas["bvhIdx"][0]))], "termination"),
        (0, [("tlas", tl, "leftRight", "hi", len(sa.tlas))], "tlas"),
        (0, [("tlas", tl, "leftRight", "hi", tl)], "termination"),
        (0, [("tlas", int(np.where(sa.tlas["leftRight"] == 0)[0][0]), "BLASidx", None, len(sa.blas))], "blas"),
        (0, [("blas", 1, "bvhIdx", None, len(sa.bvh2))], "nodes"),
        (0, [("primIdx", 3, None, None, len(sa.prims))], "prims"),
        (0, [("lights", 0, None, None, len(sa.prims))], "prims"),
        (0, [("prims", 0, "matIdx", None, len(sa.mats))], "mats"),
        (0, [("prims", 0, "objType", None, 3)], "objType switch"),
        (0, [("mats", int(sa.prims["matIdx"][0]), "texIdx", None, 0)], "textures"),
    ]
    for accel, muts, array in cases:
        for layout in (0, 1):
            v = A.audit(S.apply(sa, muts), accel, layout)
            names = {x.array for x in v}
            assert array in names or (layout == 1 and array == "nodes" and "newId" in names), (S.describe("two-blas", accel, muts), layout, v)
    # layout 1 alone: an unreachable slot of primIdx is read for its tri record
    unreach = S.apply(sa, [("bvh2", leaf2, "count", None, int(sa.bvh2["count"][leaf2]) - 1)] if sa.bvh2["count"][leaf2] > 1 else [])
    last = int(sa.bvh2["first"][leaf2] + sa.bvh2["count"][leaf2] - 1)
    m = S.apply(unreach, [("primIdx", last, None, None, len(sa.prims))])
    if sa.bvh2["count"][leaf2] > 1:
        assert A.audit(m, 0, 0) == [] and {x.array for x in A.audit(m, 0, 1)} == {"prims"}
    # the stacks and the 15-bit ids: the scenes beyond each limit
    for name, lim, accel, ok in S.limit_scenes():
        v = A.audit_both(lim, accel)
        assert (v == []) == ok, (name, v[:2])
        if not ok:
            assert {x.array for x in v} <= {"BLAS stack", "TLAS stack", "15-bit id"}, (name, v[:2])


# ---- the four mutants that were accepted --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("what, muts", [
    ("A: leaf slot with first = -5", lambda i, k: [("bvh4", i, "first", k, -5)]),
    ("A2: leaf slot with first = INT32_MIN", lambda i, k: [("bvh4", i, "first", k, S.I32_MIN)]),
    ("B: unused slot turned into first = 5,000,000, count = -7", None),
    ("B2: leaf slot turned into count = -3, first = 7,000,000", lambda i, k: [("bvh4", i, "count", k, -3), ("bvh4", i, "first", k, 7000000)]),
])
def test_bvh4_slots_that_are_neither_unused_nor_leaf_nor_child_are_refused(what, muts):
    """A BVH4 slot is unused iff first == -1; a used slot needs count >= 0 and first >= 0; count > 0 is a leaf inside primIdx, count == 0
    a child inside the node array.  traverse_bvh4 reads primIdx[first + j] of the first two on the GPU and pushes `first` of the last
    two as a node id; the layout-1 derivation wrote newId[first] on the host.  All four were accepted before the rule."""
    sa = _two_blas()
    leaf = [(i, k) for i in range(len(sa.bvh4)) for k in range(4) if sa.bvh4["count"][i][k] > 0 and sa.bvh4["first"][i][k] != -1][0]
    free = [(i, k) for i in sorted(S.topology(sa, 1)["bvh4"]) for k in range(4) if sa.bvh4["first"][i][k] == -1][0]     # of a reachable node
    m = muts(*leaf) if muts else [("bvh4", free[0], "first", free[1], 5000000), ("bvh4", free[0], "count", free[1], -7)]
    rc, msg = S.validate(S.apply(sa, m), 1)
    node, slot = m[0][1], m[0][3]
    assert rc == W.RT_E_INVALID and f"bvh4 node {node} slot {slot}" in msg, (what, rc, msg)
    assert A.audit_both(S.apply(sa, m), 1) != []


# ---- the sweep ----------------------------------------------------------------------------------------------------------------------------
def test_whatever_validation_accepts_the_audit_passes(tmp_path):
    """The mutation sweep and fuzz (validate_sweep.py) in a child process.  Accepted => audit empty under both layouts; refused =>
    RT_E_INVALID or RT_E_UNSUPPORTED with a message; the unmutated scenes and the scenes at a limit are accepted; rt_blas_ranges and
    rth_bvh4_from_nodes return on every BVH2 mutant.  A mutant the audit calls safe but validation refuses is counted and printed."""
    log, res = tmp_path / "mutants.log", tmp_path / "result.json"
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([p for p in sys.path if p]))
    tail = lambda: log.read_text().splitlines()[-1:] if log.exists() else ["(nothing logged)"]
    try:
        p = subprocess.run([sys.executable, os.path.join(HERE, "validate_sweep.py"), str(log), str(res)], env=env, capture_output=True, text=True,
                           timeout=SWEEP_TIMEOUT)
    except subprocess.TimeoutExpired:
        pytest.fail(f"the sweep did not end within {SWEEP_TIMEOUT} s (validation walking a cycle?); last mutant: {tail()}")
    last = tail()
    assert p.returncode == 0, f"the sweep's child process ended with status {p.returncode}; last mutant: {last}\n{p.stderr[-2000:]}"
    r = json.loads(res.read_text())
    print(f"{r['mutants']} mutants in {r['seconds']} s: {r['accepted']} accepted, {r['refused']} refused, of those {r['over_refused']} "
          f"the audit calls safe (unreachable or unreferenced records, shared TLAS children: not failures); per scene {r['per_scene']}")
    for line in r["over_refused_examples"][:10]:
        print("  refused though safe:", line)
    assert r["failures"] == [], f"{len(r['failures'])} failures, e.g.\n" + "\n".join(r["failures"][:12])
    assert r["mutants"] >= MIN_MUTANTS, r["mutants"]
    for key in REFUSALS:
        assert any(key in m for m in r["refusal_messages"]), f"no mutant was refused with {key!r}: {sorted(r['refusal_messages'])}"


# ---- the catalogue ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(K.CATALOGUE))
def test_catalogue_entries_are_accepted_audited_and_decidable(name):
    """Every odd-but-legal scene of validate_catalogue: accepted, audit empty, and - with the oracle in place of the kernels - its
    camera rays and the extension rays of bounces 1 and 2 (or the tree's own rays) on the float64 closest hit, above geom64's
    decidability floors.  test_gpu_validate.py asks the same of the kernels."""
    e = K.entry(name)
    for accel in e.accels:
        rc, msg = S.validate(e.sa, accel)
        assert rc == W.RT_OK, (name, accel, msg)
        assert A.audit_both(e.sa, accel) == [], (name, accel)
        o = Oracle(e.sa, C.WD, C.HD, accel=accel, **C.FRAME)
        if e.view is None:
            assert G.compare(e.gt, e.rays, C._extend(o, e.rays), "adversarial", f"{name} accel {accel}") == 1.0
            continue
        rays, cam, seeds = C.camera_rays(o, e.sa, e.view)
        acc = np.zeros((C.WD * C.HD, 4), np.float32)
        for b in range(3):
            got = C._extend(o, rays)
            fr = G.compare(e.gt, rays, got, "camera" if b == 0 else "bounce", f"{name} accel {accel}: bounce {b}")
            print(name, accel, "bounce", b, len(rays), "rays, decidable", round(fr, 4), "hits", int((got["primIdx"] != -1).sum()))
            rays, _ = o.shade(got, acc, seeds)
            assert len(rays) > 100, (name, b)


def test_a_shared_bvh2_subtree_is_accepted_until_the_visit_budget_runs_out():
    """bvh2_depth follows every path and gives up after 2 * nNodes + 2 visits, so sharing is accepted while the walk stays within that:
    the ladder whose levels share their children has 2 L + 1 nodes and 2^(L + 1) - 1 visits - L = 3: 15 <= 16, accepted; L = 4:
    31 > 20, refused as malformed although every walk is finite (the audit passes it: an over-refusal, by design of the budget)."""
    ok, over = K.shared_ladder(3), K.shared_ladder(4)
    assert S.validate(ok.sa, 0)[0] == W.RT_OK and A.audit_both(ok.sa, 0) == []
    rc, msg = S.validate(over.sa, 0)
    assert rc == W.RT_E_INVALID and "malformed BVH" in msg, (rc, msg)
    assert A.audit_both(over.sa, 0) == []


def test_debug_set_rays_refuses_without_a_context():
    """The argument checks that need no device (the band and primitive-range checks: test_gpu_validate.py)."""
    lib = W.device_lib()
    r = G.make_rays(np.zeros((1, 3), np.float32), np.ones((1, 3), np.float32))
    assert lib.rt_debug_set_rays(None, 0, W.ptr(r), 1) == W.RT_E_INVALID and b"rt_debug_set_rays" in lib.rt_last_error()

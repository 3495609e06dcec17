"""Shared pieces of the tests of k_trace_persist4_tlas (test_bvh4_tlas_cpu.py, test_gpu_bvh4_tlas.py): BVH4 combs of ANY stack need under
a caterpillar TLAS, the column sizes the selection goes by, and a stage-by-stage comparison of two contexts.

  tlas_comb(d, need)   d + 1 instances, each its own BVH4 comb written directly (capacity_check.comb's tree with a last level of 1 - 4
                       stubs, so that every need >= 1 has a comb), under capacity_check.tlas_chain's TLAS of depth d: instance 0 lies
                       deepest and is entered first, with d TLAS siblings pending under its `need` BVH4 entries (push all, pop one).
                       One ray per small triangle; one instance is turned by 180 degrees.  fat = m: the first stub's leaf of instance 0
                       holds m triangles.
  The occupancy model is capacity_check.occupancy: its `pending` is the tagged column of a lane - for a ray inside an instance the
  pending TLAS siblings (<= tlasDepth) plus the BVH4 entries (every hit interior child pushed at the visit, one popped)."""
import numpy as np

import capacity_check as CC
import collapse_check as KC
import geom64 as G
import test_groundtruth_cpu as C
import validate_catalogue as K
from helpers import bits_equal
from magr_ray_tracer_amd import _lib as W

B2, B4 = W.ACCEL_BVH2, W.ACCEL_BVH4
FIT_SEVEN = 22          # rt355.hip kFitSeven: a column of more entries (TLAS part included) spills by default
BACKUP_WORDS = 10       # the world ray, its reciprocal direction and the TLAS level's tLight, behind the column
SPILL_CAP = 12          # LDS entries of a spilling column by default (kFitSeven - kBackupWords)
LIGHT_ABOVE = 0.3       # frame combs: the light hangs this far above the last stub of the top instance
FRAME_GAP = 1.2         # frame combs: free height between two instances (the TLAS orders them by entry distance, MIN_MARGIN apart)
STAGE_COUNTERS = ("rays", "tlas_visits", "inst_visits", "node_visits", "prim_tests")


def column_entries(need, depth):
    """tlas_stack_entries of rt355.hip: the context's BLAS column (clamp(need + 1, 6, 64)), the TLAS siblings and one."""
    return CC.stack_entries(need) + depth + 1


def need_for_column(entries, depth):
    """The comb need whose column has exactly `entries` entries under a TLAS of `depth` levels."""
    need = entries - depth - 2
    assert CC.STACK_MIN <= need + 1 < CC.STACK_MAX and column_entries(need, depth) == entries
    return need


def lds_entries_admitted(shared_bytes):
    """The longest column that, with its backup words, fits the dynamic LDS a workgroup may ask for (256 lanes x 4 bytes per entry)."""
    return shared_bytes // 1024 - BACKUP_WORDS


def comb_levels(need):
    """(levels, stubs of the last level): need = 3 (levels - 1) + stubs, 1 <= stubs <= 4."""
    levels = max(1, -(-(need - 1) // 3))
    return levels, need - 3 * (levels - 1)


def _comb_block(gt, need, fat=None, dz=1.0, receiver=False, light=False):
    """Add one comb's primitives (stub p holds the small triangle of cell p at z = p dz) and write its BVH4 nodes with local ids.
    receiver: stub 0's leaf - the entry pushed first and popped last - also holds a diffuse quad GUARD below its triangle, which moves
    onto the camera's axis (the guard), and the triangle of the last stub - pushed last - swaps cells with the one on the axis.
    light: the last stub's leaf also holds a light quad above the comb.  Returns (nodes, primitive ids, primitive count, z range)."""
    levels, tail = comb_levels(need)
    assert 1 <= tail <= 4 and 3 * (levels - 1) + tail == need
    rows = -(-(need + (fat or 1) - 1) // 9)
    ymid, yhalf = 0.5 * (rows - 1), max(4.5, 0.5 * rows)
    axis = 9 * int(np.floor(ymid)) + 4
    swap = {need - 1: axis, axis: need - 1} if receiver and 0 < axis < need - 1 else {}
    ids, slots, zr, g, f0 = [], [], [], 0, gt.s.num_prims
    for p in range(need):
        first, z0, z1 = gt.s.num_prims, p * dz, p * dz
        for _ in range(fat if fat and p == 0 else 1):
            ids.append(gt.s.num_prims)
            tri = CC._small(swap.get(p, g), p * dz)
            if receiver and p == 0:            # between four cells, on the camera's axis
                tri[:, :2] += (4.5, np.floor(ymid) + 0.5)
            gt.triangles(tri[None], "red" if receiver and p == 0 else "sand")
            g += 1
        if receiver and p == 0:
            z0 -= CC.GUARD
            gt.triangles(CC._quad(-0.5, ymid - yhalf, 8.5, ymid + yhalf, z0, True), "sand")
        if light and p == need - 1:
            z1 += LIGHT_ABOVE
            for t in CC._quad(-0.5, ymid - yhalf, 8.5, ymid + yhalf, z1, False):
                gt.light(t, "white-light")
        slots.append((first - f0, gt.s.num_prims - first))
        zr.append((z0, z1))
    n = np.zeros(4 * (levels - 1) + 1 + tail, W.BVHNode4)
    n["first"][:], n["count"][:] = -1, -1

    def box(i, k, z0, z1):
        n["aabbMin"][i][k][:3] = (-CC.XY, -CC.XY, z0 - CC.PAD)
        n["aabbMax"][i][k][:3] = (CC.XY, CC.XY, z1 + CC.PAD)
    p = 0
    for l in range(levels):
        m = 4 * l
        for s in range(3 if l < levels - 1 else tail):
            st = m + 1 + s
            n["first"][m][s], n["count"][m][s] = st, 0
            n["first"][st][0], n["count"][st][0] = slots[p]
            box(m, s, *zr[p]), box(st, 0, *zr[p])
            p += 1
        if l < levels - 1:
            n["first"][m][3], n["count"][m][3] = m + 4, 0
            box(m, 3, zr[p][0], zr[-1][1])
    assert p == need
    return n, np.array(ids), gt.s.num_prims - f0, (zr[0][0], zr[-1][1])


def tlas_comb(d, need, fat=None, frame=False):
    """capacity_check.tlas_chain over combs (BVH4 only; the BVH2 array is a dummy, as in capacity_check.comb).  frame = True: the
    stubs lie capacity_check.DZ apart (a comb decides no order by distance, and the float64 bound of a shadow ray's t grows with the
    scene's extent), all instances share one lateral band, instance 0 holds the receiver and instance d the light: the shadow rays of
    bounce 0 start in instance 0's first stub and run towards +z across every stub box of every instance, so under connect - near TLAS
    child first, push all and pop one - each of them holds d TLAS siblings and `need` BVH4 entries in instance 0."""
    assert d >= 1 and (not frame or (d >= 2 and d % 2 == 0 and not fat))
    n, dz = d + 1, (CC.DZ if frame else 1.0)
    top = dz * (need - 1)
    rows, S, tpad = -(-(need + (fat or 1) - 1) // 9), (top + FRAME_GAP if frame else need + 3.0), (0.1 if frame else 0.5)
    gt = CC._gt()
    blocks, counts, idss, zrs = [], [], [], []
    for i in range(n):
        blk, ids, cnt, zr = _comb_block(gt, need, fat if i == 0 else None, dz, frame and i == 0, frame and i == d)
        gt.build_blas(1.0)
        blocks.append(blk), counts.append(cnt), idss.append(ids), zrs.append(zr)
    turned = max(1, d // 2)
    # (a frame keeps instance d, the light's, untransformed: light sampling reads the light's own vertices)
    zof = lambda i: float((i - d if frame else i) * S)
    for i in range(n):
        off = np.array([0.5 * (i % 2), 0.0 if frame else i * (rows + 1.0), zof(i)])
        T = np.eye(4, dtype=np.float32)
        if i == turned:          # local = diag(1, -1, -1) world + t: the band and the z range stay where a translation would put them
            T[1, 1] = T[2, 2] = -1.0
            T[:3, 3] = (-off[0], off[1] + rows - 1.0, off[2] + top)
        else:
            T[:3, 3] = -off
        gt.s.SetInstanceTransform(i, T)
    sa = gt.finish()
    CC._install(sa, None, blocks, counts)
    sa.bvh2 = np.zeros(len(sa.bvh4), W.BVHNode2)
    t = np.zeros(2 * n, W.TLASNode)

    def box(i, z0, z1):
        t["aabbMin"][i][:3] = (-CC.XY, -CC.XY, z0 - tpad)
        t["aabbMax"][i][:3] = (CC.XY, CC.XY, z1 + tpad)
    for i in range(n):
        t["BLASidx"][1 + i] = i
        box(1 + i, zof(i) + zrs[i][0], zof(i) + zrs[i][1])
    J = lambda k: 0 if k == 0 else n + k
    for k in range(d):
        t["leftRight"][J(k)] = (J(k + 1) if k + 1 < d else 1) + ((1 + d - k) << 16)
        box(J(k), zof(0) + zrs[0][0], zof(d - k) + zrs[d - k][1])
    sa.tlas = t
    gt._cache = {}
    V, I = G.world_triangles(gt)
    ids = np.concatenate(idss)
    at = np.searchsorted(I, ids)
    assert np.array_equal(I[at], ids)
    c = CC.Case(f"tlas_comb({d}, {need}{', fat=%d' % fat if fat else ''}{', frame' if frame else ''})", gt, sa,
                CC._aim(V[at].mean(1), zof(0) + 0.05 - CC.GUARD if frame else -1.0), ids, {B4: need}, depth=d)
    if fat:
        c.fat = np.arange(fat)
    if frame:                    # the camera: 0.9 in front of the receiver, looking at it (a camera looks along -forward)
        c.view = dict(origin=(4.0, 0.5 * (rows - 1), zof(0) + 0.9 - CC.GUARD), forward=(0.0, 0.0, 1.0), fov=100.0, aperture=0.01)
        c.info.update(guard=int(idss[0][0]), last=int(idss[0][-1]))
    return c


def shadow_rays(rec_I, rec_L, dist):
    """Origin, direction and tmax of the shadow rays connect traces for the oracle's shadow records."""
    eps = np.float32(C.W_EPS)
    return (rec_I + rec_L * eps)[:, :3], rec_L[:, :3], dist - np.float32(2) * eps


def shadow_occupancy(c, org, L, tmax, n=100):
    """capacity_check.occupancy in connect's order (any-hit: near TLAS child first, every hit interior child of a quad pushed, one
    popped) over n evenly spaced shadow rays: the fullest column holds need + depth entries, the model's verdict is the float64 one.
    Returns (how many rays reached need + depth, of how many)."""
    want = c.need[B4] + c.depth
    pick = np.unique(np.linspace(0, len(org) - 1, n).astype(np.int64))
    m = [CC.occupancy(c.sa, B4, org[i], L[i], True, tmax[i]) for i in pick]
    pend = np.array([x["pending"] for x in m])
    assert pend.max() == want and max(x["tlas"] for x in m) == c.depth and max(x["blas"] for x in m) == c.need[B4], (c.name, pend.max(), want)
    assert min(x["margin"] for x in m) >= CC.MIN_MARGIN, c.name
    occ, dec = G.any_hit(c.gt, org[pick], L[pick], tmax[pick])
    assert np.array_equal(np.array([x["hit"] for x in m])[dec], occ[dec]), c.name
    return int((pend == want).sum()), len(pick)


def same_stage(a, b, bounce, what, steps=True):
    """Two contexts after the same stage_extend: hit records and `steps` bit for bit."""
    ra, rb = a.get_rays(bounce), b.get_rays(bounce)
    assert len(ra) == len(rb), (what, len(ra), len(rb))
    for f in ra.dtype.names:
        assert bits_equal(ra[f], rb[f]), f"{what}: rays differ in {f}"
    if steps:
        assert np.array_equal(a.get_steps()[:len(ra)], b.get_steps()[:len(rb)]), f"{what}: steps differ"
    return len(ra)


def same_counters(a, b, what):
    ca, cb = a.counters(), b.counters()
    for side in ("extend_", "connect_"):
        for k in STAGE_COUNTERS:
            assert ca[side + k] == cb[side + k], (what, side + k, ca[side + k], cb[side + k])
    return ca


# ---- odd but legal, multi-BLAS (validate_catalogue has the single-BLAS forms) -----------------------------------------------------------
def holes_multi():
    gt, sa = K._multi()
    n = sa.bvh4.copy()
    for i in range(len(n)):
        for f in ("aabbMin", "aabbMax", "first", "count"):
            n[f][i] = np.roll(sa.bvh4[f][i], i % 4, axis=0)
    used = n["first"] != -1
    assert (~used[:, 0] & used[:, 2]).any() and all((~used[:, k]).any() and used[:, k].any() for k in range(4))
    return K.Entry("bvh4-holes-multi", K._regt(gt, sa), K._with(sa, bvh4=n), "multi", (B4,), K.VIEW)


def leaf_127_multi():
    """The second BLAS as ONE quad record with one leaf slot of all its 127 triangles (the largest packed leaf)."""
    gt, sa = K._one((lambda g, rng: g.triangles(C._soup(rng, 127, (-2, -3.5, 2), (2, -1, 6), 0.45), "green"),),
                    [(1, C.invT(C.rot(1, 17.0), (0.2, -0.1, 0.3)))])
    n0 = len(sa.prims) - 127
    at = np.where(sa.primIdx >= n0)[0]
    assert len(at) == 127 and np.array_equal(at, np.arange(at[0], at[0] + 127))
    n, root = sa.bvh4.copy(), int(sa.blas["bvhIdx"][1])
    n["first"][root], n["count"][root] = -1, -1
    n["first"][root][0], n["count"][root][0] = at[0], 127
    lo, hi = K._box_of(sa.prims[n0:])
    n["aabbMin"][root][0][:3], n["aabbMax"][root][0][:3] = lo, hi
    return K.Entry("leaf-127-multi", K._regt(gt, sa), K._with(sa, bvh4=n), "multi", (B4,), K.VIEW)


# ---- a living scene ---------------------------------------------------------------------------------------------------------------------
LEVELS = 7          # collapse_check.comb2(7): a BVH4 need of 22, a column of 23 + 1 + 1 = 25 entries: the spill instantiation by default
LIVING_VIEW = dict(origin=(1.5, 1.5, 9.0), forward=(0.0, 0.0, 1.0), fov=60.0, aperture=0.01)


def living():
    """Two BLAS: a soup with the lights, and a soup under a hand-made BVH2 that collapses to a comb (deep), which a rebuild replaces by
    the builder's shallow tree."""
    n2, slots = KC.comb2(LEVELS)
    s = KC.soup_scene([40, slots], seed=9)
    sa = s.arrays(bvh4=False)
    root = int(sa.blas["bvhIdx"][1])
    assert len(sa.primIdx) == 40 + slots and np.array_equal(np.sort(sa.primIdx[:40]), np.arange(40))
    n2 = n2.copy()
    n2["first"] += np.where(n2["count"] == 0, root, 40).astype(np.uint32)
    sa.bvh2 = np.concatenate([sa.bvh2[:root], n2])
    sa.primIdx = np.concatenate([sa.primIdx[:40], np.arange(40, 40 + slots, dtype=np.uint32)])
    return s, sa

"""Shared pieces of the capacity tests (test_capacity_cpu.py, test_gpu_capacity.py): hand-built trees whose worst ray fills a traversal
stack to its last entry, the rays that do it, and a float64 model of the visit rules that proves the stack was full.

Every capacity of the traversal is sized to the uploaded tree with no slack: the LDS column of a lane (`stack_entries` =
clamp(need + 1, 6, 64), a need of 64 admitted), the TLAS part on top of it, the global column of the spill instantiation, the private
TLAS stack of the nested loops (32), the 7-bit primitive count of a packed leaf (127).  The trees of a builder fork on few levels of
any one ray's path, so none of these ends is reached by the other suites.  Here the node arrays are written by hand over primitives
added through geom64.GTScene (which gives the float64 ground truth its primitive sets): a BVH only needs boxes that contain their
subtrees, so every box is XY wide across the ray bundle, every ray passes every box, and the visit order is decided along z alone.

  chain(h)         BVH2 caterpillar of height h: interior N_k covers z in [0, h - k], children N_{k+1} and the leaf of z = h - k.  A ray
                   towards +z enters N_{k+1} first at every level (extend, near child first), a ray towards -z leaves it later
                   (connect, later exit first): both reach the bottom with h entries pending.  One ray per small triangle, so the
                   answer of the ray aimed at the top triangle sits in the entry pushed first and popped last.
  comb(L)          BVH4 of L levels written directly: three one-leaf stub nodes in slots 0-2, the next level in slot 3 (four stubs on
                   the last level); slot order pushes all four and pops the last: 3 (L - 1) + 4 entries pending, 64 at L = 21.
  fat leaves       one leaf of m triangles (chain(h, fat=m), comb(L, fat=m)): m = 127 is the largest packed leaf, 128 must send the
                   scene to layout 0.
  tlas_chain(d, h) d + 1 instances, each its own copy of chain(h), under a caterpillar TLAS of depth d; instance 0 lies deepest and
                   is entered first, with d TLAS siblings pending under its h BLAS entries.  Instances are translated (and one of
                   them turned by 180 degrees, so the world ray's direction has to come back from its backup), each in its own lateral
                   band, so a ray hits one triangle of one instance.
  frame=True       the two end leaves hold a diffuse receiver (top, with a small guard triangle in the same leaf: the entry pushed
                   first) and a light (bottom); the shadow rays of bounce 0 start in the top leaf and run towards -z.

occupancy() replays the visit rules of DESIGN.md section 5 in float64 (Python floats) - it calls neither implementation."""
import math
from dataclasses import dataclass, field

import numpy as np

import geom64 as G
from magr_ray_tracer_amd import _lib as W
from magr_ray_tracer_amd.scenes import Scene, _std_materials

XY = 500.0                       # half-width of every box across the ray bundle
PAD = 0.005                      # boxes exceed their contents by this much along z
GUARD = 0.25                     # frame cases: the guard triangle hangs this far in front of the receiver
DZ = 0.03                        # frame cases: spacing of the leaves above the bottom one (see _zs)
TILT = (0.001, 0.0007)           # no ray has a zero direction component
FAR = 1e30
MIN_MARGIN = 0.5                 # the model's deciding distances must differ by at least this much
STACK_MAX, STACK_MIN, LEAF_MAX = 64, 6, 127


def stack_entries(need):
    """rebuild_common.h stack_entries: the LDS column a context keeps for a deepest need."""
    return min(max(need + 1, STACK_MIN), STACK_MAX)


@dataclass
class Case:
    name: str
    gt: object
    sa: object
    rays: np.ndarray             # extend rays, one per small triangle
    expect: np.ndarray           # the primitive each of them hits
    need: dict                   # accel -> pending entries of the worst ray (BLAS part)
    depth: int = 0               # TLAS depth
    view: dict = None            # frame cases: the camera
    fat: np.ndarray = None       # rays aimed at the triangles of the fat leaf
    info: dict = field(default_factory=dict)

    def accels(self):
        return sorted(self.need)


# ---- primitives ---------------------------------------------------------------------------------------------------------------------
def _gt():
    gt = G.GTScene(Scene())
    _std_materials(gt.s)
    return gt


def _small(g, z):
    """The small triangle of grid cell g (9 cells per row, spacing 1) at height z; its centroid is the cell centre."""
    c = np.array([g % 9, g // 9, z], np.float64)
    return np.array([c + (-0.15, -0.1, 0), c + (0.15, -0.1, 0), c + (0, 0.2, 0)])


def _quad(x0, y0, x1, y1, z, up):
    """Two triangles covering [x0, x1] x [y0, y1] at height z, normal (e1 x e2) towards +z (up) or -z."""
    a, b, c, d = (x0, y0, z), (x1, y0, z), (x1, y1, z), (x0, y1, z)
    # (v0 at the right angle: the float64 bound of t is tightest there, and these surfaces end shadow rays 2e-4 short of themselves)
    return np.array([[b, c, a], [d, a, c]] if up else [[b, a, c], [d, c, a]], np.float64)


def _aim(cen, z_from, sign=1.0):
    """Rays through the points `cen` along +-(TILT, 1), starting in the plane z = z_from."""
    D = np.array([TILT[0], TILT[1], 1.0]) * sign
    D /= np.linalg.norm(D)
    O = cen - D * ((cen[:, 2] - z_from) / D[2])[:, None]
    return G.make_rays(O.astype(np.float32), np.tile(D.astype(np.float32), (len(cen), 1)))


# ---- node arrays --------------------------------------------------------------------------------------------------------------------
def _box(n, i, z0, z1):
    n["aabbMin"][i][:3] = (-XY, -XY, z0 - PAD)
    n["aabbMax"][i][:3] = (XY, XY, z1 + PAD)


def _caterpillar(leaves):
    """BVH2 caterpillar over leaves[j] = (first, count, zmin, zmax), j = 0 (bottom, deepest) .. h (top, child of the root); node ids and
    primIdx slots local to the block.  N_0 = node 0, the children of N_k at 2k + 1 (N_{k+1}) and 2k + 2 (the leaf of j = h - k)."""
    h = len(leaves) - 1
    n = np.zeros(2 * h + 1, W.BVHNode2)
    at = lambda k: 0 if k == 0 else 2 * k - 1
    for k in range(h):
        below = leaves[:h - k + 1]
        _box(n, at(k), min(l[2] for l in below), max(l[3] for l in below))
        n["first"][at(k)], n["count"][at(k)] = 2 * k + 1, 0
        f, c, z0, z1 = leaves[h - k]
        _box(n, 2 * k + 2, z0, z1)
        n["first"][2 * k + 2], n["count"][2 * k + 2] = f, c
    f, c, z0, z1 = leaves[0]
    _box(n, at(h), z0, z1)
    n["first"][at(h)], n["count"][at(h)] = f, c
    return n


def _collapse(n2):
    out = np.zeros(len(n2), W.BVHNode4)
    assert W.host_lib().rth_bvh4_from_nodes(W.ptr(n2), len(n2), W.ptr(out)) == 0, W.host_lib().rth_last_error()
    return out


def _install(sa, blocks2, blocks4, counts):
    """Replace the scene's node arrays by the given per-BLAS blocks (local ids), BLAS b over the next counts[b] primIdx slots."""
    sa.blas = sa.blas.copy()
    out2, out4, node0, idx0 = [], [], 0, 0
    for b, cnt in enumerate(counts):
        n2 = blocks2[b].copy() if blocks2 is not None else None
        n4 = blocks4[b].copy()
        if n2 is not None:
            n2["first"] += np.where(n2["count"] == 0, node0, idx0).astype(np.uint32)
            out2.append(n2)
        live = n4["first"] != -1
        n4["first"] += np.where(live, np.where(n4["count"] == 0, node0, idx0), 0).astype(np.int32)
        out4.append(n4)
        sa.blas["bvhIdx"][b] = node0
        node0 += len(n4)
        idx0 += cnt
    if blocks2 is not None:
        sa.bvh2 = np.concatenate(out2)
    sa.bvh4 = np.concatenate(out4)
    sa.primIdx = np.arange(idx0, dtype=np.uint32)
    assert idx0 == len(sa.prims)


def _wide_tlas_root(sa, z0, z1):
    sa.tlas = sa.tlas.copy()
    sa.tlas["aabbMin"][:, :3] = (-XY, -XY, z0 - 0.5)
    sa.tlas["aabbMax"][:, :3] = (XY, XY, z1 + 0.5)


# ---- the trees ----------------------------------------------------------------------------------------------------------------------
def _zs(h, frame):
    """Heights of the leaves.  Only the bottom leaf decides an order (N_{k+1} starts and ends there, whatever lies above), so a frame
    case keeps it 1 below the others and packs those DZ apart: the float64 bound of a shadow ray's t grows with the scene's extent, and
    a ray that ends 2e-4 short of the light is decidable only in a scene a few units tall."""
    if not frame:
        return [float(j) for j in range(h + 1)]
    zs = [0.0] + [1.0 + DZ * (j - 1) for j in range(1, h + 1)]
    zs[-1] += GUARD + 0.05 - DZ if h > 1 else 0.0        # room for the guard triangle, GUARD in front of the receiver
    return zs


def _chain_prims(gt, h, fat=None, frame=False, first_cell=0, light=True, receiver=True):
    """Add one chain's primitives leaf by leaf, bottom first; returns (leaves, centroids of the small triangles, their primitive ids,
    ids of the fat leaf's triangles).  fat = m: the leaf of z = h // 2 holds m triangles.  frame: a light quad in the bottom leaf
    (light) and a guard triangle plus the receiver quad in the top leaf (receiver)."""
    leaves, cen, ids, fat_ids, g = [], [], [], [], first_cell
    rows, zs = -(-(h + 1 + (fat or 1) - 1) // 9), _zs(h, frame)
    ymid, yhalf = 0.5 * (rows - 1), max(4.5, 0.5 * rows)      # the frame's surfaces cover the grid and the camera's field of view
    # the receiver's chain keeps the triangle of level 1 - the entry pushed LAST, in the column's last slot when h = 64 - on the
    # camera's axis, where the shadow rays pass (it swaps cells with the triangle that had that cell)
    axis = 9 * math.floor(ymid) + 4
    swap = {1: axis, axis: 1} if frame and receiver and 1 < axis < h else {}
    for j in range(h + 1):
        first = gt.s.num_prims
        z0 = z1 = zs[j]
        if frame and j == 0 and light:
            for t in _quad(-0.5, ymid - yhalf, 8.5, ymid + yhalf, 0.0, True):
                gt.light(t, "white-light")
            g += 1
        elif frame and j == h and receiver:
            z0 = z1 - GUARD
            tri = _small(g, z0)                # the guard: between four cells, on the camera's axis (in nobody else's way)
            tri[:, :2] += (4.5 - g % 9, math.floor(ymid) + 0.5 - g // 9)
            gt.triangles(tri[None], "red")
            cen.append(tri.mean(0)), ids.append(first)
            gt.triangles(_quad(-0.5, ymid - yhalf, 8.5, ymid + yhalf, z1, False), "sand")
            g += 1
        else:
            for _ in range(fat if fat and j == h // 2 else 1):
                tri = _small(first_cell + swap[j] if j in swap else g, zs[j])
                cen.append(tri.mean(0)), ids.append(gt.s.num_prims)
                if fat and j == h // 2:
                    fat_ids.append(gt.s.num_prims)
                gt.triangles(tri[None], "sand")
                g += 1
        leaves.append((first, gt.s.num_prims - first, z0, z1))
    return leaves, np.array(cen), np.array(ids), np.array(fat_ids, np.int64)


def _local(leaves):
    f0 = leaves[0][0]
    return [(f - f0, c, a, b) for f, c, a, b in leaves]


def _view(top, rows):
    """The camera of a frame case: 0.9 in front of the receiver (at z = top), looking at it (a camera looks along -forward)."""
    return dict(origin=(4.0, 0.5 * (rows - 1), top - 0.9), forward=(0.0, 0.0, -1.0), fov=100.0, aperture=0.01)


def chain(h, fat=None, frame=False):
    """One BLAS: the BVH2 caterpillar of height h and its BVH4 collapse."""
    gt = _gt()
    leaves, cen, ids, fat_ids = _chain_prims(gt, h, fat, frame)
    gt.build_blas(1.0)
    sa = gt.finish()
    n2 = _caterpillar(_local(leaves))
    _install(sa, [n2], [_collapse(n2)], [len(sa.prims)])
    top = _zs(h, frame)[-1]
    _wide_tlas_root(sa, 0, top)
    rays = _aim(cen, 0.5 if frame else -1.0)               # (a frame's rays start above its light)
    c = Case(f"chain({h}{', fat=%d' % fat if fat else ''}{', frame' if frame else ''})", gt, sa, rays, ids,
             {W.ACCEL_BVH2: h, W.ACCEL_BVH4: None}, view=_view(top, -(-(h + (fat or 1)) // 9)) if frame else None)
    if fat:
        c.fat = np.where(np.isin(ids, fat_ids))[0]
    if frame:
        c.info.update(guard=int(ids[-1]), last=int(ids[0]))   # the small triangle in the receiver's leaf; the one of level 1
    return c


def comb(levels, fat=None):
    """One BLAS, BVH4 only: the comb of `levels` levels (need 3 (levels - 1) + 4); fat = m: the first stub's leaf holds m triangles."""
    need = 3 * (levels - 1) + 4
    gt = _gt()
    cen, ids, slots, g = [], [], [], 0
    for p in range(need):
        first = gt.s.num_prims
        for _ in range(fat if fat and p == 0 else 1):
            tri = _small(g, p)
            cen.append(tri.mean(0)), ids.append(gt.s.num_prims)
            gt.triangles(tri[None], "sand")
            g += 1
        slots.append((first, gt.s.num_prims - first))
    gt.build_blas(1.0)
    sa = gt.finish()
    n = np.zeros(4 * levels + 1, W.BVHNode4)
    n["first"][:], n["count"][:] = -1, -1

    def box(i, k, z0, z1):
        n["aabbMin"][i][k][:3] = (-XY, -XY, z0 - PAD)
        n["aabbMax"][i][k][:3] = (XY, XY, z1 + PAD)
    p = 0
    for l in range(levels):
        m = 4 * l
        for s in range(3 if l < levels - 1 else 4):
            st = m + 1 + s
            n["first"][m][s], n["count"][m][s] = st, 0
            n["first"][st][0], n["count"][st][0] = slots[p]
            box(m, s, p, p), box(st, 0, p, p)
            p += 1
        if l < levels - 1:
            n["first"][m][3], n["count"][m][3] = m + 4, 0
            box(m, 3, p, need - 1)
    _install(sa, None, [n], [len(sa.prims)])
    sa.bvh2 = np.zeros(len(n), W.BVHNode2)                  # (the builder's tree does not go with this primIdx: BVH4 only)
    _wide_tlas_root(sa, 0, need)
    c = Case(f"comb({levels}{', fat=%d' % fat if fat else ''})", gt, sa, _aim(np.array(cen), -1.0), np.array(ids), {W.ACCEL_BVH4: need})
    if fat:
        c.fat = np.arange(fat)
    return c


def tlas_chain(d, h, frame=False):
    """d + 1 instances of chain(h) under a caterpillar TLAS of depth d (leaves at nodes 1 .. d + 1, joints J_0 = node 0 and J_k =
    node d + 1 + k with the children J_{k+1} - at the bottom the leaf of instance 0 - and the leaf of instance d - k).  Instance i
    occupies z in [i S, i S + h] (frame: the order reversed, so that the shadow rays, which run towards -z, meet instance 0 first) in
    its own lateral band; instance max(1, d // 2) is turned by 180 degrees about x (frame: about z)."""
    n = d + 1
    top = _zs(h, frame)[-1]
    rows, S, tpad = -(-(h + 1) // 9), (top + 0.7 if frame else h + 4), (0.1 if frame else 0.5)
    gt = _gt()
    blocks2, counts, cens, idss = [], [], [], []
    for i in range(n):
        leaves, cen, ids, _ = _chain_prims(gt, h, frame=frame, light=i == d, receiver=i == 0)
        gt.build_blas(1.0)
        blocks2.append(_caterpillar(_local(leaves)))
        counts.append(sum(l[1] for l in leaves))
        cens.append(cen), idss.append(ids)
    turned = max(1, d // 2)
    zof = lambda i: float((d - i if frame else i) * S)
    for i in range(n):
        off = np.array([0.5 * (i % 2), 0.0 if frame else i * (rows + 1.0), zof(i)])    # (a frame's shadow rays stay near the axis)
        if i == turned:          # local = diag(1, -1, -1) world + t: the band and the z range stay where a translation would put them
            T = np.eye(4, dtype=np.float32)   # (a frame turns it about z instead: its shadow rays have lateral components to lose, and
            T[1, 1] = -1.0                    # along z the leaves of a frame are too close to decide an order by)
            T[0 if frame else 2, 0 if frame else 2] = -1.0
            T[:3, 3] = (off[0] + 8.0, off[1] + rows - 1.0, -off[2]) if frame else (-off[0], off[1] + rows - 1.0, off[2] + top)
        else:
            T = np.eye(4, dtype=np.float32)
            T[:3, 3] = -off
        gt.s.SetInstanceTransform(i, T)
    sa = gt.finish()
    _install(sa, blocks2, [_collapse(b) for b in blocks2], counts)
    t = np.zeros(2 * n, W.TLASNode)

    def box(i, z0, z1):
        t["aabbMin"][i][:3] = (-XY, -XY, z0 - tpad)
        t["aabbMax"][i][:3] = (XY, XY, z1 + tpad)
    for i in range(n):
        t["BLASidx"][1 + i] = i
        box(1 + i, zof(i), zof(i) + top)
    J = lambda k: 0 if k == 0 else n + k
    for k in range(d):
        t["leftRight"][J(k)] = (J(k + 1) if k + 1 < d else 1) + ((1 + d - k) << 16)
        zs = [zof(i) for i in range(d - k + 1)]
        box(J(k), min(zs), max(zs) + top)
    sa.tlas = t
    gt._cache = {}
    V, I = G.world_triangles(gt)
    ids = np.concatenate(idss)
    cen = V[np.searchsorted(I, ids)].mean(1)
    assert np.array_equal(I[np.searchsorted(I, ids)], ids)
    view = None
    if frame:
        view = _view(zof(0) + top, rows)
    return Case(f"tlas_chain({d}, {h}{', frame' if frame else ''})", gt, sa, _aim(cen, 0.5 if frame else -1.0), ids,
                {W.ACCEL_BVH2: h, W.ACCEL_BVH4: None}, depth=d, view=view, info=dict(guard=int(idss[0][-1]), last=int(idss[0][1])) if frame else {})


def without(gt, prim):
    """The ground truth of the same scene less one triangle (a record that `gt` calls occluded and this calls unoccluded has that
    triangle as its only occluder)."""
    import copy
    g = copy.copy(gt)
    g.sets = []
    for st in gt.sets:
        keep = st["tri_idx"] != prim
        g.sets.append(dict(st, tri=st["tri"][keep], tri_idx=st["tri_idx"][keep]))
    g._cache = {}
    return g


def sole_occluder(gt, prim, org, L, tmax):
    """How many decidable shadow rays are occluded by `prim` and by nothing else."""
    occ, dec = G.any_hit(gt, org, L, tmax)
    occ2, dec2 = G.any_hit(without(gt, prim), org, L, tmax)
    return int((dec & dec2 & occ & ~occ2).sum())


# ---- the occupancy model ------------------------------------------------------------------------------------------------------------
def _slab(lo, hi, O, R, t):
    """Entry and exit distance of a box, and whether the kernels visit it (tmax >= tmin, tmin < ray.t, tmax > 0)."""
    tn, tf = -math.inf, math.inf
    for k in (0, 1, 2):
        a, b = (lo[k] - O[k]) * R[k], (hi[k] - O[k]) * R[k]
        tn, tf = max(tn, min(a, b)), min(tf, max(a, b))
    return tn, tf, (tf >= tn and tn < t and tf > 0)


def _sub(a, b):
    return (a[0] - b[0], a[1] - b[1], a[2] - b[2])


def _dot(a, b):
    return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]


def _cross(a, b):
    return (a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0])


def _tri_t(v, O, D):
    """Distance of a triangle hit (Moeller-Trumbore with the kernels' acceptance rule) or None."""
    e1, e2 = _sub(v[1], v[0]), _sub(v[2], v[0])
    p = _cross(D, e2)
    det = _dot(e1, p)
    if abs(det) < 1e-8:
        return None
    s = _sub(O, v[0])
    u = _dot(s, p) / det
    q = _cross(s, e1)
    w = _dot(D, q) / det
    if u < 0 or w < 0 or u + w > 1:
        return None
    t = _dot(e2, q) / det
    return t if t >= 0 else None


def _inv(D):
    return [1.0 / x if x != 0 else math.inf for x in D]


class _Tables:
    """The scene's arrays as Python lists of float64 (one conversion per scene)."""

    def __init__(self, sa):
        f = lambda a: a.astype(np.float64).tolist()
        self.V = np.stack([sa.prims["v0"][:, :3], sa.prims["v1"][:, :3], sa.prims["v2"][:, :3]], 1).astype(np.float64).tolist()
        self.idx = sa.primIdx.tolist()
        self.lo2, self.hi2 = f(sa.bvh2["aabbMin"][:, :3]), f(sa.bvh2["aabbMax"][:, :3])
        self.first2, self.count2 = sa.bvh2["first"].tolist(), sa.bvh2["count"].tolist()
        self.lo4, self.hi4 = f(sa.bvh4["aabbMin"][:, :, :3]), f(sa.bvh4["aabbMax"][:, :, :3])
        self.first4, self.count4 = sa.bvh4["first"].tolist(), sa.bvh4["count"].tolist()
        self.lot, self.hit_ = f(sa.tlas["aabbMin"][:, :3]), f(sa.tlas["aabbMax"][:, :3])
        self.lr, self.blas = sa.tlas["leftRight"].tolist(), sa.tlas["BLASidx"].tolist()
        self.invT = [T.astype(np.float64).reshape(4, 4).tolist() for T in sa.blas["invT"]]
        self.root = sa.blas["bvhIdx"].tolist()


def _tables(sa):
    key = tuple(id(getattr(sa, k)) for k in ("prims", "bvh2", "bvh4", "primIdx", "tlas", "blas"))
    if sa.__dict__.get("_cap_key") != key:
        sa.__dict__["_cap_key"], sa.__dict__["_cap_tab"] = key, _Tables(sa)
    return sa.__dict__["_cap_tab"]


class _Walk:
    """One ray's traversal: the pending entries of the TLAS and of the BLAS level, and their maxima."""

    def __init__(self, tab, accel, anyhit, t):
        self.T, self.accel, self.anyhit, self.t = tab, accel, anyhit, t
        self.tl = self.bl = self.pending = self.max_tlas = self.max_blas = self.steps = 0
        self.margin, self.hit = math.inf, False

    def note(self):
        self.pending = max(self.pending, self.tl + self.bl)
        self.max_tlas, self.max_blas = max(self.max_tlas, self.tl), max(self.max_blas, self.bl)

    def leaf(self, first, count, O, D, t_light):
        """Test a leaf's primitives in order; True when an any-hit traversal ends here."""
        for s in range(first, first + count):
            t = _tri_t(self.T.V[self.T.idx[s]], O, D)
            if t is not None and t <= self.t:
                self.t, self.hit = t, True
                if self.anyhit and self.t < t_light:
                    return True
        return False

    def bvh2(self, root, O, D):
        T, R, t_light = self.T, _inv(D), self.t
        node, st = root, []
        while True:
            if T.count2[node] > 0:
                if self.leaf(T.first2[node], T.count2[node], O, D, t_light):
                    return True
            else:
                c1, c2 = T.first2[node], T.first2[node] + 1
                n1, x1, h1 = _slab(T.lo2[c1], T.hi2[c1], O, R, self.t)
                n2, x2, h2 = _slab(T.lo2[c2], T.hi2[c2], O, R, self.t)
                if self.anyhit:                              # connect: the child the ray leaves later first
                    if h1 and h2:
                        self.margin = min(self.margin, abs(x2 - x1))
                        node, other = (c2, c1) if x2 > x1 else (c1, c2)
                        st.append(other)
                        self.bl = len(st)
                        self.note()
                        continue
                    if h1 or h2:
                        node = c1 if h1 else c2
                        continue
                else:                                        # extend: near child first by entry distance; steps as bvh.cl counts them
                    d1, d2 = (n1 if h1 else FAR), (n2 if h2 else FAR)
                    if h1 and h2:
                        self.margin = min(self.margin, abs(d2 - d1))
                    if d1 > d2:
                        d1, d2, c1, c2 = d2, d1, c2, c1
                    if d1 < t_light:
                        self.steps += 1
                        node = c1
                        if d2 < t_light:
                            st.append(c2)
                            self.steps += 1
                            self.bl = len(st)
                            self.note()
                        continue
            if not st:
                return False
            node = st.pop()
            self.bl = len(st)

    def bvh4(self, root, O, D):
        T, R, t_light = self.T, _inv(D), self.t
        node, st = root, []
        while True:
            self.steps += 1
            first, count = T.first4[node], T.count4[node]
            vis = [first[k] != -1 and _slab(T.lo4[node][k], T.hi4[node][k], O, R, self.t)[2] for k in range(4)]   # all four at node entry
            for k in range(4):                               # slot order: leaves tested, interior children pushed
                if not vis[k]:
                    continue
                if count[k] > 0:
                    if self.leaf(first[k], count[k], O, D, t_light):
                        return True
                else:
                    st.append(first[k])
                    self.bl = len(st)
                    self.note()
            if not st:
                return False
            node = st.pop()
            self.bl = len(st)

    def instance(self, b, O, D):
        M = self.T.invT[b]
        Oi = [_dot(M[k], O) + M[k][3] for k in (0, 1, 2)]
        Di = [_dot(M[k], D) for k in (0, 1, 2)]
        self.bl = 0
        return self.bvh4(self.T.root[b], Oi, Di) if self.accel == W.ACCEL_BVH4 else self.bvh2(self.T.root[b], Oi, Di)

    def tlas(self, O, D):
        T, R, t_light = self.T, _inv(D), self.t
        node, st = 0, []
        while True:
            lr = T.lr[node]
            if lr == 0:
                if self.instance(T.blas[node], O, D):
                    return True
            else:                                            # near child first, extend and connect alike
                c1, c2 = lr & 0xffff, lr >> 16
                n1, _, h1 = _slab(T.lot[c1], T.hit_[c1], O, R, self.t)
                n2, _, h2 = _slab(T.lot[c2], T.hit_[c2], O, R, self.t)
                d1, d2 = (n1 if h1 else FAR), (n2 if h2 else FAR)
                if h1 and h2:
                    self.margin = min(self.margin, abs(d2 - d1))
                if d1 > d2:
                    d1, d2, c1, c2 = d2, d1, c2, c1
                if d1 < t_light:
                    node = c1
                    if d2 < t_light:
                        st.append(c2)
                        self.tl = len(st)
                        self.note()
                    continue
            if not st:
                return False
            node = st.pop()
            self.tl = len(st)


def occupancy(sa, accel, O, D, anyhit=False, tmax=FAR):
    """Replay one ray (O, D: 3 floats) through the scene's arrays by the documented visit rules, in float64.  Returns a dict:
    pending  most entries pending at once, TLAS siblings and BLAS entries together (the column of k_trace_persist_tlas)
    tlas, blas  the most of either kind (the private TLAS stack of the nested loops; the column of the single-BLAS kernels)
    steps    bvh.cl's `steps` (extend)       margin  the smallest difference of two distances that decided an order
    hit      a primitive was accepted (any-hit: the ray is occluded)"""
    O, D = np.asarray(O, np.float64)[:3].tolist(), np.asarray(D, np.float64)[:3].tolist()
    w = _Walk(_tables(sa), accel, anyhit, float(tmax))
    w.tlas(O, D)
    return dict(pending=w.pending, tlas=w.max_tlas, blas=w.max_blas, steps=w.steps, margin=w.margin, hit=w.hit)


def worst(case, accel, rays=None, anyhit=False, tmax=None, every=1):
    """occupancy() over a ray set (every n-th ray): the maxima, the per-ray steps and pending entries, the smallest margin."""
    rays = case.rays if rays is None else rays
    pick = np.arange(0, len(rays), every)
    if len(rays) and pick[-1] != len(rays) - 1:
        pick = np.append(pick, len(rays) - 1)
    out = [occupancy(case.sa, accel, rays["O"][i], rays["D"][i], anyhit, FAR if tmax is None else tmax[i]) for i in pick]
    return dict(pending=max(o["pending"] for o in out), tlas=max(o["tlas"] for o in out), blas=max(o["blas"] for o in out),
                margin=min(o["margin"] for o in out), steps=np.array([o["steps"] for o in out]), pick=pick,
                per_ray=np.array([o["pending"] for o in out]), hit=np.array([o["hit"] for o in out]))

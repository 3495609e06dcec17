"""Shared pieces of the TLAS tests (test_tlas_cpu.py, test_gpu_tlas.py): a plain restatement of TLAS::Build, scenes of up to 256
instances whose leaf boxes tie (or must not tie) in known ways, and the condition a frame must meet to count as a picture of the scene.

The device builds the TLAS with one 256-thread workgroup (k_tlas_build, csrc/refit.hip): FindBestMatch is an argmin inside each wave of
64, then a fold across the four waves, equal areas going to the lowest index.  What that argmin must decide is fixed by the rules below
alone; restated here from those rules (nothing of csrc/refit_common.h is used), with a count of the calls in which a tie had to be
broken and of the ties whose candidates sit in different groups of 64 positions - the ones only the cross-wave fold decides."""
import numpy as np

import geom64 as G
import test_groundtruth_cpu as C
from magr_ray_tracer_amd import _lib as W
from magr_ray_tracer_amd.scenes import Scene, _std_materials, box_tris

NS = [1, 2, 3, 63, 64, 65, 128, 129, 255, 256]
REALLYFAR = np.float32(1e30)
GRID = 16            # boxes per row of the lattice: tied neighbours (b - 16, b - 1, b + 1, b + 16) reach into other groups of 64
PITCH = 1.0          # power-of-two spacing of boxes of half-width 1/4, the grid centred on the origin
HALF = 0.25          # (a small scene around the origin: float32 keeps a bounce ray's 1e-4 offset from its surface decidable)
MATS = ["sand", "green", "red", "white"]
SOUP = 4             # soup triangles per BLAS of the layouts that must not tie
LAYOUTS = ("random", "lattice", "pairs", "stacked", "mixed")


# ---- TLAS::Build, restated -----------------------------------------------------------------------------------------------------------
def _fmin(a, b):
    """fminf as the host evaluates it: a NaN operand gives the other one, an equal pair (+0, -0) the second operand."""
    return np.where(np.isnan(a), b, np.where(np.isnan(b), a, np.where(a < b, a, b))).astype(np.float32)


def _fmax(a, b):
    return np.where(np.isnan(a), b, np.where(np.isnan(b), a, np.where(a > b, a, b))).astype(np.float32)


class Built:
    """nodes: the 2n TLAS nodes; depth: edges from node 0 to its deepest leaf; calls: FindBestMatch calls; multi: those with two or more
    candidates; tied: those with more than one candidate at the minimum; cross: tied calls whose tied candidates' positions lie in
    different groups of 64."""

    def __init__(self, nodes, depth, calls, multi, tied, cross):
        self.nodes, self.depth, self.calls, self.multi, self.tied, self.cross = nodes, depth, calls, multi, tied, cross


def build_tlas(leaf_min, leaf_max):
    """TLAS::Build over the given leaf boxes ((n, 4) float32 each, w lanes included).  Rules: node 1 + i is the leaf of instance i;
    FindBestMatch(list, N, A) scans B = 0 .. N - 1 (B != A) for the smallest union area ex * ey + ey * ez + ez * ex, strict <,
    starting at RT_REALLYFAR; the nearest-neighbour chain A -> B -> C joins A and B when C == A, into node nodesUsed++ with children
    (slot[A], slot[B] << 16) and the fmin / fmax of all four lanes; slot[A] becomes the join, slot[B] the last live slot; node 0 is a
    copy of the last node standing.  Returns Built, or None when a call finds no partner."""
    mn, mx = np.asarray(leaf_min, np.float32).reshape(-1, 4), np.asarray(leaf_max, np.float32).reshape(-1, 4)
    n = len(mn)
    assert 1 <= n <= 256
    nodes = np.zeros(2 * n, W.TLASNode)
    nodes["aabbMin"][1:n + 1], nodes["aabbMax"][1:n + 1] = mn, mx
    nodes["BLASidx"][1:n + 1] = np.arange(n)
    slot = list(range(1, n + 1))
    live, used = n, n + 1
    stat = dict(calls=0, multi=0, tied=0, cross=0)

    def find_best_match(N, A):
        stat["calls"] += 1
        s = slot[:N]
        a_mn, a_mx = nodes["aabbMin"][slot[A]], nodes["aabbMax"][slot[A]]
        with np.errstate(invalid="ignore", over="ignore"):
            e = _fmax(a_mx[None, :3], nodes["aabbMax"][s][:, :3]) - _fmin(a_mn[None, :3], nodes["aabbMin"][s][:, :3])
            area = (e[:, 0] * e[:, 1] + e[:, 1] * e[:, 2] + e[:, 2] * e[:, 0]).astype(np.float32)
        smallest, best = float(REALLYFAR), -1
        areas = area.tolist()            # (float32 values as Python floats: the comparisons are the same)
        for B in range(N):
            if B != A and areas[B] < smallest:
                smallest, best = areas[B], B
        if N > 2:
            stat["multi"] += 1
        if best >= 0:
            at = [B for B in range(N) if B != A and areas[B] == smallest]
            if len(at) > 1:
                stat["tied"] += 1
                stat["cross"] += len({B // 64 for B in at}) > 1
        return best

    A = 0
    B = find_best_match(live, A) if live > 1 else -1
    while live > 1:
        if B < 0:
            return None
        Cc = find_best_match(live, B)
        if Cc < 0:
            return None
        if A == Cc:
            ia, ib = slot[A], slot[B]
            nodes["leftRight"][used] = ia + (ib << 16)
            nodes["aabbMin"][used] = _fmin(nodes["aabbMin"][ia], nodes["aabbMin"][ib])
            nodes["aabbMax"][used] = _fmax(nodes["aabbMax"][ia], nodes["aabbMax"][ib])
            slot[A] = used
            used += 1
            slot[B] = slot[live - 1]
            live -= 1
            B = find_best_match(live, A) if live > 1 else -1
        else:
            A, B = B, Cc
    nodes[0] = nodes[slot[A]]
    return Built(nodes, tlas_depth(nodes), **stat)


def tlas_depth(t):
    d, st = 0, [(0, 0)]
    while st:
        i, k = st.pop()
        d = max(d, k)
        lr = int(t["leftRight"][i])
        if lr:
            st += [(lr & 0xffff, k + 1), (lr >> 16, k + 1)]
    return d


def host_leaf_boxes(sa):
    """The leaf boxes the host gave the instances (nodes 1 .. n of its TLAS)."""
    n = len(sa.blas)
    return sa.tlas["aabbMin"][1:n + 1].copy(), sa.tlas["aabbMax"][1:n + 1].copy()


def root_leaf_boxes(sa):
    """The BLAS root boxes: the leaf boxes of identity instances, bit for bit."""
    r = sa.blas["bvhIdx"]
    return sa.bvh2["aabbMin"][r].copy(), sa.bvh2["aabbMax"][r].copy()


# ---- scenes -------------------------------------------------------------------------------------------------------------------------
def _extent(n):
    """(columns, rows) of the grid that n boxes occupy."""
    return min(n, GRID), (n + GRID - 1) // GRID


def positions(n, layout):
    """World position of every instance's box centre."""
    cols, rows = _extent(n)
    if layout in ("random", "mixed"):
        rng = np.random.default_rng(100 + n)
        lo, hi = np.array([-8.0, -8.0, -3.0]), np.array([PITCH * max(cols - 1, 1) - 8.0, PITCH * max(rows - 1, 1) - 8.0, 3.0])
        return rng.uniform(lo, hi, (n, 3)).astype(np.float32).astype(np.float64)
    b = np.arange(n)
    if layout == "pairs":
        b = b // 2
    if layout == "stacked":
        return np.zeros((n, 3))
    return np.stack([PITCH * (b % GRID) - 8.0, PITCH * (b // GRID) - 8.0, 0.0 * b], axis=1).astype(np.float64)


def transforms(n, layout, pos):
    """invT (world -> instance) of every instance, None = identity: the random layouts place their geometry by translation; `mixed` puts
    every third instance under a rotation, a non-uniform scale or a mirror on top of it."""
    kinds = ["rigid", "scale", "mirror"]
    out = []
    for b in range(n):
        if layout == "mixed" and b % 3 == 2:
            T = C.TRANSFORMS[kinds[(b // 3) % 3]]
            A = T[:3, :3].astype(np.float64)
            out.append(C.invT(A, T[:3, 3].astype(np.float64) - A @ pos[b]))
        elif b == 0:
            out.append(None)             # (BLAS 0 holds the floor and the light in world coordinates)
        else:
            out.append(C.invT(np.eye(3), -pos[b]))
    return out


def _room(n, layout):
    """Where the floor and the light of BLAS 0 go: under and above the boxes.  `stacked` keeps them inside the one box all its
    instances share (a room seen from inside), so that all n leaf boxes stay identical."""
    cols, rows = _extent(n)
    if layout == "stacked":
        return (-0.5, 0.5), -0.55, 0.6, 0.5
    return (-9.0, PITCH * (cols - 1) - 7.0), -8.8, PITCH * (rows - 1) - 6.8, 2.0


def _box(at, half):
    """The 12 triangles of a cube of half-width `half`, turned (so that no face lies in an axis plane, where an axis-parallel ray running
    in it would touch it along its whole length) with its corners on multiples of 2^-10: added to a lattice position the sums are exact,
    and every copy has the same bounding box relative to its place."""
    v = box_tris((-half,) * 3, (half,) * 3).astype(np.float64) @ (C.rot(1, 20.0) @ C.rot(0, 15.0)).T
    return (np.round(v * 1024.0) / 1024.0 + at).astype(np.float32)


def instances_scene(n, layout, baked=None, soup=None):
    """n BLAS of one 12-triangle box each (plus `soup` small triangles: distinct boxes, no ties), an emissive quad and a floor in
    BLAS 0, built through geom64.GTScene.  Returns (gt, sa, view); the view looks at the boxes (forward points from the scene to the
    camera).

    random    distinct soups at random places; the place is the instance transform (a translation)
    mixed     random, every third instance under a rotation, a non-uniform scale or a mirror as well
    lattice   identical boxes baked into the geometry on a 16-wide grid of pitch 1 under identity instances: leaf box == root box
              bit for bit, a box's four neighbours tie exactly at the minimum
    pairs     the lattice with every box present twice at one place
    stacked   n identical boxes at one place (a turned room of half-width 1, the camera, the floor and the light inside it): every call ties
              on every candidate
    baked: geometry at its world position under identity instances (the default for lattice / pairs / stacked; random with baked=True
    is the scene the primitive-only updates start from).  Every layout adds its primitives in the same order with the same materials
    when `soup` is the same, so the records of one can be handed to rt_update_scene of another."""
    assert layout in LAYOUTS
    baked = layout in ("lattice", "pairs", "stacked") if baked is None else baked
    soup = (SOUP if layout in ("random", "mixed") else 0) if soup is None else soup
    assert baked or layout in ("random", "mixed")
    pos = positions(n, layout)
    half = 1.0 if layout == "stacked" else HALF
    rng = np.random.default_rng(7)
    gt = G.GTScene(Scene())
    _std_materials(gt.s)
    (x0, x1), yf, yl, zr = _room(n, layout)
    for b in range(n):
        at = pos[b] if baked else np.zeros(3)
        tris = [_box(at, half)]
        if soup:
            tris.append(C._soup(rng, soup, at - HALF, at + HALF, 0.4 * HALF))
        gt.triangles(np.concatenate(tris), MATS[b % 4])
        if b == 0:
            xm, (w, d) = 0.5 * (x0 + x1), ((0.4, 0.25) if layout == "stacked" else (0.8, 0.5))
            gt.light([(xm - w, yl, -d), (xm + w, yl, -d), (xm + w, yl, d)], "white-light")
            gt.light([(xm + w, yl, d), (xm - w, yl, d), (xm - w, yl, -d)], "white-light")
            gt.triangles(np.array([[(x0, yf, -zr), (x1, yf, -zr), (x1, yf, zr)], [(x1, yf, zr), (x0, yf, zr), (x0, yf, -zr)]], np.float32), "grey")
        gt.build_blas(1.0)
    if not baked:
        for b, T in enumerate(transforms(n, layout, pos)):
            if T is not None:
                gt.s.SetInstanceTransform(b, T)
    sa = gt.finish()
    merge_duplicates(gt)
    cols, rows = _extent(n)
    cx, cy = 0.5 * PITCH * (cols - 1) - 8.0, 0.5 * PITCH * (rows - 1) - 8.0
    if layout == "stacked":
        view = dict(origin=(0.1, 0.05, 0.8), forward=(0.0, 0.1, 1.0), fov=70.0, aperture=0.01)
    else:
        dist = 3.0 + 1.1 * max(PITCH * cols, PITCH * rows)
        view = dict(origin=(cx + 0.08, cy + 0.1, dist), forward=(0.0, 0.02, 1.0), fov=60.0, aperture=0.01)
    return gt, sa, view


def merge_duplicates(gt):
    """The same three float32 vertices in the same order under the same instance transform are one hit, whichever BLAS reports it
    (`pairs`, `stacked`): geom64's duplicate classes, which it forms per BLAS, joined across BLAS."""
    seen = {}
    for b, st in enumerate(gt.sets):
        key = gt.sa.blas["invT"][b].tobytes()
        for v, i in zip(st["tri"], st["tri_idx"]):
            gt.dup[i] = seen.setdefault((key, v.astype(np.float32).tobytes()), int(gt.dup[i]))


# ---- a frame that shows the scene ------------------------------------------------------------------------------------------------------
def assert_seen(extend, connect, what=""):
    """The oracle's work counters of a frame (Oracle.render's extend and connect counters): the frame entered instances, walked BLAS
    nodes, tested primitives and traced shadow rays.  A camera facing away from the scene has tlas_visits == rays and nothing else."""
    assert extend["inst_visits"] > extend["rays"] / 20 and extend["node_visits"] > 0 and extend["prim_tests"] > 0 and connect["rays"] >= 1, \
        f"{what}: the frame does not show the scene (extend {extend}, shadow rays {connect['rays']})"
    return f"{extend['inst_visits']} / {extend['rays']}"

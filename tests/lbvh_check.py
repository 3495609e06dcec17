"""Shared pieces of the linear BVH builder's tests (test_lbvh_cpu.py, test_gpu_lbvh.py): the input scenes and the structural
invariants every tree the builder emits must satisfy, restated in numpy from the wire format alone."""
import numpy as np

from magr_ray_tracer_amd import _lib as W
from magr_ray_tracer_amd.scenes import Scene, _std_materials

MAX_DEPTH = 63      # lbvh_common.h: height <= 3k + b <= 63 < the 64-entry traversal stack


# ---- inputs -------------------------------------------------------------------------------------------------------------------------
def _soup(rng, n, lo=-4.0, hi=4.0, size=0.45):
    c = rng.uniform(lo, hi, (n, 1, 3))
    return (c + size * rng.normal(size=(n, 3, 3))).astype(np.float32)


def _scene():
    s = Scene()
    _std_materials(s)
    return s


def soup(n, seed=1):
    s = _scene()
    s.AddTriangles(_soup(np.random.default_rng(seed), n), "sand")
    return s


def mixed():
    """Triangles and spheres, with a plane inside the range (it keeps the empty box)."""
    rng = np.random.default_rng(2)
    s = _scene()
    s.AddTriangles(_soup(rng, 300), "sand")
    for k in range(40):
        s.AddSphere(rng.uniform(-4, 4, 3), rng.uniform(0.1, 0.7), "red")
        if k == 20:
            s.AddPlane((0, 1, 0), 3.0, "grey")
    s.AddTriangles(_soup(rng, 100), "green")
    return s


def one_centroid(n=4097):
    """Triangles and spheres whose boxes are symmetric about the origin: every centroid is exactly (0, 0, 0)."""
    rng = np.random.default_rng(3)
    s = _scene()
    a = rng.uniform(0.1, 2.0, (n // 2, 3)).astype(np.float32)
    tris = np.stack([-a, a, np.zeros_like(a)], axis=1)
    s.AddTriangles(tris, "sand")
    for r in rng.uniform(0.1, 1.0, n - n // 2):
        s.AddSphere((0, 0, 0), r, "red")
    return s


def duplicates():
    rng = np.random.default_rng(4)
    s = _scene()
    s.AddTriangles(np.tile(_soup(rng, 5), (300, 1, 1)), "sand")
    return s


def flat_patch():
    """A 40 x 40 grid of triangles in the plane y = 1.5: zero centroid extent on one axis."""
    s = _scene()
    g = np.linspace(-3, 3, 41, dtype=np.float32)
    X, Z = np.meshgrid(g, g)
    P = np.stack([X, np.full_like(X, 1.5), Z], -1)
    a, b, c, d = P[:-1, :-1], P[1:, :-1], P[1:, 1:], P[:-1, 1:]
    tris = np.concatenate([np.stack([a, b, c], -2).reshape(-1, 3, 3), np.stack([a, c, d], -2).reshape(-1, 3, 3)])
    s.AddTriangles(tris, "grey")
    return s


def wide_range():
    """Triangles of size 1e-3 to 1e4 at distances up to 1e6 in one scene."""
    rng = np.random.default_rng(5)
    n = 3000
    scale = 10.0 ** rng.uniform(-3, 4, (n, 1, 1))
    centre = np.sign(rng.normal(size=(n, 1, 3))) * 10.0 ** rng.uniform(-3, 6, (n, 1, 3))
    s = _scene()
    s.AddTriangles((centre + scale * rng.normal(size=(n, 3, 3))).astype(np.float32), "sand")
    return s


def non_finite():
    """A soup with one triangle whose last vertex is NaN (its box keeps a NaN lane) and one with an infinite vertex."""
    rng = np.random.default_rng(6)
    t = _soup(rng, 500)
    t[100, 2, 1] = np.nan
    t[300, 0, 0] = np.inf
    t[301, 1, 2] = -np.inf
    s = _scene()
    s.AddTriangles(t, "sand")
    return s


def geometric(n=160):
    """Small triangles at positions 1.2^i along the diagonal: each quantized position halves towards cell 0, the Morton codes share
    ever longer prefixes and the radix tree degenerates into a chain as deep as the Morton bits allow (the index bits of the many
    triangles left in cell 0 continue it).  wide-range drives the height closest to the 3k + b bound."""
    base = (1.2 ** np.arange(n))[:, None, None] * np.ones((1, 1, 3))
    off = np.array([[0, 0, 0], [1e-7, 0, 0], [0, 1e-7, 0]])
    s = _scene()
    s.AddTriangles((base * (1 + off)).astype(np.float32), "sand")
    return s


INPUTS = {
    "soup-1": lambda: soup(1), "soup-2": lambda: soup(2), "soup-3": lambda: soup(3), "soup-7": lambda: soup(7),
    "soup-600": lambda: soup(600), "soup-50k": lambda: soup(50000), "mixed": mixed, "one-centroid": one_centroid,
    "duplicates": duplicates, "flat-patch": flat_patch, "wide-range": wide_range, "non-finite": non_finite, "geometric": geometric,
}


def prims_of(s):
    """The scene's primitive array (no acceleration structure needed)."""
    from magr_ray_tracer_amd.scene import _view
    return _view(s._lib.rth_primitives, s._h, W.Primitive)


# ---- invariants -----------------------------------------------------------------------------------------------------------------------
def _lo(a, b):
    return np.where(a < b, a, b)


def _hi(a, b):
    return np.where(a > b, a, b)


def tmin(a, b):
    """lbvh_common.h lb_min: NaN ignored, -0 < +0."""
    return np.where(np.isnan(a), b, np.where(np.isnan(b), a, np.where(a < b, a, np.where(b < a, b, np.where(np.signbit(a), a, b)))))


def tmax(a, b):
    return np.where(np.isnan(a), b, np.where(np.isnan(b), a, np.where(a > b, a, np.where(b > a, b, np.where(np.signbit(a), b, a)))))


def prim_boxes(prims):
    """BVH2::CreateBVHPrimData's boxes, (n, 4) min and max."""
    n = len(prims)
    mn = np.tile(np.array([1e34, 1e34, 1e34, 0], np.float32), (n, 1))
    mx = np.tile(np.array([-1e34, -1e34, -1e34, 0], np.float32), (n, 1))
    zero = np.zeros((n, 1), np.float32)
    tri = prims["objType"] == W.PRIM_TRIANGLE
    sph = prims["objType"] == W.PRIM_SPHERE
    pts = [prims[v][:, :3] for v in ("v0", "v1", "v2")]
    sph_pos = prims["v0"][:, :3]
    sph_r = prims["v1"][:, 0:1]                        # RtSphere: pos (16 B), then r
    pts_s = [sph_pos + sph_r, sph_pos - sph_r]
    for p, sel in [(pts[0], tri), (pts[1], tri), (pts[2], tri), (pts_s[0], sph), (pts_s[1], sph)]:
        p4 = np.concatenate([p.astype(np.float32), zero], 1)
        mn = np.where(sel[:, None], _lo(mn, p4), mn)
        mx = np.where(sel[:, None], _hi(mx, p4), mx)
    return mn, mx


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def check_tree(prims, first, count, nodes, idx, stats, node_base=0, idx_base=0, max_leaf=8, what=""):
    """Every structural invariant of one appended LBVH block; returns the tree's height."""
    n = count
    assert len(idx) == n and len(nodes) == 2 * stats["leaves"] - 1 == stats["nodes"], what
    # each primitive of the range exactly once
    assert np.array_equal(np.sort(idx.astype(np.int64)), np.arange(first, first + n)), f"{what}: primIdx is not a permutation of the range"
    cnt, fst = nodes["count"].astype(np.int64), nodes["first"].astype(np.int64)
    leaf = cnt > 0
    assert leaf.sum() == stats["leaves"], what
    assert ((cnt[leaf] >= 1) & (cnt[leaf] <= max_leaf)).all(), f"{what}: leaf counts {cnt[leaf].min()}..{cnt[leaf].max()}"
    lstart = fst[leaf] - idx_base
    assert ((lstart >= 0) & (lstart + cnt[leaf] <= n)).all(), f"{what}: leaf range outside the block's primIdx"
    # interior: the pair (first, first + 1) lies inside the block; walk from the root, every node exactly once
    kid = fst[~leaf] - node_base
    assert ((kid >= 1) & (kid + 1 < len(nodes)) & (kid % 2 == 1)).all(), f"{what}: child pair outside the appended block"
    depth = np.full(len(nodes), -1)
    depth[0] = 0
    order = [0]
    for i in order:
        if cnt[i] == 0:
            c = int(fst[i] - node_base)
            for j in (c, c + 1):
                assert depth[j] == -1, f"{what}: node {j} reached twice"
                depth[j] = depth[i] + 1
                order.append(j)
    assert (depth >= 0).all(), f"{what}: unreachable nodes"
    # the leaves' ranges tile the block's primIdx
    cover = np.zeros(n, np.int64)
    np.add.at(cover, np.concatenate([np.arange(s, s + c) for s, c in zip(lstart, cnt[leaf])]), 1)
    assert (cover == 1).all(), f"{what}: leaf ranges overlap or leave gaps"
    # boxes: interior = union of its children, bit for bit; leaf = union of its primitives' boxes
    mn, mx = nodes["aabbMin"], nodes["aabbMax"]
    ii = np.where(~leaf)[0]
    L, R = kid, kid + 1
    assert np.array_equal(_bits(mn[ii]), _bits(tmin(mn[L], mn[R]))) and np.array_equal(_bits(mx[ii]), _bits(tmax(mx[L], mx[R]))), \
        f"{what}: an interior box is not the union of its children"
    pmn, pmx = prim_boxes(prims)
    li = np.where(leaf)[0]
    acc_mn, acc_mx = pmn[idx[lstart]].copy(), pmx[idx[lstart]].copy()
    for j in range(1, int(cnt[leaf].max())):
        sel = cnt[leaf] > j
        g = idx[lstart[sel] + j]
        acc_mn[sel], acc_mx[sel] = tmin(acc_mn[sel], pmn[g]), tmax(acc_mx[sel], pmx[g])
    assert np.array_equal(_bits(mn[li]), _bits(acc_mn)) and np.array_equal(_bits(mx[li]), _bits(acc_mx)), \
        f"{what}: a leaf box is not the union of its primitives' boxes"
    height = int(depth.max())
    b = int(np.ceil(np.log2(n))) if n > 1 else 0
    bound = 3 * stats["morton_bits"] + b
    assert stats["depth"] == height <= bound <= MAX_DEPTH, (what, stats["depth"], height, bound)
    # SAH cost in BVH2::TotalCost's metric (sum over leaves of count * area, float32): within rounding of the float64 sum
    e = (mx[li, :3].astype(np.float64) - mn[li, :3].astype(np.float64))
    ref = float(np.sum(cnt[leaf] * (e[:, 0] * e[:, 1] + e[:, 1] * e[:, 2] + e[:, 2] * e[:, 0])))
    if np.isfinite(ref) and ref > 0:
        assert abs(stats["sah_cost"] - ref) <= 1e-3 * ref, (what, stats["sah_cost"], ref)
    return height


def validate(sa, accel):
    """rt_validate_scene (the host-side checks rt_upload_scene runs) on a scene's arrays."""
    lib = W.device_lib()
    nodes = sa.nodes(accel)
    P = W.ptr
    return lib.rt_validate_scene(accel, P(sa.prims), len(sa.prims), P(sa.mats), len(sa.mats), P(sa.tex) if len(sa.tex) else None,
                                 len(sa.tex), P(sa.lights) if len(sa.lights) else None, len(sa.lights), P(nodes), len(nodes),
                                 P(sa.primIdx), len(sa.primIdx), P(sa.tlas), len(sa.tlas), P(sa.blas), len(sa.blas))

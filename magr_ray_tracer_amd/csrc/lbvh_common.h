// lbvh_common.h — the scalar rules of the linear BVH builder (rt_build_bvh2, include/rt355.h), compiled by hipcc for the device
// build (lbvh.hip) and by g++ for its sequential host restatement (host/lbvh_host.cpp).  Both builds call these functions and
// nothing else that computes a value, so they produce identical node and primIdx arrays; that equality is the builder's oracle.
//
// The build of the primitives [first, first + n) of a scene:
//   1. box:   each primitive's box by the rule of BVH2::CreateBVHPrimData (accel_build.cpp): triangles fold v0, v1, v2 into the
//             empty box (+-1e34, w 0) with a < b ? a : b, spheres pos -+ r, planes keep the empty box.  centroid = (min + max) * 0.5.
//   2. keys:  centroids quantized to k bits per axis against the bounds of the finite centroids, Morton-interleaved into 3k bits,
//             then the local index in b = ceil(log2 n) bits: key = morton << b | i.  k = min(21, (63 - b) / 3), so every key has at
//             most L = 3k + b <= 63 significant bits and all keys are distinct: the sort order is fully determined.
//   3. sort:  ascending keys (the device sorts pairs by radix, the host by std::sort).
//   4. tree:  Karras (HPG 2012) radix tree: internal node i of n - 1 (root 0), leaf k of n is sorted position k.  One bottom-up pass
//             (the second visitor of a node computes it) fills box, count, SAH cost, TotalCost and height.
//   5. SAH collapse: a node becomes one leaf when count <= RT_MIN_LEAF_PRIMS, or count <= max_leaf and
//             C_i * count * A <= C_t * A + cost(L) + cost(R)   (A: BVH2::CalculateNodeCost's area, cost(leaf) = C_i * count * A).
//   6. emit:  wire format of BVH2 (RtBVHNode2 + primIdx).  The root is node nodeBase.  Internal node i survives when neither it nor
//             any ancestor collapsed; the r-th survivor in index order (r = exclusive prefix count of survivors) puts its children
//             at nodeBase + 1 + 2r and nodeBase + 2 + 2r.  A leaf holds primIdx[idxBase + s, + count) where s is the start of its
//             sorted range; primIdx[idxBase + s] = global id of the s-th primitive in key order.  Nodes: 1 + 2 * survivors.
//
// Depth bound.  Distinct keys of L significant bits: the root's common prefix is >= 64 - L bits, an internal node's prefix is
// strictly longer than its parent's, and two distinct keys share at most 63 bits.  So a root-to-leaf path passes at most L internal
// nodes and the tree's height (edges, BVH2::Depth and scene.hip's bvh2_depth, which counts the root as 0) is <= L <= 63: every
// tree fits the 64-entry traversal stack rt_validate_scene checks.  The collapse only lowers it.
//
// Floating point: strict binary32 in source order on both sides (-ffp-contract=off everywhere, correctly rounded division on the
// device); no libm call.  Unions of boxes use lb_min / lb_max, a total order (NaN is ignored, -0 < +0), so a union is the same
// whatever order it is taken in; fminf / fmaxf differ on +-0 between x86 and AMDGPU.
#pragma once
#include <stdint.h>
#include "../../include/rt355_types.h"

#if defined(__HIPCC__) || defined(__CUDACC__)
#define LB_HD __host__ __device__ inline
#else
#define LB_HD inline
#endif

namespace lbvh {

constexpr int kMaxAxisBits = 21;
constexpr uint32_t kNone = 0xffffffffu;

// defaults: measured on the MI355X, see profiles/r05_lbvh.txt
constexpr int   kDefaultMaxLeaf = 8;
constexpr float kDefaultCostTraverse = 1.0f;
constexpr float kDefaultCostIntersect = 1.0f;
constexpr int   kMaxLeafLimit = 127;           // larger leaves would lose the derived traversal layout (scene.hip, layout 1)

struct Box { float mn[4], mx[4]; };

// per node of the radix tree (internal i at i, leaf k at n - 1 + k)
struct NodeRec {
    Box box;
    uint32_t count, first;                     // primitives; start of the sorted range
    float cost, total;                         // SAH cost with C_t / C_i; BVH2::TotalCost of the emitted subtree
    uint32_t height, leaves, collapse, _pad;   // collapse: this node is emitted as one leaf
};

LB_HD float lo(float a, float b) { return a < b ? a : b; }   // Aabb::Grow of accel_build.cpp
LB_HD float hi(float a, float b) { return a > b ? a : b; }
LB_HD bool  isnan_(float a) { return a != a; }
LB_HD bool  neg_(float a) { uint32_t u; __builtin_memcpy(&u, &a, 4); return (u >> 31) != 0; }
// total-order min / max for unions: a NaN operand is ignored, -0 < +0
LB_HD float lb_min(float a, float b)
{
    if (isnan_(a)) return b;
    if (isnan_(b)) return a;
    if (a < b) return a;
    if (b < a) return b;
    return neg_(a) ? a : b;
}
LB_HD float lb_max(float a, float b)
{
    if (isnan_(a)) return b;
    if (isnan_(b)) return a;
    if (a > b) return a;
    if (b > a) return b;
    return neg_(a) ? b : a;
}

LB_HD Box empty_box()
{
    Box b;
    for (int k = 0; k < 3; k++) { b.mn[k] = 1e34f; b.mx[k] = -1e34f; }
    b.mn[3] = b.mx[3] = 0.0f;
    return b;
}
LB_HD void grow(Box& b, float x, float y, float z)
{
    b.mn[0] = lo(b.mn[0], x); b.mn[1] = lo(b.mn[1], y); b.mn[2] = lo(b.mn[2], z); b.mn[3] = lo(b.mn[3], 0.0f);
    b.mx[0] = hi(b.mx[0], x); b.mx[1] = hi(b.mx[1], y); b.mx[2] = hi(b.mx[2], z); b.mx[3] = hi(b.mx[3], 0.0f);
}
// BVH2::CreateBVHPrimData
LB_HD Box prim_box(const RtPrimitive& p)
{
    Box b = empty_box();
    if (p.objType == RT_PRIM_TRIANGLE) {
        const RtTriangle& t = p.obj.triangle;
        grow(b, t.v0.x, t.v0.y, t.v0.z); grow(b, t.v1.x, t.v1.y, t.v1.z); grow(b, t.v2.x, t.v2.y, t.v2.z);
    } else if (p.objType == RT_PRIM_SPHERE) {
        const RtSphere& s = p.obj.sphere;
        grow(b, s.pos.x + s.r, s.pos.y + s.r, s.pos.z + s.r);
        grow(b, s.pos.x - s.r, s.pos.y - s.r, s.pos.z - s.r);
    }
    return b;
}
LB_HD Box box_union(const Box& a, const Box& b)
{
    Box r;
    for (int k = 0; k < 4; k++) { r.mn[k] = lb_min(a.mn[k], b.mn[k]); r.mx[k] = lb_max(a.mx[k], b.mx[k]); }
    return r;
}
LB_HD float centroid(const Box& b, int axis) { return (b.mn[axis] + b.mx[axis]) * 0.5f; }
LB_HD bool  finite_(float a) { return a - a == 0.0f; }
// BVH2::CalculateNodeCost's area (no clamp: empty and NaN boxes give inf / NaN, which the comparisons below handle)
LB_HD float area(const Box& b)
{
    const float ex = b.mx[0] - b.mn[0], ey = b.mx[1] - b.mn[1], ez = b.mx[2] - b.mn[2];
    return ex * ey + ey * ez + ez * ex;
}

// Centroid bounds are reduced as order-preserving 32-bit keys (the device with atomicMin / atomicMax, the host in a loop): over finite
// values the key order is lb_min's (-0 < +0), so both sides find the same bounds in any order.
LB_HD uint32_t order_key(float f) { uint32_t u; __builtin_memcpy(&u, &f, 4); return (u >> 31) ? ~u : (u | 0x80000000u); }
LB_HD float order_unkey(uint32_t k) { const uint32_t u = (k >> 31) ? (k & 0x7fffffffu) : ~k; float f; __builtin_memcpy(&f, &u, 4); return f; }
constexpr uint32_t kKeyMinInit = 0xffffffffu, kKeyMaxInit = 0u;   // no finite centroid seen

// b = ceil(log2 n) index bits, k Morton bits per axis
LB_HD int index_bits(uint32_t n) { int b = 0; while (b < 32 && ((uint64_t)1 << b) < n) b++; return b; }
LB_HD int axis_bits(uint32_t n) { const int k = (63 - index_bits(n)) / 3; return k < kMaxAxisBits ? k : kMaxAxisBits; }

// Quantizer parameters of one axis from the bounds of the finite centroids (lo > hi: there were none).  An axis of zero, negative
// or overflowing extent gets scale 0: every centroid lands in cell 0 of it.
LB_HD float axis_scale(float clo, float chi, int k)
{
    if (!(clo <= chi)) return 0.0f;
    const float ext = chi - clo;
    return (ext > 0.0f && finite_(ext)) ? (float)(1u << k) / ext : 0.0f;
}
// Total: NaN, -inf and values below the bounds go to cell 0, +inf and values above to the last cell.  The clamp is done in float
// so that the conversion only ever sees [0, 2^k - 1] (out-of-range float -> int is undefined and differs between x86 and AMDGPU).
LB_HD uint32_t quantize(float c, float clo, float scale, int k)
{
    float q = (c - clo) * scale;
    const float top = (float)((1u << k) - 1u);
    if (!(q > 0.0f)) q = 0.0f;
    if (q > top) q = top;
    return (uint32_t)q;
}
LB_HD uint64_t spread3(uint32_t v)   // bit j of v -> bit 3j
{
    uint64_t x = v & 0x1fffffu;
    x = (x | x << 32) & 0x1f00000000ffffull;
    x = (x | x << 16) & 0x1f0000ff0000ffull;
    x = (x | x << 8) & 0x100f00f00f00f00full;
    x = (x | x << 4) & 0x10c30c30c30c30c3ull;
    x = (x | x << 2) & 0x1249249249249249ull;
    return x;
}
// key of local primitive i: x in the highest bit of each triple
LB_HD uint64_t make_key(const Box& b, const float clo[3], const float scale[3], int k, int bIdx, uint32_t i)
{
    const uint64_t m = spread3(quantize(centroid(b, 0), clo[0], scale[0], k)) << 2 |
                       spread3(quantize(centroid(b, 1), clo[1], scale[1], k)) << 1 |
                       spread3(quantize(centroid(b, 2), clo[2], scale[2], k));
    return m << bIdx | (uint64_t)i;
}

LB_HD int clz64(uint64_t x) { return x ? __builtin_clzll(x) : 64; }
LB_HD int delta(const uint64_t* keys, int64_t n, int64_t i, int64_t j)
{
    if (j < 0 || j >= n) return -1;
    return clz64(keys[i] ^ keys[j]);
}
// Karras 2012, internal node i of n - 1 over distinct sorted keys: children (tree ids: internal < n - 1 <= leaf) and sorted range
LB_HD void karras_node(const uint64_t* keys, int64_t n, int64_t i, uint32_t& left, uint32_t& right, uint32_t& first, uint32_t& last)
{
    const int d = delta(keys, n, i, i + 1) > delta(keys, n, i, i - 1) ? 1 : -1;
    const int dmin = delta(keys, n, i, i - d);
    int64_t lmax = 2;
    while (delta(keys, n, i, i + lmax * d) > dmin) lmax *= 2;
    int64_t l = 0;
    for (int64_t t = lmax / 2; t >= 1; t /= 2)
        if (delta(keys, n, i, i + (l + t) * d) > dmin) l += t;
    const int64_t j = i + l * d;
    const int dnode = delta(keys, n, i, j);
    int64_t s = 0, t = l;
    do {
        t = (t + 1) >> 1;
        if (delta(keys, n, i, i + (s + t) * d) > dnode) s += t;
    } while (t > 1);
    const int64_t g = i + s * d + (d < 0 ? -1 : 0);
    const int64_t a = i < j ? i : j, z = i < j ? j : i;
    left = (uint32_t)(a == g ? (n - 1) + g : g);
    right = (uint32_t)(z == g + 1 ? (n - 1) + g + 1 : g + 1);
    first = (uint32_t)a; last = (uint32_t)z;
}

struct Params { uint32_t maxLeaf; float ct, ci; };

// Quantizer of the range from its reduced centroid key bounds (minKey / maxKey as left by the reduction)
LB_HD void quantizer(const uint32_t minKey[3], const uint32_t maxKey[3], int k, float clo[3], float scale[3])
{
    for (int a = 0; a < 3; a++) {
        const bool any = minKey[a] != kKeyMinInit;
        clo[a] = any ? order_unkey(minKey[a]) : 0.0f;
        scale[a] = any ? axis_scale(clo[a], order_unkey(maxKey[a]), k) : 0.0f;
    }
}

// The argument checks both builds share (nothing is launched or written when they fail); NULL when the call is valid.
inline const char* check_args(const RtBuildOptions* o, const RtPrimitive* prims, int32_t nPrims, int32_t first, int32_t count,
                              uint32_t nodeBase, uint32_t idxBase, const RtBVHNode2* nodes, int32_t nodeCap, const int32_t* nNodes,
                              const uint32_t* primIdx, Params& P)
{
    P = Params{ (uint32_t)kDefaultMaxLeaf, kDefaultCostTraverse, kDefaultCostIntersect };
    if (o) {
        if (o->max_leaf < RT_MIN_LEAF_PRIMS || o->max_leaf > kMaxLeafLimit) return "max_leaf must be in [RT_MIN_LEAF_PRIMS, 127]";
        if (!(o->cost_traverse >= 0.0f && o->cost_traverse <= 1e30f)) return "cost_traverse must be finite and >= 0";
        if (!(o->cost_intersect > 0.0f && o->cost_intersect <= 1e30f)) return "cost_intersect must be finite and > 0";
        P = Params{ (uint32_t)o->max_leaf, o->cost_traverse, o->cost_intersect };
    }
    if (!prims || !nodes || !nNodes || !primIdx) return "missing array";
    if (count <= 0) return "empty primitive range (count <= 0)";
    if (count > (1 << 30)) return "more than 2^30 primitives";
    if (first < 0 || nPrims < 0 || (int64_t)first + count > (int64_t)nPrims) return "primitive range outside [0, nPrims)";
    if ((int64_t)nodeCap < 2 * (int64_t)count - 1) return "nodeCap is smaller than 2 * count - 1";
    if ((uint64_t)nodeBase + 2 * (uint64_t)count - 1 > 0xffffffffull || (uint64_t)idxBase + (uint64_t)count > 0xffffffffull)
        return "nodeBase / idxBase + the tree overflow 32-bit ids";
    return nullptr;
}

LB_HD NodeRec leaf_rec(const Box& b, uint32_t k, const Params& P)
{
    NodeRec r;
    r.box = b; r.count = 1; r.first = k;
    const float A = area(b);
    r.total = 1.0f * A;
    r.cost = P.ci * r.total;
    r.height = 0; r.leaves = 1; r.collapse = 1; r._pad = 0;
    return r;
}
// internal node from its children (left, right in this order: the result does not depend on which child finished last)
LB_HD NodeRec combine(const NodeRec& L, const NodeRec& R, uint32_t first, const Params& P)
{
    NodeRec r;
    r.box = box_union(L.box, R.box);
    r.count = L.count + R.count; r.first = first;
    const float A = area(r.box);
    const float asLeaf = (float)r.count * A;                   // CalculateNodeCost(node, count)
    const float leafCost = P.ci * asLeaf;
    const float splitCost = P.ct * A + L.cost + R.cost;
    r.collapse = (r.count <= (uint32_t)RT_MIN_LEAF_PRIMS || (r.count <= P.maxLeaf && leafCost <= splitCost)) ? 1u : 0u;
    if (r.collapse) { r.cost = leafCost; r.total = asLeaf; r.height = 0; r.leaves = 1; }
    else {
        r.cost = splitCost; r.total = L.total + R.total;
        r.height = 1 + (L.height > R.height ? L.height : R.height); r.leaves = L.leaves + R.leaves;
    }
    r._pad = 0;
    return r;
}
// internal node i survives (is emitted as an interior node): it did not collapse and no ancestor did.  An ancestor can only have
// collapsed while its count is <= max_leaf, so the walk stops at the first ancestor above that (at most max_leaf steps).
LB_HD uint32_t survives(const NodeRec* rec, const uint32_t* parent, uint32_t i, uint32_t maxLeaf)
{
    if (rec[i].collapse) return 0;
    for (uint32_t p = parent[i]; p != kNone && rec[p].count <= maxLeaf; p = parent[p])
        if (rec[p].collapse) return 0;
    return 1;
}
// emitted node for tree node c (internal or leaf id), given the survivor ranks
LB_HD RtBVHNode2 emit(const NodeRec& r, uint32_t c, uint32_t nInternal, const uint32_t* rank, uint32_t nodeBase, uint32_t idxBase)
{
    RtBVHNode2 o;
    o.aabbMin = RtFloat4{ r.box.mn[0], r.box.mn[1], r.box.mn[2], r.box.mn[3] };
    o.aabbMax = RtFloat4{ r.box.mx[0], r.box.mx[1], r.box.mx[2], r.box.mx[3] };
    if (c >= nInternal || r.collapse) { o.first = idxBase + r.first; o.count = r.count; }
    else { o.first = nodeBase + 1 + 2 * rank[c]; o.count = 0; }
    o._pad[0] = o._pad[1] = 0;
    return o;
}

} // namespace lbvh

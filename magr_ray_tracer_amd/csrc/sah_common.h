// sah_common.h — the rules of the GPU build of the default SAH BLAS (rt_build_bvh2_sah, include/rt355.h), compiled by hipcc for the
// device build (sah.hip) and by g++ for its sequential host restatement (host/sah_host.cpp).  Both call these functions and nothing
// else that computes a value.  Their arrays equal what BVH2::BuildBLAS (host/accel_build.cpp) appends with alpha = 1, byte for byte.
//
// Why that is possible.  With alpha >= 1 BuildBLAS never evaluates a spatial split: the overlap of two child boxes can never exceed
// the BLAS root's area, so `overlap / rootArea > alpha` is never true (accel_build.cpp:183).  What is left is a pure function of the
// primitive boxes: per node three min / max folds (node bounds, centroid bounds, 8 bin boxes per axis), a fixed sweep over 7 planes
// x 3 axes with strict '<', a stable partition, and the LIFO numbering of the work stack (accel_build.cpp:166-214).
//
// The formulation.  Level by level, every open node owns a segment [home, home + cnt) of the ref arrays; its children split that
// segment (left part first), so a ref never leaves its node's segment and each node's refs stay in ascending primitive order.  A
// node of more than kSmall refs is evaluated by reductions over its segment; a node of at most kSmall refs is finished, with its
// whole subtree, by build_small (one thread on the device), which replays BuildBVH's work stack on that subtree.  Numbering comes
// afterwards: interior counts bottom-up, then top-down the pop rank r of every node (interior nodes popped before it) and its ref
// offset.  The r-th interior node popped puts its children at nodeBase + 1 + 2r and nodeBase + 2 + 2r; a right child is popped
// right after its parent, a left child after the parent's whole right subtree; leaves take primIdx in pop order.
//
// Ties.  BuildBLAS folds in ref order and a tie goes to the later element: lo / hi below (Aabb::Grow) and glibc's fminf / fmaxf
// (UpdateNodeBounds) return their second operand when the two compare equal, so the sign of a zero in a box depends on the order
// of the refs.  A parallel fold reduces 64-bit keys (value order, then ref position, then the sign bit): min / max of keys is
// order-independent and selects the last of the equal values, as the sequential fold does.  No float atomics.
//
// Floating point: strict binary32 in source order on both sides (-ffp-contract=off, correctly rounded division on the device,
// denormals kept); no libm call.
#pragma once
#include <stdint.h>
#include "../../include/rt355_types.h"

#if defined(__HIPCC__) || defined(__CUDACC__)
#define SAH_HD __host__ __device__ inline
// a real call on the device (decide: see there); inline for linkage only, so that every translation unit may include the rules
#define SAH_HD_CALL __host__ __device__ inline __attribute__((noinline))
#else
#define SAH_HD inline
#define SAH_HD_CALL inline
#endif

namespace sah {

constexpr int      kBins = RT_BVH_BINS;        // 8
constexpr uint32_t kSmall = 32;                // subtrees of at most this many refs are finished by build_small
constexpr uint32_t kNone = 0xffffffffu;
constexpr float    kEmpty = 1e34f;             // Aabb's empty box (rt_host.h)
constexpr float    kFar = RT_REALLYFAR;        // initial value of the node-bounds and centroid-bounds folds

// refusals found during the build (bits of the device's status word)
constexpr uint32_t kBadInput = 1;              // a primitive box or centroid is not finite
constexpr uint32_t kBadBin = 2;                // a bin index from a NaN or an infinity
constexpr uint32_t kNoDecision = 4;            // > RT_MIN_LEAF_PRIMS refs, no leaf and no object split
constexpr uint32_t kInternal = 8;              // an inconsistency of the device build itself

// node kinds
constexpr uint32_t kOpen = 0, kLeaf = 1, kSplit = 2, kSmallRoot = 3;

struct Prim { float mn[3], mx[3], c[3]; uint32_t _pad; };   // box (w is +0 and not stored) and centroid of one primitive

SAH_HD float lo(float a, float b) { return a < b ? a : b; }   // accel_build.cpp:33
SAH_HD float hi(float a, float b) { return a > b ? a : b; }   // accel_build.cpp:34
SAH_HD uint32_t bits(float a) { uint32_t u; __builtin_memcpy(&u, &a, 4); return u; }
SAH_HD float from_bits(uint32_t u) { float a; __builtin_memcpy(&a, &u, 4); return a; }
SAH_HD bool finite_(float a) { return (bits(a) & 0x7f800000u) != 0x7f800000u; }

// CreateBVHPrimData (accel_build.cpp:85-102) and Aabb::Center (rt_host.h).  Grow folds with lo / hi from the empty box; its w
// lanes are lo(0, 0.0f) = hi(0, 0.0f) = +0 for every primitive, so every node's w lanes are +0 too and are not carried.
SAH_HD Prim prim_data(const RtPrimitive& p)
{
    Prim d;
    for (int k = 0; k < 3; k++) { d.mn[k] = kEmpty; d.mx[k] = -kEmpty; }
    auto grow = [&](float x, float y, float z) {
        d.mn[0] = lo(d.mn[0], x); d.mn[1] = lo(d.mn[1], y); d.mn[2] = lo(d.mn[2], z);
        d.mx[0] = hi(d.mx[0], x); d.mx[1] = hi(d.mx[1], y); d.mx[2] = hi(d.mx[2], z);
    };
    if (p.objType == RT_PRIM_TRIANGLE) {
        const RtTriangle& t = p.obj.triangle;
        grow(t.v0.x, t.v0.y, t.v0.z); grow(t.v1.x, t.v1.y, t.v1.z); grow(t.v2.x, t.v2.y, t.v2.z);
    } else if (p.objType == RT_PRIM_SPHERE) {
        const RtSphere& s = p.obj.sphere;
        const float r = s.r;
        grow(s.pos.x + r, s.pos.y + r, s.pos.z + r);
        grow(s.pos.x - r, s.pos.y - r, s.pos.z - r);
    }   // planes keep the empty box
    for (int a = 0; a < 3; a++) d.c[a] = (d.mn[a] + d.mx[a]) * 0.5f;
    d._pad = 0;
    return d;
}
SAH_HD bool prim_finite(const Prim& d)
{
    bool ok = true;
    for (int a = 0; a < 3; a++) ok = ok && finite_(d.mn[a]) && finite_(d.mx[a]) && finite_(d.c[a]);
    return ok;
}

// ---- order-independent folds -------------------------------------------------------------------------------------------------
// Key = value order (with -0 == +0) << 32 | position field << 1 | sign bit.  The smallest key_min is the smallest value and, among
// equal values, the largest position; the largest key_max is the largest value and, among equal values, the largest position:
// both are the element the sequential fold `acc = lo(acc, x)` / `acc = hi(acc, x)` ends on.  Positions are local primitive
// indices (< 2^30), which ascend along every node's refs.
constexpr uint64_t kKeyMinEmpty = ~0ull, kKeyMaxEmpty = 0ull;
SAH_HD uint32_t order32(float v)
{
    uint32_t u = bits(v);
    if ((u & 0x7fffffffu) == 0) u = 0;
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
SAH_HD uint64_t key_min(float v, uint32_t pos) { return ((uint64_t)order32(v) << 32) | ((uint64_t)(0x7fffffffu - pos) << 1) | (bits(v) >> 31); }
SAH_HD uint64_t key_max(float v, uint32_t pos) { return ((uint64_t)order32(v) << 32) | ((uint64_t)pos << 1) | (bits(v) >> 31); }
SAH_HD float key_value(uint64_t k)
{
    const uint32_t o = (uint32_t)(k >> 32);
    uint32_t u = (o & 0x80000000u) ? (o & 0x7fffffffu) : ~o;
    if (u == 0 && (k & 1)) u = 0x80000000u;
    return from_bits(u);
}

// Keys per open node: kmin[6] = min of box mn (x, y, z), min of centroid; kmax[6] = max of box mx, max of centroid.
SAH_HD void node_keys(const Prim& d, uint32_t pos, uint64_t kmin[6], uint64_t kmax[6])
{
    for (int a = 0; a < 3; a++) {
        kmin[a] = key_min(d.mn[a], pos); kmin[3 + a] = key_min(d.c[a], pos);
        kmax[a] = key_max(d.mx[a], pos); kmax[3 + a] = key_max(d.c[a], pos);
    }
}
// Node bounds (UpdateNodeBounds, accel_build.cpp:119-131: fminf / fmaxf from +-RT_REALLYFAR) and centroid bounds
// (FindBestObjectSplitPlane, :307-308: lo / hi from +-RT_REALLYFAR) of a non-empty node: the initial value is the first element
// of the fold, so the result is lo / hi of it and the last-selected element.  (glibc fminf(x, y) = x < y ? x : y for numbers.)
SAH_HD void node_from_keys(const uint64_t* kmin, const uint64_t* kmax, float mn[3], float mx[3], float cmin[3], float cmax[3])
{
    for (int a = 0; a < 3; a++) {
        mn[a] = lo(kFar, key_value(kmin[a])); cmin[a] = lo(kFar, key_value(kmin[3 + a]));
        mx[a] = hi(-kFar, key_value(kmax[a])); cmax[a] = hi(-kFar, key_value(kmax[3 + a]));
    }
}

// ---- split search (FindBestObjectSplitPlane, accel_build.cpp:303-336, without the overlap) ---------------------------------------
struct Bins { uint32_t n[3][kBins]; float mn[3][kBins][3], mx[3][kBins][3]; };   // per axis: counts, boxes (Aabb from the empty box)
constexpr int kBinKeys = 3 * kBins * 3;        // per open node: bin box keys (axis, bin, x y z); counts: 3 * kBins

// The bin of centroid c on an axis with centroid bounds cmin != cmax (:311-314).  False when the host's (int) conversion would see
// a NaN or an infinity: a centroid extent that overflows, or one so small that 8 / extent overflows.
SAH_HD bool bin_of(float c, float cmin, float cmax, int& b)
{
    const float scale = (float)kBins / (cmax - cmin);
    const float f = (c - cmin) * scale;
    if (!finite_(f)) return false;
    b = (int)f;
    if (b > kBins - 1) b = kBins - 1;
    return true;
}
SAH_HD void bins_clear(Bins& B)
{
    for (int a = 0; a < 3; a++) for (int b = 0; b < kBins; b++) {
        B.n[a][b] = 0;
        for (int k = 0; k < 3; k++) { B.mn[a][b][k] = kEmpty; B.mx[a][b][k] = -kEmpty; }
    }
}
SAH_HD void bins_from_keys(const uint64_t* bkmin, const uint64_t* bkmax, const uint32_t* bcnt, Bins& B)
{
    for (int a = 0; a < 3; a++) for (int b = 0; b < kBins; b++) {
        const int s = a * kBins + b;
        B.n[a][b] = bcnt[s];
        for (int k = 0; k < 3; k++) {
            B.mn[a][b][k] = bcnt[s] ? lo(kEmpty, key_value(bkmin[s * 3 + k])) : kEmpty;
            B.mx[a][b][k] = bcnt[s] ? hi(-kEmpty, key_value(bkmax[s * 3 + k])) : -kEmpty;
        }
    }
}
SAH_HD float area(const float mn[3], const float mx[3])          // Aabb::Area (:53-57)
{
    const float e0 = mx[0] - mn[0], e1 = mx[1] - mn[1], e2 = mx[2] - mn[2];
    return hi(0.0f, e0 * e1 + e0 * e2 + e1 * e2);
}
SAH_HD float node_cost(uint32_t count, const float mn[3], const float mx[3])   // CalculateNodeCost (:79-83)
{
    const float ex = mx[0] - mn[0], ey = mx[1] - mn[1], ez = mx[2] - mn[2];
    return (float)count * (ex * ey + ey * ez + ez * ex);
}

struct Decision { uint32_t kind; int32_t axis; float pos, leafCost; };

// The sweep (:317-333) and the leaf test of BuildBVH (:185; spatialCost stays RT_REALLYFAR).  False: the host builder's
// behaviour is undefined (it would take its spatial-split branch with axis -1).  Not inlined on the device: inlined behind the key
// decoding of k_sah_decide, ROCm 7.2's clang crashes in AMDGPU instruction selection.
SAH_HD_CALL bool decide(uint32_t count, const float mn[3], const float mx[3], const float cmin[3], const float cmax[3], const Bins& B,
                   Decision& d)
{
    float best = kFar, pos = 0.0f;
    int axis = 0;
    for (int a = 0; a < 3; a++) {
        if (cmin[a] == cmax[a]) continue;
        float lArea[kBins - 1], rArea[kBins - 1];
        int lCount[kBins - 1], rCount[kBins - 1];
        float lmn[3] = { kEmpty, kEmpty, kEmpty }, lmx[3] = { -kEmpty, -kEmpty, -kEmpty };
        float rmn[3] = { kEmpty, kEmpty, kEmpty }, rmx[3] = { -kEmpty, -kEmpty, -kEmpty };
        int sumL = 0, sumR = 0;
        for (int i = 0; i < kBins - 1; i++) {
            sumL += (int)B.n[a][i]; lCount[i] = sumL;
            for (int k = 0; k < 3; k++) { lmn[k] = lo(lmn[k], B.mn[a][i][k]); lmx[k] = hi(lmx[k], B.mx[a][i][k]); }
            lArea[i] = area(lmn, lmx);
            const int j = kBins - 1 - i;
            sumR += (int)B.n[a][j]; rCount[j - 1] = sumR;
            for (int k = 0; k < 3; k++) { rmn[k] = lo(rmn[k], B.mn[a][j][k]); rmx[k] = hi(rmx[k], B.mx[a][j][k]); }
            rArea[j - 1] = area(rmn, rmx);
        }
        const float scale = (cmax[a] - cmin[a]) / (float)kBins;
        for (int i = 0; i < kBins - 1; i++) {
            const float cost = (float)lCount[i] * lArea[i] + (float)rCount[i] * rArea[i];   // 0 * inf = NaN: never '<'
            if (cost < best) { best = cost; axis = a; pos = cmin[a] + scale * (float)(i + 1); }
        }
    }
    d.axis = axis; d.pos = pos;
    d.leafCost = node_cost(count, mn, mx);
    if (count <= RT_MIN_LEAF_PRIMS || d.leafCost < best) { d.kind = kLeaf; return true; }
    if (best < kFar) { d.kind = kSplit; return true; }
    return false;
}
SAH_HD bool goes_left(const Prim& d, int axis, float pos) { return d.c[axis] <= pos; }   // ObjectSplit (:337-340)

// ---- small subtrees ------------------------------------------------------------------------------------------------------------
struct LNode { float mn[3], mx[3]; uint32_t first, count, depth; float cost; };   // local ids and ref offsets
struct SubResult { uint32_t interiors, depth; float cost; };
constexpr int kErrBin = 1, kErrNoDecision = 2;

// One node evaluated as BuildBVH evaluates it, with sequential folds over refs[0, n).  Returns 0 or kErr*.
SAH_HD int eval_seq(const Prim* P, const uint32_t* refs, uint32_t n, float mn[3], float mx[3], Decision& d)
{
    float cmin[3], cmax[3];
    for (int a = 0; a < 3; a++) { mn[a] = kFar; mx[a] = -kFar; cmin[a] = kFar; cmax[a] = -kFar; }
    for (uint32_t i = 0; i < n; i++) {
        const Prim& p = P[refs[i]];
        for (int a = 0; a < 3; a++) {
            mn[a] = lo(mn[a], p.mn[a]); mx[a] = hi(mx[a], p.mx[a]);
            cmin[a] = lo(cmin[a], p.c[a]); cmax[a] = hi(cmax[a], p.c[a]);
        }
    }
    Bins B;
    bins_clear(B);
    for (int a = 0; a < 3; a++) {
        if (cmin[a] == cmax[a]) continue;
        for (uint32_t i = 0; i < n; i++) {
            const Prim& p = P[refs[i]];
            int b;
            if (!bin_of(p.c[a], cmin[a], cmax[a], b)) return kErrBin;
            B.n[a][b]++;
            for (int k = 0; k < 3; k++) { B.mn[a][b][k] = lo(B.mn[a][b][k], p.mn[k]); B.mx[a][b][k] = hi(B.mx[a][b][k], p.mx[k]); }
        }
    }
    return decide(n, mn, mx, cmin, cmax, B, d) ? 0 : kErrNoDecision;
}

// BuildBVH's work stack (:166-214) on a subtree of n <= kSmall refs: refs[0, n) in order (partitioned in place), tmp: n words,
// out: the refs in pop order, nodes: local ids (root 0; the k-th interior node popped has children 1 + 2k, 2 + 2k), 2n - 1 records.
// Leaves' `first` are offsets into out.  Returns 0 or kErr*.
SAH_HD int build_small(const Prim* P, uint32_t* refs, uint32_t* tmp, uint32_t n, uint32_t* out, LNode* nodes, SubResult& res)
{
    uint32_t stId[kSmall], stS[kSmall], stN[kSmall];     // each entry holds >= 1 ref of disjoint ranges: at most n <= kSmall
    int sp = 0;
    stId[sp] = 0; stS[sp] = 0; stN[sp] = n; sp++;
    uint32_t next = 1, outN = 0;
    while (sp > 0) {
        sp--;
        const uint32_t id = stId[sp], s = stS[sp], len = stN[sp];
        LNode& N = nodes[id];
        Decision d;
        const int rc = eval_seq(P, refs + s, len, N.mn, N.mx, d);
        if (rc) return rc;
        N.cost = d.leafCost; N.depth = 0;
        uint32_t nL = 0;
        bool leaf = d.kind == kLeaf;
        if (!leaf) {
            uint32_t k = 0;
            for (uint32_t i = 0; i < len; i++) if (goes_left(P[refs[s + i]], d.axis, d.pos)) tmp[k++] = refs[s + i];
            nL = k;
            for (uint32_t i = 0; i < len; i++) if (!goes_left(P[refs[s + i]], d.axis, d.pos)) tmp[k++] = refs[s + i];
            leaf = nL == 0 || nL == len;                  // the termination guard (:198): a forced leaf, refs in their order
            if (!leaf) for (uint32_t i = 0; i < len; i++) refs[s + i] = tmp[i];
        }
        if (leaf) {
            N.first = outN; N.count = len;
            for (uint32_t i = 0; i < len; i++) out[outN++] = refs[s + i];
            continue;
        }
        N.first = next; N.count = 0;
        next += 2;
        stId[sp] = N.first; stS[sp] = s; stN[sp] = nL; sp++;
        stId[sp] = N.first + 1; stS[sp] = s + nL; stN[sp] = len - nL; sp++;   // popped first
    }
    // BVH2::Depth and BVH2::TotalCost (:62-78) bottom-up: children have larger ids than their parent
    for (uint32_t j = next; j-- > 0;) {
        LNode& N = nodes[j];
        if (N.count > 0) continue;
        const LNode &L = nodes[N.first], &R = nodes[N.first + 1];
        N.depth = (L.depth > R.depth ? L.depth : R.depth) + 1;
        N.cost = L.cost + R.cost;
    }
    res.interiors = (next - 1) / 2; res.depth = nodes[0].depth; res.cost = nodes[0].cost;
    return 0;
}

// ---- the level-synchronous part and the numbering ----------------------------------------------------------------------------
struct BNode {
    float mn[3], mx[3];              // node bounds
    uint32_t home, cnt, kind, big;   // segment of the ref arrays; kOpen / kLeaf / kSplit / kSmallRoot; rank among the level's open nodes
    uint32_t left, nL;               // kSplit: build id of the left child (the right one is left + 1), refs going left
    int32_t axis; float pos;         // kSplit: the plane
    uint32_t interiors, depth;       // bottom-up: interior nodes and height of the subtree (BVH2::Depth)
    float cost;                      // bottom-up: BVH2::TotalCost of the subtree
    uint32_t rank, offset, gid;      // top-down: interior nodes popped before it, offset of its refs, output index (from nodeBase)
};

SAH_HD BNode open_node(uint32_t home, uint32_t cnt, uint32_t big)
{
    BNode N;
    for (int a = 0; a < 3; a++) { N.mn[a] = 0.0f; N.mx[a] = 0.0f; }
    N.home = home; N.cnt = cnt; N.kind = cnt > kSmall ? kOpen : kSmallRoot; N.big = cnt > kSmall ? big : kNone;
    N.left = kNone; N.nL = 0; N.axis = 0; N.pos = 0.0f;
    N.interiors = 0; N.depth = 0; N.cost = 0.0f;
    N.rank = 0; N.offset = 0; N.gid = 0;
    return N;
}
SAH_HD void apply_decision(BNode& N, const Decision& d)
{
    N.kind = d.kind; N.axis = d.axis; N.pos = d.pos; N.cost = d.leafCost;
    N.interiors = 0; N.depth = 0;
}
SAH_HD void apply_small(BNode& N, const LNode& root, const SubResult& r)
{
    for (int a = 0; a < 3; a++) { N.mn[a] = root.mn[a]; N.mx[a] = root.mx[a]; }
    N.interiors = r.interiors; N.depth = r.depth; N.cost = r.cost;
}
// After the partition counted nL: a split that leaves one side empty closes the node as a leaf (:198).  Returns the children's
// contribution (1 | big children << 32) to the exclusive scan that places them.
SAH_HD uint64_t count_split(BNode& N, uint32_t nL)
{
    if (N.kind != kSplit) return 0;
    if (nL == 0 || nL == N.cnt) { N.kind = kLeaf; return 0; }
    N.nL = nL;
    return 1ull | ((uint64_t)((nL > kSmall) + (N.cnt - nL > kSmall)) << 32);
}
// Children of a split node: scan = its exclusive prefix (splits before it | big children before it << 32); levelEnd: first id of
// the next level.
SAH_HD void make_children(BNode& N, uint64_t scan, uint32_t levelEnd, BNode& L, BNode& R)
{
    const uint32_t rank = (uint32_t)scan, big = (uint32_t)(scan >> 32);
    N.left = levelEnd + 2 * rank;
    L = open_node(N.home, N.nL, big);
    R = open_node(N.home + N.nL, N.cnt - N.nL, big + (N.nL > kSmall ? 1 : 0));
}
// Destination of the ref at position p of split node N (stable partition of the segment); lrank: refs going left before p.
SAH_HD uint32_t scatter_dst(const BNode& N, uint32_t p, uint32_t lrank, bool left)
{
    return left ? N.home + lrank : N.home + N.nL + (p - N.home - lrank);
}
SAH_HD void up(BNode& N, const BNode& L, const BNode& R)
{
    N.interiors = 1 + L.interiors + R.interiors;
    N.depth = (L.depth > R.depth ? L.depth : R.depth) + 1;
    N.cost = L.cost + R.cost;                        // TotalCost(first) + TotalCost(first + 1)
}
SAH_HD void down(const BNode& N, BNode& L, BNode& R)
{
    R.rank = N.rank + 1;                             // popped right after its parent
    L.rank = N.rank + 1 + R.interiors;               // after the parent's whole right subtree
    R.offset = N.offset;
    L.offset = N.offset + R.cnt;
    L.gid = 1 + 2 * N.rank;
    R.gid = 2 + 2 * N.rank;
}
SAH_HD RtBVHNode2 make_node(const float mn[3], const float mx[3], uint32_t first, uint32_t count)
{
    RtBVHNode2 o;
    o.aabbMin.x = mn[0]; o.aabbMin.y = mn[1]; o.aabbMin.z = mn[2]; o.aabbMin.w = 0.0f;
    o.aabbMax.x = mx[0]; o.aabbMax.y = mx[1]; o.aabbMax.z = mx[2]; o.aabbMax.w = 0.0f;
    o.first = first; o.count = count; o._pad[0] = 0; o._pad[1] = 0;
    return o;
}
// A node of the level part (not kSmallRoot), at output index N.gid
SAH_HD RtBVHNode2 emit_level(const BNode& N, uint32_t nodeBase, uint32_t idxBase)
{
    return N.kind == kSplit ? make_node(N.mn, N.mx, nodeBase + 1 + 2 * N.rank, 0) : make_node(N.mn, N.mx, idxBase + N.offset, N.cnt);
}
// Local node j of the small subtree rooted at N: its output index, and the record
SAH_HD uint32_t small_index(const BNode& N, uint32_t j) { return j == 0 ? N.gid : 2 * N.rank + j; }
SAH_HD RtBVHNode2 emit_small(const BNode& N, const LNode& L, uint32_t nodeBase, uint32_t idxBase)
{
    return L.count > 0 ? make_node(L.mn, L.mx, idxBase + N.offset + L.first, L.count) : make_node(L.mn, L.mx, nodeBase + 2 * N.rank + L.first, 0);
}

// rt_build_bvh2_sah's argument checks (those of rt_build_bvh2); nullptr when they pass
inline const char* check_args(const RtPrimitive* prims, int32_t nPrims, int32_t first, int32_t count, uint32_t nodeBase,
                              uint32_t idxBase, const RtBVHNode2* nodes, int32_t nodeCap, const int32_t* nNodes, const uint32_t* primIdx)
{
    if (!prims || !nodes || !nNodes || !primIdx) return "missing array";
    if (count <= 0) return "empty primitive range (count <= 0)";
    if (count > (1 << 30)) return "more than 2^30 primitives";
    if (first < 0 || nPrims < 0 || (int64_t)first + count > (int64_t)nPrims) return "primitive range outside [0, nPrims)";
    if ((int64_t)nodeCap < 2 * (int64_t)count - 1) return "nodeCap is smaller than 2 * count - 1";
    if ((uint64_t)nodeBase + 2 * (uint64_t)count - 1 > 0xffffffffull || (uint64_t)idxBase + (uint64_t)count > 0xffffffffull)
        return "nodeBase / idxBase + the tree overflow 32-bit ids";
    return nullptr;
}
inline const char* status_text(uint32_t st)
{
    if (st & kInternal) return "inconsistent device result";
    if (st & kBadInput) return "a primitive box or centroid is not finite";
    if (st & kBadBin) return "a bin index from a NaN or an infinity (centroid extent overflows or vanishes): BuildBLAS is undefined here";
    if (st & kNoDecision) return "a node with neither a leaf nor an object split (areas near 1e30): BuildBLAS is undefined here";
    return "ok";
}

} // namespace sah

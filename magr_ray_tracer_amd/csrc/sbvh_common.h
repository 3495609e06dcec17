// sbvh_common.h — the rules of the GPU build of SBVH BLAS trees (rt_build_bvh2_sbvh, include/rt355.h): BVH2::BuildBLAS
// (host/accel_build.cpp:166-505) for any alpha in [0, 1], spatial splits included.  Compiled by hipcc for the device build (sbvh.hip)
// and by g++ for its sequential host restatement (host/sbvh_host.cpp); both call these functions and nothing else that computes a
// value, and their arrays equal what BuildBLAS appends byte for byte.  Keys, lo / hi, area, node_cost, up / down and make_node are
// those of sah_common.h, which this header includes and does not change.
//
// The formulation.  Level by level, every node of the level owns a segment [home, home + cnt) of the level's ref array.  A ref is a
// box (exact), the local primitive id and the `clipped` flag of RefBounds (accel_build.cpp:112-117).  A node's refs stay in ascending
// primitive order and a primitive occurs at most once per node (a split yields at most one left and one right fragment), so the
// 64-bit key folds of sah_common.h stay valid with the primitive id as position: node bounds (of the padded boxes), centroid bounds,
// exact bounds, object bins and spatial bins (one contribution per ref and bin).  A split node's refs emit 0, 1 or 2 fragments into
// the next level's array: the left child's segment first, then the right child's; the refs of leaves leave the working arrays.
// There is no per-thread small-subtree path: a small subtree may duplicate its refs beyond any fixed local capacity, so every
// node goes through the level passes (a level costs a handful of launches over the refs that are still alive).
//
// Numbering is the LIFO numbering of sah_common.h with "refs of the leaves below" in place of "segment length": up() gives interior
// counts, heights and costs, after it a split node's cnt is overwritten with the refs of its subtree's leaves so that down() places
// the left child's refs after the right subtree's.
//
// Refusals (RT_E_UNSUPPORTED) are those of sah_common.h plus one: a spatial bin index f = scale * (x - bmin) that is not finite, is
// <= -1 or is >= 2^31 (kBadSpatialBin).  There BuildBLAS converts to int and indexes bins[]; BVH2::FindBestSpatialSplitPlane throws
// by the same rule.  The rule is applied where the index is computed: an input that never evaluates a spatial split is not refused.
//
// Floating point: strict binary32 in source order on both sides, as in sah_common.h; the square root of sphereSlice is the correctly
// rounded one on both sides; nextafterf is written as integer operations on the bits.
#pragma once
#include "sah_common.h"

namespace sbvh {

using namespace sah;

constexpr uint32_t kBadSpatialBin = 16;        // status bit: a spatial bin index outside what (int) conversion and bins[] define
constexpr int      kMaxPoly = 16;              // a triangle clipped by six half-spaces has at most 9 corners; beyond kMaxPoly: kInternal
constexpr int      kNodeKeys = 9;              // per node and fold direction: padded bounds, centroids, exact bounds (x, y, z each)
constexpr int      kSpCnt = 3 * kBins;         // per node: entries, exits (axis, bin)
constexpr uint32_t kWantSpatial = 1, kSpatial = 2;   // SNode::flags: the overlap test asks for a spatial search; the split is spatial

struct Ref { float mn[3], mx[3]; uint32_t prim, clipped; };   // BVHPrimData: exact box (w is +0), local primitive id, RefBounds' flag

struct SNode {
    BNode b;                         // sah_common.h; big is unused, nL = refs of the left child
    uint32_t nR, flags;              // refs of the right child; kWantSpatial | kSpatial
    float objCost, objPos, overlap;  // FindBestObjectSplitPlane's result
    int32_t objAxis;
};

SAH_HD float next_down(float x)      // nextafterf(x, -INFINITY)
{
    const uint32_t u = bits(x);
    if ((u & 0x7fffffffu) > 0x7f800000u || u == 0xff800000u) return x;
    if ((u & 0x7fffffffu) == 0) return from_bits(0x80000001u);
    return from_bits((u & 0x80000000u) ? u + 1 : u - 1);
}
SAH_HD float next_up(float x)        // nextafterf(x, INFINITY)
{
    const uint32_t u = bits(x);
    if ((u & 0x7fffffffu) > 0x7f800000u || u == 0x7f800000u) return x;
    if ((u & 0x7fffffffu) == 0) return from_bits(0x00000001u);
    return from_bits((u & 0x80000000u) ? u - 1 : u + 1);
}
SAH_HD float center(const Ref& r, int a) { return (r.mn[a] + r.mx[a]) * 0.5f; }   // Aabb::Center
SAH_HD Ref ref_of(const Prim& d, uint32_t prim)
{
    Ref r;
    for (int a = 0; a < 3; a++) { r.mn[a] = d.mn[a]; r.mx[a] = d.mx[a]; }
    r.prim = prim; r.clipped = 0;
    return r;
}

// Keys of one ref: [0, 3) RefBounds (the box padded by one ulp per side when clipped), [3, 6) centroid, [6, 9) the exact box
SAH_HD void ref_keys(const Ref& r, uint64_t kmin[kNodeKeys], uint64_t kmax[kNodeKeys])
{
    for (int a = 0; a < 3; a++) {
        const float pmn = r.clipped ? next_down(r.mn[a]) : r.mn[a], pmx = r.clipped ? next_up(r.mx[a]) : r.mx[a];
        const float c = center(r, a);
        kmin[a] = key_min(pmn, r.prim); kmin[3 + a] = key_min(c, r.prim); kmin[6 + a] = key_min(r.mn[a], r.prim);
        kmax[a] = key_max(pmx, r.prim); kmax[3 + a] = key_max(c, r.prim); kmax[6 + a] = key_max(r.mx[a], r.prim);
    }
}
// bmin / bmax of FindBestSpatialSplitPlane (:429-430): lo / hi folds of the exact boxes from +-RT_REALLYFAR
SAH_HD void exact_from_keys(const uint64_t* kmin, const uint64_t* kmax, float emn[3], float emx[3])
{
    for (int a = 0; a < 3; a++) { emn[a] = lo(kFar, key_value(kmin[6 + a])); emx[a] = hi(-kFar, key_value(kmax[6 + a])); }
}

// ---- object splits (FindBestObjectSplitPlane, :303-336, with the overlap of the winning plane) ---------------------------------------
struct ObjSplit { float cost, pos, overlap; int axis; };
SAH_HD_CALL void object_sweep(const float cmin[3], const float cmax[3], const Bins& B, ObjSplit& o)
{
    float best = kFar, pos = 0.0f, overlap = 0.0f;
    int axis = 0;
    for (int a = 0; a < 3; a++) {
        if (cmin[a] == cmax[a]) continue;
        float lArea[kBins - 1], rArea[kBins - 1];
        float lmn[kBins - 1][3], lmx[kBins - 1][3], rmn[kBins - 1][3], rmx[kBins - 1][3];
        int lCount[kBins - 1], rCount[kBins - 1];
        float amn[3] = { kEmpty, kEmpty, kEmpty }, amx[3] = { -kEmpty, -kEmpty, -kEmpty };
        float bmn[3] = { kEmpty, kEmpty, kEmpty }, bmx[3] = { -kEmpty, -kEmpty, -kEmpty };
        int sumL = 0, sumR = 0;
        for (int i = 0; i < kBins - 1; i++) {
            sumL += (int)B.n[a][i]; lCount[i] = sumL;
            for (int k = 0; k < 3; k++) { amn[k] = lo(amn[k], B.mn[a][i][k]); amx[k] = hi(amx[k], B.mx[a][i][k]); lmn[i][k] = amn[k]; lmx[i][k] = amx[k]; }
            lArea[i] = area(amn, amx);
            const int j = kBins - 1 - i;
            sumR += (int)B.n[a][j]; rCount[j - 1] = sumR;
            for (int k = 0; k < 3; k++) { bmn[k] = lo(bmn[k], B.mn[a][j][k]); bmx[k] = hi(bmx[k], B.mx[a][j][k]); rmn[j - 1][k] = bmn[k]; rmx[j - 1][k] = bmx[k]; }
            rArea[j - 1] = area(bmn, bmx);
        }
        const float scale = (cmax[a] - cmin[a]) / (float)kBins;
        for (int i = 0; i < kBins - 1; i++) {
            const float cost = (float)lCount[i] * lArea[i] + (float)rCount[i] * rArea[i];   // 0 * inf = NaN: never '<'
            if (cost < best) {
                best = cost; axis = a; pos = cmin[a] + scale * (float)(i + 1);
                float imn[3], imx[3];                                                       // lBox[i].Intersection(rBox[i]).Area()
                for (int k = 0; k < 3; k++) { imn[k] = hi(lmn[i][k], rmn[i][k]); imx[k] = lo(lmx[i][k], rmx[i][k]); }
                overlap = area(imn, imx);
            }
        }
    }
    o.cost = best; o.pos = pos; o.overlap = overlap; o.axis = axis;
}
// First decision step of a node whose bounds N.b.mn / mx are set: the object split, the leaf cost, and the test of BuildBVH (:183)
// against the BLAS root's area.
SAH_HD void decide_object(SNode& N, const float cmin[3], const float cmax[3], const Bins& B, float rootArea, float alpha)
{
    ObjSplit o;
    object_sweep(cmin, cmax, B, o);
    N.objCost = o.cost; N.objPos = o.pos; N.overlap = o.overlap; N.objAxis = o.axis;
    N.b.cost = node_cost(N.b.cnt, N.b.mn, N.b.mx);
    N.flags = (o.overlap / rootArea > alpha) ? kWantSpatial : 0;
}

// ---- clipping (:343-409) ---------------------------------------------------------------------------------------------------------------
struct V3 { float v[3]; };
SAH_HD V3 cut_edge(const V3& p, const V3& q, int axis, float plane)
{
    const bool pq = p.v[axis] < q.v[axis];
    const V3 s = pq ? p : q, e = pq ? q : p;
    V3 d, r;
    for (int k = 0; k < 3; k++) d.v[k] = e.v[k] - s.v[k];
    const float f = (plane - s.v[axis]) / d.v[axis];
    for (int k = 0; k < 3; k++) r.v[k] = s.v[k] + d.v[k] * f;
    return r;
}
// ClipTriangleToAABB: omn / omx is the clipped polygon's box (grown from the empty box).  overflow: more than kMaxPoly corners.
SAH_HD bool clip_triangle(const float bmn[3], const float bmx[3], const RtTriangle& t, float omn[3], float omx[3], bool& overflow)
{
    V3 P[kMaxPoly], Q[kMaxPoly];
    int n = 3;
    P[0].v[0] = t.v0.x; P[0].v[1] = t.v0.y; P[0].v[2] = t.v0.z;
    P[1].v[0] = t.v1.x; P[1].v[1] = t.v1.y; P[1].v[2] = t.v1.z;
    P[2].v[0] = t.v2.x; P[2].v[1] = t.v2.y; P[2].v[2] = t.v2.z;
    for (int a = 0; a < 3; a++) for (int side = 0; side < 2; side++) {
        const float plane = side == 0 ? bmn[a] : bmx[a];
        const float sign = side == 0 ? 1.0f : -1.0f;
        int m = 0;
        for (int i = 0; i < n; i++) {
            const V3 cur = P[i], nxt = P[i + 1 == n ? 0 : i + 1];
            const bool inCur = (cur.v[a] - plane) * sign >= 0, inNxt = (nxt.v[a] - plane) * sign >= 0;
            if (inCur) { if (m >= kMaxPoly) { overflow = true; return false; } Q[m++] = cur; }
            if (inCur != inNxt) { if (m >= kMaxPoly) { overflow = true; return false; } Q[m++] = cut_edge(cur, nxt, a, plane); }
        }
        for (int i = 0; i < m; i++) P[i] = Q[i];
        n = m;
    }
    if (n < 3) return false;
    for (int k = 0; k < 3; k++) { omn[k] = kEmpty; omx[k] = -kEmpty; }
    for (int i = 0; i < n; i++) for (int k = 0; k < 3; k++) { omn[k] = lo(omn[k], P[i].v[k]); omx[k] = hi(omx[k], P[i].v[k]); }
    return true;
}
SAH_HD void sphere_slice(const float pos[3], float d, int axis, float plane, V3 pts[4])
{
    int n = 0;
    for (int axisL = 0; axisL < 3; axisL++) {
        if (axisL == axis) continue;
        int axisF = 0;
        while (axisF == axisL || axisF == axis) axisF++;
        V3 p;
        p.v[0] = 0.0f; p.v[1] = 0.0f; p.v[2] = 0.0f;
        p.v[axis] = plane; p.v[axisL] = pos[axisL];
        const float a = -2.0f * pos[axisF];
        const float by = -2.0f * pos[axisL] * p.v[axisL];
        const float cz = -2.0f * pos[axis] * p.v[axis];
        const float y2 = p.v[axisL] * p.v[axisL], z2 = p.v[axis] * p.v[axis];
        const float D = a * a - 4.0f * (y2 + z2 + by + cz + d);
        const float s = __builtin_sqrtf(D);
        p.v[axisF] = (-a + s) * 0.5f; pts[n++] = p;
        p.v[axisF] = (-a - s) * 0.5f; pts[n++] = p;
    }
}
SAH_HD bool clip_sphere(const float bmn[3], const float bmx[3], const RtSphere& sp, float omn[3], float omx[3])
{
    const float pos[3] = { sp.pos.x, sp.pos.y, sp.pos.z };
    const float r = sp.r;
    for (int k = 0; k < 3; k++) { omn[k] = kEmpty; omx[k] = -kEmpty; }
    for (int k = 0; k < 3; k++) { const float p = pos[k] + r; omn[k] = lo(omn[k], p); omx[k] = hi(omx[k], p); }
    for (int k = 0; k < 3; k++) { const float p = pos[k] - r; omn[k] = lo(omn[k], p); omx[k] = hi(omx[k], p); }
    for (int a = 0; a < 3; a++) for (int side = 0; side < 2; side++) {
        const float plane = side == 0 ? bmn[a] : bmx[a];
        const float sign = side == 0 ? 1.0f : -1.0f;
        const float farPos = pos[a] + r * sign;
        if (!(farPos * sign > plane * sign)) return false;   // sphere entirely outside
        const float nearPos = pos[a] - r * sign;
        if (nearPos * sign < plane * sign) {
            const float d = pos[0] * pos[0] + pos[1] * pos[1] + pos[2] * pos[2] - r * r;
            V3 pts[4];
            sphere_slice(pos, d, a, plane, pts);
            float tmn[3] = { kEmpty, kEmpty, kEmpty }, tmx[3] = { -kEmpty, -kEmpty, -kEmpty };
            for (int i = 0; i < 4; i++) for (int k = 0; k < 3; k++) { tmn[k] = lo(tmn[k], pts[i].v[k]); tmx[k] = hi(tmx[k], pts[i].v[k]); }
            for (int k = 0; k < 3; k++) { const float p = k == a ? farPos : pos[k]; tmn[k] = lo(tmn[k], p); tmx[k] = hi(tmx[k], p); }
            for (int k = 0; k < 3; k++) { omn[k] = hi(omn[k], tmn[k]); omx[k] = lo(omx[k], tmx[k]); }   // out.Intersection(tight)
        }
    }
    return true;
}
// One primitive clipped to a box, as FindBestSpatialSplitPlane and SpatialSplit clip it (planes never hit)
SAH_HD bool clip_prim(const float bmn[3], const float bmx[3], const RtPrimitive& p, float omn[3], float omx[3], bool& overflow)
{
    if (p.objType == RT_PRIM_TRIANGLE) return clip_triangle(bmn, bmx, p.obj.triangle, omn, omx, overflow);
    if (p.objType == RT_PRIM_SPHERE) return clip_sphere(bmn, bmx, p.obj.sphere, omn, omx);
    return false;
}

// ---- spatial splits (FindBestSpatialSplitPlane, :424-481) ---------------------------------------------------------------------------
SAH_HD void spatial_edges(float bmin, float bmax, float& scale, float left[kBins], float right[kBins])
{
    scale = (float)kBins / (bmax - bmin);
    for (int b = 0; b < kBins; b++) {
        left[b] = bmin + (float)b * (1.0f / scale);
        right[b] = b == kBins - 1 ? bmax : bmin + (float)(b + 1) * (1.0f / scale);
    }
}
// (int)(scale * (x - bmin)), clamped from above (:440-441).  False: the conversion or the index is undefined (the new refusal).
SAH_HD bool spatial_index(float scale, float x, float bmin, int& b)
{
    const float f = scale * (x - bmin);
    if (!finite_(f) || f <= -1.0f || f >= 2147483648.0f) return false;
    b = (int)f;
    if (b > kBins - 1) b = kBins - 1;
    return true;
}
// The contributions of one ref to the spatial bins of axis a of its node (exact bounds bmin != bmax): emit(bin, mn, mx) once per bin
// whose box it grows; first / last: the bins whose entries / exits it counts in, or -1.  Returns 0 or a status bit.
template <class Emit>
SAH_HD uint32_t spatial_ref(const Ref& r, const RtPrimitive& prim, int a, float bmin, float bmax, int& first, int& last, Emit&& emit)
{
    float scale, left[kBins], right[kBins];
    spatial_edges(bmin, bmax, scale, left, right);
    first = -1; last = -1;
    int lb, rb;
    if (!spatial_index(scale, r.mn[a], bmin, lb) || !spatial_index(scale, r.mx[a], bmin, rb)) return kBadSpatialBin;
    while (r.mn[a] <= left[lb] && lb > 0) lb--;
    while (r.mn[a] > right[lb] && lb != kBins - 1) lb++;
    while (r.mx[a] < left[rb] && rb > 0) rb--;
    while (r.mx[a] >= right[rb] && rb != kBins - 1) rb++;
    if (lb == rb) { emit(lb, r.mn, r.mx); first = lb; last = rb; return 0; }
    int f = kBins, l = -1;
    for (int b = lb; b <= rb; b++) {
        float smn[3], smx[3], cmn[3], cmx[3];
        for (int k = 0; k < 3; k++) { smn[k] = r.mn[k]; smx[k] = r.mx[k]; }
        smn[a] = left[b]; smx[a] = right[b];
        bool overflow = false;
        const bool hit = clip_prim(smn, smx, prim, cmn, cmx, overflow);
        if (overflow) return kInternal;
        if (hit) {
            if (b < f) f = b;
            if (b > l) l = b;
            emit(b, cmn, cmx);
        }
    }
    if (f <= l) { first = f; last = l; }
    return 0;
}

struct SBins { uint32_t entries[3][kBins], exits[3][kBins]; float mn[3][kBins][3], mx[3][kBins][3]; };
SAH_HD void sbins_from_keys(const uint64_t* skmin, const uint64_t* skmax, const uint32_t* sent, const uint32_t* sext, SBins& S)
{
    for (int a = 0; a < 3; a++) for (int b = 0; b < kBins; b++) {
        const int s = a * kBins + b;
        S.entries[a][b] = sent[s]; S.exits[a][b] = sext[s];
        for (int k = 0; k < 3; k++) {
            S.mn[a][b][k] = skmin[s * 3 + k] != kKeyMinEmpty ? lo(kEmpty, key_value(skmin[s * 3 + k])) : kEmpty;
            S.mx[a][b][k] = skmax[s * 3 + k] != kKeyMaxEmpty ? hi(-kEmpty, key_value(skmax[s * 3 + k])) : -kEmpty;
        }
    }
}
// The prefix / suffix merge and the sweep (:468-478)
SAH_HD_CALL void spatial_sweep(const float emn[3], const float emx[3], const SBins& S, float& best, int& axis, float& pos)
{
    for (int a = 0; a < 3; a++) {
        if (emn[a] == emx[a]) continue;
        float scale, left[kBins], right[kBins];
        spatial_edges(emn[a], emx[a], scale, left, right);
        // suffix[i]: bins i .. kBins - 1 merged from the right
        float sArea[kBins]; uint32_t sExits[kBins];
        {
            float amn[3] = { kEmpty, kEmpty, kEmpty }, amx[3] = { -kEmpty, -kEmpty, -kEmpty };
            uint32_t ex = 0;
            for (int i = kBins - 1; i >= 0; i--) {
                for (int k = 0; k < 3; k++) { amn[k] = lo(amn[k], S.mn[a][i][k]); amx[k] = hi(amx[k], S.mx[a][i][k]); }
                ex += S.exits[a][i];
                sArea[i] = area(amn, amx); sExits[i] = ex;
            }
        }
        float amn[3] = { kEmpty, kEmpty, kEmpty }, amx[3] = { -kEmpty, -kEmpty, -kEmpty }, accRight = -kFar;
        uint32_t en = 0;
        for (int i = 0; i < kBins - 1; i++) {
            for (int k = 0; k < 3; k++) { amn[k] = lo(amn[k], S.mn[a][i][k]); amx[k] = hi(amx[k], S.mx[a][i][k]); }
            en += S.entries[a][i];
            accRight = hi(accRight, right[i]);
            if (en == 0 || sExits[i + 1] == 0) continue;
            const float cost = (float)(int)en * area(amn, amx) + (float)(int)sExits[i + 1] * sArea[i + 1];
            if (cost < best) { best = cost; axis = a; pos = accRight; }
        }
    }
}
// Second decision step (:185-194): the spatial search when asked for (S), the leaf test, object against spatial.  False: BuildBLAS
// would take its spatial branch with axis -1.
SAH_HD bool decide_final(SNode& N, const float emn[3], const float emx[3], const SBins* S)
{
    float spCost = kFar, spPos = kFar;
    int spAxis = -1;
    if (N.flags & kWantSpatial) spatial_sweep(emn, emx, *S, spCost, spAxis, spPos);
    N.b.interiors = 0; N.b.depth = 0;
    const float leafCost = N.b.cost;
    if (N.b.cnt <= RT_MIN_LEAF_PRIMS || (leafCost < N.objCost && leafCost < spCost)) { N.b.kind = kLeaf; return true; }
    if (N.objCost < spCost) { N.b.kind = kSplit; N.b.axis = N.objAxis; N.b.pos = N.objPos; return true; }
    if (spAxis < 0) return false;
    N.b.kind = kSplit; N.b.axis = spAxis; N.b.pos = spPos; N.flags |= kSpatial;
    return true;
}

// ---- the partition (ObjectSplit :337-340, SpatialSplit :482-505) ------------------------------------------------------------------------
constexpr uint32_t kEmitL = 1, kEmitR = 2, kStraddle = 4;
// What ref r of split node N hands to the children: kEmitL / kEmitR with the fragments L / R, kStraddle when it was clipped (counted
// in prims_clipped even if both clips fail and the ref vanishes).
SAH_HD uint32_t split_ref(const SNode& N, const Ref& r, const RtPrimitive& prim, Ref& L, Ref& R, bool& overflow)
{
    const int axis = N.b.axis;
    const float pos = N.b.pos;
    if (!(N.flags & kSpatial)) {
        if (center(r, axis) <= pos) { L = r; return kEmitL; }
        R = r; return kEmitR;
    }
    const float mn = r.mn[axis], mx = r.mx[axis];
    if (mn < pos && mx > pos) {
        float lmn[3], lmx[3], rmn[3], rmx[3];
        for (int k = 0; k < 3; k++) { lmn[k] = rmn[k] = r.mn[k]; lmx[k] = rmx[k] = r.mx[k]; }
        lmx[axis] = pos; rmn[axis] = pos;
        uint32_t out = kStraddle;
        L.prim = R.prim = r.prim; L.clipped = R.clipped = 1;
        if (clip_prim(lmn, lmx, prim, L.mn, L.mx, overflow)) out |= kEmitL;
        if (clip_prim(rmn, rmx, prim, R.mn, R.mx, overflow)) out |= kEmitR;
        return out;
    }
    if (mx <= pos) { L = r; return kEmitL; }
    R = r; return kEmitR;
}

// ---- the level-synchronous part --------------------------------------------------------------------------------------------------------
SAH_HD SNode open_snode(uint32_t home, uint32_t cnt)
{
    SNode N;
    N.b = open_node(home, cnt, 0);
    N.b.kind = kOpen; N.b.big = 0;
    N.nR = 0; N.flags = 0; N.objCost = 0.0f; N.objPos = 0.0f; N.overlap = 0.0f; N.objAxis = 0;
    return N;
}
// After the partition counted the fragments: the termination guard (:198) closes the node as a forced leaf over its own refs.
// spatial / forced: what the node adds to stat_spatial_splits (counted before the guard) and stat_forced_leaves.  Returns the node's
// contribution (1 | refs of both children << 32) to the exclusive scan that places the children and their segments.
SAH_HD uint64_t count_node(SNode& N, uint32_t nL, uint32_t nR, uint32_t& spatial, uint32_t& forced)
{
    spatial = 0; forced = 0;
    if (N.b.kind != kSplit) return 0;
    if (N.flags & kSpatial) spatial = 1;
    if (nL == 0 || nR == 0 || (nL >= N.b.cnt && nR >= N.b.cnt)) { N.b.kind = kLeaf; forced = 1; return 0; }
    N.b.nL = nL; N.nR = nR;
    return 1ull | ((uint64_t)(nL + nR) << 32);
}
SAH_HD void make_schildren(SNode& N, uint64_t scan, uint32_t levelEnd, SNode& L, SNode& R)
{
    const uint32_t rank = (uint32_t)scan, base = (uint32_t)(scan >> 32);
    N.b.left = levelEnd + 2 * rank;
    L = open_snode(base, N.b.nL);
    R = open_snode(base + N.b.nL, N.nR);
}
SAH_HD void sup(SNode& N, const SNode& L, const SNode& R)
{
    up(N.b, L.b, R.b);
    N.b.cnt = L.b.cnt + R.b.cnt;     // from here on: the refs of the subtree's leaves (down() offsets the left child by R's)
}

// rt_build_bvh2_sbvh's argument checks (those of rt_build_bvh2_sah without the capacities, and alpha); nullptr when they pass
inline const char* check_args(float alpha, const RtPrimitive* prims, int32_t nPrims, int32_t first, int32_t count, const RtBVHNode2* nodes,
                              int32_t nodeCap, const int32_t* nNodes, const uint32_t* primIdx, int32_t idxCap, const int32_t* nIdx)
{
    if (!prims || !nodes || !nNodes || !primIdx || !nIdx) return "missing array";
    if (count <= 0) return "empty primitive range (count <= 0)";
    if (count > (1 << 30)) return "more than 2^30 primitives";
    if (first < 0 || nPrims < 0 || (int64_t)first + count > (int64_t)nPrims) return "primitive range outside [0, nPrims)";
    if (nodeCap < 0 || idxCap < 0) return "negative nodeCap / idxCap";
    if (!(alpha >= 0.0f && alpha <= 1.0f)) return "alpha must lie in [0, 1]";
    return nullptr;
}
inline const char* sstatus_text(uint32_t st)
{
    if (st & kInternal) return "inconsistent build state (or a clipped polygon of more than 16 corners)";
    if (st & kBadSpatialBin)
        return "a spatial bin index that is not finite, <= -1 or >= 2^31 (an inverted or empty ref box among the refs): BuildBLAS is undefined here";
    return status_text(st);
}
constexpr uint32_t kMaxRefs = 0x7fffffffu;     // refs alive in one level, nodes of one build

} // namespace sbvh

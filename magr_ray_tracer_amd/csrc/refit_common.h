// refit_common.h — the scalar rules of an in-place scene update (rt_update_scene, include/rt355.h), compiled by hipcc for the device
// path (scene.hip's upload, refit.hip's kernels) and by g++ for the host restatement (host/refit_host.cpp, rth_refit) and the host
// TLAS builder (accel_build.cpp).  Every value an update writes is computed by one of these functions on both sides, so that the
// device arrays after an update are bit for bit those a fresh rt_upload_scene of the host-refit scene produces.
//
//   node boxes   a leaf's box starts from BVH2::UpdateNodeBounds' initial box (+-RT_REALLYFAR, w 0) and takes the union of its
//                primitives' boxes by BVH2::CreateBVHPrimData's rule (lbvh::prim_box: unclipped, planes empty); an interior node's
//                box is union(left, right).  Unions use lbvh::lb_min / lb_max (a total order: the result does not depend on the
//                order in which threads arrive; fminf / fmaxf differ on +-0 between x86 and AMDGPU).
//   records      the derived layouts rt_upload_scene writes: pair records (layout 1), triangle records, shading records, light
//                records, TLAS pair records (both encodings) and instance records.
//   TLAS         TLAS::Build's instance boxes (identity: the root box as is; otherwise instance_world_box in fp64) and its merge
//                rule, which keeps fminf / fmaxf as x86-64 glibc evaluates them (tlas_min / tlas_max below).
//
// Floating point: strict binary32 / binary64 in source order (-ffp-contract=off on both sides), no libm call but nextafterf (exact
// on both sides).
#pragma once
#include <stdint.h>
#include <math.h>
#include "../../include/rt355_types.h"
#include "lbvh_common.h"
#include <vector>

namespace refit {

using lbvh::Box;

constexpr uint32_t kNone = 0xffffffffu;
constexpr int kMaxInstances = 256;                                    // TLAS::Build's limit

LB_HD uint32_t f2u(float f) { uint32_t u; __builtin_memcpy(&u, &f, 4); return u; }
LB_HD float u2f(uint32_t u) { float f; __builtin_memcpy(&f, &u, 4); return f; }
LB_HD RtFloat4 f4(float x, float y, float z, float w) { RtFloat4 r; r.x = x; r.y = y; r.z = z; r.w = w; return r; }
// An entry helper or a record decoder is a mask or a lane shuffle: always inlined, like the kernels' own helpers
#define LB_DEC __attribute__((always_inline)) LB_HD

// ---- entries: the 32-bit words by which a derived record names a child (integers only) -------------------------------------------
// The one statement of every encoding; the writers below and in rebuild_common.h / collapse_common.h and the traversal kernels
// (rt355_kernels.h) all go through it, tools/records_main.cpp round-trips it.
//   BLAS entry   (pair and quad records, the instance record's root, rootEntry[])
//                  interior   its id in the dense pair (BVH2) or quad (BVH4) table, below 2^29
//                  leaf       kLeafBit | count << 24 | first    count <= 127 primitives from primIdx / triRecs slot first < 2^24
//                  unused     kNoChild: an empty slot of a quad record.  No legal entry: as a leaf it would be 127 primitives from slot
//                             2^24 - 1, and a leaf ends at or below nIdx < 2^24 (rebuild::takes_layout1)
//   plain TLAS   (tlasPairs, DevScene.tlasRoot: traverse_tlas)
//                  interior   its TLAS node id            leaf   kLeafBit | instance id
//                on traverse_tlas' 16-bit stack (tlas_pack16): bit 15 = leaf, the id in bits 14..0
//   tagged TLAS  (tlasPairsP, DevScene.tlasRootP: the event loops, which keep BLAS and TLAS entries on ONE stack column)
//                  bits 31..29 = 010 (kTagTlas)  TLAS interior, id in bits 28..0
//                  bits 31..29 = 011 (kTagInst)  TLAS leaf, instance id in bits 28..0
//                beside the BLAS entries: 1xx a leaf, 000 an interior node.  kTagInst contains kTagTlas' bit: tagged_tlas answers for
//                an entry that is neither a leaf nor an instance.
// What an entry is comes back as the masked word, which the caller compares (plain_leaf(e) != 0, tagged_tag(e) == kTagInst,
// tagged_tlas(e) != 0): a helper that returns bool changes the traversal kernels' machine code, one that returns the word does not.
// The event loops write the two tagged tests out, (e & kTagMask) == kTagInst and (e & kTagTlas) != 0, with these constants: inside
// their && chains even the word-returning helpers change the code (profiles/r20_record_layouts.txt).
constexpr uint32_t kLeafBit = 0x80000000u, kLeafCountMask = 0x7fu, kLeafFirstMask = 0x00ffffffu, kNoChild = 0xffffffffu;
constexpr int kLeafCountShift = 24;
constexpr uint32_t kTagTlas = 0x40000000u, kTagInst = 0x60000000u, kTagMask = 0xe0000000u, kIdMask = 0x1fffffffu;
LB_DEC uint32_t leaf_entry(uint32_t first, uint32_t count) { return kLeafBit | (count << kLeafCountShift) | first; }
LB_DEC uint32_t leaf_first(uint32_t e) { return e & kLeafFirstMask; }
LB_DEC uint32_t leaf_count(uint32_t e) { return (e >> kLeafCountShift) & kLeafCountMask; }
// the leaf (first, count) without its first primitive (count > 1)
LB_DEC uint32_t leaf_rest(uint32_t first, uint32_t count) { return kLeafBit | ((count - 1) << kLeafCountShift) | (first + 1); }
LB_DEC uint32_t tlas_leaf_entry(bool tagged, uint32_t inst) { return (tagged ? kTagInst : kLeafBit) | inst; }
LB_DEC uint32_t tlas_node_entry(bool tagged, uint32_t node) { return tagged ? (kTagTlas | node) : node; }
LB_DEC uint32_t plain_leaf(uint32_t e) { return e & kLeafBit; }
LB_DEC uint32_t plain_inst(uint32_t e) { return e & ~kLeafBit; }
LB_DEC uint16_t tlas_pack16(uint32_t e) { return (uint16_t)((e >> 16) | (e & 0x7fffu)); }
LB_DEC uint32_t tlas_unpack16(uint32_t v) { return ((v & 0x8000u) << 16) | (v & 0x7fffu); }
LB_DEC uint32_t tagged_tag(uint32_t e) { return e & kTagMask; }
LB_DEC uint32_t tagged_tlas(uint32_t e) { return e & kTagTlas; }
LB_DEC uint32_t tagged_id(uint32_t e) { return e & kIdMask; }

// ---- node boxes --------------------------------------------------------------------------------------------------------------
LB_HD Box leaf_init()   // BVH2::UpdateNodeBounds' initial box
{
    Box b;
    for (int k = 0; k < 3; k++) { b.mn[k] = RT_REALLYFAR; b.mx[k] = -RT_REALLYFAR; }
    b.mn[3] = b.mx[3] = 0.0f;
    return b;
}
LB_HD Box node_box(const RtBVHNode2& n)
{
    Box b;
    b.mn[0] = n.aabbMin.x; b.mn[1] = n.aabbMin.y; b.mn[2] = n.aabbMin.z; b.mn[3] = n.aabbMin.w;
    b.mx[0] = n.aabbMax.x; b.mx[1] = n.aabbMax.y; b.mx[2] = n.aabbMax.z; b.mx[3] = n.aabbMax.w;
    return b;
}
LB_HD void set_box(RtBVHNode2& n, const Box& b)
{
    n.aabbMin = f4(b.mn[0], b.mn[1], b.mn[2], b.mn[3]);
    n.aabbMax = f4(b.mx[0], b.mx[1], b.mx[2], b.mx[3]);
}
// the box of the leaf over primIdx[first, first + count)
LB_HD Box leaf_box(const RtPrimitive* prims, const uint32_t* primIdx, uint32_t first, uint32_t count)
{
    Box b = leaf_init();
    for (uint32_t s = first; s < first + count; s++) b = lbvh::box_union(b, lbvh::prim_box(prims[primIdx[s]]));
    return b;
}

// ---- derived records (rt_upload_scene) ----------------------------------------------------------------------------------------
// Every record is a few 16-byte vectors, and each has its decoders right below its encoder: templates over any vector type V with
// lanes .x .y .z .w (RtFloat4 here, float4 and the scalar-cache vector in the kernels), given the record's vectors in order.  A
// decoded box or edge is a V with w = 0.
//
// Pair record (layout 1, 64 B: one cache-line-aligned fetch per interior visit) of an interior node with children a (first) and b
// (first + 1); the node array itself stays as uploaded.  Both child boxes in q0..q2 (pair_boxes: BLAS pairs[], and TLAS tlasPairs[] /
// tlasPairsP[] from the TLAS node array); q3 = (entry(a), entry(b), 0, 0) depends on the topology only (rebuild::pair_record, tlas_pair)
//   q0 = (a.min.xyz, a.max.x)   q1 = (a.max.yz, b.min.xy)   q2 = (b.min.z, b.max.xyz)
template <class N> LB_HD void pair_boxes(const N& a, const N& b, RtFloat4 out[3])
{
    out[0] = f4(a.aabbMin.x, a.aabbMin.y, a.aabbMin.z, a.aabbMax.x);
    out[1] = f4(a.aabbMax.y, a.aabbMax.z, b.aabbMin.x, b.aabbMin.y);
    out[2] = f4(b.aabbMin.z, b.aabbMax.x, b.aabbMax.y, b.aabbMax.z);
}
template <class V> LB_DEC V pair_min1(const V& q0, const V&, const V&) { return V{ q0.x, q0.y, q0.z, 0.0f }; }
template <class V> LB_DEC V pair_max1(const V& q0, const V& q1, const V&) { return V{ q0.w, q1.x, q1.y, 0.0f }; }
template <class V> LB_DEC V pair_min2(const V&, const V& q1, const V& q2) { return V{ q1.z, q1.w, q2.x, 0.0f }; }
template <class V> LB_DEC V pair_max2(const V&, const V&, const V& q2) { return V{ q2.y, q2.z, q2.w, 0.0f }; }
template <class V> LB_DEC uint32_t pair_entry1(const V& q3) { return f2u(q3.x); }
template <class V> LB_DEC uint32_t pair_entry2(const V& q3) { return f2u(q3.y); }
// Triangle record (48 B) of leaf slot s (primitive `prim` = primIdx[s]), in leaf order, so that a leaf's triangles are contiguous and
// the primIdx indirection disappears: v0 and the edges v1 - v0, v2 - v0 - the first two operations of the reference's triangle test
// (primitives.cl:49-50), done once with the same IEEE subtraction - the id and the "not plain" flag (a sphere, a plane, or a vertex
// with a non-zero w lane: the reference-layout test)
//   a = (v0.xyz, e1.x)   b = (e1.yz, e2.xy)   c = (e2.z, prim, not plain, 0)
LB_HD void tri_rec(const RtPrimitive& p, uint32_t prim, RtFloat4 out[3])
{
    const RtTriangle& t = p.obj.triangle;
    const bool plain = p.objType == RT_PRIM_TRIANGLE && t.v0.w == 0.0f && t.v1.w == 0.0f && t.v2.w == 0.0f;
    const float e1x = t.v1.x - t.v0.x, e1y = t.v1.y - t.v0.y, e1z = t.v1.z - t.v0.z;
    const float e2x = t.v2.x - t.v0.x, e2y = t.v2.y - t.v0.y, e2z = t.v2.z - t.v0.z;
    out[0] = f4(t.v0.x, t.v0.y, t.v0.z, e1x);
    out[1] = f4(e1y, e1z, e2x, e2y);
    out[2] = f4(e2z, u2f(prim), u2f(plain ? 0u : 1u), 0.0f);
}
template <class V> LB_DEC V tri_v0(const V& a, const V&, const V&) { return V{ a.x, a.y, a.z, 0.0f }; }
template <class V> LB_DEC V tri_edge1(const V& a, const V& b, const V&) { return V{ a.w, b.x, b.y, 0.0f }; }
template <class V> LB_DEC V tri_edge2(const V&, const V& b, const V& c) { return V{ b.z, b.w, c.x, 0.0f }; }
template <class V> LB_DEC uint32_t tri_prim(const V& c) { return f2u(c.y); }
template <class V> LB_DEC uint32_t tri_not_plain(const V& c) { return f2u(c.z); }   // != 0 (the word, as for the entries)
// shading record (k_shade): geometric normal + material id + type
LB_HD RtFloat4 shade_rec(const RtPrimitive& p)
{
    const RtFloat4 N = p.objType == RT_PRIM_TRIANGLE ? p.obj.triangle.N : (p.objType == RT_PRIM_PLANE ? p.obj.plane.N : f4(0, 0, 0, 0));
    uint32_t tag = ((uint32_t)p.objType << 28) | ((uint32_t)p.matIdx & 0x07ffffffu) | (lbvh::neg_(N.w) ? 0x08000000u : 0u);
    // a triangle/plane normal with a non-zero w lane cannot be represented: mark it like a sphere (reference-layout path)
    if (p.objType != RT_PRIM_SPHERE && N.w != 0.0f) tag = ((uint32_t)RT_PRIM_SPHERE << 28) | ((uint32_t)p.matIdx & 0x07ffffffu);
    return f4(N.x, N.y, N.z, u2f(tag));
}
// light record words 0..4 (k_shade, NEE): the first 64 bytes of the light's Primitive, {objType, area}; word 5, its material's
// emittance, does not depend on the geometry
LB_HD void light_rec(const RtPrimitive& p, RtFloat4 out[5])
{
    __builtin_memcpy(out, &p.obj, 64);
    out[4] = f4(u2f((uint32_t)p.objType), p.area, 0.0f, 0.0f);
}
// TLAS interior node i (children lr & 0xffff, lr >> 16): a pair record of the TLAS node array - one fetch per interior visit where the
// reference array costs the node's leftRight word, then the two child nodes, and none per leaf: its instance sits in the parent's
// record.  tagged: the entries of the event loops (tlasPairsP), else the plain ones (tlasPairs).  Leaves have an all-zero record.
LB_HD void tlas_pair(const RtTLASNode* t, uint32_t i, bool tagged, RtFloat4 out[4])
{
    const uint32_t lr = t[i].leftRight;
    if (lr == 0) { for (int k = 0; k < 4; k++) out[k] = f4(0, 0, 0, 0); return; }
    pair_boxes(t[lr & 0xffffu], t[lr >> 16], out);
    uint32_t e[2];
    for (int k = 0; k < 2; k++) {
        const uint32_t n = k == 0 ? (lr & 0xffffu) : (lr >> 16);
        e[k] = t[n].leftRight == 0 ? tlas_leaf_entry(tagged, t[n].BLASidx) : tlas_node_entry(tagged, n);
    }
    out[3] = f4(u2f(e[0]), u2f(e[1]), 0.0f, 0.0f);
}
// Instance record (64 B: one fetch where the reference reads BVHInstance.invT and the root separately): rows 0..2 of invT - row k
// maps a point p to dot(axis, p) + shift, a direction to dot(axis, d) - then {encoded BLAS root (layout 1; else 0), bvhIdx, 0, 0}
LB_HD void inst_rec(const RtBVHInstance& inst, uint32_t rootEntry, RtFloat4 out[4])
{
    const float* T = inst.invT;
    out[0] = f4(T[0], T[1], T[2], T[3]);
    out[1] = f4(T[4], T[5], T[6], T[7]);
    out[2] = f4(T[8], T[9], T[10], T[11]);
    out[3] = f4(u2f(rootEntry), u2f(inst.bvhIdx), 0.0f, 0.0f);
}
template <class V> LB_DEC V inst_axis(const V& row) { return V{ row.x, row.y, row.z, 0.0f }; }
template <class V> LB_DEC float inst_shift(const V& row) { return row.w; }
template <class V> LB_DEC uint32_t inst_root(const V& t3) { return f2u(t3.x); }
template <class V> LB_DEC uint32_t inst_bvh(const V& t3) { return f2u(t3.y); }

// ---- TLAS::Build ----------------------------------------------------------------------------------------------------------------
// fminf / fmaxf as TLAS::Build's host build evaluates them (x86-64 glibc: minss / maxss, an equal pair returns the second operand,
// a NaN operand returns the other one)
LB_HD float tlas_min(float a, float b) { if (a != a) return b; if (b != b) return a; return a < b ? a : b; }
LB_HD float tlas_max(float a, float b) { if (a != a) return b; if (b != b) return a; return a > b ? a : b; }
// FindBestMatch's area of the union of two TLAS boxes
LB_HD float tlas_pair_area(const float amn[3], const float amx[3], const float bmn[3], const float bmx[3])
{
    const float ex = tlas_max(amx[0], bmx[0]) - tlas_min(amn[0], bmn[0]);
    const float ey = tlas_max(amx[1], bmx[1]) - tlas_min(amn[1], bmn[1]);
    const float ez = tlas_max(amx[2], bmx[2]) - tlas_min(amn[2], bmn[2]);
    return ex * ey + ey * ez + ez * ex;
}
LB_HD bool is_identity(const float* T)
{
    bool bits = true;   // memcmp with the identity
    for (int k = 0; k < 16; k++) bits = bits && f2u(T[k]) == f2u((k % 5) == 0 ? 1.0f : 0.0f);
    return bits || (T[0] == 1 && T[5] == 1 && T[10] == 1 && T[1] == 0 && T[2] == 0 && T[3] == 0 && T[4] == 0 &&
                    T[6] == 0 && T[7] == 0 && T[8] == 0 && T[9] == 0 && T[11] == 0);
}
LB_HD double inst_det(const float* invT)
{
    const double a[3][3] = { { invT[0], invT[1], invT[2] }, { invT[4], invT[5], invT[6] }, { invT[8], invT[9], invT[10] } };
    return a[0][0] * (a[1][1] * a[2][2] - a[1][2] * a[2][1]) - a[0][1] * (a[1][0] * a[2][2] - a[1][2] * a[2][0]) +
           a[0][2] * (a[1][0] * a[2][1] - a[1][1] * a[2][0]);
}
LB_HD bool singular(const float* invT) { const double d = inst_det(invT); return !((d < 0 ? -d : d) > 1e-30); }
// World-space bounds of an instance whose transform is not the identity: the eight corners of the root box mapped by inverse(invT)
// and bounded, padded by a few ulp of the box size (the leaf test must never be tighter than the instance's own root test).
// Returns false for a singular transform (TLAS::Build refuses it).
LB_HD bool instance_world_box(const float* invT, const RtFloat4& rmn, const RtFloat4& rmx, RtFloat4& mn, RtFloat4& mx)
{
    // inverse of the affine map p' = A p + t (rows 0-2 of invT; row-major, translation in cells 3/7/11): p = A^-1 (p' - t)
    const double a[3][3] = { { invT[0], invT[1], invT[2] }, { invT[4], invT[5], invT[6] }, { invT[8], invT[9], invT[10] } };
    const double t[3] = { invT[3], invT[7], invT[11] };
    const double det = inst_det(invT);
    if (!((det < 0 ? -det : det) > 1e-30)) return false;
    double inv[3][3];
    for (int r = 0; r < 3; r++) for (int c = 0; c < 3; c++) {
        const int r1 = (c + 1) % 3, r2 = (c + 2) % 3, c1 = (r + 1) % 3, c2 = (r + 2) % 3;
        inv[r][c] = (a[r1][c1] * a[r2][c2] - a[r1][c2] * a[r2][c1]) / det;
    }
    double lo[3] = { 1e300, 1e300, 1e300 }, hi[3] = { -1e300, -1e300, -1e300 };
    const float bx[2][3] = { { rmn.x, rmn.y, rmn.z }, { rmx.x, rmx.y, rmx.z } };
    for (int k = 0; k < 8; k++) {
        const double p[3] = { bx[k & 1][0] - t[0], bx[(k >> 1) & 1][1] - t[1], bx[(k >> 2) & 1][2] - t[2] };
        for (int r = 0; r < 3; r++) {
            const double w = inv[r][0] * p[0] + inv[r][1] * p[1] + inv[r][2] * p[2];
            lo[r] = (w < lo[r]) ? w : lo[r];     // std::min(lo, w)
            hi[r] = (hi[r] < w) ? w : hi[r];     // std::max(hi, w)
        }
    }
    float fl[3], fh[3];
    for (int r = 0; r < 3; r++) {
        const double alo = lo[r] < 0 ? -lo[r] : lo[r], ahi = hi[r] < 0 ? -hi[r] : hi[r];
        const double pad = 1e-5 * (hi[r] - lo[r]) + 1e-6 * ((alo < ahi) ? ahi : alo) + 1e-30;
        fl[r] = nextafterf((float)(lo[r] - pad), -INFINITY); fh[r] = nextafterf((float)(hi[r] + pad), INFINITY);
    }
    mn = f4(fl[0], fl[1], fl[2], 0.0f); mx = f4(fh[0], fh[1], fh[2], 0.0f);
    return true;
}

// ---- topology (host only: computed once, at upload and by rth_refit) ------------------------------------------------------------
// The nodes reachable from the BLAS roots, breadth-first root by root (children after their parent: a walk backwards visits every
// child before its parent), the parent of each (kNone for roots and for unreachable slots, whose fields may be garbage), and the
// reachable leaves.  Instances may share a root; any other node reached twice (a DAG) makes the scene non-refittable.  Child ids and
// leaf ranges must already be valid (rt_validate_scene).  Returns NULL or why the tree cannot be refit.
struct Topology { std::vector<uint32_t> parent, order, leaves; };
inline const char* build_topology(const RtBVHNode2* n, int32_t nNodes, const RtBVHInstance* inst, int32_t nInst, Topology& t)
{
    t.parent.assign((size_t)nNodes, kNone); t.order.clear(); t.leaves.clear();
    std::vector<uint8_t> seen((size_t)nNodes, 0), isRoot((size_t)nNodes, 0);
    for (int32_t b = 0; b < nInst; b++) {
        const uint32_t root = inst[b].bvhIdx;
        if (root >= (uint32_t)nNodes) return "an instance's bvhIdx is out of range";
        if (isRoot[root]) continue;
        if (seen[root]) return "a BLAS root is also a node of another BLAS";
        isRoot[root] = seen[root] = 1;
        size_t head = t.order.size();
        t.order.push_back(root);
        for (; head < t.order.size(); head++) {
            const uint32_t i = t.order[head];
            if (n[i].count > 0) { t.leaves.push_back(i); continue; }
            for (uint32_t c = n[i].first; c <= n[i].first + 1; c++) {
                if (c >= (uint32_t)nNodes) return "a child index is out of range";
                if (seen[c]) return "a node is reachable twice";
                seen[c] = 1; t.parent[c] = i; t.order.push_back(c);
            }
        }
    }
    return nullptr;
}

} // namespace refit

// collapse_common.h — the rules of the BVH2 -> BVH4 collapse (BVH4::Convert / Collapse, host/accel_build.cpp, reference bvh.cpp:695-787)
// and of what rt_upload_scene derives from the collapsed tree (quad records, stack need), compiled by hipcc for the kernels of
// collapse.hip and by g++ for the host restatement (host/collapse_host.cpp, rth_build_bvh4_levels), like rebuild_common.h.
//
// Collapse(index) changes only the record of `index`, and the children it absorbs are still as Convert wrote them (two slots): the
// recursion into the surviving children comes after the loop.  A surviving node's final record is therefore a function of the BVH2
// below it alone, and the survivors of one level can be processed side by side (final_record reads the BVH2, never a BVH4 record).
//
//   converted    the record Convert writes for BVH2 node i: slot k = child first + k's box and (first, count) of a leaf child or
//                (first + k, 0) of an interior one, slots 2 and 3 unused; all zero for a leaf; the one-slot record for a BLAS root
//                that is a leaf.
//   greedy step  child count = slots before the first count == RT_INVALID; candidates are the interior slots with n - 1 + nc <= 4;
//                the largest half area dx * dy + dy * dz + dz * dx wins, strictly (the first of equal areas, never a NaN area); the
//                absorbed child's slot 0 replaces the picked slot, its slots 1.. are appended.
//   live ids     the surviving nodes, breadth-first, BLAS by BLAS in the order in which the instances first name their roots: the
//                order in which scene.hip's quad_records numbers them.
//   quad record  six float4 of boxes (slot-major x/y/z pairs, transposed), then the four packed child entries, then zero.
//   stack need   top down: a live node entered with `base` entries below it needs base + kids; its j-th interior child in slot order
//                is entered with base + j.  The maximum over a BLAS equals scene.hip's bvh4_stack_need (a depth-first replay of the same rule).
#pragma once
#include <stdint.h>
#include <math.h>
#include <string>
#include <vector>
#include "../../include/rt355_types.h"
#include "refit_common.h"
#include "rebuild_common.h"

namespace collapse {

constexpr uint32_t kNone = 0xffffffffu;
constexpr uint32_t kMaxLevels = RT_BVH4_STACK;   // a BVH4 level descends at least one BVH2 level: a BLAS deeper than this is refused

LB_HD int child_count(const RtBVHNode4& n)   // BVH4::GetChildCount
{
    int c = 0;
    while (c < 4 && n.count[c] != RT_INVALID) c++;
    return c;
}
LB_HD void zero_record(RtBVHNode4& q)
{
    for (int k = 0; k < 4; k++) { q.aabbMin[k] = refit::f4(0, 0, 0, 0); q.aabbMax[k] = refit::f4(0, 0, 0, 0); q.first[k] = 0; q.count[k] = 0; }
}
// are both children of interior record i inside the array?  (first + 1 wraps for first = 0xffffffff)
LB_HD bool children_inside(const RtBVHNode2* n, uint32_t nNodes, uint32_t i)
{
    const uint32_t c = n[i].first;
    return c < nNodes && c + 1 < nNodes && c + 1 > c;
}
// Convert's record of BVH2 node i (children_inside(i) holds for an interior node)
LB_HD void converted(const RtBVHNode2* n, uint32_t i, RtBVHNode4& q)
{
    zero_record(q);
    if (n[i].count > 0) return;
    for (uint32_t k = 0; k < 2; k++) {
        const uint32_t c = n[i].first + k;
        q.aabbMin[k] = n[c].aabbMin; q.aabbMax[k] = n[c].aabbMax;
        if (n[c].count > 0) { q.first[k] = (int32_t)n[c].first; q.count[k] = (int32_t)n[c].count; }
        else { q.first[k] = (int32_t)c; q.count[k] = 0; }
    }
    for (int k = 2; k < 4; k++) q.first[k] = q.count[k] = RT_INVALID;
}
// the record of a BLAS root that is a leaf (accel_build.cpp, Convert's second loop)
LB_HD void leaf_root(const RtBVHNode2* n, uint32_t root, RtBVHNode4& q)
{
    zero_record(q);
    q.aabbMin[0] = n[root].aabbMin; q.aabbMax[0] = n[root].aabbMax;
    q.first[0] = (int32_t)n[root].first; q.count[0] = (int32_t)n[root].count;
    for (int k = 1; k < 4; k++) q.first[k] = q.count[k] = RT_INVALID;
}
// One pass of Collapse's loop over `node`: picks the slot to absorb, or RT_INVALID.  An interior slot names an un-collapsed BVH2
// interior node, whose converted record has two children (nc = 2).
LB_HD int greedy_pick(const RtBVHNode4& node, int n)
{
    const int nc = 2;
    float bestArea = -INFINITY; int pick = RT_INVALID;
    for (int i = 0; i < n; i++) {
        if (node.count[i] > 0) continue;
        if (!(n - 1 + nc <= 4)) continue;
        const float dx = node.aabbMax[i].x - node.aabbMin[i].x, dy = node.aabbMax[i].y - node.aabbMin[i].y, dz = node.aabbMax[i].z - node.aabbMin[i].z;
        const float half = dx * dy + dy * dz + dz * dx;
        if (half > bestArea) { bestArea = half; pick = i; }
    }
    return pick;
}
// The final record of surviving node `node` (a BLAS root or a child slot of a surviving node), from the BVH2 alone.  false: a child
// index it had to follow lies outside the array (nothing is written then).
LB_HD bool final_record(const RtBVHNode2* n, uint32_t nNodes, uint32_t node, RtBVHNode4& out)
{
    if (node >= nNodes) return false;
    if (n[node].count > 0) { leaf_root(n, node, out); return true; }
    if (!children_inside(n, nNodes, node)) return false;
    RtBVHNode4 q;
    converted(n, node, q);
    for (;;) {
        const int cnt = child_count(q);
        const int pick = greedy_pick(q, cnt);
        if (pick == RT_INVALID) break;
        const uint32_t c = (uint32_t)q.first[pick];
        if (!children_inside(n, nNodes, c)) return false;
        RtBVHNode4 child;
        converted(n, c, child);
        const int nc = child_count(child);
        q.aabbMin[pick] = child.aabbMin[0]; q.aabbMax[pick] = child.aabbMax[0];
        q.first[pick] = child.first[0]; q.count[pick] = child.count[0];
        for (int i = 1; i < nc; i++) {
            q.aabbMin[cnt - 1 + i] = child.aabbMin[i]; q.aabbMax[cnt - 1 + i] = child.aabbMax[i];
            q.first[cnt - 1 + i] = child.first[i]; q.count[cnt - 1 + i] = child.count[i];
        }
    }
    out = q;
    return true;
}
// is slot k of a final record a child that survives (and gets a live id)?  The slots were written from checked BVH2 records.
LB_HD bool is_child(const RtBVHNode4& q, int k) { return q.first[k] != RT_INVALID && q.count[k] == 0; }
// the largest leaf of a record (0: none)
LB_HD uint32_t largest_leaf(const RtBVHNode4& q)
{
    uint32_t m = 0;
    for (int k = 0; k < 4; k++) if (q.first[k] != RT_INVALID && q.count[k] > 0 && (uint32_t)q.count[k] > m) m = (uint32_t)q.count[k];
    return m;
}
// The quad record of a live node (layout 1 of a BVH4, 128 B, derived from the unchanged BVHNode4 array; newId maps node ids to live
// ids): floats 0..23 = {min.xyz, max.xyz} of child slots 0..3 - so q0..q2 hold slots 0 and 1 and q3..q5 slots 2 and 3 exactly as a
// pair record holds its two children - q6 = the four entries (refit: kNoChild for an unused slot, else the live id or the leaf entry),
// q7 = 0.  A visit is 7 sixteen-byte loads from two 64-B lines instead of 10 from three, and triangles come from the leaf-ordered
// triRecs.  The decoders follow refit_common.h's: given the record's vectors in order, K = the slot.
LB_HD void quad_record(const RtBVHNode4& q, int32_t nNodes, int32_t nIdx, const uint32_t* newId, RtFloat4 out[8])
{
    float b[24]; uint32_t e[4];
    for (int k = 0; k < 4; k++) {
        const RtFloat4& mn = q.aabbMin[k]; const RtFloat4& mx = q.aabbMax[k];
        b[k * 6 + 0] = mn.x; b[k * 6 + 1] = mn.y; b[k * 6 + 2] = mn.z; b[k * 6 + 3] = mx.x; b[k * 6 + 4] = mx.y; b[k * 6 + 5] = mx.z;
        const int slot = rebuild::bvh4_slot(q, k, nNodes, nIdx);
        if (slot == rebuild::kSlotLeaf) e[k] = refit::leaf_entry((uint32_t)q.first[k], (uint32_t)q.count[k]);
        else if (slot == rebuild::kSlotChild) e[k] = newId[(uint32_t)q.first[k]];
        else e[k] = refit::kNoChild;   // (unused; validate_scene has refused kSlotBad)
    }
    for (int v = 0; v < 6; v++) out[v] = refit::f4(b[v * 4], b[v * 4 + 1], b[v * 4 + 2], b[v * 4 + 3]);
    out[6] = refit::f4(refit::u2f(e[0]), refit::u2f(e[1]), refit::u2f(e[2]), refit::u2f(e[3]));
    out[7] = refit::f4(0, 0, 0, 0);
}
template <int K, class V> LB_DEC V quad_min(const V& q0, const V& q1, const V& q2, const V& q3, const V& q4, const V& q5)
{
    static_assert(K >= 0 && K < 4, "a quad record has four child slots");
    return K == 0 ? refit::pair_min1(q0, q1, q2) : K == 1 ? refit::pair_min2(q0, q1, q2) : K == 2 ? refit::pair_min1(q3, q4, q5) : refit::pair_min2(q3, q4, q5);
}
template <int K, class V> LB_DEC V quad_max(const V& q0, const V& q1, const V& q2, const V& q3, const V& q4, const V& q5)
{
    static_assert(K >= 0 && K < 4, "a quad record has four child slots");
    return K == 0 ? refit::pair_max1(q0, q1, q2) : K == 1 ? refit::pair_max2(q0, q1, q2) : K == 2 ? refit::pair_max1(q3, q4, q5) : refit::pair_max2(q3, q4, q5);
}
template <int K, class V> LB_DEC uint32_t quad_entry(const V& q6)
{
    static_assert(K >= 0 && K < 4, "a quad record has four child slots");
    return refit::f2u(K == 0 ? q6.x : K == 1 ? q6.y : K == 2 ? q6.z : q6.w);
}

// ---- argument checks (host only), shared by rt_build_bvh4, rt_upload_scene_bvh2 and rth_build_bvh4_levels ---------------------------
// Every index the kernels follow, before any launch: k_c4_convert reads both children of EVERY interior record, reachable or not.
// blas: the distinct roots in the order in which `roots` first names them, with the BVH2 height (edges) and the interior nodes below.
struct Blas { uint32_t root, height, interiors; };
inline int check_args(const RtBVHNode2* n, int32_t nNodes, int32_t nIdx, const uint32_t* roots, int32_t nRoots, std::vector<Blas>& blas, std::string& why)
{
    blas.clear();
    if (!n || !roots || nNodes <= 0 || nIdx <= 0 || nRoots <= 0) { why = "missing array or a count <= 0 (nodes, roots, nNodes, nIdx and nRoots are required)"; return RT_E_INVALID; }
    for (int32_t b = 0; b < nRoots; b++) if (roots[b] >= (uint32_t)nNodes) { why = "root " + std::to_string(b) + ": node " + std::to_string(roots[b]) + " is out of range"; return RT_E_INVALID; }
    for (int32_t i = 0; i < nNodes; i++) {
        if (n[i].count == 0 && !children_inside(n, (uint32_t)nNodes, (uint32_t)i)) {
            why = "node " + std::to_string(i) + ": child index " + std::to_string(n[i].first) + " out of range (an unreachable interior record is converted too)";
            return RT_E_INVALID;
        }
        if (n[i].count > 0 && (uint64_t)n[i].first + n[i].count > (uint64_t)nIdx) { why = "node " + std::to_string(i) + ": leaf range exceeds nIdx"; return RT_E_INVALID; }
    }
    std::vector<uint8_t> seen((size_t)nNodes, 0), isRoot((size_t)nNodes, 0);
    std::vector<std::pair<uint32_t, uint32_t>> st;
    for (int32_t b = 0; b < nRoots; b++) {
        const uint32_t root = roots[b];
        if (isRoot[root]) continue;   // a BLAS named before
        if (seen[root]) { why = "node " + std::to_string(root) + " is reachable twice (a root inside another BLAS)"; return RT_E_INVALID; }
        isRoot[root] = 1; seen[root] = 1;
        Blas s{ root, 0, 0 };
        st.assign(1, { root, 0u });
        while (!st.empty()) {
            const auto [i, d] = st.back(); st.pop_back();
            if (d > s.height) s.height = d;
            if (n[i].count > 0) continue;
            s.interiors++;
            for (uint32_t c = n[i].first; c <= n[i].first + 1; c++) {
                if (seen[c]) { why = "node " + std::to_string(c) + " is reachable twice"; return RT_E_INVALID; }
                seen[c] = 1; st.push_back({ c, d + 1 });
            }
        }
        blas.push_back(s);
    }
    for (const Blas& s : blas) if (s.height > kMaxLevels) {
        why = "the BLAS at node " + std::to_string(s.root) + " is " + std::to_string(s.height) + " levels deep, at most " + std::to_string(kMaxLevels) + " are supported";
        return RT_E_UNSUPPORTED;
    }
    return RT_OK;
}
// frontier bound of level l of a BLAS with `interiors` interior nodes: at most 4^l live nodes, and every live node but a leaf root is
// an interior node of the BVH2
LB_HD uint32_t level_bound(uint32_t l, uint32_t interiors)
{
    const uint64_t full = l < 16 ? (1ull << (2 * l)) : (1ull << 32);
    const uint64_t most = interiors > 0 ? interiors : 1;
    return (uint32_t)(full < most ? full : most);
}

} // namespace collapse

// rebuild_common.h — the rules by which a scene's derived layout follows from its BVH2 (rt_upload_scene derives it on the host,
// rt_rebuild_scene on the device: rebuild.hip), and the detection of the primitive range each BLAS covers.  Compiled by hipcc for the
// device path and by g++ for the host restatement (host/rebuild_host.cpp, rth_rebuild), like refit_common.h.
//
//   pair ids     interior nodes are renumbered breadth-first, BLAS by BLAS in the order in which the instances first name their
//                roots: level by level, parents in frontier order, child `first` before `first + 1`, interior children only.
//   pair record  both child boxes (refit::pair_boxes) and the children's entries: a leaf is refit::leaf_entry (so a leaf holds at
//                most kMaxPackedLeaf primitives and primIdx fewer than kMaxPackedIdx slots), an interior node is its pair id.
//   stack        a BLAS of height h (edges, the root counts 0) needs h entries; a context keeps clamp(max h + 1, 6, RT_BVH4_STACK).
#pragma once
#include <stdint.h>
#include <algorithm>
#include <string>
#include <utility>
#include <vector>
#include "../../include/rt355.h"
#include "refit_common.h"

namespace rebuild {

constexpr uint32_t kNone = 0xffffffffu;
constexpr uint32_t kMaxPackedLeaf = 127;          // primitives of a leaf in the packed entry
constexpr int32_t kMaxPackedIdx = 1 << 24;        // primIdx slots the packed entry addresses
constexpr int kMinStackEntries = 6;               // flush_counters reuses 36 words of the LDS stack
static_assert(refit::kLeafCountMask == kMaxPackedLeaf && refit::kLeafFirstMask == (uint32_t)kMaxPackedIdx - 1u &&
              kMaxPackedIdx == 1 << refit::kLeafCountShift && (refit::kLeafBit >> refit::kLeafCountShift) == kMaxPackedLeaf + 1u,
              "a leaf entry is the leaf bit, a count of up to kMaxPackedLeaf and a slot below kMaxPackedIdx, with no bit shared or left over");

// the packed entry of node n in layout 1 (newId: its pair id if it is an interior node)
LB_HD uint32_t child_entry(uint32_t first, uint32_t count, uint32_t newId)
{
    return count > 0 ? refit::leaf_entry(first, count) : newId;
}
LB_HD uint32_t child_entry(const RtBVHNode2& n, uint32_t newId) { return child_entry(n.first, n.count, newId); }
// the packed entries of both children of interior node `node`; newId maps node ids to pair ids
LB_HD void pair_entries(const RtBVHNode2* nodes, uint32_t node, const uint32_t* newId, uint32_t e[2])
{
    const uint32_t c = nodes[node].first;
    for (uint32_t k = 0; k < 2; k++) {
        const uint32_t count = nodes[c + k].count;   // (an interior node's pair id is only read for interior nodes)
        e[k] = child_entry(nodes[c + k].first, count, count > 0 ? 0u : newId[c + k]);
    }
}
// the pair record of interior node `node`: both child boxes, then {entries, 0, 0} as bit patterns
LB_HD void pair_record(const RtBVHNode2* nodes, uint32_t node, const uint32_t* newId, RtFloat4 out[4])
{
    const uint32_t c = nodes[node].first;
    uint32_t e[2];
    refit::pair_boxes(nodes[c], nodes[c + 1], out);
    pair_entries(nodes, node, newId, e);
    out[3] = refit::f4(refit::u2f(e[0]), refit::u2f(e[1]), 0.0f, 0.0f);
}
// does the scene take the derived layout 1?  (BVH2 only; extend_variant 1 keeps the reference arrays)
LB_HD bool takes_layout1(bool variantAllows, int32_t nIdx, uint32_t largestLeaf)
{
    return variantAllows && nIdx < kMaxPackedIdx && largestLeaf <= kMaxPackedLeaf;
}
// A BLAS whose traversal needs more than RT_BVH4_STACK entries (BVH2: its height in edges) is refused: by rt_upload_scene
// (validate_scene), by rt_rebuild_scene for a tree it has just built, and by the host restatement rth_rebuild alike
LB_HD bool exceeds_stack(int64_t need) { return need > (int64_t)RT_BVH4_STACK; }
// LDS stack entries of a context whose deepest BLAS needs `need` (not exceeds_stack(need), checked by the caller)
LB_HD int stack_entries(int need)
{
    const int e = need + 1 > kMinStackEntries ? need + 1 : kMinStackEntries;
    return e < RT_BVH4_STACK ? e : RT_BVH4_STACK;
}

// What one slot k of an RtBVHNode4 is - the one rule validate_scene, the stack-need replay and the layout-1 derivation go by.
// traverse_bvh4 calls a slot used iff first != RT_INVALID, reads primIdx[first + j] for j < count when count > 0 and pushes `first`
// as a node id otherwise, so a used slot must have count >= 0 and first >= 0: a leaf's range must lie in primIdx, a child in the node
// array.  (The collapse only ever writes first = count = -1 into an unused slot.)
enum Bvh4Slot { kSlotUnused = 0, kSlotLeaf = 1, kSlotChild = 2, kSlotBad = -1 };
LB_HD int bvh4_slot(int32_t first, int32_t count, int32_t nNodes, int32_t nIdx)
{
    if (first == RT_INVALID) return kSlotUnused;
    if (first < 0 || count < 0) return kSlotBad;
    if (count > 0) return (int64_t)first + (int64_t)count <= (int64_t)nIdx ? kSlotLeaf : kSlotBad;
    return first < nNodes ? kSlotChild : kSlotBad;
}
LB_HD int bvh4_slot(const RtBVHNode4& n, int k, int32_t nNodes, int32_t nIdx) { return bvh4_slot(n.first[k], n.count[k], nNodes, nIdx); }

// ---- BLAS ranges (host only) ------------------------------------------------------------------------------------------------------
// A scene can be rebuilt BLAS by BLAS when the primitives each distinct BLAS references form one contiguous range (a primitive may be
// referenced several times, as SBVH leaves do), the ranges are disjoint and they come in the order of the roots - what appending BLAS
// after BLAS (BVH2::BuildBLAS) produces.  ranges: one per distinct BLAS in increasing order; instBlas[i]: the range of instance i.
// Returns NULL or why the scene is not of that shape.  Checks every index it follows.
struct BlasRange { uint32_t root, first, count; };
inline const char* find_blas_ranges(const RtBVHNode2* n, int32_t nNodes, const uint32_t* primIdx, int32_t nIdx, int32_t nPrims,
                                    const RtBVHInstance* inst, int32_t nInst, std::vector<BlasRange>& ranges, std::vector<int32_t>& instBlas)
{
    ranges.clear(); instBlas.assign((size_t)(nInst > 0 ? nInst : 0), -1);
    if (!n || !primIdx || !inst || nNodes <= 0 || nIdx <= 0 || nPrims <= 0 || nInst <= 0) return "missing array";
    std::vector<int32_t> owner((size_t)nPrims, -1), rootBlas((size_t)nNodes, -1);
    std::vector<uint8_t> seen((size_t)nNodes, 0);
    std::vector<uint32_t> stack;
    for (int32_t b = 0; b < nInst; b++) {
        const uint32_t root = inst[b].bvhIdx;
        if (root >= (uint32_t)nNodes) return "an instance's bvhIdx is out of range";
        if (rootBlas[root] >= 0) { instBlas[(size_t)b] = rootBlas[root]; continue; }
        if (seen[root]) return "a BLAS root is also a node of another BLAS";
        const int32_t k = (int32_t)ranges.size();
        rootBlas[root] = k; instBlas[(size_t)b] = k;
        uint32_t lo = kNone, hi = 0, distinct = 0;
        stack.assign(1, root); seen[root] = 1;
        while (!stack.empty()) {
            const uint32_t i = stack.back(); stack.pop_back();
            if (n[i].count > 0) {
                if ((uint64_t)n[i].first + n[i].count > (uint64_t)nIdx) return "a leaf range exceeds primIdx";
                for (uint32_t s = n[i].first; s < n[i].first + n[i].count; s++) {
                    const uint32_t p = primIdx[s];
                    if (p >= (uint32_t)nPrims) return "primIdx out of range";
                    if (owner[p] == k) continue;
                    if (owner[p] >= 0) return "two BLAS reference the same primitive";
                    owner[p] = k; distinct++;
                    if (p < lo) lo = p;
                    if (p > hi) hi = p;
                }
                continue;
            }
            for (uint32_t c = n[i].first; c <= n[i].first + 1; c++) {
                if (c >= (uint32_t)nNodes || c < n[i].first) return "a child index is out of range";
                if (seen[c]) return "a node is reachable twice";
                seen[c] = 1; stack.push_back(c);
            }
        }
        if (distinct == 0 || hi - lo + 1 != distinct) return "the primitives of a BLAS are not one contiguous range";
        ranges.push_back(BlasRange{ root, lo, distinct });
    }
    // in the order of the roots
    std::vector<int32_t> byFirst(ranges.size());
    for (size_t k = 0; k < ranges.size(); k++) byFirst[k] = (int32_t)k;
    for (size_t a = 1; a < byFirst.size(); a++)   // insertion sort by range start (few BLAS, usually sorted already)
        for (size_t j = a; j > 0 && ranges[(size_t)byFirst[j]].first < ranges[(size_t)byFirst[j - 1]].first; j--) std::swap(byFirst[j], byFirst[j - 1]);
    for (size_t a = 1; a < byFirst.size(); a++)
        if (ranges[(size_t)byFirst[a]].root < ranges[(size_t)byFirst[a - 1]].root) return "the primitive ranges are not in the order of the BLAS roots";
    std::vector<BlasRange> sorted(ranges.size());
    std::vector<int32_t> newOf(ranges.size());
    for (size_t a = 0; a < byFirst.size(); a++) { sorted[a] = ranges[(size_t)byFirst[a]]; newOf[(size_t)byFirst[a]] = (int32_t)a; }
    ranges.swap(sorted);
    for (int32_t& v : instBlas) v = newOf[(size_t)v];
    return nullptr;
}

// ---- kept trees (rt_rebuild_ranges, RT_REBUILD_KEEP; host only but for relocated_first) ---------------------------------------------
// A bound BLAS is compact when the nodes reachable from its root are exactly the ids [root, root + nodes), nodes odd, and its leaves'
// primIdx ranges tile one interval [idxLo, idxLo + idxSlots) without gap or overlap - what BuildBLAS, the GPU builders and every in-place
// rebuild or resize produce.  Such a tree moves as a block: node i goes to i - oldRoot + newRoot, and only the `first` word changes.
// height: of the tree in edges (the root counts 0, so 0 exactly when nodes == 1): the builders' depth.
struct BlasBlock { uint32_t nodes, idxLo, idxSlots; uint8_t compact; uint32_t height; };
// The relocation rule, one for the kernel (k_blas_relocate) and the host mirror (rth_rebuild_ranges): the `first` word of a record that
// moves by nodeDelta = newRoot - oldRoot node ids and whose leaves' slots move by idxDelta = newIdxBase - oldIdxBase (both modulo 2^32);
// an interior record (count == 0) names a child pair, a leaf its first primIdx slot.  Boxes, count and the pad words stay.
LB_HD uint32_t relocated_first(uint32_t first, uint32_t count, uint32_t nodeDelta, uint32_t idxDelta)
{
    return first + (count == 0 ? nodeDelta : idxDelta);
}
// ... and the same for the derived pair record of a kept or refit BLAS (k_pairs_relocate, rt_debug_relocate_pairs): one of the two
// entries of its fourth vector.  A leaf entry (leaf bit set) adds idxDelta to its 24-bit slot field, an interior entry adds pairDelta =
// newPairBase - oldPairBase to its pair id (both modulo 2^32).  No carry leaves the slot field: the bound entry's slot lies below the
// bound nIdx, the moved one below the new nIdx, and both scenes passed the layout check (takes_layout1: nIdx < kMaxPackedIdx), so the
// sum modulo 2^24 is the new slot itself and the count and leaf bits above it stay.
LB_HD uint32_t relocated_entry(uint32_t entry, uint32_t pairDelta, uint32_t idxDelta)
{
    if (entry & refit::kLeafBit) return (entry & ~refit::kLeafFirstMask) | ((entry + idxDelta) & refit::kLeafFirstMask);
    return entry + pairDelta;
}
// The block of every range of a scene find_blas_ranges has accepted (it checked every index followed here and that no node is reachable
// twice).  A range that is not compact reports the nodes and slots it reaches; naming it RT_REBUILD_KEEP is refused.
inline void find_blas_blocks(const RtBVHNode2* n, const std::vector<BlasRange>& ranges, std::vector<BlasBlock>& blocks)
{
    blocks.assign(ranges.size(), BlasBlock{ 0u, 0u, 0u, 0, 0u });
    std::vector<std::pair<uint32_t, uint32_t>> stack;   // (node, its depth)
    std::vector<std::pair<uint32_t, uint32_t>> leaves;
    for (size_t k = 0; k < ranges.size(); k++) {
        const uint32_t root = ranges[k].root;
        uint32_t lo = root, hi = root, m = 0, height = 0;
        uint64_t slots = 0;
        leaves.clear(); stack.assign(1, { root, 0u });
        while (!stack.empty()) {
            const auto [i, d] = stack.back(); stack.pop_back();
            m++; lo = std::min(lo, i); hi = std::max(hi, i); height = std::max(height, d);
            if (n[i].count > 0) { leaves.push_back({ n[i].first, n[i].count }); slots += n[i].count; }
            else { stack.push_back({ n[i].first, d + 1 }); stack.push_back({ n[i].first + 1, d + 1 }); }
        }
        std::sort(leaves.begin(), leaves.end());
        bool tiles = true;
        for (size_t a = 1; a < leaves.size() && tiles; a++) tiles = leaves[a].first == leaves[a - 1].first + leaves[a - 1].second;
        blocks[k] = BlasBlock{ m, leaves[0].first, (uint32_t)std::min<uint64_t>(slots, 0xffffffffu),
                               (uint8_t)(lo == root && hi - lo + 1 == m && (m & 1u) && tiles && slots <= 0x7fffffffu ? 1 : 0), height };
    }
}
// (The replacement window may intersect built and refit ranges: a refit range takes its boxes from the primitives as they are afterwards.)
// The checks of a plan (one RT_REBUILD_* word per range) against the ranges it is for, the blocks where they are known (NULL: every
// range counts as compact) and the replacement window [first, first + count): RT_OK, or RT_E_INVALID / RT_E_UNSUPPORTED with msg.
inline int check_plan(const int32_t* plan, int32_t nRanges, const std::vector<BlasRange>& ranges, const BlasBlock* blocks, int32_t first, int32_t count,
                      std::string& msg)
{
    if (!plan) { msg = "null plan"; return RT_E_INVALID; }
    if (nRanges != (int32_t)ranges.size()) {
        msg = "the plan has " + std::to_string(nRanges) + " words, the scene " + std::to_string(ranges.size()) + " distinct BLAS";
        return RT_E_INVALID;
    }
    for (int32_t k = 0; k < nRanges; k++) {
        if (plan[k] == RT_REBUILD_REFIT) {
            msg = "plan[" + std::to_string(k) + "]: RT_REBUILD_REFIT is not a per-range plan (refit one BLAS with RT_REBUILD_REFIT_RANGE, the whole scene with rt_rebuild_scene)";
            return RT_E_INVALID;
        }
        if (plan[k] != RT_REBUILD_SAH && plan[k] != RT_REBUILD_LBVH && plan[k] != RT_REBUILD_SBVH && plan[k] != RT_REBUILD_KEEP && plan[k] != RT_REBUILD_REFIT_RANGE) {
            msg = "plan[" + std::to_string(k) + "]: unknown word " + std::to_string(plan[k]);
            return RT_E_INVALID;
        }
    }
    for (int32_t k = 0; k < nRanges; k++) {
        if (plan[k] != RT_REBUILD_KEEP) continue;
        const BlasRange& r = ranges[(size_t)k];
        const std::string name = "BLAS " + std::to_string(k) + " (primitives [" + std::to_string(r.first) + ", " + std::to_string((uint64_t)r.first + r.count) + "))";
        if (count > 0 && (int64_t)first < (int64_t)r.first + (int64_t)r.count && (int64_t)first + count > (int64_t)r.first) {
            msg = "the replaced primitives [" + std::to_string(first) + ", " + std::to_string((int64_t)first + count) + ") intersect " + name +
                  ", which the plan keeps: its boxes would go stale";
            return RT_E_INVALID;
        }
    }
    for (int32_t k = 0; k < nRanges; k++) {   // a kept and a refit tree alike move as a block
        if ((plan[k] != RT_REBUILD_KEEP && plan[k] != RT_REBUILD_REFIT_RANGE) || !blocks || blocks[k].compact) continue;
        const BlasRange& r = ranges[(size_t)k];
        msg = std::string(plan[k] == RT_REBUILD_KEEP ? "RT_REBUILD_KEEP" : "RT_REBUILD_REFIT_RANGE") + " for BLAS " + std::to_string(k) + " (primitives [" + std::to_string(r.first) + ", " + std::to_string((uint64_t)r.first + r.count) +
              ")): its bound tree is not compact (its nodes are not exactly the ids [root, root + nodes), or its leaves do not tile one primIdx interval); build it instead";
        return RT_E_UNSUPPORTED;
    }
    return RT_OK;
}

} // namespace rebuild

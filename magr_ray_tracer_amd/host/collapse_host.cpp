// collapse_host.cpp — the sequential host restatement of the GPU BVH2 -> BVH4 collapse (rth_build_bvh4_levels).  It runs the level
// loop of csrc/collapse.hip step by step over the rules of csrc/collapse_common.h: Convert's record for every node, then per BLAS and
// level the final record of every surviving node from the BVH2 alone, live ids in frontier order, the next frontier in slot order.  It
// is not a call into BVH4::Convert; its arrays equal BuildBVH4's (tests/test_collapse_cpu.py).  Bvh4RefitHost (rth_bvh4_refit) restates
// the in-place collapse of a refit BVH2 (k_c4_refit and the fallback behind it, RT_REBUILD_REFIT) the same way.
#include <chrono>
#include <cstring>
#include <string>
#include <utility>
#include <vector>
#include "../../include/rt355.h"
#include "../../include/rt355_host.h"
#include "../csrc/collapse_common.h"
#include "rt_host.h"

namespace rt355 {

int Bvh4LevelsHost(const RtBVHNode2* n, int32_t nNodes, int32_t nIdx, const uint32_t* roots, int32_t nRoots, RtBVHNode4* out4, RtBvh4Stats* stats,
                   RtFloat4* quads, uint32_t* rootEntry, uint32_t* quadNode, std::string& err)
{
    using namespace collapse;
    const auto t0 = std::chrono::steady_clock::now();
    const std::string who = "rth_build_bvh4_levels: ";
    std::vector<Blas> blas;
    std::string why;
    if (const int rc = check_args(n, nNodes, nIdx, roots, nRoots, blas, why)) { err = who + why; return rc; }
    if (!out4) { err = who + "missing array (out4)"; return RT_E_INVALID; }
    try {
        std::vector<RtBVHNode4> q((size_t)nNodes);
        for (int32_t i = 0; i < nNodes; i++) converted(n, (uint32_t)i, q[(size_t)i]);   // k_c4_convert
        std::vector<uint32_t> newId((size_t)nNodes, kNone), order;
        uint32_t need = 0, leaf = 0, levels = 0;
        for (const Blas& b : blas) {
            std::vector<std::pair<uint32_t, uint32_t>> front{ { b.root, 0u } }, next;   // (node, stack entries below it)
            const uint32_t nLevels = b.height > 0 ? b.height : 1;
            for (uint32_t l = 0; l < nLevels && !front.empty(); l++) {
                if (front.size() > level_bound(l, b.interiors)) { err = who + "a frontier overflows its bound (inconsistent tree)"; return RT_E_DEVICE; }
                next.clear();
                for (const auto& [node, base] : front) {   // k_c4_frontier, k_c4_next
                    RtBVHNode4 rec;
                    if (!final_record(n, (uint32_t)nNodes, node, rec)) { err = who + "a child index is out of range"; return RT_E_DEVICE; }
                    q[node] = rec;
                    newId[node] = (uint32_t)order.size(); order.push_back(node);
                    uint32_t kids = 0;
                    for (int k = 0; k < 4; k++) if (is_child(rec, k)) next.push_back({ (uint32_t)rec.first[k], base + kids++ });
                    if (base + kids > need) need = base + kids;
                    if (largest_leaf(rec) > leaf) leaf = largest_leaf(rec);
                }
                if (l + 1 > levels) levels = l + 1;
                front.swap(next);
            }
            if (!front.empty()) { err = who + "the walk did not end at the tree's height (inconsistent tree)"; return RT_E_DEVICE; }
        }
        memcpy(out4, q.data(), sizeof(RtBVHNode4) * (size_t)nNodes);
        if (quads) for (size_t k = 0; k < order.size(); k++) quad_record(q[order[k]], nNodes, nIdx, newId.data(), quads + k * 8);   // k_c4_quads
        if (quadNode) memcpy(quadNode, order.data(), sizeof(uint32_t) * order.size());
        if (rootEntry) for (int32_t r = 0; r < nRoots; r++) rootEntry[r] = newId[roots[r]];   // k_c4_roots
        if (stats) {
            stats->live_nodes = (int32_t)order.size(); stats->levels = (int32_t)levels; stats->stack_need = (int32_t)need; stats->largest_leaf = (int32_t)leaf;
            stats->device_ms = 0;
            stats->wall_ms = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count();
        }
        return RT_OK;
    } catch (const std::exception& e) {
        err = who + e.what();
        return RT_E_NOMEM;
    }
}

// RT_REBUILD_REFIT's collapse: Convert's records, the final record of every live node of the collapse `inout4` holds (quadNode: live
// id -> node) from the refit BVH2, and the count of those whose slots differ from inout4's.  None: these records are the collapse of
// the refit BVH2.  Otherwise the level loop above runs.
int Bvh4RefitHost(const RtBVHNode2* n, int32_t nNodes, int32_t nIdx, const uint32_t* roots, int32_t nRoots, RtBVHNode4* inout4, const uint32_t* quadNode,
                  int32_t nLive, int32_t* changedNodes, std::string& err)
{
    using namespace collapse;
    const std::string who = "rth_bvh4_refit: ";
    std::vector<Blas> blas;
    std::string why;
    if (const int rc = check_args(n, nNodes, nIdx, roots, nRoots, blas, why)) { err = who + why; return rc; }
    if (!inout4 || !quadNode || nLive <= 0 || nLive > nNodes) { err = who + "missing array (inout4, quadNode) or a live count outside [1, nNodes]"; return RT_E_INVALID; }
    for (int32_t q = 0; q < nLive; q++) if (quadNode[q] >= (uint32_t)nNodes) { err = who + "quadNode[" + std::to_string(q) + "] is out of range"; return RT_E_INVALID; }
    try {
        std::vector<RtBVHNode4> rec4((size_t)nNodes);
        for (int32_t i = 0; i < nNodes; i++) converted(n, (uint32_t)i, rec4[(size_t)i]);   // k_c4_convert
        int32_t changed = 0;
        for (int32_t q = 0; q < nLive; q++) {   // k_c4_refit
            const uint32_t node = quadNode[q];
            RtBVHNode4 rec;
            if (!final_record(n, (uint32_t)nNodes, node, rec)) { err = who + "a child index is out of range"; return RT_E_DEVICE; }
            rec4[node] = rec;
            bool same = true;
            for (int k = 0; k < 4; k++) same = same && rec.first[k] == inout4[node].first[k] && rec.count[k] == inout4[node].count[k];
            if (!same) changed++;
        }
        if (changedNodes) *changedNodes = changed;
        if (changed == 0) { memcpy(inout4, rec4.data(), sizeof(RtBVHNode4) * (size_t)nNodes); return RT_OK; }
    } catch (const std::exception& e) {
        err = who + e.what();
        return RT_E_NOMEM;
    }
    return Bvh4LevelsHost(n, nNodes, nIdx, roots, nRoots, inout4, nullptr, nullptr, nullptr, nullptr, err);   // the fallback
}

} // namespace rt355

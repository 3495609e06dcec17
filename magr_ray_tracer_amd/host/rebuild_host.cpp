// rebuild_host.cpp — the host restatement of rt_rebuild_scene's BLAS rebuild (BVH2::Rebuild, rth_rebuild, include/rt355_host.h): every
// distinct BLAS of the scene is built again over the primitive range it covers (csrc/rebuild_common.h finds the ranges), in increasing
// order of the ranges and appended the way BuildBLAS appends BLAS after BLAS, with the host restatement of the chosen GPU builder.
// Together with TLAS::Build it is the ground truth the device rebuild must match bit for bit.  Under a per-range plan
// (BVH2::RebuildRanges, rth_rebuild_ranges: rt_rebuild_ranges' restatement) a BLAS the plan keeps is appended as its bound block of
// nodes, relocated by the rule the device kernel applies (rebuild::relocated_first); a BLAS it refits (RT_REBUILD_REFIT_RANGE) likewise,
// and then takes the boxes refit_common.h's rules give it over the primitives as they are.
#include <cstring>
#include <string>
#include <vector>
#include "../../include/rt355.h"
#include "../csrc/rebuild_common.h"
#include "rt_host.h"

namespace rt355 {

std::vector<rebuild::BlasRange> BlasRangesHost(const std::vector<RtBVHNode2>& nodes, const std::vector<uint32_t>& primIdx, size_t nPrims,
                                               const std::vector<RtBVHInstance>& inst, std::vector<int32_t>& instBlas)
{
    std::vector<rebuild::BlasRange> ranges;
    if (const char* why = rebuild::find_blas_ranges(nodes.data(), (int32_t)nodes.size(), primIdx.data(), (int32_t)primIdx.size(), (int32_t)nPrims,
                                                    inst.data(), (int32_t)inst.size(), ranges, instBlas))
        throw LbvhError(RT_E_UNSUPPORTED, std::string("rth_rebuild: ") + why);
    return ranges;
}

// Throws LbvhError and leaves everything unchanged when the rebuild is refused.
void BVH2::Rebuild(int builder, const RtBuildOptions* opt)
{
    if (builder != RT_REBUILD_SAH && builder != RT_REBUILD_LBVH && builder != RT_REBUILD_SBVH)
        throw LbvhError(RT_E_INVALID, "rth_rebuild: unknown builder " + std::to_string(builder));
    RebuildPlan("rth_rebuild", &builder, -1, opt);
}
// rt_rebuild_ranges' restatement: plan[nRanges], one word per distinct BLAS in increasing order of the ranges; a kept BLAS is appended
// as its bound block, relocated by the rule the kernel applies (rebuild::relocated_first).
void BVH2::RebuildRanges(const int32_t* plan, int nRanges, const RtBuildOptions* opt) { RebuildPlan("rth_rebuild_ranges", plan, nRanges, opt); }
// The one loop of both: nRanges < 0 means "every range: plan[0]" (checked by the caller).
void BVH2::RebuildPlan(const char* who, const int32_t* plan, int nRanges, const RtBuildOptions* opt)
{
    const std::string pre = std::string(who) + ": ";
    if (nRanges < 0) {   // (rth_rebuild answers a bad alpha before it looks at the scene)
        const float a0 = plan[0] == RT_REBUILD_SBVH && opt ? opt->alpha : 0.0f;
        if (!(a0 >= 0.0f && a0 <= 1.0f)) throw LbvhError(RT_E_INVALID, pre + "alpha must lie in [0, 1]");
    }
    if (bvhNodes.empty() || blasNodes.empty()) throw LbvhError(RT_E_INVALID, pre + "the scene has no BLAS (BuildBLAS comes first)");
    std::vector<int32_t> instBlas;
    std::vector<rebuild::BlasRange> ranges;
    if (const char* why = rebuild::find_blas_ranges(bvhNodes.data(), (int32_t)bvhNodes.size(), primIdx.data(), (int32_t)primIdx.size(), (int32_t)primitives_.size(),
                                                    blasNodes.data(), (int32_t)blasNodes.size(), ranges, instBlas))
        throw LbvhError(RT_E_UNSUPPORTED, pre + why);
    std::vector<int32_t> words(ranges.size(), nRanges < 0 ? plan[0] : 0);
    std::vector<rebuild::BlasBlock> blocks;
    if (nRanges >= 0) {
        rebuild::find_blas_blocks(bvhNodes.data(), ranges, blocks);
        std::string msg;
        if (const int rc = rebuild::check_plan(plan, nRanges, ranges, blocks.data(), 0, 0, msg)) throw LbvhError(rc, pre + msg);
        words.assign(plan, plan + nRanges);
    }
    bool anySbvh = false;
    for (const int32_t w : words) anySbvh = anySbvh || w == RT_REBUILD_SBVH;
    const float a = anySbvh && opt ? opt->alpha : 0.0f;   // (NULL or a zero-filled record: the full SBVH)
    if (!(a >= 0.0f && a <= 1.0f)) throw LbvhError(RT_E_INVALID, pre + "alpha must lie in [0, 1]");
    std::vector<RtBVHNode2> nodes;
    std::vector<uint32_t> idx, roots;
    uint32_t depth = 0, spatialSplits = 0, primsClipped = 0, forcedLeaves = 0; float cost = 0, wall = 0;
    auto too_deep = [&pre](const rebuild::BlasRange& r, int d) {   // rt_rebuild_scene's rule (validate_scene's): rt_upload_scene would refuse this tree
        return LbvhError(RT_E_UNSUPPORTED, pre + "the new BLAS over primitives [" + std::to_string(r.first) + ", " + std::to_string(r.first + r.count) +
                         ") needs " + std::to_string(d) + " stack entries, at most " + std::to_string(RT_BVH4_STACK) + " are supported");
    };
    for (size_t k = 0; k < ranges.size(); k++) {
        const rebuild::BlasRange& r = ranges[k];
        const int builder = words[k];
        const bool sbvh = builder == RT_REBUILD_SBVH;
        const uint32_t nodeBase = (uint32_t)nodes.size(), idxBase = (uint32_t)idx.size();
        if (builder == RT_REBUILD_KEEP || builder == RT_REBUILD_REFIT_RANGE) {   // the bound block, relocated; its primIdx slots as they are
            const rebuild::BlasBlock& blk = blocks[k];
            if (nodes.size() + blk.nodes > 0x7fffffffull || idx.size() + blk.idxSlots > 0x7fffffffull)
                throw LbvhError(RT_E_UNSUPPORTED, pre + "the new trees have 2^31 nodes or index slots, or more");
            const uint32_t nodeDelta = nodeBase - r.root, idxDelta = idxBase - blk.idxLo;
            roots.push_back(nodeBase);
            nodes.insert(nodes.end(), bvhNodes.begin() + r.root, bvhNodes.begin() + r.root + blk.nodes);
            for (size_t i = nodeBase; i < nodes.size(); i++) nodes[i].first = rebuild::relocated_first(nodes[i].first, nodes[i].count, nodeDelta, idxDelta);
            idx.insert(idx.end(), primIdx.begin() + blk.idxLo, primIdx.begin() + blk.idxLo + blk.idxSlots);
            if (blk.height > depth) depth = blk.height;
            if (builder == RT_REBUILD_REFIT_RANGE) {
                // ... and its boxes anew from the primitives as they are now, by rt_update_scene's rules (refit_common.h): breadth-first
                // from the root, then backwards, so every child comes before its parent
                std::vector<uint32_t> bfs(1, nodeBase);
                for (size_t head = 0; head < bfs.size(); head++)
                    if (nodes[bfs[head]].count == 0) { bfs.push_back(nodes[bfs[head]].first); bfs.push_back(nodes[bfs[head]].first + 1); }
                for (size_t a = bfs.size(); a-- > 0;) {
                    RtBVHNode2& n = nodes[bfs[a]];
                    if (n.count > 0) refit::set_box(n, refit::leaf_box(primitives_.data(), idx.data(), n.first, n.count));
                    else refit::set_box(n, lbvh::box_union(refit::node_box(nodes[n.first]), refit::node_box(nodes[n.first + 1])));
                }
            }
            continue;
        }
        if (sbvh) {   // the tree's size is known only once it is built: `written` nodes and nIdx indices are appended
            std::vector<RtBVHNode2> bn;
            std::vector<uint32_t> bi;
            RtSbvhStats st{};
            std::string err;
            const int rc = SbvhBuildVectors(a, primitives_.data(), (int32_t)r.first, (int32_t)r.count, nodeBase, idxBase, bn, bi, &st, err);
            if (rc != RT_OK) throw LbvhError(rc, err);
            if (rebuild::exceeds_stack(st.depth)) throw too_deep(r, st.depth);
            if (nodes.size() + bn.size() > 0x7fffffffull || idx.size() + bi.size() > 0x7fffffffull)
                throw LbvhError(RT_E_UNSUPPORTED, pre + "the new trees have 2^31 nodes or index slots, or more");
            roots.push_back(nodeBase);
            nodes.insert(nodes.end(), bn.begin(), bn.end());
            idx.insert(idx.end(), bi.begin(), bi.end());
            if ((uint32_t)st.depth > depth) depth = (uint32_t)st.depth;
            cost += st.sah_cost; wall += st.wall_ms;
            spatialSplits += (uint32_t)st.spatial_splits; primsClipped += (uint32_t)st.prims_clipped; forcedLeaves += (uint32_t)st.forced_leaves;
            continue;
        }
        std::vector<RtBVHNode2> bn((size_t)(2 * (int64_t)r.count - 1));
        std::vector<uint32_t> bi((size_t)r.count);
        RtBuildStats st{};
        int32_t written = 0;
        std::string err;
        const int rc = builder == RT_REBUILD_SAH
            ? SahBuildHost(primitives_.data(), (int32_t)primitives_.size(), (int32_t)r.first, (int32_t)r.count, nodeBase, idxBase, bn.data(),
                           (int32_t)bn.size(), &written, bi.data(), &st, err)
            : LbvhBuildHost(opt, primitives_.data(), (int32_t)primitives_.size(), (int32_t)r.first, (int32_t)r.count, nodeBase, idxBase, bn.data(),
                            (int32_t)bn.size(), &written, bi.data(), &st, err);
        if (rc != RT_OK) throw LbvhError(rc, err);
        if (rebuild::exceeds_stack(st.depth)) throw too_deep(r, st.depth);
        roots.push_back(nodeBase);
        nodes.insert(nodes.end(), bn.begin(), bn.begin() + written);
        idx.insert(idx.end(), bi.begin(), bi.end());
        if ((uint32_t)st.depth > depth) depth = (uint32_t)st.depth;
        cost += st.sah_cost; wall += st.wall_ms;
        if (builder == RT_REBUILD_LBVH) lastLbvh = st;
    }
    bvhNodes.swap(nodes);
    primIdx.swap(idx);
    for (size_t i = 0; i < blasNodes.size(); i++) blasNodes[i].bvhIdx = roots[(size_t)instBlas[i]];   // the transforms stay
    nodesUsed_ = rootNodeIdx_ = (uint32_t)bvhNodes.size();
    stat_build_time = wall; stat_node_count = nodesUsed_; stat_depth = depth; stat_sah_cost = cost;
    stat_prim_count = (uint32_t)primitives_.size();
    stat_spatial_splits = spatialSplits; stat_prims_clipped = primsClipped; stat_forced_leaves = forcedLeaves;   // (0 unless RT_REBUILD_SBVH)
    if (anySbvh) alpha = a;
}

} // namespace rt355

// rebuild_host.cpp — the host restatement of rt_rebuild_scene's BLAS rebuild (BVH2::Rebuild, rth_rebuild, include/rt355_host.h): every
// distinct BLAS of the scene is built again over the primitive range it covers (csrc/rebuild_common.h finds the ranges), in increasing
// order of the ranges and appended the way BuildBLAS appends BLAS after BLAS, with the host restatement of the chosen GPU builder.
// Together with TLAS::Build it is the ground truth the device rebuild must match bit for bit.
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
    const bool sbvh = builder == RT_REBUILD_SBVH;
    const float a = sbvh && opt ? opt->alpha : 0.0f;   // (NULL or a zero-filled record: the full SBVH)
    if (!(a >= 0.0f && a <= 1.0f)) throw LbvhError(RT_E_INVALID, "rth_rebuild: alpha must lie in [0, 1]");
    if (bvhNodes.empty() || blasNodes.empty()) throw LbvhError(RT_E_INVALID, "rth_rebuild: the scene has no BLAS (BuildBLAS comes first)");
    std::vector<int32_t> instBlas;
    const std::vector<rebuild::BlasRange> ranges = BlasRangesHost(bvhNodes, primIdx, primitives_.size(), blasNodes, instBlas);
    std::vector<RtBVHNode2> nodes;
    std::vector<uint32_t> idx, roots;
    uint32_t depth = 0, spatialSplits = 0, primsClipped = 0, forcedLeaves = 0; float cost = 0, wall = 0;
    auto too_deep = [](const rebuild::BlasRange& r, int d) {   // rt_rebuild_scene's rule (validate_scene's): rt_upload_scene would refuse this tree
        return LbvhError(RT_E_UNSUPPORTED, "rth_rebuild: the new BLAS over primitives [" + std::to_string(r.first) + ", " + std::to_string(r.first + r.count) +
                         ") needs " + std::to_string(d) + " stack entries, at most " + std::to_string(RT_BVH4_STACK) + " are supported");
    };
    for (const rebuild::BlasRange& r : ranges) {
        const uint32_t nodeBase = (uint32_t)nodes.size(), idxBase = (uint32_t)idx.size();
        if (sbvh) {   // the tree's size is known only once it is built: `written` nodes and nIdx indices are appended
            std::vector<RtBVHNode2> bn;
            std::vector<uint32_t> bi;
            RtSbvhStats st{};
            std::string err;
            const int rc = SbvhBuildVectors(a, primitives_.data(), (int32_t)r.first, (int32_t)r.count, nodeBase, idxBase, bn, bi, &st, err);
            if (rc != RT_OK) throw LbvhError(rc, err);
            if (rebuild::exceeds_stack(st.depth)) throw too_deep(r, st.depth);
            if (nodes.size() + bn.size() > 0x7fffffffull || idx.size() + bi.size() > 0x7fffffffull)
                throw LbvhError(RT_E_UNSUPPORTED, "rth_rebuild: the new trees have 2^31 nodes or index slots, or more");
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
    if (sbvh) alpha = a;
}

} // namespace rt355

// lbvh_host.cpp — the linear BVH builder's sequential host restatement (rth_build_bvh2_lbvh) and its Scene path
// (BVH2::BuildBLASLBVH, rth_build_blas_lbvh).  Every value comes from the rules of csrc/lbvh_common.h, which the GPU build
// (rt_build_bvh2, csrc/lbvh.hip) calls too: the two produce identical arrays, and this file is the oracle of the device build.
#include <algorithm>
#include <chrono>
#include <cstring>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>
#include "../../include/rt355.h"
#include "../../include/rt355_host.h"
#include "../csrc/lbvh_common.h"
#include "rt_host.h"

using namespace lbvh;

namespace rt355 {

int LbvhBuildHost(const RtBuildOptions* opt, const RtPrimitive* prims, int32_t nPrims, int32_t first, int32_t count,
                  uint32_t nodeBase, uint32_t idxBase, RtBVHNode2* nodes, int32_t nodeCap, int32_t* nNodes,
                  uint32_t* primIdx, RtBuildStats* stats, std::string& err)
{
    const auto t0 = std::chrono::steady_clock::now();
    Params P;
    if (const char* msg = check_args(opt, prims, nPrims, first, count, nodeBase, idxBase, nodes, nodeCap, nNodes, primIdx, P)) {
        err = std::string("rth_build_bvh2_lbvh: ") + msg;
        return RT_E_INVALID;
    }
    try {
        const uint32_t n = (uint32_t)count, nInt = n - 1;
        const int bIdx = index_bits(n), k = axis_bits(n);
        // 1. boxes and centroid bounds
        std::vector<Box> boxes(n);
        uint32_t cb[6] = { kKeyMinInit, kKeyMinInit, kKeyMinInit, kKeyMaxInit, kKeyMaxInit, kKeyMaxInit };
        for (uint32_t i = 0; i < n; i++) {
            boxes[i] = prim_box(prims[first + i]);
            for (int a = 0; a < 3; a++) {
                const float c = centroid(boxes[i], a);
                if (finite_(c)) { cb[a] = std::min(cb[a], order_key(c)); cb[3 + a] = std::max(cb[3 + a], order_key(c)); }
            }
        }
        // 2. keys, 3. sort (keys are distinct)
        float clo[3], scale[3];
        quantizer(cb, cb + 3, k, clo, scale);
        std::vector<std::pair<uint64_t, uint32_t>> kv(n);
        for (uint32_t i = 0; i < n; i++) kv[i] = { make_key(boxes[i], clo, scale, k, bIdx, i), i };
        std::sort(kv.begin(), kv.end());
        std::vector<uint64_t> keys(n);
        for (uint32_t i = 0; i < n; i++) keys[i] = kv[i].first;
        // 4. radix tree, then the bottom-up pass: a node is computed by the second of its children to arrive
        std::vector<uint32_t> left(n), right(n), rfirst(n), parent(2 * (size_t)n - 1, kNone), tickets(n, 0);
        for (uint32_t i = 0; i < nInt; i++) {
            uint32_t last;
            karras_node(keys.data(), n, i, left[i], right[i], rfirst[i], last);
            parent[left[i]] = i;
            parent[right[i]] = i;
        }
        std::vector<NodeRec> rec(2 * (size_t)n - 1);
        for (uint32_t s = 0; s < n; s++) {
            rec[nInt + s] = leaf_rec(boxes[kv[s].second], s, P);
            for (uint32_t p = parent[nInt + s]; p != kNone; p = parent[p]) {
                if (tickets[p]++ == 0) break;
                rec[p] = combine(rec[left[p]], rec[right[p]], rfirst[p], P);
            }
        }
        // 5./6. survivors, their pair slots (exclusive prefix count), emit
        std::vector<uint32_t> flags(nInt), rank(nInt);
        uint32_t run = 0;
        for (uint32_t i = 0; i < nInt; i++) { flags[i] = survives(rec.data(), parent.data(), i, P.maxLeaf); rank[i] = run; run += flags[i]; }
        const uint32_t outNodes = 2 * rec[0].leaves - 1;
        nodes[0] = emit(rec[0], 0, nInt, rank.data(), nodeBase, idxBase);
        for (uint32_t i = 0; i < nInt; i++) if (flags[i]) {
            nodes[1 + 2 * rank[i]] = emit(rec[left[i]], left[i], nInt, rank.data(), nodeBase, idxBase);
            nodes[2 + 2 * rank[i]] = emit(rec[right[i]], right[i], nInt, rank.data(), nodeBase, idxBase);
        }
        for (uint32_t s = 0; s < n; s++) primIdx[s] = (uint32_t)first + kv[s].second;
        *nNodes = (int32_t)outNodes;
        if (stats) {
            stats->nodes = (int32_t)outNodes; stats->leaves = (int32_t)rec[0].leaves; stats->depth = (int32_t)rec[0].height;
            stats->morton_bits = k; stats->sah_cost = rec[0].total; stats->device_ms = 0;
            stats->wall_ms = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count();
            stats->_reserved = 0;
        }
        return RT_OK;
    } catch (const std::exception& e) {
        err = std::string("rth_build_bvh2_lbvh: ") + e.what();
        return RT_E_NOMEM;
    }
}

// BuildBLAS's bookkeeping for a BLAS built elsewhere, rooted at nodeBase = bvhNodes.size(): instance record, appended arrays, statistics
void BVH2::AppendBuiltBLAS(uint32_t nodeBase, const RtBVHNode2* nodes, size_t nN, const uint32_t* idx, size_t nI, float wall_ms, int32_t depth,
                           float cost)
{
    RtBVHInstance inst;
    memset(&inst, 0, sizeof inst);
    inst.bvhIdx = nodeBase;
    inst.invT[0] = inst.invT[5] = inst.invT[10] = inst.invT[15] = 1.0f;
    blasNodes.push_back(inst);
    bvhNodes.insert(bvhNodes.end(), nodes, nodes + nN);
    primIdx.insert(primIdx.end(), idx, idx + nI);
    nodesUsed_ = rootNodeIdx_ = (uint32_t)bvhNodes.size();
    stat_build_time += wall_ms;
    stat_node_count = nodesUsed_;
    if ((uint32_t)depth > stat_depth) stat_depth = (uint32_t)depth;
    stat_sah_cost += cost;
    stat_prim_count = (uint32_t)primitives_.size();
}

// The linear builder, appended as BuildBLAS appends.  The scene is left unchanged when the build is refused.
void BVH2::BuildBLASLBVH(int startIdx, int device, const RtBuildOptions* opt)
{
    const int64_t n = (int64_t)primitives_.size() - startIdx;
    if (startIdx < 0 || n <= 0) throw std::runtime_error("BuildBLASLBVH: empty primitive range");
    if (n > (1 << 30)) throw std::runtime_error("BuildBLASLBVH: more than 2^30 primitives");
    const uint32_t nodeBase = (uint32_t)bvhNodes.size(), idxBase = (uint32_t)primIdx.size();
    std::vector<RtBVHNode2> nodes((size_t)(2 * n - 1));
    std::vector<uint32_t> idx((size_t)n);
    RtBuildStats st{};
    int32_t written = 0;
    std::string err;
    const int rc = device < 0
        ? LbvhBuildHost(opt, primitives_.data(), (int32_t)primitives_.size(), startIdx, (int32_t)n, nodeBase, idxBase, nodes.data(),
                        (int32_t)nodes.size(), &written, idx.data(), &st, err)
        : rt_build_bvh2(device, opt, primitives_.data(), (int32_t)primitives_.size(), startIdx, (int32_t)n, nodeBase, idxBase, nodes.data(),
                        (int32_t)nodes.size(), &written, idx.data(), &st);
    if (rc != RT_OK) throw LbvhError(rc, device < 0 ? err : std::string(rt_last_error()));
    AppendBuiltBLAS(nodeBase, nodes.data(), (size_t)written, idx.data(), idx.size(), st.wall_ms, st.depth, st.sah_cost);
    lastLbvh = st;
}

} // namespace rt355

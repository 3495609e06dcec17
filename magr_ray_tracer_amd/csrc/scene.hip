// scene.hip — the device copy of a scene (SceneBag, scene_dev.h) through its life: the host-side checks of the arrays, the upload and
// what it derives, in-place updates and rebuilds, the debug views.  Host code only: the kernels it drives are refit.hip's, rebuild.hip's
// and the builders'; of the contexts that render from a copy (rt355.hip) it knows SceneBag::wait_holders and nothing else.
#include <chrono>
#include <cstdlib>
#include <cstring>
#include <string>
#include "scene_dev.h"
#include "resize_common.h"

using namespace scenedev;

static int bvh2_depth(const RtBVHNode2* n, int32_t nNodes, uint32_t root)
{
    // iterative depth of the subtree at `root`; also validates child indices
    std::vector<std::pair<uint32_t, int>> st; st.push_back({ root, 0 });
    int best = 0; size_t visited = 0;
    while (!st.empty()) {
        auto [i, d] = st.back(); st.pop_back();
        if (i >= (uint32_t)nNodes || ++visited > (size_t)nNodes * 2 + 2) return -1;
        if (d > best) best = d;
        if (n[i].count == 0) { st.push_back({ n[i].first, d + 1 }); st.push_back({ n[i].first + 1, d + 1 }); }
    }
    return best;
}
static int bvh4_stack_need(const RtBVHNode4* n, int32_t nNodes, int32_t nIdx, uint32_t root)
{
    // worst-case live stack entries of the unordered 4-wide traversal (push every interior child, pop one); the slots have passed
    // rebuild::bvh4_slot, so a child is what the kernel pushes
    std::vector<std::pair<uint32_t, int>> st; st.push_back({ root, 0 });
    int best = 0; size_t visited = 0;
    while (!st.empty()) {
        auto [i, base] = st.back(); st.pop_back();
        if (++visited > (size_t)nNodes + 1) return -1;   // (in range: the root by the caller's check, a child by the slot rule)
        int kids = 0;
        for (int k = 0; k < 4; k++) if (rebuild::bvh4_slot(n[i], k, nNodes, nIdx) == rebuild::kSlotChild) kids++;
        if (base + kids > best) best = base + kids;
        int pushed = 0;
        for (int k = 0; k < 4; k++) if (rebuild::bvh4_slot(n[i], k, nNodes, nIdx) == rebuild::kSlotChild) {
            // child k is popped when the (kids-1-pushed) later siblings are gone: entries below it = base + pushed
            st.push_back({ (uint32_t)n[i].first[k], base + pushed });
            pushed++;
        }
    }
    return best;
}

// Host-side shape checks of a scene (no device needed; rt_upload_scene runs them first): a kernel that walks a malformed tree can
// fault the GPU.  Also sizes the LDS traversal stack and the texture padding.
int scenedev::validate_scene(int accel, const HostScene& in, int* stackEntriesOut, int64_t* texPadOut, int* tlasDepthOut)
{
    const auto& [prims, nPrims, mats, nMats, textures, nTexels, lights, nLights, bvhNodes, nNodes, primIdx, nIdx, tlas, nTlas, blas, nBlas] = in;
    if (accel != RT_ACCEL_BVH2 && accel != RT_ACCEL_BVH4) return fail(RT_E_INVALID, "rt_upload_scene: unknown accel %d", accel);
    if (!prims || nPrims <= 0 || !mats || nMats <= 0 || !bvhNodes || nNodes <= 0 || !primIdx || nIdx <= 0 || !tlas || nTlas <= 0 || !blas || nBlas <= 0)
        return fail(RT_E_INVALID, "rt_upload_scene: missing array (prims/materials/bvh/primIdx/tlas/blas are required)");
    if (nLights < 0 || nTexels < 0) return fail(RT_E_INVALID, "rt_upload_scene: negative count (nLights %d, nTexels %d)", nLights, nTexels);
    if (nLights > 0 && !lights) return fail(RT_E_INVALID, "rt_upload_scene: nLights > 0 but lights == NULL");
    if (nTexels > 0 && !textures) return fail(RT_E_INVALID, "rt_upload_scene: nTexels > 0 but textures == NULL");
    // Child ids and instance ids of the TLAS travel as 15-bit values on the traversal stacks (bit 15 = leaf; the reference's own
    // TLASNode packs two 16-bit child ids into leftRight and TLAS::Build stops at 256 instances, tlas.cpp:11): larger trees are refused.
    if (nTlas > 0x8000 || nBlas > 0x8000) return fail(RT_E_UNSUPPORTED, "rt_upload_scene: %d TLAS nodes / %d instances exceed the 32768 the traversal stacks encode", nTlas, nBlas);
    for (int32_t i = 0; i < nPrims; i++) {
        if (prims[i].matIdx < 0 || prims[i].matIdx >= nMats) return fail(RT_E_INVALID, "primitive %d: matIdx %d out of range", i, prims[i].matIdx);
        if (prims[i].objType < 0 || prims[i].objType > 2) return fail(RT_E_INVALID, "primitive %d: objType %d", i, prims[i].objType);
    }
    for (int32_t i = 0; i < nIdx; i++) if (primIdx[i] >= (uint32_t)nPrims) return fail(RT_E_INVALID, "primIdx[%d] = %u out of range", i, primIdx[i]);
    for (int32_t i = 0; i < nLights; i++) if (lights[i] >= (uint32_t)nPrims) return fail(RT_E_INVALID, "lights[%d] out of range", i);
    int64_t texPad = 2; // the reference's lookup can land one row + one texel past a texture (uv == 1): pad the atlas
    if (const int32_t m = resize::check_materials(mats, nMats, nTexels, &texPad); m >= 0)   // (rt_update_materials holds a new table to the same rule)
        return fail(RT_E_INVALID, "material %d: texture window exceeds the atlas", m);
    for (int32_t i = 0; i < nTlas; i++) {
        const uint32_t lr = tlas[i].leftRight;
        if (lr == 0) { if (tlas[i].BLASidx >= (uint32_t)nBlas) return fail(RT_E_INVALID, "tlas node %d: BLASidx out of range", i); }
        else if ((lr & 0xffffu) >= (uint32_t)nTlas || (lr >> 16) >= (uint32_t)nTlas) return fail(RT_E_INVALID, "tlas node %d: child out of range", i);
    }
    int tlasDepth = 0;
    {   // walk the TLAS from node 0: a back reference would make traverse_tlas spin forever, and its private stack holds
        // RT_TLAS_STACK entries (the ordered descent keeps at most one pending sibling per level, so depth bounds the stack)
        std::vector<std::pair<uint32_t, int>> st; st.push_back({ 0u, 0 });
        size_t visited = 0;
        while (!st.empty()) {
            auto [i, d] = st.back(); st.pop_back();
            if (++visited > (size_t)nTlas) return fail(RT_E_INVALID, "tlas: a node is reachable twice (cycle or shared child)");
            tlasDepth = std::max(tlasDepth, d);
            const uint32_t lr = tlas[i].leftRight;
            if (lr != 0) { st.push_back({ lr & 0xffffu, d + 1 }); st.push_back({ lr >> 16, d + 1 }); }
        }
        if (tlasDepth > RT_TLAS_STACK) return fail(RT_E_UNSUPPORTED, "tlas: depth %d exceeds the %d-entry traversal stack", tlasDepth, RT_TLAS_STACK);
    }
    // The reference kernels give BVH2 32 and BVH4 64 stack entries (bvh.cl:15,57) and overflow silently beyond that
    // (SBVH trees at alpha = 0 do get deeper than 32); this library sizes the LDS stack to the tree, up to 64 entries.
    const int stackCap = RT_BVH4_STACK;
    int stackNeed = 1;
    if (accel == RT_ACCEL_BVH4) {   // every slot of every node, before anything follows one (the rule: rebuild_common.h, bvh4_slot)
        const RtBVHNode4* n4 = (const RtBVHNode4*)bvhNodes;
        for (int32_t i = 0; i < nNodes; i++) for (int k = 0; k < 4; k++) if (rebuild::bvh4_slot(n4[i], k, nNodes, nIdx) == rebuild::kSlotBad)
            return fail(RT_E_INVALID, "bvh4 node %d slot %d: first %d, count %d is neither unused (first = -1), a leaf range inside primIdx nor a child node", i, k,
                        n4[i].first[k], n4[i].count[k]);
    }
    for (int32_t b = 0; b < nBlas; b++) {
        if (blas[b].bvhIdx >= (uint32_t)nNodes) return fail(RT_E_INVALID, "instance %d: bvhIdx out of range", b);
        int need = accel == RT_ACCEL_BVH4 ? bvh4_stack_need((const RtBVHNode4*)bvhNodes, nNodes, nIdx, blas[b].bvhIdx)
                                          : bvh2_depth((const RtBVHNode2*)bvhNodes, nNodes, blas[b].bvhIdx);
        if (need < 0) return fail(RT_E_INVALID, "instance %d: malformed BVH (child index out of range or cycle)", b);
        if (rebuild::exceeds_stack(need)) return fail(RT_E_UNSUPPORTED, "instance %d: traversal needs %d stack entries, at most %d are supported", b, need, stackCap);
        stackNeed = std::max(stackNeed, need);
    }
    if (accel == RT_ACCEL_BVH2) {
        const RtBVHNode2* n2 = (const RtBVHNode2*)bvhNodes;
        for (int32_t i = 0; i < nNodes; i++) if (n2[i].count > 0 && (uint64_t)n2[i].first + n2[i].count > (uint64_t)nIdx)
            return fail(RT_E_INVALID, "bvh node %d: leaf range exceeds primIdx", i);
    }
    if (stackEntriesOut) *stackEntriesOut = rebuild::stack_entries(stackNeed);   // (rebuild_common.h: rt_rebuild_scene sizes it the same way)
    if (texPadOut) *texPadOut = texPad;
    if (tlasDepthOut) *tlasDepthOut = tlasDepth;
    return RT_OK;
}
extern "C" int rt_validate_scene(int32_t accel, const RtPrimitive* prims, int32_t nPrims, const RtMaterial* mats, int32_t nMats,
                                 const RtFloat4* textures, int32_t nTexels, const uint32_t* lights, int32_t nLights,
                                 const void* bvhNodes, int32_t nNodes, const uint32_t* primIdx, int32_t nIdx,
                                 const RtTLASNode* tlas, int32_t nTlas, const RtBVHInstance* blas, int32_t nBlas)
{
    return validate_scene(accel, HostScene{ prims, nPrims, mats, nMats, textures, nTexels, lights, nLights, bvhNodes, nNodes, primIdx, nIdx, tlas, nTlas, blas, nBlas },
                          nullptr, nullptr, nullptr);
}

// What rt_update_scene needs of an upload: the counts, the host shadow of the fields an update must keep, and the refit topology on
// the device (parents, reachable leaves, pair id -> node id).  A scene the update cannot handle records why (refitRefusal).
// (a BVH4 copy that keeps its BVH2 - in.bvhNodes is the BVH2 - is prepared like a BVH2 copy: it can be rebuilt; rt_update_scene refuses
// every BVH4 context before it comes here)
static int prepare_update(SceneBag& b, int accel, int extendVariant, const HostScene& in, const std::vector<uint32_t>& pairNode)
{
    const auto& [prims, nPrims, mats, nMats, textures, nTexels, lights, nLights, bvhNodes, nNodes, primIdx, nIdx, tlas, nTlas, blas, nBlas] = in;
    b.nPrims = nPrims; b.nNodes = nNodes; b.nIdx = nIdx; b.nLights = nLights; b.nTlas = nTlas; b.nBlas = nBlas;
    b.nPairs = (int32_t)pairNode.size(); b.accel = accel;
    if (accel != RT_ACCEL_BVH2 && !b.keepsBvh2) { b.refitRefusal = "BVH4 scenes cannot be refit"; return RT_OK; }
    if (nBlas > refit::kMaxInstances) { b.refitRefusal = "more than 256 instances (TLAS::Build's limit)"; return RT_OK; }
    if (nTlas != 2 * nBlas) { b.refitRefusal = "the TLAS does not have TLAS::Build's 2 x instances nodes"; return RT_OK; }
    refit::Topology t;
    if (const char* why = refit::build_topology((const RtBVHNode2*)bvhNodes, nNodes, blas, nBlas, t)) { b.refitRefusal = why; return RT_OK; }
    b.primType.resize((size_t)nPrims); b.primMat.resize((size_t)nPrims);
    for (int32_t i = 0; i < nPrims; i++) { b.primType[(size_t)i] = prims[i].objType; b.primMat[(size_t)i] = prims[i].matIdx; }
    b.inst.assign(blas, blas + nBlas);
    b.variantLayout1 = extendVariant != 1;
    // rt_rebuild_scene: the primitive range of each BLAS (rebuild_common.h)
    b.rebuildRefusal = rebuild::find_blas_ranges((const RtBVHNode2*)bvhNodes, nNodes, primIdx, nIdx, nPrims, blas, nBlas, b.ranges, b.instBlas);
    if (!b.rebuildRefusal) {   // RT_REBUILD_REFIT: root, interior nodes and height of every BLAS (build_topology has walked the trees: no cycle)
        const RtBVHNode2* n2 = (const RtBVHNode2*)bvhNodes;
        const size_t nR = b.ranges.size();
        rebuild::find_blas_blocks(n2, b.ranges, b.blasBlock);   // rt_rebuild_ranges: which of them can be kept, and what they occupy
        b.blasRoot.assign(nR, 0u); b.blasInteriors.assign(nR, 0u); b.blasHeight.assign(nR, 0u);
        std::vector<uint8_t> done(nR, 0);
        std::vector<std::pair<uint32_t, uint32_t>> st;
        for (int32_t i = 0; i < nBlas; i++) {
            const size_t k = (size_t)b.instBlas[(size_t)i];
            if (done[k]) continue;
            done[k] = 1; b.blasRoot[k] = blas[i].bvhIdx;
            st.assign(1, { blas[i].bvhIdx, 0u });
            while (!st.empty()) {
                const auto [node, d] = st.back(); st.pop_back();
                b.blasHeight[k] = std::max(b.blasHeight[k], d);
                if (n2[node].count > 0) continue;
                b.blasInteriors[k]++;
                st.push_back({ n2[node].first, d + 1 }); st.push_back({ n2[node].first + 1, d + 1 });
            }
        }
    }
    b.nLeaves = (uint32_t)t.leaves.size(); b.nReach = (uint32_t)t.order.size();
    int rc = dalloc(b.allocs, &b.dParent, t.parent.size());
    if (rc == RT_OK) rc = dalloc(b.allocs, &b.dLeaves, t.leaves.size());
    if (rc == RT_OK) rc = dalloc(b.allocs, &b.dTickets, (size_t)nNodes);
    if (rc == RT_OK) rc = dalloc(b.allocs, &b.dPairNode, pairNode.size());
    if (rc != RT_OK) return rc;
    HIPCHK(hipMemcpy(b.dParent, t.parent.data(), sizeof(uint32_t) * t.parent.size(), hipMemcpyHostToDevice));
    if (!t.leaves.empty()) HIPCHK(hipMemcpy(b.dLeaves, t.leaves.data(), sizeof(uint32_t) * t.leaves.size(), hipMemcpyHostToDevice));
    if (!pairNode.empty()) HIPCHK(hipMemcpy(b.dPairNode, pairNode.data(), sizeof(uint32_t) * pairNode.size(), hipMemcpyHostToDevice));
    return RT_OK;
}

// ---- scene upload: validate (above), derive, copy to device, bind.  What it derives, as functions of the host arrays; the record rules
// are refit_common.h's and rebuild_common.h's (the kernels of an update or a rebuild write the same records) ---------------------------
static std::vector<RtFloat4> shade_records(const RtPrimitive* prims, int32_t nPrims)   // k_shade: geometric normal + material id + type per primitive
{
    std::vector<RtFloat4> recs((size_t)nPrims);
    for (int32_t i = 0; i < nPrims; i++) recs[(size_t)i] = refit::shade_rec(prims[i]);
    return recs;
}
// k_shade, NEE: the first 64 bytes of the light's Primitive, {objType, area}, its material's emittance (k_light_recs rewrites words 0..4)
static std::vector<RtFloat4> light_records(const RtPrimitive* prims, const RtMaterial* mats, const uint32_t* lights, int32_t nLights)
{
    std::vector<RtFloat4> lr(std::max<size_t>((size_t)nLights, 1) * 8, RtFloat4{ 0, 0, 0, 0 });
    for (int32_t i = 0; i < nLights; i++) {
        const RtPrimitive& p = prims[lights[i]];
        refit::light_rec(p, &lr[(size_t)i * 8]);
        lr[(size_t)i * 8 + 5] = mats[p.matIdx].emittance;
    }
    return lr;
}
static std::vector<RtFloat4> triangle_records(const RtPrimitive* prims, const uint32_t* primIdx, int32_t nIdx)   // leaf-ordered vertices + primitive id
{
    std::vector<RtFloat4> recs((size_t)nIdx * 3);
    for (int32_t s = 0; s < nIdx; s++) refit::tri_rec(prims[primIdx[s]], primIdx[s], &recs[(size_t)s * 3]);
    return recs;
}
// The nodes a derived table keeps, renumbered breadth-first, BLAS by BLAS, and stored densely: breadth-first puts the top levels of
// the (first) tree, which every ray visits, into the first records.  kids(i, number) calls number(c) for every child c of node i that
// gets a record; newId (all rebuild::kNone) receives node id -> record id.
template <class Kids> static std::vector<uint32_t> breadth_first(const std::vector<uint32_t>& roots, std::vector<uint32_t>& newId, Kids kids)
{
    std::vector<uint32_t> order;
    auto number = [&](uint32_t c) { if (newId[c] == rebuild::kNone) { newId[c] = (uint32_t)order.size(); order.push_back(c); } };
    for (const uint32_t root : roots) {
        size_t head = order.size();
        number(root);
        for (; head < order.size(); head++) kids(order[head], number);
    }
    return order;
}
// Layout 1 of a BVH2 (rt355_kernels.h, traverse_bvh2_packed): a record per interior node - the reference array interleaves leaves and
// interior nodes (children are allocated in pairs), so a table indexed by the reference's node id would be half holes.  `order`
// receives pair id -> node id (rt_update_scene rewrites the pairs' boxes), `roots` every instance's encoded root.
static std::vector<RtFloat4> pair_records(const RtBVHNode2* n2, int32_t nNodes, const RtBVHInstance* blas, int32_t nBlas, std::vector<uint32_t>& order,
                                          std::vector<uint32_t>& roots)
{
    std::vector<uint32_t> newId((size_t)nNodes, rebuild::kNone), interiorRoots;
    for (int32_t b = 0; b < nBlas; b++) if (n2[blas[b].bvhIdx].count == 0) interiorRoots.push_back(blas[b].bvhIdx);
    order = breadth_first(interiorRoots, newId, [&](uint32_t i, auto& number) {
        for (uint32_t c = n2[i].first; c <= n2[i].first + 1; c++) if (n2[c].count == 0) number(c);
    });
    std::vector<RtFloat4> pairs(std::max<size_t>(order.size(), 1) * 4, RtFloat4{ 0, 0, 0, 0 });
    for (size_t k = 0; k < order.size(); k++) rebuild::pair_record(n2, order[k], newId.data(), &pairs[k * 4]);   // (k_pair_boxes rewrites the boxes)
    for (int32_t b = 0; b < nBlas; b++) roots[(size_t)b] = rebuild::child_entry(n2[blas[b].bvhIdx], newId[blas[b].bvhIdx]);
    return pairs;
}
// Layout 1 of a BVH4: four child boxes + four encoded child entries per node.  The collapse (bvh.cpp:695-803) leaves the absorbed BVH2
// nodes in the array: only the nodes still reachable from a BLAS root are kept (on the bench scene 1 node in 4 is alive).
static std::vector<RtFloat4> quad_records(const RtBVHNode4* n4, int32_t nNodes, int32_t nIdx, const RtBVHInstance* blas, int32_t nBlas, std::vector<uint32_t>& roots)
{
    std::vector<uint32_t> newId((size_t)nNodes, rebuild::kNone), all((size_t)nBlas);
    for (int32_t b = 0; b < nBlas; b++) all[(size_t)b] = blas[b].bvhIdx;
    const std::vector<uint32_t> order = breadth_first(all, newId, [&](uint32_t i, auto& number) {
        for (int k = 0; k < 4; k++) if (rebuild::bvh4_slot(n4[i], k, nNodes, nIdx) == rebuild::kSlotChild) number((uint32_t)n4[i].first[k]);
    });
    std::vector<RtFloat4> quads(std::max<size_t>(order.size(), 1) * 8, RtFloat4{ 0, 0, 0, 0 });
    for (size_t q = 0; q < order.size(); q++) collapse::quad_record(n4[order[q]], nNodes, nIdx, newId.data(), &quads[q * 8]);   // (k_c4_quads writes the same)
    for (int32_t b = 0; b < nBlas; b++) roots[(size_t)b] = newId[blas[b].bvhIdx];
    return quads;
}
// TLAS interior records (traverse_tlas; tagged: the children in the encoding of k_trace_persist_tlas) and instance records (traverse_instance)
static std::vector<RtFloat4> tlas_records(const RtTLASNode* tlas, int32_t nTlas, bool tagged)
{
    std::vector<RtFloat4> tp((size_t)nTlas * 4, RtFloat4{ 0, 0, 0, 0 });
    for (int32_t i = 0; i < nTlas; i++) refit::tlas_pair(tlas, (uint32_t)i, tagged, &tp[(size_t)i * 4]);   // (k_tlas_build)
    return tp;
}
static std::vector<RtFloat4> instance_records(const RtBVHInstance* blas, int32_t nBlas, const std::vector<uint32_t>& roots)
{
    std::vector<RtFloat4> ir((size_t)nBlas * 4);
    for (int32_t b = 0; b < nBlas; b++) refit::inst_rec(blas[b], roots[(size_t)b], &ir[(size_t)b * 4]);
    return ir;
}

template <class T> static int upload(SceneBag& b, T** dst, const T* src, size_t count)
{
    const int rc = dalloc(b.allocs, dst, count);
    if (rc != RT_OK) return rc;
    if (count) HIPCHK(hipMemcpy(*dst, src, count * sizeof(T), hipMemcpyHostToDevice));
    return RT_OK;
}
template <class T> static int upload(SceneBag& b, T** dst, const std::vector<T>& v) { return upload(b, dst, v.data(), v.size()); }

static int collapse_uploaded(SceneBag& b, SceneArrays& sc, int extendVariant, const HostScene& in, const std::vector<collapse::Blas>& blas4, int& layout,
                             int& stackEntries, std::vector<uint32_t>& roots);   // (below, with the rebuild's helpers it shares)

int scenedev::upload_scene(SceneBag& b, int accel, int extendVariant, const HostScene& in, int stackEntries, int64_t texPad, int tlasDepth,
                           const std::vector<collapse::Blas>* blas4)
{
    const auto& [prims, nPrims, mats, nMats, textures, nTexels, lights, nLights, bvhNodes, nNodes, primIdx, nIdx, tlas, nTlas, blas, nBlas] = in;
    // ---- derive.  Layout 1 (pair or quad records, triangle records, encoded roots) only when the encodings fit (rebuild_common.h,
    // shared with rt_rebuild_scene's kernels); in layout 0 the instance records carry root entry 0
    const RtBVHNode2* n2 = (const RtBVHNode2*)bvhNodes; const RtBVHNode4* n4 = (const RtBVHNode4*)bvhNodes;
    std::vector<uint32_t> pairNode, roots((size_t)nBlas, 0u);
    std::vector<RtFloat4> pairs, quads;
    int layout = 0;
    if (accel == RT_ACCEL_BVH2) {
        uint32_t largestLeaf = 0;
        for (int32_t i = 0; i < nNodes; i++) largestLeaf = std::max(largestLeaf, n2[i].count);
        if (rebuild::takes_layout1(extendVariant != 1, nIdx, largestLeaf)) { pairs = pair_records(n2, nNodes, blas, nBlas, pairNode, roots); layout = 1; }
    } else if (blas4) {
        // (the layout follows from the collapse on the device, below)
    } else if (extendVariant != 1 && nIdx < (1 << 24)) {
        bool fits = true;
        for (int32_t i = 0; i < nNodes && fits; i++) for (int k = 0; k < 4; k++) if (n4[i].first[k] != RT_INVALID && n4[i].count[k] > (int32_t)rebuild::kMaxPackedLeaf) fits = false;
        if (fits) { quads = quad_records(n4, nNodes, nIdx, blas, nBlas, roots); layout = 1; }
    }
    // ---- copy to device
    SceneArrays sc{};
    int rc = upload(b, &sc.prims, prims, (size_t)nPrims);
    if (rc == RT_OK) rc = upload(b, &sc.mats, mats, (size_t)nMats);
    if (rc == RT_OK) rc = dalloc(b.allocs, &sc.tex, (size_t)nTexels + (size_t)texPad);   // zero-padded atlas (texPad: validate_scene)
    if (rc == RT_OK) {
        HIPCHK(hipMemset(sc.tex, 0, sizeof(RtFloat4) * ((size_t)nTexels + (size_t)texPad)));
        if (nTexels) HIPCHK(hipMemcpy(sc.tex, textures, sizeof(RtFloat4) * (size_t)nTexels, hipMemcpyHostToDevice));
    }
    if (rc == RT_OK) rc = upload(b, &sc.lights, lights, (size_t)nLights);
    if (rc == RT_OK) rc = accel == RT_ACCEL_BVH4 && !blas4 ? upload(b, &sc.bvh4, n4, (size_t)nNodes) : upload(b, &sc.bvh2, n2, (size_t)nNodes);
    if (rc == RT_OK) rc = upload(b, &sc.primIdx, primIdx, (size_t)nIdx);
    if (rc == RT_OK) rc = upload(b, &sc.tlas, tlas, (size_t)nTlas);
    if (rc == RT_OK) rc = upload(b, &sc.blas, blas, (size_t)nBlas);
    if (rc == RT_OK) rc = upload(b, &sc.shadeRecs, shade_records(prims, nPrims));
    if (rc == RT_OK) rc = upload(b, &sc.lightRecs, light_records(prims, mats, lights, nLights));
    if (rc == RT_OK && blas4) rc = collapse_uploaded(b, sc, extendVariant, in, *blas4, layout, stackEntries, roots);
    else if (rc == RT_OK && layout == 1) {
        rc = accel == RT_ACCEL_BVH4 ? upload(b, &sc.quads, quads) : upload(b, &sc.pairs, pairs);
        if (rc == RT_OK) rc = upload(b, &sc.triRecs, triangle_records(prims, primIdx, nIdx));
        if (rc == RT_OK) rc = upload(b, &sc.rootEntry, roots);
    }
    if (rc == RT_OK) rc = upload(b, &sc.tlasPairs, tlas_records(tlas, nTlas, false));
    if (rc == RT_OK) rc = upload(b, &sc.instRecs, instance_records(blas, nBlas, roots));
    if (rc == RT_OK) rc = upload(b, &sc.tlasPairsP, tlas_records(tlas, nTlas, true));
    if (rc != RT_OK) return rc;
    const bool leafRoot = tlas[0].leftRight == 0;
    sc.tlasRoot = leafRoot ? (refit::kLeafBit | tlas[0].BLASidx) : 0u;
    sc.tlasRootP = leafRoot ? (refit::kTagInst | tlas[0].BLASidx) : refit::kTagTlas;
    sc.nLights = nLights; sc.nPrims = nPrims; sc.nBlas = nBlas; sc.nTex = nTexels; sc.nMats = nMats;
    // ---- bind: the copy's facts, and what updates and rebuilds need of this upload
    b.sc = sc;
    b.hMats.assign(mats, mats + nMats); b.texPad = texPad; b.texCap = (size_t)nTexels + (size_t)texPad;   // (rt_update_materials)
    b.layout = layout; b.stackEntries = stackEntries; b.tlasDepth = tlasDepth; b.nInterior = (int)pairNode.size(); b.singleBlas = leafRoot;
    if (!blas4) b.nQuads = (int32_t)(quads.size() / 8);
    return prepare_update(b, accel, extendVariant, in, pairNode);
}

// ---- in-place scene updates (rt_update_scene; kernels: refit.hip, rules: refit_common.h) and what they share with a rebuild -----------
namespace refitdev {
hipError_t launch_refit(hipStream_t s, RtBVHNode2* nodes, uint32_t nNodes, const RtPrimitive* prims, const uint32_t* primIdx, const uint32_t* leaves,
                        uint32_t nLeaves, const uint32_t* parent, uint32_t* tickets);
hipError_t launch_tlas(hipStream_t s, const RtBVHNode2* nodes, const RtBVHInstance* inst, int n, const uint32_t* rootEntry, RtTLASNode* tlas, RtFloat4* tp,
                       RtFloat4* tpP, RtFloat4* ir, int32_t* status);
hipError_t launch_records(hipStream_t s, const RtPrimitive* prims, const RtBVHNode2* nodes, const uint32_t* primIdx, uint32_t nIdx, const uint32_t* lights,
                          uint32_t nLights, uint32_t first, uint32_t count, const uint32_t* pairNode, uint32_t nPairs, RtFloat4* pairs, RtFloat4* triRecs,
                          RtFloat4* shadeRecs, RtFloat4* lightRecs);
}

// Capacities of what scales with the trees (SceneBag::RebuildSet, the derivation's scratch, rt_update_scene's staging nodes): index
// slots at first, twice as many nodes; RT355_REBUILD_INITIAL_CAP=k (read per call; tests, A/B runs) starts smaller or larger.  An array
// that a finished tree outgrows goes to the need plus need / kRebuildHeadroomDiv: a quarter covers the frame-to-frame drift of an
// animated SBVH scene (its slot count moved by a few percent between the deformations tried), so a per-frame rebuild stops allocating
// once both sets have grown, and costs at most that much idle memory.
constexpr size_t kRebuildHeadroomDiv = 4;
static size_t rebuild_initial_cap(const SceneBag& b)
{
    if (const char* env = getenv("RT355_REBUILD_INITIAL_CAP")) {
        const long long k = atoll(env);
        if (k > 0) return (size_t)std::min<long long>(k, 1ll << 30);
    }
    return (size_t)std::max(b.nPrims, 1);
}

// What an update and a rebuild refuse alike, before anything is written: `prims` replaces the primitives [first, first + count), `blas`
// (may be NULL) the instances.  typeSuffix ends the message about a changed objType / matIdx.
static int check_change(const char* who, const SceneBag& b, const RtPrimitive* prims, int32_t first, int32_t count, const RtBVHInstance* blas, int32_t nBlas,
                        const char* typeSuffix)
{
    if (count < 0 || (count > 0 && !prims)) return fail(RT_E_INVALID, "%s: bad primitive count %d / NULL records", who, count);
    if (count > 0 && (first < 0 || (int64_t)first + count > (int64_t)b.nPrims))
        return fail(RT_E_INVALID, "%s: primitive range [%d, %lld) outside the %d uploaded", who, first, (long long)first + count, b.nPrims);
    for (int32_t i = 0; i < count; i++) {
        const size_t g = (size_t)first + (size_t)i;
        if (prims[i].objType != b.primType[g] || prims[i].matIdx != b.primMat[g])
            return fail(RT_E_INVALID, "%s: primitive %zu changes its objType / matIdx (%d / %d -> %d / %d)%s", who, g,
                        b.primType[g], b.primMat[g], prims[i].objType, prims[i].matIdx, typeSuffix);
    }
    if (blas) {
        if (nBlas != b.nBlas) return fail(RT_E_INVALID, "%s: %d instances given, %d uploaded", who, nBlas, b.nBlas);
        for (int32_t k = 0; k < nBlas; k++) {
            if (blas[k].bvhIdx != b.inst[(size_t)k].bvhIdx) return fail(RT_E_INVALID, "%s: instance %d changes its bvhIdx", who, k);
            if (refit::singular(blas[k].invT)) return fail(RT_E_INVALID, "%s: instance %d: the transform is singular", who, k);
        }
    }
    return RT_OK;
}
// k_tlas_build's two status words (what went wrong, the height of the new TLAS) as the error of the call that ran it
static int tlas_status_error(const char* who, const int32_t status[2])
{
    if (status[0] == 1) return fail(RT_E_INVALID, "%s: an instance transform is singular", who);
    if (status[0] != 0) return fail(RT_E_UNSUPPORTED, "%s: the TLAS clustering found no partner (boxes of area >= RT_REALLYFAR or NaN)", who);
    if (status[1] > RT_TLAS_STACK)
        return fail(RT_E_UNSUPPORTED, "%s: the rebuilt TLAS is %d levels deep, the traversal stack holds %d; the scene is unchanged", who, status[1], RT_TLAS_STACK);
    return RT_OK;
}

// A Grown array to at least `count` records, keeping the first `keep`: the one place that replaces (and frees) a buffer of a copy.
// `nomem` (a format of `count`) replaces the message of a failed allocation.
template <class T> static int rebuild_grow(SceneBag& b, SceneBag::Grown<T>& a, size_t count, size_t keep, const char* what, const char* nomem = nullptr)
{
    if (count <= a.cap && a.p) return RT_OK;
    count = std::max<size_t>(count, 1);
    void* q = nullptr;
    if (hipMalloc(&q, count * sizeof(T)) != hipSuccess)
        return nomem ? fail(RT_E_NOMEM, nomem, count) : fail(RT_E_NOMEM, "in-place scene change: %zu bytes of device memory for %s", count * sizeof(T), what);
    b.rallocs++;
    if (a.p) {
        hipError_t e = keep ? hipMemcpyAsync(q, a.p, keep * sizeof(T), hipMemcpyDeviceToDevice, b.stream) : hipSuccess;
        if (e == hipSuccess) e = hipStreamSynchronize(b.stream);
        if (e != hipSuccess) { (void)hipFree(q); return fail(RT_E_DEVICE, "in-place scene change: moving %s failed: %s", what, hipGetErrorString(e)); }
        (void)hipFree(a.p);
    }
    a.p = (T*)q; a.cap = count;
    return RT_OK;
}
// An array that scales with the primitives, the instances or the lights (a RebuildSet's, the update's staging): made to fit exactly, and
// once a resize outgrows it replaced by one of the need plus a kRebuildHeadroomDiv-th.  Nothing in it is kept.
template <class T> static int rebuild_fit(SceneBag& b, SceneBag::Grown<T>& a, size_t need, const char* what)
{
    need = std::max<size_t>(need, 1);
    if (a.p && need <= a.cap) return RT_OK;
    return rebuild_grow(b, a, a.p ? need + need / kRebuildHeadroomDiv : need, 0, what);
}

// ---- the BVH2 -> BVH4 collapse of a copy that keeps its BVH2 (kernels: collapse.hip, rules: collapse_common.h) --------------------------
// The collapse's scratch for trees of nodeNeed nodes in all; grows as the derivation's scratch does (rebuild_scratch).  b.c4 lacks the
// tables the collapse leaves behind (newId, quadNode and their capacity): collapse_work adds those of the arrays that are collapsed.
static collapsedev::Work collapse_work(const SceneBag& b, uint32_t* newId, uint32_t* quadNode, size_t quadCap)
{
    collapsedev::Work w = b.c4;
    w.newId = newId; w.quadNode = quadNode; w.quadCap = (uint32_t)std::min<size_t>(quadCap, 0x7fffffffu);
    return w;
}
static int collapse_scratch(SceneBag& b, size_t nodeNeed)
{
    const bool have = b.c4Cap != 0;
    size_t cap = nodeNeed <= b.c4Cap ? b.c4Cap : nodeNeed + (have ? nodeNeed / kRebuildHeadroomDiv : 0);
    cap = (cap + 1) & ~(size_t)1;
    const size_t front = cap / 2 + 1;
    if (4 * front > (size_t)0x7fffffff) return fail(RT_E_UNSUPPORTED, "the BVH4 collapse takes at most 2^30 nodes (%zu given)", nodeNeed);
    int rc = rebuild_grow(b, b.c4FrontA, front, 0, "collapse scratch");
    if (rc == RT_OK) rc = rebuild_grow(b, b.c4FrontB, front, 0, "collapse scratch");
    if (rc == RT_OK) rc = rebuild_grow(b, b.c4Flags, 4 * front, 0, "collapse scratch");
    if (rc == RT_OK) rc = rebuild_grow(b, b.c4Ranks, 4 * front, 0, "collapse scratch");
    if (rc == RT_OK) rc = rebuild_grow(b, b.c4Kids, 4 * front, 0, "collapse scratch");
    if (rc == RT_OK) rc = rebuild_grow(b, b.c4Ctr, collapsedev::kCtrWords, 0, "collapse scratch");
    if (rc != RT_OK) return rc;
    b.c4Cap = cap;
    const size_t frontCap = std::min(std::min(b.c4FrontA.cap, b.c4FrontB.cap), std::min(std::min(b.c4Flags.cap, b.c4Ranks.cap), b.c4Kids.cap) / 4);
    size_t scanBytes = 0;
    HIPCHK(collapsedev::scan_bytes((uint32_t)(4 * frontCap), b.stream, &scanBytes));
    rc = rebuild_grow(b, b.c4Scan, std::max<size_t>(scanBytes, 256), 0, "scan workspace");
    if (rc != RT_OK) return rc;
    b.c4 = collapsedev::Work{ b.c4FrontA.p, b.c4FrontB.p, (uint32_t)frontCap, b.c4Flags.p, b.c4Ranks.p, b.c4Kids.p, nullptr, nullptr, 0u, b.c4Ctr.p,
                              b.c4Scan.p, b.c4Scan.cap };
    return RT_OK;
}
// What a collapse left in its status words: a failed walk, a BLAS that needs more stack than there is.  `tail` ends the stack message.
static int collapse_status_error(const char* who, const uint32_t st[collapsedev::kStatusWords], const char* tail)
{
    using namespace collapsedev;
    if (st[kWalkWord - kStatus]) return fail(RT_E_DEVICE, "%s: the BVH4 level walk does not match the BVH2 (inconsistent device result)", who);
    if (rebuild::exceeds_stack(st[kNeed - kStatus]))   // validate_scene's rule for a BVH4
        return fail(RT_E_UNSUPPORTED, "%s: a collapsed BLAS: traversal needs %u stack entries, at most %d are supported%s", who, st[kNeed - kStatus], RT_BVH4_STACK, tail);
    return RT_OK;
}
static uint32_t collapse_largest_leaf(const uint32_t st[collapsedev::kStatusWords])
{
    return std::max(std::max(st[collapsedev::kLeaf - collapsedev::kStatus], st[collapsedev::kLeafAny - collapsedev::kStatus]), 1u);
}
// rt_upload_scene_bvh2 on a BVH4 context, after the wire arrays are on the device: the collapse into sc.bvh4, then the layout, the stack
// size and the layout-1 records (quads, root entries, triangle records) as rt_upload_scene derives them from the host's collapse
static int collapse_uploaded(SceneBag& b, SceneArrays& sc, int extendVariant, const HostScene& in, const std::vector<collapse::Blas>& blas4, int& layout,
                             int& stackEntries, std::vector<uint32_t>& roots)
{
    using namespace collapsedev;
    const char* who = "rt_upload_scene_bvh2";
    const int32_t nNodes = in.nNodes, nIdx = in.nIdx, nBlas = in.nBlas;
    if (!b.stream) HIPCHK(hipStreamCreateWithFlags(&b.stream, hipStreamNonBlocking));
    hipStream_t s = b.stream;
    size_t quadCap = 0;   // a live node per interior node and leaf root at most
    for (const collapse::Blas& k : blas4) quadCap += std::max(k.interiors, 1u);
    int rc = dalloc(b.allocs, &sc.bvh4, (size_t)nNodes);
    if (rc == RT_OK) rc = dalloc(b.allocs, &b.liveNewId, (size_t)nNodes);   // the copy's own: RT_REBUILD_REFIT reads them
    if (rc == RT_OK) rc = dalloc(b.allocs, &b.liveQuadNode, quadCap);
    if (rc == RT_OK) rc = collapse_scratch(b, (size_t)nNodes);
    if (rc != RT_OK) return rc;
    Work w = collapse_work(b, b.liveNewId, b.liveQuadNode, quadCap);
    HIPCHK(begin(s, w, sc.bvh2, (uint32_t)nNodes, sc.bvh4));
    for (const collapse::Blas& k : blas4) HIPCHK(collapse_blas(s, w, sc.bvh2, (uint32_t)nNodes, k.root, k.interiors, k.height, sc.bvh4));
    uint32_t st[kStatusWords] = { 0 };
    HIPCHK(hipMemcpyAsync(st, b.c4.ctr + kStatus, sizeof st, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    if ((rc = collapse_status_error(who, st, "")) != RT_OK) return rc;
    const uint32_t live = st[kLive - kStatus];
    b.nLive = live; b.c4Need = st[kNeed - kStatus];
    layout = rebuild::takes_layout1(extendVariant != 1, nIdx, collapse_largest_leaf(st)) ? 1 : 0;
    stackEntries = rebuild::stack_entries((int)std::max(st[kNeed - kStatus], 1u));
    b.nQuads = layout == 1 ? (int32_t)live : 0;
    b.keepsBvh2 = true;
    if (layout != 1) return RT_OK;
    rc = dalloc(b.allocs, &sc.quads, (size_t)std::max(live, 1u) * 8);
    if (rc == RT_OK) rc = dalloc(b.allocs, &sc.rootEntry, (size_t)nBlas);
    if (rc == RT_OK) rc = dalloc(b.allocs, &sc.triRecs, (size_t)nIdx * 3);
    if (rc != RT_OK) return rc;
    w.quadCap = std::min(w.quadCap, std::max(live, 1u));   // what sc.quads holds
    HIPCHK(finish(s, w, sc.bvh4, (uint32_t)nNodes, (uint32_t)nIdx, (const uint32_t*)sc.blas, (uint32_t)(sizeof(RtBVHInstance) / 4), (uint32_t)nBlas, sc.quads, sc.rootEntry));
    HIPCHK(refitdev::launch_records(s, sc.prims, sc.bvh2, sc.primIdx, (uint32_t)nIdx, sc.lights, (uint32_t)in.nLights, 0u, (uint32_t)in.nPrims, nullptr, 0u, nullptr,
                                    sc.triRecs, sc.shadeRecs, sc.lightRecs));
    HIPCHK(hipMemcpyAsync(roots.data(), sc.rootEntry, sizeof(uint32_t) * (size_t)nBlas, hipMemcpyDeviceToHost, s));   // (the instance records carry them)
    HIPCHK(hipStreamSynchronize(s));
    return RT_OK;
}

int scenedev::update_scene(SceneBag& b, const RtPrimitive* prims, int32_t first, int32_t count, const RtBVHInstance* blas, int32_t nBlas, RtUpdateStats* stats)
{
    const char* who = "rt_update_scene";
    // ---- refusals: before anything is written
    if (b.refitRefusal) return fail(RT_E_UNSUPPORTED, "rt_update_scene: %s", b.refitRefusal);
    if (const int rc = check_change(who, b, prims, first, count, blas, nBlas, ": topology must not change")) return rc;
    HIPCHK(hipSetDevice(b.device));
    // ---- staging buffers (the first update makes them; one after a resize that outgrew them replaces them)
    if (!b.stream) HIPCHK(hipStreamCreateWithFlags(&b.stream, hipStreamNonBlocking));   // (a rebuild may have made it already)
    for (hipEvent_t& e : b.ev) if (!e) HIPCHK(hipEventCreate(&e));
    {
        int rc = rebuild_fit(b, b.sPrims, (size_t)b.nPrims, "the staging primitives");
        if (rc == RT_OK) rc = rebuild_fit(b, b.sInst, (size_t)b.nBlas, "the staging instances");
        if (rc == RT_OK) rc = rebuild_fit(b, b.sTlas, (size_t)b.nTlas, "the staging TLAS");
        if (rc == RT_OK) rc = rebuild_fit(b, b.sTp, (size_t)b.nTlas * 4, "the staging TLAS records");
        if (rc == RT_OK) rc = rebuild_fit(b, b.sTpP, (size_t)b.nTlas * 4, "the staging TLAS records");
        if (rc == RT_OK) rc = rebuild_fit(b, b.sIr, (size_t)b.nBlas * 4, "the staging instance records");
        if (rc == RT_OK && !b.sStatus) { rc = dalloc(b.allocs, &b.sStatus, 2); if (rc == RT_OK) b.rallocs++; }
        if (rc != RT_OK) return rc;
    }
    if (!b.sNodes.p || (size_t)b.nNodes > b.sNodes.cap) {
        // the staging nodes: at first room for every tree the SAH and the linear builder can bind later; an SBVH rebuild may bind more
        // nodes than that, then the array grows as the rebuild's sets do (nothing in it outlives a call)
        const size_t n = (size_t)b.nNodes, cap = b.sNodes.p ? n + n / kRebuildHeadroomDiv : std::max(n, 2 * rebuild_initial_cap(b));
        if (const int rc = rebuild_grow(b, b.sNodes, cap, 0, "the staging nodes", "rt_update_scene: %zu staging nodes")) return rc;
    }
    const SceneArrays& sc = b.sc;
    hipStream_t s = b.stream;
    // ---- stage: the new primitives, the refit tree and the rebuilt TLAS in scratch
    HIPCHK(hipEventRecord(b.ev[0], s));
    HIPCHK(hipMemcpyAsync(b.sPrims.p, sc.prims, sizeof(RtPrimitive) * (size_t)b.nPrims, hipMemcpyDeviceToDevice, s));
    if (count) HIPCHK(hipMemcpyAsync(b.sPrims.p + first, prims, sizeof(RtPrimitive) * (size_t)count, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(b.sNodes.p, sc.bvh2, sizeof(RtBVHNode2) * (size_t)b.nNodes, hipMemcpyDeviceToDevice, s));
    if (blas) HIPCHK(hipMemcpyAsync(b.sInst.p, blas, sizeof(RtBVHInstance) * (size_t)b.nBlas, hipMemcpyHostToDevice, s));
    else HIPCHK(hipMemcpyAsync(b.sInst.p, sc.blas, sizeof(RtBVHInstance) * (size_t)b.nBlas, hipMemcpyDeviceToDevice, s));
    HIPCHK(refitdev::launch_refit(s, b.sNodes.p, (uint32_t)b.nNodes, b.sPrims.p, sc.primIdx, b.dLeaves, b.nLeaves, b.dParent, b.dTickets));
    HIPCHK(refitdev::launch_tlas(s, b.sNodes.p, b.sInst.p, b.nBlas, b.layout == 1 ? sc.rootEntry : nullptr, b.sTlas.p, b.sTp.p, b.sTpP.p, b.sIr.p, b.sStatus));
    int32_t status[2] = { 0, 0 };
    HIPCHK(hipEventRecord(b.ev[1], s));
    HIPCHK(hipMemcpyAsync(status, b.sStatus, sizeof status, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    if (const int rc = tlas_status_error(who, status)) return rc;
    // ---- commit: no kernel of a context holding this copy may read the arrays while they are rewritten
    if (const int rc = b.wait_holders()) return rc;
    HIPCHK(hipEventRecord(b.ev[2], s));
    if (count) HIPCHK(hipMemcpyAsync(sc.prims + first, b.sPrims.p + first, sizeof(RtPrimitive) * (size_t)count, hipMemcpyDeviceToDevice, s));
    HIPCHK(hipMemcpyAsync(sc.bvh2, b.sNodes.p, sizeof(RtBVHNode2) * (size_t)b.nNodes, hipMemcpyDeviceToDevice, s));
    HIPCHK(hipMemcpyAsync(sc.blas, b.sInst.p, sizeof(RtBVHInstance) * (size_t)b.nBlas, hipMemcpyDeviceToDevice, s));
    HIPCHK(hipMemcpyAsync(sc.tlas, b.sTlas.p, sizeof(RtTLASNode) * (size_t)b.nTlas, hipMemcpyDeviceToDevice, s));
    HIPCHK(hipMemcpyAsync(sc.tlasPairs, b.sTp.p, sizeof(RtFloat4) * 4 * (size_t)b.nTlas, hipMemcpyDeviceToDevice, s));
    HIPCHK(hipMemcpyAsync(sc.tlasPairsP, b.sTpP.p, sizeof(RtFloat4) * 4 * (size_t)b.nTlas, hipMemcpyDeviceToDevice, s));
    HIPCHK(hipMemcpyAsync(sc.instRecs, b.sIr.p, sizeof(RtFloat4) * 4 * (size_t)b.nBlas, hipMemcpyDeviceToDevice, s));
    HIPCHK(refitdev::launch_records(s, sc.prims, sc.bvh2, sc.primIdx, (uint32_t)b.nIdx, sc.lights, (uint32_t)b.nLights, (uint32_t)std::max(first, 0),
                                    (uint32_t)count, b.dPairNode, (uint32_t)b.nPairs, b.layout == 1 ? sc.pairs : nullptr,
                                    b.layout == 1 ? sc.triRecs : nullptr, sc.shadeRecs, sc.lightRecs));
    HIPCHK(hipEventRecord(b.ev[3], s));
    HIPCHK(hipStreamSynchronize(s));
    if (blas) b.inst.assign(blas, blas + nBlas);
    const bool reconfigure = status[1] != b.tlasDepth;
    if (reconfigure) { b.tlasDepth = status[1]; b.generation++; }
    if (stats) {
        float ms = 0, ms2 = 0;   // GPU time of both phases (not the wait for the holders in between)
        (void)hipEventElapsedTime(&ms, b.ev[0], b.ev[1]); (void)hipEventElapsedTime(&ms2, b.ev[2], b.ev[3]);
        ms += ms2;
        *stats = RtUpdateStats{};
        stats->gpu_ms = ms; stats->prims = count; stats->nodes = (int32_t)b.nReach; stats->tlas_nodes = b.nTlas; stats->tlas_depth = status[1];
        stats->reconfigured = reconfigure ? 1 : 0;
    }
    return RT_OK;
}

// ---- in-place rebuilds (rt_rebuild_scene; builders: sah.hip / lbvh.hip / sbvh.hip, derivation: rebuild.hip, rules: rebuild_common.h) ----
// Room in the set `t` (not live) for idxNeed index slots and nodeNeed nodes, keeping the keepIdx slots and keepNodes records emitted so
// far; nR: the BLAS the trees belong to.  An array that is too small goes to the need plus kRebuildHeadroomDiv-th of it; one that NOMEM
// stopped is taken up by a later call.
static int rebuild_reserve(SceneBag& b, SceneBag::RebuildSet& t, size_t nR, size_t idxNeed, size_t nodeNeed, size_t keepIdx, size_t keepNodes)
{
    const bool have = t.nodes.p != nullptr;   // (the first allocation is exact: the initial capacity)
    const size_t idxCap = idxNeed <= t.primIdx.cap ? t.primIdx.cap : idxNeed + (have ? idxNeed / kRebuildHeadroomDiv : 0);
    size_t nodeCap = nodeNeed <= t.nodes.cap ? t.nodes.cap : nodeNeed + (have ? nodeNeed / kRebuildHeadroomDiv : 0);
    nodeCap = (nodeCap + 1) & ~(size_t)1;
    int rc = rebuild_grow(b, t.primIdx, idxCap, keepIdx, "primIdx");
    if (rc == RT_OK) rc = rebuild_grow(b, t.nodes, nodeCap, keepNodes, "nodes");
    if (rc == RT_OK) rc = rebuild_grow(b, t.triRecs, idxCap * 3, 0, "triangle records");
    if (rc == RT_OK) rc = rebuild_grow(b, t.parent, nodeCap, 0, "parent links");
    if (rc == RT_OK) rc = rebuild_grow(b, t.tickets, nodeCap, 0, "tickets");
    if (rc == RT_OK) rc = rebuild_grow(b, t.pairs, std::max<size_t>(nodeCap / 2, 1) * 4, 0, "pair records");
    if (rc == RT_OK) rc = rebuild_grow(b, t.leaves, nodeCap / 2, 0, "leaves");
    if (rc == RT_OK) rc = rebuild_grow(b, t.pairNode, nodeCap / 2, 0, "pair nodes");
    if (b.accel == RT_ACCEL_BVH4) {   // (a copy that keeps its BVH2: the collapsed records, and a quad record per interior node and leaf root at most)
        if (rc == RT_OK) rc = rebuild_grow(b, t.bvh4, nodeCap, 0, "BVH4 nodes");
        if (rc == RT_OK) rc = rebuild_grow(b, t.quads, (nodeCap / 2 + nR) * 8, 0, "quad records");
        if (rc == RT_OK) rc = rebuild_grow(b, t.newId, nodeCap, 0, "live ids");
        if (rc == RT_OK) rc = rebuild_grow(b, t.quadNode, nodeCap / 2 + nR, 0, "live nodes");
    }
    return rc;
}
// The derivation's scratch for trees of nodeNeed nodes in all (flags / ranks / newId: a word per node, the frontiers: per interior node)
static int rebuild_scratch(SceneBag& b, size_t nodeNeed)
{
    const bool have = b.dwFlags.p != nullptr;
    size_t cap = nodeNeed <= b.dwFlags.cap ? b.dwFlags.cap : nodeNeed + (have ? nodeNeed / kRebuildHeadroomDiv : 0);
    cap = (cap + 1) & ~(size_t)1;
    int rc = rebuild_grow(b, b.dwFlags, cap, 0, "scratch");
    if (rc == RT_OK) rc = rebuild_grow(b, b.dwRanks, cap, 0, "scratch");
    if (rc == RT_OK) rc = rebuild_grow(b, b.dwNewId, cap, 0, "scratch");
    if (rc == RT_OK) rc = rebuild_grow(b, b.dwFrontA, cap / 2, 0, "scratch");
    if (rc == RT_OK) rc = rebuild_grow(b, b.dwFrontB, cap / 2, 0, "scratch");
    if (rc != RT_OK) return rc;
    size_t scanBytes = 0;
    HIPCHK(rebuilddev::scan_bytes((uint32_t)b.dwFlags.cap, b.stream, &scanBytes));
    rc = rebuild_grow(b, b.dwScan, std::max<size_t>(scanBytes, 256), 0, "scan workspace");
    if (rc != RT_OK) return rc;
    b.dw.flags = b.dwFlags.p; b.dw.ranks = b.dwRanks.p; b.dw.newId = b.dwNewId.p; b.dw.frontA = b.dwFrontA.p; b.dw.frontB = b.dwFrontB.p;
    b.dw.frontCap = (uint32_t)std::min(b.dwFrontA.cap, b.dwFrontB.cap);
    b.dw.scan = b.dwScan.p; b.dw.scanBytes = b.dwScan.cap;
    return RT_OK;
}
// What the trees of a call are built over: the bound scene's own shape (a rebuild) or the caller's (a resize)
struct Shape {
    int32_t nPrims, nBlas, nLights;                  // (a resize learns nLights on the device: reserve_lights follows)
    const std::vector<rebuild::BlasRange>* ranges;   // the primitive range of every distinct BLAS, in increasing order (root: not read)
    const std::vector<int32_t>* instBlas;            // instance -> its range
    int32_t nTlas() const { return 2 * nBlas; }      // TLAS::Build's node count
};
// The lights' arrays of the set `t` (not live): one record at least, as at upload
static int reserve_lights(SceneBag& b, SceneBag::RebuildSet& t, size_t nLights)
{
    const int rc = rebuild_fit(b, t.lights, nLights, "the light list");
    return rc != RT_OK ? rc : rebuild_fit(b, t.lightRecs, std::max<size_t>(nLights, 1) * 8, "light records");
}
static int rebuild_alloc(SceneBag& b, SceneBag::RebuildSet& t, const Shape& sh, bool resize)
{
    const size_t nP = (size_t)sh.nPrims, nB = (size_t)sh.nBlas, nT = (size_t)sh.nTlas();
    int rc = RT_OK;
    // every piece is made on its own: a call that ran out of memory half way is taken up where it stopped
    auto need = [&](auto** p, size_t count) { if (rc == RT_OK && !*p) { rc = dalloc(b.allocs, p, count); if (rc == RT_OK) b.rallocs++; } };
    if (!b.stream) HIPCHK(hipStreamCreateWithFlags(&b.stream, hipStreamNonBlocking));
    for (hipEvent_t& e : b.rev) if (!e) HIPCHK(hipEventCreate(&e));
    if (!b.spool) b.spool = sbvhdev::pool_create();
    const size_t cap0 = rebuild_initial_cap(b);
    // the scratch both sets share
    need(&b.rStatus, 2); need(&b.dw.ctr, rebuilddev::kCtrWords);
    if (rc == RT_OK && !b.dwScan.p) rc = rebuild_scratch(b, 2 * cap0);
    if (rc != RT_OK) return rc;
    // what scales with the shape
    rc = rebuild_fit(b, t.prims, nP, "primitives");
    if (rc == RT_OK) rc = rebuild_fit(b, t.shadeRecs, nP, "shade records");
    if (rc == RT_OK) rc = rebuild_fit(b, t.blas, nB, "instances");
    if (rc == RT_OK) rc = rebuild_fit(b, t.tlas, nT, "TLAS nodes");
    if (rc == RT_OK) rc = rebuild_fit(b, t.tp, nT * 4, "TLAS records");
    if (rc == RT_OK) rc = rebuild_fit(b, t.tpP, nT * 4, "TLAS records");
    if (rc == RT_OK) rc = rebuild_fit(b, t.ir, nB * 4, "instance records");
    if (rc == RT_OK) rc = rebuild_fit(b, t.rootEntry, nB, "root entries");
    // (a rebuild carries the bound light records, and the light list only once a resize has put it into a set; a resize sizes both
    // when its scan has counted the lights)
    if (rc == RT_OK && !resize) rc = rebuild_fit(b, t.lightRecs, std::max<size_t>((size_t)sh.nLights, 1) * 8, "light records");
    if (rc == RT_OK && !resize && b.lightsInSet) rc = rebuild_fit(b, t.lights, (size_t)sh.nLights, "the light list");
    // ... and with the trees (the first allocation: the initial capacity)
    if (rc == RT_OK && !t.nodes.p) rc = rebuild_reserve(b, t, sh.ranges->size(), std::max(cap0, t.primIdx.cap), std::max(2 * cap0, t.nodes.cap), 0, 0);
    return rc;
}

static double ms_between(std::chrono::steady_clock::time_point a, std::chrono::steady_clock::time_point b)
{
    return std::chrono::duration<double, std::milli>(b - a).count();
}

// The checks of the builder and its options that need no scene: an unknown builder, a refit where there is no tree, alpha
static int check_builder(const char* who, int32_t builder, const RtBuildOptions* opts, bool refitAllowed)
{
    if (builder != RT_REBUILD_SAH && builder != RT_REBUILD_LBVH && builder != RT_REBUILD_SBVH && builder != RT_REBUILD_REFIT)
        return fail(RT_E_INVALID, "%s: unknown builder %d", who, builder);
    if (builder == RT_REBUILD_REFIT && !refitAllowed) return fail(RT_E_INVALID, "%s: RT_REBUILD_REFIT: a resized scene has no tree to refit", who);
    const float alpha = builder == RT_REBUILD_SBVH && opts ? opts->alpha : 0.0f;
    if (!(alpha >= 0.0f && alpha <= 1.0f)) return fail(RT_E_INVALID, "%s: alpha must lie in [0, 1]", who);
    return RT_OK;
}
// The builders' own argument checks, BLAS by BLAS under plan[k], one RT_REBUILD_SAH / LBVH / SBVH / KEEP per range (node and index ids as
// the host appends BLAS after BLAS: a kept BLAS takes its block's - blocks NULL: a SAH tree's at most - and the ids behind an SBVH tree
// are known only as the trees are built: its ranges hold at most 2^30 primitives each, and alpha is checked by check_builder)
static int check_ranges(const char* who, const int32_t* plan, const RtBuildOptions* opts, int32_t nPrims, const std::vector<rebuild::BlasRange>& ranges,
                        const rebuild::BlasBlock* blocks, lbvh::Params& P)
{
    uint32_t nodeBase = 0, idxBase = 0;
    for (size_t k = 0; k < ranges.size(); k++) {
        const rebuild::BlasRange& r = ranges[k];
        const uint32_t cap = 2 * r.count - 1;
        if (plan[k] == RT_REBUILD_SAH || plan[k] == RT_REBUILD_LBVH) {
            const char* msg = plan[k] == RT_REBUILD_SAH ? sahdev::check_args(nPrims, (int32_t)r.first, (int32_t)r.count, nodeBase, idxBase)
                                                        : lbvhdev::check_args(opts, nPrims, (int32_t)r.first, (int32_t)r.count, nodeBase, idxBase, P);
            if (msg) return fail(RT_E_INVALID, "%s: %s", who, msg);
            nodeBase += cap; idxBase += r.count;
        } else if (plan[k] == RT_REBUILD_SBVH) {
            if (r.count == 0 || r.count > (1u << 30)) return fail(RT_E_INVALID, "%s: a BLAS of %u primitives", who, r.count);
        } else {
            nodeBase += blocks ? blocks[k].nodes : cap; idxBase += blocks ? blocks[k].idxSlots : r.count;
        }
    }
    return RT_OK;
}
// alpha, when a plan has an SBVH range (check_builder's rule)
static int check_plan_alpha(const char* who, const int32_t* plan, size_t n, const RtBuildOptions* opts)
{
    for (size_t k = 0; k < n; k++) if (plan[k] == RT_REBUILD_SBVH) return check_builder(who, RT_REBUILD_SBVH, opts, false);
    return RT_OK;
}

// The one body of rt_rebuild_scene and rt_resize_scene.  A rebuild (newPrims NULL) keeps the bound shape `sh` and takes the replacement
// records prims / first / count and blas as rt_update_scene does; a resize builds the caller's shape over newPrims (host or device memory,
// sh.nPrims records), blas (NULL: identity) carrying the transforms.  plan[k] says what becomes of range k: built with RT_REBUILD_SAH /
// LBVH / SBVH, or (RT_REBUILD_KEEP, a rebuild of a compact bound tree only) its bound tree moved to where the new scene numbers it; an
// empty plan is RT_REBUILD_REFIT of the whole scene.  The arguments have passed the checks that need no device.
static int rebuild_body(SceneBag& b, const char* who, const Shape& sh, const void* newPrims, const RtPrimitive* prims, int32_t first, int32_t count,
                        const RtBVHInstance* blas, const std::vector<int32_t>& plan, const RtBuildOptions* opts, const lbvh::Params& P, RtRebuildStats* stats)
{
    using clock = std::chrono::steady_clock;
    const auto t0 = clock::now();
    const bool resize = newPrims != nullptr;
    const bool refit = plan.empty();   // (refit: no builder runs, opts is ignored)
    const float alpha = opts ? opts->alpha : 0.0f;   // (read by SBVH ranges only; check_builder has seen it if there is one)
    const std::vector<rebuild::BlasRange>& ranges = *sh.ranges;
    const std::vector<int32_t>& instBlas = *sh.instBlas;
    const size_t nR = ranges.size();
    // what the ranges behind range k need that is known beforehand: a kept tree its block, a SAH or LBVH tree count slots and
    // 2 * count - 1 nodes at most (an SBVH tree is sized when it is built: size, then place)
    std::vector<size_t> restIdx(nR + 1, 0), restNodes(nR + 1, 0);
    bool anyKnown = false;
    for (size_t k = nR; k-- > 0 && !refit;) {
        const bool keep = plan[k] == RT_REBUILD_KEEP, known = keep || plan[k] != RT_REBUILD_SBVH;
        restIdx[k] = restIdx[k + 1] + (keep ? b.blasBlock[k].idxSlots : known ? ranges[k].count : 0u);
        restNodes[k] = restNodes[k + 1] + (keep ? b.blasBlock[k].nodes : known ? 2 * (size_t)ranges[k].count - 1 : 0u);
        anyKnown = anyKnown || known;
    }
    HIPCHK(hipSetDevice(b.device));
    SceneBag::RebuildSet& t = b.rset[b.rnext];
    if (const int rc = rebuild_alloc(b, t, sh, resize)) return rc;
    hipStream_t s = b.stream;
    if (refit) {   // room for the bound trees (nR spare nodes: see the SBVH builder below)
        if (const int rc = rebuild_reserve(b, t, nR, (size_t)b.nIdx, (size_t)b.nNodes + nR, 0, 0)) return rc;
    } else if (anyKnown) {
        // room for the kept trees and for every tree the SAH and the linear builder can make (a set or the scratch that started smaller,
        // or has only held SBVH trees so far); nR spare nodes: see the SBVH builder below.  With every range built by those two this is
        // nPrims slots and 2 * nPrims nodes for ranges that tile the primitives
        if (restIdx[0] > 0x7fffffffull || restNodes[0] + nR > 0x7fffffffull)
            return fail(RT_E_UNSUPPORTED, "%s: the new trees have 2^31 nodes or index slots, or more; the scene is unchanged", who);
        if (const int rc = rebuild_reserve(b, t, nR, restIdx[0], restNodes[0] + nR, 0, 0)) return rc;
        // the builders' workspace, over the ranges they build
        size_t need = 0;
        for (size_t k = 0; k < nR; k++) {
            if (plan[k] != RT_REBUILD_SAH && plan[k] != RT_REBUILD_LBVH) continue;
            size_t bytes = 0;
            const int rc = plan[k] == RT_REBUILD_SAH ? sahdev::work_bytes(who, ranges[k].count, s, &bytes) : lbvhdev::work_bytes(who, ranges[k].count, s, &bytes);
            if (rc != RT_OK) return rc;
            need = std::max(need, bytes);
        }
        if (need > b.rwork.cap)
            if (const int rc = rebuild_grow(b, b.rwork, need, 0, "the builders' workspace", "in-place scene change: %zu bytes of builder workspace")) return rc;
    }
    const SceneArrays& sc = b.sc;
    int32_t nLights = sh.nLights;
    const uint32_t* lights = sc.lights;
    // ---- stage: the new primitives into the set that is not live
    HIPCHK(hipEventRecord(b.rev[0], s));
    if (resize) {
        // one path for host and device input: copied first (the set is not live, so checking after the copy is safe), then checked
        // where it lies; the light list and the light records come from the same pass
        if (const int rc = rebuild_scratch(b, (size_t)sh.nPrims)) return rc;   // (flags and ranks: a word per primitive)
        if (const int rc = rebuild_fit(b, b.rPacked, (size_t)sh.nPrims, "the packed objType / matIdx pairs")) return rc;
        uint32_t* bad = (uint32_t*)b.rStatus;
        HIPCHK(hipMemcpyAsync(t.prims.p, newPrims, sizeof(RtPrimitive) * (size_t)sh.nPrims, hipMemcpyDefault, s));
        HIPCHK(rebuilddev::resize_check(s, b.dw, t.prims.p, (uint32_t)sh.nPrims, sc.mats, sc.nMats, b.rPacked.p, bad));
        uint32_t firstBad = resize::kNoBad, lastRank = 0, lastFlag = 0;
        HIPCHK(hipMemcpyAsync(&firstBad, bad, sizeof firstBad, hipMemcpyDeviceToHost, s));
        HIPCHK(hipMemcpyAsync(&lastRank, b.dw.ranks + (sh.nPrims - 1), sizeof lastRank, hipMemcpyDeviceToHost, s));
        HIPCHK(hipMemcpyAsync(&lastFlag, b.dw.flags + (sh.nPrims - 1), sizeof lastFlag, hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));
        if (firstBad != resize::kNoBad) {
            int2 pm{ 0, 0 };
            HIPCHK(hipMemcpy(&pm, b.rPacked.p + firstBad, sizeof pm, hipMemcpyDeviceToHost));
            return fail(RT_E_INVALID, "%s: primitive %u: objType %d / matIdx %d out of range (objType: one of RT_PRIM_*, matIdx: [0, %d)); the scene is unchanged", who,
                        firstBad, pm.x, pm.y, sc.nMats);
        }
        nLights = (int32_t)(lastRank + lastFlag);
        if (const int rc = reserve_lights(b, t, (size_t)nLights)) return rc;
        HIPCHK(rebuilddev::light_emit(s, b.dw, t.prims.p, (uint32_t)sh.nPrims, sc.mats, (uint32_t)nLights, t.lights.p, t.lightRecs.p));
        lights = t.lights.p;
    } else {
        HIPCHK(hipMemcpyAsync(t.prims.p, sc.prims, sizeof(RtPrimitive) * (size_t)b.nPrims, hipMemcpyDeviceToDevice, s));
        if (count) HIPCHK(hipMemcpyAsync(t.prims.p + first, prims, sizeof(RtPrimitive) * (size_t)count, hipMemcpyHostToDevice, s));
        HIPCHK(hipMemcpyAsync(t.lightRecs.p, sc.lightRecs, sizeof(RtFloat4) * 8 * std::max<size_t>((size_t)b.nLights, 1), hipMemcpyDeviceToDevice, s));   // (the emittance words stay)
        if (b.lightsInSet) {   // the light list lives in a set since a resize: it moves on with the arrays
            if (nLights) HIPCHK(hipMemcpyAsync(t.lights.p, sc.lights, sizeof(uint32_t) * (size_t)nLights, hipMemcpyDeviceToDevice, s));
            lights = t.lights.p;
        }
    }
    const auto t1 = clock::now();
    // ---- every BLAS anew, in the order of the ranges (a refit: the bound trees, their boxes anew)
    std::vector<uint32_t> rootOf(nR), interiors(nR), depth(nR), idxOf(nR), slotsOf(nR);
    uint32_t nNodes = 0, nIdx = 0, maxDepth = 0;
    int32_t nBuilt = 0;
    uint64_t spatialSplits = 0, primsClipped = 0;
    if (refit) {
        // the bound trees and their refit topology into the set, then the boxes anew: no BLAS is built, so node ids, leaf ranges,
        // primIdx and pair ids stay
        nNodes = (uint32_t)b.nNodes; nIdx = (uint32_t)b.nIdx;
        HIPCHK(hipMemcpyAsync(t.nodes.p, sc.bvh2, sizeof(RtBVHNode2) * (size_t)nNodes, hipMemcpyDeviceToDevice, s));
        HIPCHK(hipMemcpyAsync(t.primIdx.p, sc.primIdx, sizeof(uint32_t) * (size_t)nIdx, hipMemcpyDeviceToDevice, s));
        HIPCHK(hipMemcpyAsync(t.parent.p, b.dParent, sizeof(uint32_t) * (size_t)nNodes, hipMemcpyDeviceToDevice, s));
        if (b.nLeaves) HIPCHK(hipMemcpyAsync(t.leaves.p, b.dLeaves, sizeof(uint32_t) * (size_t)b.nLeaves, hipMemcpyDeviceToDevice, s));
        if (b.nPairs) HIPCHK(hipMemcpyAsync(t.pairNode.p, b.dPairNode, sizeof(uint32_t) * (size_t)b.nPairs, hipMemcpyDeviceToDevice, s));
        HIPCHK(refitdev::launch_refit(s, t.nodes.p, nNodes, t.prims.p, t.primIdx.p, t.leaves.p, b.nLeaves, t.parent.p, t.tickets.p));
        rootOf = b.blasRoot; interiors = b.blasInteriors; depth = b.blasHeight;
        for (size_t k = 0; k < nR; k++) maxDepth = std::max(maxDepth, depth[k]);
    }
    // Kept trees move as segments: adjacent kept BLAS whose node and index offsets agree are one (rebuilddev::relocate), and their
    // primIdx slots, whose values are global primitive ids of a range that did not move, one plain copy.  A segment is queued when the
    // next range does not extend it, so before anything else touches the set.
    struct Segment { uint32_t srcNode = 0, dstNode = 0, nNodes = 0, nodeDelta = 0, srcIdx = 0, dstIdx = 0, nIdx = 0, idxDelta = 0; } seg;
    auto flush = [&]() -> int {
        if (!seg.nNodes) return RT_OK;
        HIPCHK(rebuilddev::relocate(s, sc.bvh2 + seg.srcNode, t.nodes.p + seg.dstNode, seg.nNodes, seg.nodeDelta, seg.idxDelta));
        HIPCHK(hipMemcpyAsync(t.primIdx.p + seg.dstIdx, sc.primIdx + seg.srcIdx, sizeof(uint32_t) * (size_t)seg.nIdx, hipMemcpyDeviceToDevice, s));
        seg = Segment{};
        return RT_OK;
    };
    for (size_t k = 0; k < nR && !refit; k++) {
        const rebuild::BlasRange& r = ranges[k];
        Built built{};
        uint32_t slots = r.count;
        const bool sbvh = plan[k] == RT_REBUILD_SBVH;
        if (plan[k] == RT_REBUILD_KEEP) {   // (room: reserved above; the bound values stand for the builder's)
            const rebuild::BlasBlock& blk = b.blasBlock[k];
            const uint32_t nodeDelta = nNodes - b.blasRoot[k], idxDelta = nIdx - blk.idxLo;
            if (seg.nNodes && seg.nodeDelta == nodeDelta && seg.idxDelta == idxDelta && seg.srcNode + seg.nNodes == b.blasRoot[k] && seg.srcIdx + seg.nIdx == blk.idxLo) {
                seg.nNodes += blk.nodes; seg.nIdx += blk.idxSlots;
            } else {
                if (const int rc = flush()) return rc;
                seg = Segment{ b.blasRoot[k], nNodes, blk.nodes, nodeDelta, blk.idxLo, nIdx, blk.idxSlots, idxDelta };
            }
            rootOf[k] = nNodes; interiors[k] = b.blasInteriors[k]; depth[k] = b.blasHeight[k]; idxOf[k] = nIdx; slotsOf[k] = blk.idxSlots;
            maxDepth = std::max(maxDepth, depth[k]);
            nNodes += blk.nodes; nIdx += blk.idxSlots;
            continue;
        }
        if (const int rc = flush()) return rc;
        nBuilt++;
        if (sbvh) {
            // size, then place: the tree stays in the builder's own memory until the set has room for it (one tree at a time)
            struct TreeGuard { sbvhdev::Tree* p = nullptr; ~TreeGuard() { sbvhdev::destroy(p); } } tree;
            SbvhBuilt sb{};
            if (const int rc = sbvhdev::build(who, s, alpha, t.prims.p + r.first, r.count, r.first, nNodes, nIdx, nullptr, nullptr, b.spool, &tree.p, &sb)) return rc;
            if (sb.nIdx == 0 || (uint64_t)nNodes + sb.nodes + nR > 0x7fffffffull || (uint64_t)nIdx + sb.nIdx > 0x7fffffffull)
                return fail(RT_E_UNSUPPORTED, "%s: the new trees have 2^31 nodes or index slots, or more; the scene is unchanged", who);
            // (nR spare nodes: the leaf and pair arrays hold half the node capacity, and k trees have k leaves more than interior nodes)
            // (... and what the ranges behind this one are known to need)
            if ((uint64_t)nNodes + sb.nodes + restNodes[k + 1] + nR > 0x7fffffffull || (uint64_t)nIdx + sb.nIdx + restIdx[k + 1] > 0x7fffffffull)
                return fail(RT_E_UNSUPPORTED, "%s: the new trees have 2^31 nodes or index slots, or more; the scene is unchanged", who);
            if (const int rc = rebuild_reserve(b, t, nR, (size_t)nIdx + sb.nIdx + restIdx[k + 1], (size_t)nNodes + sb.nodes + restNodes[k + 1] + nR, nIdx, nNodes)) return rc;
            if (const int rc = sbvhdev::emit(who, s, tree.p, t.nodes.p + nNodes, t.primIdx.p + nIdx)) return rc;
            built.nodes = sb.nodes; built.depth = sb.depth; slots = sb.nIdx;
            spatialSplits += sb.spatialSplits; primsClipped += sb.primsClipped;
        } else {
            const int rc = plan[k] == RT_REBUILD_SAH
                ? sahdev::build(who, s, b.rwork.p, t.prims.p + r.first, r.count, r.first, nNodes, nIdx, t.nodes.p + nNodes, t.primIdx.p + nIdx, nullptr, nullptr, &built)
                : lbvhdev::build(who, s, b.rwork.p, P, t.prims.p + r.first, r.count, r.first, nNodes, nIdx, t.nodes.p + nNodes, t.primIdx.p + nIdx, nullptr, nullptr, &built);
            if (rc != RT_OK) return rc;
        }
        if (built.nodes == 0 || (built.nodes & 1u) == 0 || (!sbvh && built.nodes > 2 * r.count - 1))
            return fail(RT_E_DEVICE, "%s: inconsistent builder result (%u nodes for %u primitives)", who, built.nodes, r.count);
        if ((built.depth == 0) != (built.nodes == 1))
            return fail(RT_E_DEVICE, "%s: inconsistent builder result (height %u with %u nodes)", who, built.depth, built.nodes);
        if (rebuild::exceeds_stack(built.depth))   // validate_scene's rule
            return fail(RT_E_UNSUPPORTED, "%s: the new BLAS %zu needs %u stack entries, at most %d are supported; the scene is unchanged", who, k,
                        built.depth, RT_BVH4_STACK);
        rootOf[k] = nNodes; interiors[k] = (built.nodes - 1) / 2; depth[k] = built.depth; idxOf[k] = nIdx; slotsOf[k] = slots;
        maxDepth = std::max(maxDepth, built.depth);
        nNodes += built.nodes; nIdx += slots;
    }
    if (const int rc = flush()) return rc;
    if (!refit) if (const int rc = rebuild_scratch(b, (size_t)nNodes + nR)) return rc;
    const bool bvh4 = b.accel == RT_ACCEL_BVH4;
    if (bvh4) if (const int rc = collapse_scratch(b, (size_t)nNodes + nR)) return rc;
    const auto t2 = clock::now();
    // ---- the instances (host: at most 256 records), then everything upload derives
    std::vector<RtBVHInstance> inst;
    if (blas) inst.assign(blas, blas + sh.nBlas);
    else if (!resize) inst = b.inst;
    else {   // a resize without transforms: BuildBLAS's identity
        inst.assign((size_t)sh.nBlas, RtBVHInstance{});
        for (RtBVHInstance& r : inst) r.invT[0] = r.invT[5] = r.invT[10] = r.invT[15] = 1.0f;
    }
    for (int32_t i = 0; i < sh.nBlas; i++) inst[(size_t)i].bvhIdx = rootOf[(size_t)instBlas[(size_t)i]];
    HIPCHK(hipMemcpyAsync(t.blas.p, inst.data(), sizeof(RtBVHInstance) * (size_t)sh.nBlas, hipMemcpyHostToDevice, s));
    HIPCHK(hipEventRecord(b.rev[1], s));
    uint32_t nPairs = 0;
    const bool layout1 = b.layout == 1;
    if (refit) {   // the pair records (launch_records rewrites their boxes) and the root entries as they are bound
        nPairs = (uint32_t)b.nPairs;
        if (layout1 && !bvh4) {
            HIPCHK(hipMemcpyAsync(t.pairs.p, sc.pairs, sizeof(RtFloat4) * 4 * std::max<size_t>(nPairs, 1), hipMemcpyDeviceToDevice, s));
            HIPCHK(hipMemcpyAsync(t.rootEntry.p, sc.rootEntry, sizeof(uint32_t) * (size_t)b.nBlas, hipMemcpyDeviceToDevice, s));
        }
    } else {
        HIPCHK(rebuilddev::begin(s, b.dw, t.parent.p, nNodes));
        {   // pair ids: BLAS by BLAS in the order in which the instances first name them
            std::vector<uint8_t> done(nR, 0);
            for (int32_t i = 0; i < sh.nBlas; i++) {
                const size_t k = (size_t)instBlas[(size_t)i];
                if (done[k]) continue;
                done[k] = 1;
                HIPCHK(rebuilddev::number_blas(s, b.dw, t.nodes.p, nNodes, rootOf[k], interiors[k], depth[k], nPairs, (uint32_t)t.pairNode.cap, t.pairNode.p, t.parent.p));
                nPairs += interiors[k];
            }
        }
        HIPCHK(rebuilddev::finish(s, b.dw, t.nodes.p, nNodes, nPairs, nNodes - nPairs, t.blas.p, (uint32_t)sh.nBlas, t.pairNode.p, layout1 && !bvh4 ? t.pairs.p : nullptr,
                                  t.rootEntry.p, t.leaves.p));
    }
    const uint32_t nLeaves = refit ? b.nLeaves : nNodes - nPairs;
    uint32_t c4st[collapsedev::kStatusWords] = { 0 };
    int32_t refitPath = refit ? 1 : 0;
    if (bvh4) {   // the collapse into the set's bvh4, BLAS by BLAS in the same order; quad records and root entries (layout 1)
        const collapsedev::Work w = collapse_work(b, t.newId.p, t.quadNode.p, std::min(t.quadNode.cap, t.quads.cap / 8));
        HIPCHK(collapsedev::begin(s, w, t.nodes.p, nNodes, t.bvh4.p));
        if (refit) {
            // in place: the live records anew under the bound live ids (the set takes the bound tables over); if no slot of any of
            // them changed, they are the collapse of the refit trees and the level loop is skipped
            HIPCHK(hipMemcpyAsync(t.newId.p, b.liveNewId, sizeof(uint32_t) * (size_t)nNodes, hipMemcpyDeviceToDevice, s));
            HIPCHK(hipMemcpyAsync(t.quadNode.p, b.liveQuadNode, sizeof(uint32_t) * (size_t)b.nLive, hipMemcpyDeviceToDevice, s));
            HIPCHK(collapsedev::refit_records(s, w, t.nodes.p, nNodes, sc.bvh4, t.quadNode.p, b.nLive, t.bvh4.p));
            HIPCHK(hipMemcpyAsync(c4st, w.ctr + collapsedev::kStatus, sizeof c4st, hipMemcpyDeviceToHost, s));
            HIPCHK(hipStreamSynchronize(s));
            if (const int rc = collapse_status_error(who, c4st, "; the scene is unchanged")) return rc;
            const char* env = getenv("RT355_REFIT_RECOLLAPSE");
            refitPath = env && atoi(env) == 1 ? 3 : c4st[collapsedev::kChanged - collapsedev::kStatus] ? 2 : 1;
            if (refitPath != 1) HIPCHK(collapsedev::begin(s, w, t.nodes.p, nNodes, t.bvh4.p));   // the fallback: the rebuild's collapse
        }
        std::vector<uint8_t> done(nR, refitPath == 1 ? 1 : 0);
        for (int32_t i = 0; i < sh.nBlas; i++) {
            const size_t k = (size_t)instBlas[(size_t)i];
            if (done[k]) continue;
            done[k] = 1;
            HIPCHK(collapsedev::collapse_blas(s, w, t.nodes.p, nNodes, rootOf[k], interiors[k], depth[k], t.bvh4.p));
        }
        HIPCHK(collapsedev::finish(s, w, t.bvh4.p, nNodes, nIdx, (const uint32_t*)t.blas.p, (uint32_t)(sizeof(RtBVHInstance) / 4), (uint32_t)sh.nBlas,
                                   layout1 ? t.quads.p : nullptr, t.rootEntry.p));
    }
    const bool boxes = refit && layout1 && !bvh4;
    HIPCHK(refitdev::launch_records(s, t.prims.p, t.nodes.p, t.primIdx.p, nIdx, lights, (uint32_t)nLights, 0u, (uint32_t)sh.nPrims,
                                    boxes ? t.pairNode.p : nullptr, boxes ? nPairs : 0u, boxes ? t.pairs.p : nullptr, layout1 ? t.triRecs.p : nullptr,
                                    t.shadeRecs.p, t.lightRecs.p));
    HIPCHK(hipEventRecord(b.rev[2], s));
    HIPCHK(refitdev::launch_tlas(s, t.nodes.p, t.blas.p, sh.nBlas, layout1 ? t.rootEntry.p : nullptr, t.tlas.p, t.tp.p, t.tpP.p, t.ir.p, b.rStatus));
    HIPCHK(hipEventRecord(b.rev[3], s));
    int32_t status[2] = { 0, 0 };
    uint32_t walk[2] = { 0, 0 };
    HIPCHK(hipMemcpyAsync(status, b.rStatus, sizeof status, hipMemcpyDeviceToHost, s));
    if (!refit) HIPCHK(hipMemcpyAsync(walk, b.dw.ctr + rebuilddev::kStatus, sizeof walk, hipMemcpyDeviceToHost, s));
    const uint32_t changed = c4st[collapsedev::kChanged - collapsedev::kStatus];
    if (bvh4 && refitPath != 1) HIPCHK(hipMemcpyAsync(c4st, b.c4.ctr + collapsedev::kStatus, sizeof c4st, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    if (bvh4 && refitPath == 1) c4st[collapsedev::kNeed - collapsedev::kStatus] = b.c4Need;   // (a top-down figure: carried over with the live ids)
    if (walk[0]) return fail(RT_E_DEVICE, "%s: the breadth-first walk does not match the builder's tree (inconsistent device result)", who);
    if (bvh4) {
        if (const int rc = collapse_status_error(who, c4st, "; the scene is unchanged")) return rc;
        walk[1] = collapse_largest_leaf(c4st);   // the layout rule of a BVH4 looks at the collapsed records
    }
    if (const int rc = tlas_status_error(who, status)) return rc;
    const int stackNeed = bvh4 ? (int)c4st[collapsedev::kNeed - collapsedev::kStatus] : (int)maxDepth;
    // (a refit moves no leaf size: a BVH2 copy keeps its layout, a BVH4 copy's check cannot fail)
    if (!(refit && !bvh4) && rebuild::takes_layout1(b.variantLayout1, (int32_t)nIdx, std::max(walk[1], 1u)) != layout1)
        return fail(RT_E_UNSUPPORTED, "%s: the new trees would change the scene's derived layout (largest leaf %u primitives, %u index slots; "
                    "layout %d is bound): upload the rebuilt scene instead; the scene is unchanged", who, walk[1], nIdx, b.layout);
    std::vector<int2> packed;   // a resize: the host's shadow of objType / matIdx, the only per-primitive data that comes back
    if (resize) {
        packed.resize((size_t)sh.nPrims);
        HIPCHK(hipMemcpy(packed.data(), b.rPacked.p, sizeof(int2) * packed.size(), hipMemcpyDeviceToHost));
    }
    const auto t3 = clock::now();
    // ---- commit: swap the arrays once no kernel of a holder reads the old ones
    if (const int rc = b.wait_holders()) return rc;
    SceneArrays n = b.sc;
    n.prims = t.prims.p; n.bvh2 = t.nodes.p; n.primIdx = t.primIdx.p; n.blas = t.blas.p; n.tlas = t.tlas.p;
    n.tlasPairs = t.tp.p; n.tlasPairsP = t.tpP.p; n.instRecs = t.ir.p;
    n.shadeRecs = t.shadeRecs.p; n.lightRecs = t.lightRecs.p;
    if (resize || b.lightsInSet) n.lights = t.lights.p;
    if (layout1 && !bvh4 && nPairs == 0) HIPCHK(hipMemsetAsync(t.pairs.p, 0, sizeof(RtFloat4) * 4, s));   // no interior node: one zero record, as at upload
    if (layout1 && !bvh4) n.pairs = t.pairs.p;
    if (layout1) { n.triRecs = t.triRecs.p; n.rootEntry = t.rootEntry.p; }
    if (bvh4) { n.bvh4 = t.bvh4.p; if (layout1) n.quads = t.quads.p; }
    if (resize) {   // the new shape: the counts, the TLAS root (a leaf iff there is one instance: TLAS::Build copies it to node 0)
        n.nPrims = sh.nPrims; n.nLights = nLights; n.nBlas = sh.nBlas;
        const bool leafRoot = sh.nBlas == 1;
        n.tlasRoot = leafRoot ? refit::kLeafBit : 0u;
        n.tlasRootP = leafRoot ? refit::kTagInst : refit::kTagTlas;
        b.singleBlas = leafRoot; b.lightsInSet = true;
        b.nPrims = sh.nPrims; b.nLights = nLights; b.nBlas = sh.nBlas; b.nTlas = sh.nTlas();
        b.primType.resize(packed.size()); b.primMat.resize(packed.size());
        for (size_t i = 0; i < packed.size(); i++) { b.primType[i] = packed[i].x; b.primMat[i] = packed[i].y; }
        std::vector<rebuild::BlasRange> bound = ranges;
        for (size_t k = 0; k < nR; k++) bound[k].root = rootOf[k];
        const std::vector<int32_t> map = instBlas;   // (sh may alias the bag's own)
        b.ranges.swap(bound); b.instBlas = map;
    }
    b.sc = n;
    b.dParent = t.parent.p; b.dLeaves = t.leaves.p; b.dTickets = t.tickets.p; b.dPairNode = t.pairNode.p;
    b.nNodes = (int32_t)nNodes; b.nIdx = (int32_t)nIdx; b.nPairs = layout1 && !bvh4 ? (int32_t)nPairs : 0; b.nLeaves = nLeaves;
    if (!refit) b.nReach = nNodes;
    b.nQuads = layout1 && bvh4 ? (int32_t)c4st[collapsedev::kLive - collapsedev::kStatus] : 0;
    if (!refit) {   // (a refit moves no tree: the blocks stay)
        b.blasBlock.resize(nR);
        for (size_t k = 0; k < nR; k++) b.blasBlock[k] = rebuild::BlasBlock{ 2 * interiors[k] + 1, idxOf[k], slotsOf[k], 1 };
    }
    b.blasRoot = rootOf; b.blasInteriors = interiors; b.blasHeight = depth;
    if (bvh4) {   // the live collapse's tables follow the sets
        b.liveNewId = t.newId.p; b.liveQuadNode = t.quadNode.p;
        b.nLive = c4st[collapsedev::kLive - collapsedev::kStatus]; b.c4Need = c4st[collapsedev::kNeed - collapsedev::kStatus];
    }
    if (refit) b.refitInfo = RtRefitInfo{ refitPath, bvh4 ? (int32_t)b.nLive : 0, (int32_t)changed, stackNeed };
    b.inst = inst;
    const bool reconfigure = status[1] != b.tlasDepth || rebuild::stack_entries(std::max(stackNeed, 1)) != b.stackEntries;
    b.tlasDepth = status[1];
    b.stackEntries = rebuild::stack_entries(std::max(stackNeed, 1));   // (a BVH4: the collapsed trees' need, as validate_scene replays it)
    b.nInterior = layout1 && !bvh4 ? (int)nPairs : 0;
    b.generation++;   // every holder takes the new arrays (and re-derives its traversal kernels) before its next launch
    b.rnext ^= 1;
    const auto t4 = clock::now();
    if (stats) {
        float ms = 0, derive = 0, tlas = 0;
        (void)hipEventElapsedTime(&ms, b.rev[0], b.rev[3]); (void)hipEventElapsedTime(&derive, b.rev[1], b.rev[2]); (void)hipEventElapsedTime(&tlas, b.rev[2], b.rev[3]);
        *stats = RtRebuildStats{};
        stats->gpu_ms = ms; stats->wall_ms = ms_between(t0, t4);
        stats->stage_ms = ms_between(t0, t1); stats->build_ms = ms_between(t1, t2); stats->derive_ms = derive; stats->tlas_ms = tlas;
        if (refit) { float fit = 0; (void)hipEventElapsedTime(&fit, b.rev[0], b.rev[1]); stats->build_ms = fit; }   // (GPU: the staging copies and the refit)
        stats->commit_ms = ms_between(t3, t4);
        stats->prims = resize ? sh.nPrims : count; stats->blas_built = nBuilt; stats->nodes = (int32_t)nNodes; stats->n_idx = (int32_t)nIdx;
        stats->max_depth = (int32_t)maxDepth; stats->tlas_nodes = b.nTlas; stats->tlas_depth = status[1]; stats->reconfigured = reconfigure ? 1 : 0;
        stats->spatial_splits = (int32_t)std::min<uint64_t>(spatialSplits, 0x7fffffffu); stats->prims_clipped = (int32_t)std::min<uint64_t>(primsClipped, 0x7fffffffu);
    }
    return RT_OK;
}
int scenedev::rebuild_scene(SceneBag& b, const RtPrimitive* prims, int32_t first, int32_t count, const RtBVHInstance* blas, int32_t nBlas,
                            int32_t builder, const RtBuildOptions* opts, RtRebuildStats* stats)
{
    const char* who = "rt_rebuild_scene";
    // ---- refusals that need no device work
    if (b.refitRefusal) return fail(RT_E_UNSUPPORTED, "rt_rebuild_scene: %s", b.refitRefusal);
    if (b.rebuildRefusal) return fail(RT_E_UNSUPPORTED, "rt_rebuild_scene: %s", b.rebuildRefusal);
    if (const int rc = check_builder(who, builder, opts, true)) return rc;
    if (const int rc = check_change(who, b, prims, first, count, blas, nBlas, "")) return rc;
    lbvh::Params P{};
    const std::vector<int32_t> plan(builder == RT_REBUILD_REFIT ? 0 : b.ranges.size(), builder);   // every range: `builder`
    if (!plan.empty()) if (const int rc = check_ranges(who, plan.data(), opts, b.nPrims, b.ranges, nullptr, P)) return rc;
    const Shape sh{ b.nPrims, b.nBlas, b.nLights, &b.ranges, &b.instBlas };
    return rebuild_body(b, who, sh, nullptr, prims, first, count, blas, plan, opts, P, stats);
}
// The checks of a plan that need no device: the plan itself (rebuild::check_plan), alpha and the builders' own argument checks
static int plan_check_args(const char* who, int32_t nPrims, const std::vector<rebuild::BlasRange>& ranges, const rebuild::BlasBlock* blocks, const int32_t* plan,
                           int32_t nRanges, int32_t first, int32_t count, const RtBuildOptions* opts, lbvh::Params& P)
{
    std::string msg;
    if (const int rc = rebuild::check_plan(plan, nRanges, ranges, blocks, first, count, msg)) return fail(rc, "%s: %s", who, msg.c_str());
    if (const int rc = check_plan_alpha(who, plan, ranges.size(), opts)) return rc;
    return check_ranges(who, plan, opts, nPrims, ranges, blocks, P);
}
extern "C" int rt_rebuild_ranges_check(int32_t nPrims, const int32_t* rangeFirst, const int32_t* rangeCount, const int32_t* compact, int32_t nBound,
                                       const int32_t* plan, int32_t nRanges, int32_t first, int32_t count, const RtBuildOptions* opts)
{
    const char* who = "rt_rebuild_ranges";
    if (nPrims <= 0 || nBound <= 0 || !rangeFirst || !rangeCount) return fail(RT_E_INVALID, "%s: the ranges of at least one BLAS are needed (nPrims %d, %d ranges)", who, nPrims, nBound);
    std::vector<rebuild::BlasRange> ranges((size_t)nBound);
    std::vector<rebuild::BlasBlock> blocks((size_t)nBound);
    int64_t next = 0;
    for (int32_t k = 0; k < nBound; k++) {
        if (rangeCount[k] < 1 || rangeFirst[k] < next || (int64_t)rangeFirst[k] + rangeCount[k] > (int64_t)nPrims)
            return fail(RT_E_INVALID, "%s: range %d (first %d, count %d): ranges hold at least one primitive, lie in [0, %d) and come in increasing order without overlap",
                        who, k, rangeFirst[k], rangeCount[k], nPrims);
        next = (int64_t)rangeFirst[k] + rangeCount[k];
        ranges[(size_t)k] = rebuild::BlasRange{ 0u, (uint32_t)rangeFirst[k], (uint32_t)rangeCount[k] };
        blocks[(size_t)k] = rebuild::BlasBlock{ 2 * (uint32_t)rangeCount[k] - 1, 0u, (uint32_t)rangeCount[k], (uint8_t)(!compact || compact[k] ? 1 : 0) };
    }
    if (count < 0 || (count > 0 && (first < 0 || (int64_t)first + count > (int64_t)nPrims)))
        return fail(RT_E_INVALID, "%s: primitive range [%d, %lld) outside the %d uploaded", who, first, (long long)first + count, nPrims);
    lbvh::Params P{};
    return plan_check_args(who, nPrims, ranges, blocks.data(), plan, nRanges, first, count, opts, P);
}
int scenedev::rebuild_ranges(SceneBag& b, const RtPrimitive* prims, int32_t first, int32_t count, const RtBVHInstance* blas, int32_t nBlas,
                             const int32_t* plan, int32_t nRanges, const RtBuildOptions* opts, RtRebuildStats* stats)
{
    const char* who = "rt_rebuild_ranges";
    // ---- refusals that need no device work
    if (b.refitRefusal) return fail(RT_E_UNSUPPORTED, "%s: %s", who, b.refitRefusal);
    if (b.rebuildRefusal) return fail(RT_E_UNSUPPORTED, "%s: %s", who, b.rebuildRefusal);
    if (const int rc = check_change(who, b, prims, first, count, blas, nBlas, "")) return rc;
    lbvh::Params P{};
    if (const int rc = plan_check_args(who, b.nPrims, b.ranges, b.blasBlock.data(), plan, nRanges, first, count, opts, P)) return rc;
    const Shape sh{ b.nPrims, b.nBlas, b.nLights, &b.ranges, &b.instBlas };
    return rebuild_body(b, who, sh, nullptr, prims, first, count, blas, std::vector<int32_t>(plan, plan + nRanges), opts, P, stats);
}
int scenedev::blas_blocks(const SceneBag& b, int32_t* n, int32_t* primFirst, int32_t* primCount, int32_t* nodes, int32_t* idxSlots, int32_t* compact, int32_t cap)
{
    if (b.rebuildRefusal) return fail(RT_E_UNSUPPORTED, "rt_scene_blas_blocks: %s", b.rebuildRefusal);
    if (b.blasBlock.size() != b.ranges.size()) return fail(RT_E_UNSUPPORTED, "rt_scene_blas_blocks: %s", b.refitRefusal ? b.refitRefusal : "the scene's BLAS ranges are not known");
    if (n) *n = (int32_t)b.ranges.size();
    for (size_t k = 0; k < b.ranges.size() && (int64_t)k < (int64_t)cap; k++) {
        if (primFirst) primFirst[k] = (int32_t)b.ranges[k].first;
        if (primCount) primCount[k] = (int32_t)b.ranges[k].count;
        if (nodes) nodes[k] = (int32_t)b.blasBlock[k].nodes;
        if (idxSlots) idxSlots[k] = (int32_t)b.blasBlock[k].idxSlots;
        if (compact) compact[k] = b.blasBlock[k].compact;
    }
    return RT_OK;
}

// The ranges of a caller's shape as the builders take them (root: assigned by the build)
static std::vector<rebuild::BlasRange> shape_ranges(const RtSceneShape& shape)
{
    std::vector<rebuild::BlasRange> r((size_t)shape.nRanges);
    uint32_t first = 0;
    for (int32_t k = 0; k < shape.nRanges; k++) { r[(size_t)k] = rebuild::BlasRange{ 0u, first, (uint32_t)shape.rangeCount[k] }; first += (uint32_t)shape.rangeCount[k]; }
    return r;
}
// What rt_resize_scene checks without a device or a scene (rt_resize_check): the shape, the builder, its options
// (ranges receives the shape's ranges)
static int resize_check_args(const char* who, int32_t nPrims, const RtSceneShape* shape, int32_t builder, const RtBuildOptions* opts, lbvh::Params& P,
                             std::vector<rebuild::BlasRange>& ranges)
{
    if (!shape) return fail(RT_E_INVALID, "%s: null shape", who);
    std::string msg;
    if (resize::check_shape(nPrims, shape->nRanges, shape->rangeCount, shape->nBlas, shape->instRange, shape->blas, msg)) return fail(RT_E_INVALID, "%s: %s", who, msg.c_str());
    if (const int rc = check_builder(who, builder, opts, false)) return rc;
    ranges = shape_ranges(*shape);
    const std::vector<int32_t> plan(ranges.size(), builder);
    return check_ranges(who, plan.data(), opts, nPrims, ranges, nullptr, P);
}
extern "C" int rt_resize_check(int32_t nPrims, const RtSceneShape* shape, int32_t builder, const RtBuildOptions* opts)
{
    lbvh::Params P{};
    std::vector<rebuild::BlasRange> ranges;
    return resize_check_args("rt_resize_scene", nPrims, shape, builder, opts, P, ranges);
}
int scenedev::resize_scene(SceneBag& b, const void* prims, int32_t nPrims, const RtSceneShape* shape, int32_t builder, const RtBuildOptions* opts,
                           RtRebuildStats* stats)
{
    const char* who = "rt_resize_scene";
    // ---- refusals that need no device work
    lbvh::Params P{};
    std::vector<rebuild::BlasRange> ranges;
    if (const int rc = resize_check_args(who, nPrims, shape, builder, opts, P, ranges)) return rc;
    if (b.refitRefusal) return fail(RT_E_UNSUPPORTED, "rt_resize_scene: %s", b.refitRefusal);
    if (b.rebuildRefusal) return fail(RT_E_UNSUPPORTED, "rt_resize_scene: %s", b.rebuildRefusal);
    {   // the bound ranges (in increasing order) must tile the bound primitives
        uint32_t next = 0;
        for (const rebuild::BlasRange& r : b.ranges) {
            if (r.first != next) return fail(RT_E_UNSUPPORTED, "rt_resize_scene: the bound scene's BLAS ranges leave a gap: primitives [%u, %u) belong to no BLAS", next, r.first);
            next = r.first + r.count;
        }
        if (next != (uint32_t)b.nPrims)
            return fail(RT_E_UNSUPPORTED, "rt_resize_scene: the bound scene's BLAS ranges leave a gap: primitives [%u, %d) belong to no BLAS", next, b.nPrims);
    }
    const std::vector<int32_t> instBlas(shape->instRange, shape->instRange + shape->nBlas);
    const Shape sh{ nPrims, shape->nBlas, 0, &ranges, &instBlas };
    return rebuild_body(b, who, sh, prims, nullptr, 0, 0, shape->blas, std::vector<int32_t>(ranges.size(), builder), opts, P, stats);   // (never RT_REBUILD_KEEP)
}

// ---- in-place material updates (rt_update_materials; kernels: rebuild.hip, rules: resize_common.h) -------------------------------------
// validate_scene's checks of a material table against an atlas of nTexels texels, with its message; texPad receives the atlas pad
static int materials_check(const char* who, const RtMaterial* mats, int32_t nMats, int64_t nTexels, int64_t* texPad)
{
    if (!mats || nMats <= 0) return fail(RT_E_INVALID, "%s: a material table holds at least one material (nMats %d)", who, nMats);
    if (nTexels < 0) return fail(RT_E_INVALID, "%s: negative atlas length %lld", who, (long long)nTexels);
    if (const int32_t m = resize::check_materials(mats, nMats, nTexels, texPad); m >= 0)
        return fail(RT_E_INVALID, "material %d: texture window exceeds the atlas", m);
    return RT_OK;
}
extern "C" int rt_materials_check(const RtMaterial* mats, int32_t nMats, int32_t nTexels)
{
    return materials_check("rt_materials_check", mats, nMats, nTexels, nullptr);
}
int scenedev::update_materials(SceneBag& b, const RtMaterialUpdate& u, RtMaterialStats* stats)
{
    using clock = std::chrono::steady_clock;
    const char* who = "rt_update_materials";
    const auto t0 = clock::now();
    const SceneArrays& sc = b.sc;
    // ---- refusals that need no device work: counts and ranges, then the table that will be bound against the atlas that will be bound
    const bool newTable = u.mats != nullptr;
    if (newTable && u.nMats <= 0) return fail(RT_E_INVALID, "%s: a material table holds at least one material (nMats %d)", who, u.nMats);
    if (u.nTexels < -1) return fail(RT_E_INVALID, "%s: nTexels %d (the new atlas length, or -1 to keep the bound one)", who, u.nTexels);
    if (u.texFirst < 0 || u.texCount < 0) return fail(RT_E_INVALID, "%s: negative texel range (first %d, count %d)", who, u.texFirst, u.texCount);
    if (u.primFirst < 0 || u.primCount < 0) return fail(RT_E_INVALID, "%s: negative primitive range (first %d, count %d)", who, u.primFirst, u.primCount);
    if (u.texCount > 0 && !u.texels) return fail(RT_E_INVALID, "%s: texCount %d but texels == NULL", who, u.texCount);
    if (u.primCount > 0 && !u.primMat) return fail(RT_E_INVALID, "%s: primCount %d but primMat == NULL", who, u.primCount);
    const int32_t oldTex = sc.nTex, nTex = u.nTexels < 0 ? sc.nTex : u.nTexels;
    if (u.texels && (int64_t)u.texFirst + u.texCount > (int64_t)nTex)
        return fail(RT_E_INVALID, "%s: texel range [%d, %lld) outside the new atlas of %d texels", who, u.texFirst, (long long)u.texFirst + u.texCount, nTex);
    if (u.primMat && (int64_t)u.primFirst + u.primCount > (int64_t)b.nPrims)
        return fail(RT_E_INVALID, "%s: primitive range [%d, %lld) outside the %d bound", who, u.primFirst, (long long)u.primFirst + u.primCount, b.nPrims);
    const bool writeTex = u.texels && u.texCount > 0, assign = u.primMat && u.primCount > 0;
    const int32_t nMats = newTable ? u.nMats : sc.nMats;
    int64_t texPad = b.texPad;
    if (newTable || nTex != oldTex)   // (mats NULL: the bound table, from its host shadow, against a new atlas length)
        if (const int rc = materials_check(who, newTable ? u.mats : b.hMats.data(), nMats, nTex, &texPad)) return rc;
    const bool lightsChange = newTable || assign, padChange = nTex != oldTex || texPad != b.texPad;
    if (stats) { *stats = RtMaterialStats{}; stats->lights = b.nLights; }
    if (!lightsChange && !writeTex && !padChange) return RT_OK;   // nothing to do: nothing is touched
    HIPCHK(hipSetDevice(b.device));
    if (!b.stream) HIPCHK(hipStreamCreateWithFlags(&b.stream, hipStreamNonBlocking));
    for (hipEvent_t& e : b.rev) if (!e) HIPCHK(hipEventCreate(&e));
    hipStream_t s = b.stream;
    // ---- device memory: everything is made before anything is written (a call that ran out of memory is taken up where it stopped)
    SceneBag::Grown<RtMaterial>& M = b.mmats[b.mmatsNext];
    SceneBag::LightSet& L = b.mlights[b.mlightsNext];
    SceneBag::Grown<RtFloat4>& T = b.mtex[b.mtexNext];
    const size_t texNeed = (size_t)nTex + (size_t)texPad;
    const bool moveTex = texNeed > b.texCap;
    if (lightsChange) {
        if (!b.rStatus) { if (const int rc = dalloc(b.allocs, &b.rStatus, 2)) return rc; b.rallocs++; }
        if (const int rc = rebuild_scratch(b, (size_t)b.nPrims)) return rc;   // (flags and ranks: a word per primitive)
        if (newTable) if (const int rc = rebuild_fit(b, M, (size_t)nMats, "the material table")) return rc;
        if (assign) if (const int rc = rebuild_fit(b, b.mAssign, (size_t)u.primCount, "the new matIdx values")) return rc;
    }
    if (moveTex) if (const int rc = rebuild_fit(b, T, texNeed, "the texture atlas")) return rc;
    // ---- stage, in memory no holder reads: the table, the new assignment (one path for host and device input), the light list and the
    // complete light records under both; an atlas that has to move, whole
    HIPCHK(hipEventRecord(b.rev[0], s));
    int32_t nLights = b.nLights;
    const int32_t* dAssign = nullptr;
    if (lightsChange) {
        const RtMaterial* dMats = sc.mats;
        if (newTable) { HIPCHK(hipMemcpyAsync(M.p, u.mats, sizeof(RtMaterial) * (size_t)nMats, hipMemcpyHostToDevice, s)); dMats = M.p; }
        if (assign) { HIPCHK(hipMemcpyAsync(b.mAssign.p, u.primMat, sizeof(int32_t) * (size_t)u.primCount, hipMemcpyDefault, s)); dAssign = b.mAssign.p; }
        uint32_t* bad = (uint32_t*)b.rStatus;
        const uint32_t first = (uint32_t)u.primFirst, count = assign ? (uint32_t)u.primCount : 0u;
        HIPCHK(rebuilddev::mat_flags(s, b.dw, sc.prims, (uint32_t)b.nPrims, dAssign, first, count, dMats, nMats, bad));
        uint32_t firstBad = resize::kNoBad, lastRank = 0, lastFlag = 0;
        HIPCHK(hipMemcpyAsync(&firstBad, bad, sizeof firstBad, hipMemcpyDeviceToHost, s));
        HIPCHK(hipMemcpyAsync(&lastRank, b.dw.ranks + (b.nPrims - 1), sizeof lastRank, hipMemcpyDeviceToHost, s));
        HIPCHK(hipMemcpyAsync(&lastFlag, b.dw.flags + (b.nPrims - 1), sizeof lastFlag, hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));
        if (firstBad != resize::kNoBad) {   // a new value out of range, or a bound primitive the new, shorter table no longer serves
            int32_t mat = 0;
            const bool inRange = dAssign && firstBad - first < count;
            HIPCHK(hipMemcpy(&mat, inRange ? (const void*)(dAssign + (firstBad - first)) : (const void*)&sc.prims[firstBad].matIdx, sizeof mat, hipMemcpyDeviceToHost));
            return fail(RT_E_INVALID, "%s: primitive %u: matIdx %d outside the new table (nMats %d); the scene is unchanged", who, firstBad, mat, nMats);
        }
        nLights = (int32_t)(lastRank + lastFlag);
        int rc = rebuild_fit(b, L.lights, (size_t)nLights, "the light list");
        if (rc == RT_OK) rc = rebuild_fit(b, L.lightRecs, std::max<size_t>((size_t)nLights, 1) * 8, "light records");
        if (rc != RT_OK) return rc;
        HIPCHK(rebuilddev::mat_emit(s, b.dw, sc.prims, (uint32_t)b.nPrims, dAssign, first, count, dMats, (uint32_t)nLights, L.lights.p, L.lightRecs.p));
    }
    if (moveTex) {   // the kept part device to device, the rest and the pad zero, then the range
        const size_t keep = (size_t)std::min(oldTex, nTex);
        if (keep) HIPCHK(hipMemcpyAsync(T.p, sc.tex, sizeof(RtFloat4) * keep, hipMemcpyDeviceToDevice, s));
        HIPCHK(hipMemsetAsync(T.p + keep, 0, sizeof(RtFloat4) * (texNeed - keep), s));
        if (writeTex) HIPCHK(hipMemcpyAsync(T.p + u.texFirst, u.texels, sizeof(RtFloat4) * (size_t)u.texCount, hipMemcpyDefault, s));
    }
    HIPCHK(hipEventRecord(b.rev[1], s));
    HIPCHK(hipStreamSynchronize(s));
    // ---- commit: no kernel of a holder may read the arrays while they are patched; then the swap
    if (const int rc = b.wait_holders()) return rc;
    HIPCHK(hipEventRecord(b.rev[2], s));
    if (assign) HIPCHK(rebuilddev::mat_assign(s, sc.prims, dAssign, (uint32_t)u.primFirst, (uint32_t)u.primCount, sc.shadeRecs));
    if (!moveTex) {   // the live atlas has the room: what an in-place growth uncovers is zeroed, then the range, then the pad
        if (nTex > oldTex) HIPCHK(hipMemsetAsync(sc.tex + oldTex, 0, sizeof(RtFloat4) * (size_t)(nTex - oldTex), s));
        if (writeTex) HIPCHK(hipMemcpyAsync(sc.tex + u.texFirst, u.texels, sizeof(RtFloat4) * (size_t)u.texCount, hipMemcpyDefault, s));
        if (padChange) HIPCHK(hipMemsetAsync(sc.tex + nTex, 0, sizeof(RtFloat4) * (size_t)texPad, s));
    }
    HIPCHK(hipEventRecord(b.rev[3], s));
    HIPCHK(hipStreamSynchronize(s));
    SceneArrays n = b.sc;
    if (newTable) { n.mats = M.p; n.nMats = nMats; b.mmatsNext ^= 1; b.hMats.assign(u.mats, u.mats + nMats); }
    if (lightsChange) {
        n.lights = L.lights.p; n.lightRecs = L.lightRecs.p; n.nLights = nLights;
        b.nLights = nLights; b.mlightsNext ^= 1;
        b.lightsInSet = true;   // later rebuilds carry the list from set to set, as after a resize
    }
    if (moveTex) { n.tex = T.p; b.texCap = T.cap; b.mtexNext ^= 1; }
    n.nTex = nTex; b.texPad = texPad;
    if (assign && !b.primMat.empty())   // the host shadow of matIdx: the range's values, the only per-primitive data that comes back
        HIPCHK(hipMemcpy(b.primMat.data() + u.primFirst, dAssign, sizeof(int32_t) * (size_t)u.primCount, hipMemcpyDeviceToHost));
    const bool rebind = n.mats != sc.mats || n.lights != sc.lights || n.lightRecs != sc.lightRecs || n.tex != sc.tex || n.nMats != sc.nMats ||
                        n.nLights != sc.nLights || n.nTex != sc.nTex;
    b.sc = n;
    if (rebind) b.generation++;   // every holder takes the new arrays and counts before its next launch
    if (stats) {
        float ms = 0, ms2 = 0;   // GPU time of both phases (not the wait for the holders in between)
        (void)hipEventElapsedTime(&ms, b.rev[0], b.rev[1]); (void)hipEventElapsedTime(&ms2, b.rev[2], b.rev[3]);
        stats->gpu_ms = ms + ms2; stats->wall_ms = ms_between(t0, clock::now());
        stats->mats = newTable ? nMats : 0; stats->texels = writeTex ? u.texCount : 0; stats->prims = assign ? u.primCount : 0;
        stats->lights = nLights; stats->atlas_reallocated = moveTex ? 1 : 0;
    }
    return RT_OK;
}
int64_t scenedev::rebuild_allocations(const SceneBag& b) { return (int64_t)(b.rallocs + sbvhdev::pool_allocations(b.spool)); }
// The primitive range of every instance's BLAS (rebuild_common.h), for callers that want to know beforehand whether rt_rebuild_scene
// will take a scene; no device needed.
extern "C" int rt_blas_ranges(const RtBVHNode2* nodes, int32_t nNodes, const uint32_t* primIdx, int32_t nIdx, int32_t nPrims,
                              const RtBVHInstance* blas, int32_t nBlas, int32_t* firstOut, int32_t* countOut)
{
    std::vector<rebuild::BlasRange> ranges; std::vector<int32_t> instBlas;
    if (const char* why = rebuild::find_blas_ranges(nodes, nNodes, primIdx, nIdx, nPrims, blas, nBlas, ranges, instBlas))
        return fail(why == std::string("missing array") ? RT_E_INVALID : RT_E_UNSUPPORTED, "rt_blas_ranges: %s", why);
    for (int32_t i = 0; i < nBlas; i++) {
        if (firstOut) firstOut[i] = (int32_t)ranges[(size_t)instBlas[(size_t)i]].first;
        if (countOut) countOut[i] = (int32_t)ranges[(size_t)instBlas[(size_t)i]].count;
    }
    return RT_OK;
}
// ... and the block of every distinct BLAS, in the order a plan names them (rt_rebuild_ranges), as rt_upload_scene finds them
extern "C" int rt_blas_blocks(const RtBVHNode2* nodes, int32_t nNodes, const uint32_t* primIdx, int32_t nIdx, int32_t nPrims, const RtBVHInstance* blas, int32_t nBlas,
                              int32_t* n, int32_t* primFirst, int32_t* primCount, int32_t* nodesOut, int32_t* idxSlots, int32_t* compact, int32_t cap)
{
    std::vector<rebuild::BlasRange> ranges; std::vector<int32_t> instBlas;
    if (const char* why = rebuild::find_blas_ranges(nodes, nNodes, primIdx, nIdx, nPrims, blas, nBlas, ranges, instBlas))
        return fail(why == std::string("missing array") ? RT_E_INVALID : RT_E_UNSUPPORTED, "rt_blas_blocks: %s", why);
    std::vector<rebuild::BlasBlock> blocks;
    rebuild::find_blas_blocks(nodes, ranges, blocks);
    if (n) *n = (int32_t)ranges.size();
    for (size_t k = 0; k < ranges.size() && (int64_t)k < (int64_t)cap; k++) {
        if (primFirst) primFirst[k] = (int32_t)ranges[k].first;
        if (primCount) primCount[k] = (int32_t)ranges[k].count;
        if (nodesOut) nodesOut[k] = (int32_t)blocks[k].nodes;
        if (idxSlots) idxSlots[k] = (int32_t)blocks[k].idxSlots;
        if (compact) compact[k] = blocks[k].compact;
    }
    return RT_OK;
}
int scenedev::scene_array(const SceneBag& b, int32_t which, const void** src, size_t* n)
{
    const SceneArrays& sc = b.sc;
    switch (which) {
    case RT_SCENE_PRIMS:        *src = sc.prims; *n = sizeof(RtPrimitive) * (size_t)b.nPrims; break;
    case RT_SCENE_BVH:          *src = b.accel == RT_ACCEL_BVH4 ? (const void*)sc.bvh4 : (const void*)sc.bvh2;
                                *n = (b.accel == RT_ACCEL_BVH4 ? sizeof(RtBVHNode4) : sizeof(RtBVHNode2)) * (size_t)b.nNodes; break;
    case RT_SCENE_TLAS:         *src = sc.tlas; *n = sizeof(RtTLASNode) * (size_t)b.nTlas; break;
    case RT_SCENE_INSTANCES:    *src = sc.blas; *n = sizeof(RtBVHInstance) * (size_t)b.nBlas; break;
    case RT_SCENE_PAIRS:        *src = sc.pairs; *n = sc.pairs ? sizeof(RtFloat4) * 4 * (size_t)b.nPairs : 0; break;
    case RT_SCENE_TRI_RECS:     *src = sc.triRecs; *n = sc.triRecs ? sizeof(RtFloat4) * 3 * (size_t)b.nIdx : 0; break;
    case RT_SCENE_SHADE_RECS:   *src = sc.shadeRecs; *n = sizeof(RtFloat4) * (size_t)b.nPrims; break;
    case RT_SCENE_LIGHT_RECS:   *src = sc.lightRecs; *n = sizeof(RtFloat4) * 8 * (size_t)b.nLights; break;
    case RT_SCENE_TLAS_PAIRS:   *src = sc.tlasPairs; *n = sizeof(RtFloat4) * 4 * (size_t)b.nTlas; break;
    case RT_SCENE_TLAS_PAIRS_P: *src = sc.tlasPairsP; *n = sizeof(RtFloat4) * 4 * (size_t)b.nTlas; break;
    case RT_SCENE_INST_RECS:    *src = sc.instRecs; *n = sizeof(RtFloat4) * 4 * (size_t)b.nBlas; break;
    case RT_SCENE_QUADS:        *src = sc.quads; *n = sc.quads ? sizeof(RtFloat4) * 8 * (size_t)std::max(b.nQuads, 1) : 0; break;
    case RT_SCENE_ROOT_ENTRY:   *src = sc.rootEntry; *n = sc.rootEntry ? sizeof(uint32_t) * (size_t)b.nBlas : 0; break;
    case RT_SCENE_LIGHTS:       *src = sc.lights; *n = sizeof(uint32_t) * (size_t)b.nLights; break;
    case RT_SCENE_MATERIALS:    *src = sc.mats; *n = sizeof(RtMaterial) * (size_t)sc.nMats; break;
    case RT_SCENE_TEXTURES:     *src = sc.tex; *n = sizeof(RtFloat4) * ((size_t)sc.nTex + (size_t)b.texPad); break;
    case RT_SCENE_BVH2_KEPT:    *src = sc.bvh2; *n = b.keepsBvh2 ? sizeof(RtBVHNode2) * (size_t)b.nNodes : 0; break;
    default: return fail(RT_E_INVALID, "rt_debug_get_scene_array: unknown array %d", which);
    }
    return RT_OK;
}

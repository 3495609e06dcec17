// scene.hip — the device copy of a scene (SceneBag, scene_dev.h): the host-side checks of the arrays, the upload with what it derives and
// collapses, what the in-place changes (scene_rebuild.hip, scene_materials.hip) share with it and with each other, the rt_blas_* queries
// and the debug views.  Host code only: the kernels it drives are refit.hip's, rebuild.hip's and collapse.hip's; of the contexts that
// render from a copy (rt355.hip) the three files know SceneBag::wait_holders and nothing else.
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
int scenedev::validate_scene(int accel, const HostScene& in, SceneFacts* factsOut, int64_t* texPadOut)
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
    if (factsOut) { factsOut->stackEntries = rebuild::stack_entries(stackNeed); factsOut->tlasDepth = tlasDepth; }   // (rebuild_common.h: rt_rebuild_scene sizes it the same way)
    if (texPadOut) *texPadOut = texPad;
    return RT_OK;
}
extern "C" int rt_validate_scene(int32_t accel, const RtPrimitive* prims, int32_t nPrims, const RtMaterial* mats, int32_t nMats,
                                 const RtFloat4* textures, int32_t nTexels, const uint32_t* lights, int32_t nLights,
                                 const void* bvhNodes, int32_t nNodes, const uint32_t* primIdx, int32_t nIdx,
                                 const RtTLASNode* tlas, int32_t nTlas, const RtBVHInstance* blas, int32_t nBlas)
{
    return validate_scene(accel, HostScene{ prims, nPrims, mats, nMats, textures, nTexels, lights, nLights, bvhNodes, nNodes, primIdx, nIdx, tlas, nTlas, blas, nBlas },
                          nullptr, nullptr);
}

// What rt_update_scene needs of an upload: the host shadow of the fields an update must keep, and in `live` the trees' counts, their refit
// topology on the device (parents, reachable leaves, pair id -> node id) and one record per BLAS.  A scene the update cannot handle
// records why (refitRefusal).
// (a BVH4 copy that keeps its BVH2 - in.bvhNodes is the BVH2 - is prepared like a BVH2 copy: it can be rebuilt; rt_update_scene refuses
// every BVH4 context before it comes here)
static int prepare_update(SceneBag& b, LiveTrees& live, int accel, int extendVariant, const HostScene& in, const std::vector<uint32_t>& pairNode)
{
    const auto& [prims, nPrims, mats, nMats, textures, nTexels, lights, nLights, bvhNodes, nNodes, primIdx, nIdx, tlas, nTlas, blas, nBlas] = in;
    live.nNodes = nNodes; live.nIdx = nIdx; live.nTlas = nTlas; live.nPairs = (uint32_t)pairNode.size(); b.accel = accel;
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
    b.rebuildRefusal = rebuild::find_blas_ranges((const RtBVHNode2*)bvhNodes, nNodes, primIdx, nIdx, nPrims, blas, nBlas, live.ranges, live.instBlas);
    // ... and what it occupies: nodes, index slots, height, and whether it can be kept (rt_rebuild_ranges); build_topology has walked
    // the trees: no cycle
    if (!b.rebuildRefusal) {
        rebuild::find_blas_blocks((const RtBVHNode2*)bvhNodes, live.ranges, live.block);
        // where each BLAS's pair ids (pair_records) and leaves (build_topology) lie: both go root by root as the instances first name them
        live.pairLo.assign(live.ranges.size(), 0u); live.leafLo.assign(live.ranges.size(), 0u);
        std::vector<uint8_t> named(live.ranges.size(), 0);
        uint32_t pairLo = 0, leafLo = 0;
        for (const int32_t k : live.instBlas) {
            if (named[(size_t)k]) continue;
            named[(size_t)k] = 1;
            live.pairLo[(size_t)k] = pairLo; live.leafLo[(size_t)k] = leafLo;
            pairLo += live.interiors((size_t)k); leafLo += live.interiors((size_t)k) + 1;
        }
    }
    live.nLeaves = (uint32_t)t.leaves.size(); live.nReach = (uint32_t)t.order.size();
    int rc = dalloc(b.allocs, &live.parent, t.parent.size());
    if (rc == RT_OK) rc = dalloc(b.allocs, &live.leaves, t.leaves.size());
    if (rc == RT_OK) rc = dalloc(b.allocs, &live.tickets, (size_t)nNodes);
    if (rc == RT_OK) rc = dalloc(b.allocs, &live.pairNode, pairNode.size());
    if (rc != RT_OK) return rc;
    HIPCHK(hipMemcpy(live.parent, t.parent.data(), sizeof(uint32_t) * t.parent.size(), hipMemcpyHostToDevice));
    if (!t.leaves.empty()) HIPCHK(hipMemcpy(live.leaves, t.leaves.data(), sizeof(uint32_t) * t.leaves.size(), hipMemcpyHostToDevice));
    if (!pairNode.empty()) HIPCHK(hipMemcpy(live.pairNode, pairNode.data(), sizeof(uint32_t) * pairNode.size(), hipMemcpyHostToDevice));
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
// The two device-free entries that pin the relocation of pair records (include/rt355.h)
extern "C" int rt_debug_derive_pairs(const RtBVHNode2* nodes, int32_t nNodes, const RtBVHInstance* blas, int32_t nBlas, RtFloat4* pairs, uint32_t* pairNode,
                                     int32_t pairCap, uint32_t* rootEntry, int32_t* nPairs)
{
    if (!nodes || !blas || nNodes <= 0 || nBlas <= 0 || !nPairs) return fail(RT_E_INVALID, "rt_debug_derive_pairs: null argument");
    refit::Topology t;   // (checks every index pair_records follows)
    if (const char* why = refit::build_topology(nodes, nNodes, blas, nBlas, t)) return fail(RT_E_INVALID, "rt_debug_derive_pairs: %s", why);
    std::vector<uint32_t> order, roots((size_t)nBlas, 0u);
    const std::vector<RtFloat4> recs = pair_records(nodes, nNodes, blas, nBlas, order, roots);
    *nPairs = (int32_t)order.size();
    if ((pairs || pairNode) && (int64_t)order.size() > (int64_t)pairCap) return fail(RT_E_INVALID, "rt_debug_derive_pairs: %zu pair records, room for %d", order.size(), pairCap);
    if (pairs) std::copy(recs.begin(), recs.begin() + (ptrdiff_t)order.size() * 4, pairs);
    if (pairNode) std::copy(order.begin(), order.end(), pairNode);
    if (rootEntry) std::copy(roots.begin(), roots.end(), rootEntry);
    return RT_OK;
}
extern "C" int rt_debug_relocate_pairs(const RtFloat4* in, int32_t n, uint32_t pairDelta, uint32_t idxDelta, RtFloat4* out)
{
    if (n < 0 || (n > 0 && (!in || !out))) return fail(RT_E_INVALID, "rt_debug_relocate_pairs: null argument");
    for (int32_t k = 0; k < n; k++) {
        for (int w = 0; w < 3; w++) out[(size_t)k * 4 + w] = in[(size_t)k * 4 + w];
        const RtFloat4 q = in[(size_t)k * 4 + 3];
        out[(size_t)k * 4 + 3] = refit::f4(refit::u2f(rebuild::relocated_entry(refit::f2u(q.x), pairDelta, idxDelta)),
                                           refit::u2f(rebuild::relocated_entry(refit::f2u(q.y), pairDelta, idxDelta)), q.z, q.w);
    }
    return RT_OK;
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

static int collapse_uploaded(SceneBag& b, SceneArrays& sc, SceneFacts& facts, LiveTrees& live, int extendVariant, const HostScene& in,
                             const std::vector<collapse::Blas>& blas4, std::vector<uint32_t>& roots);   // (below)

int scenedev::upload_scene(SceneBag& b, int accel, int extendVariant, const HostScene& in, SceneFacts facts, int64_t texPad, const std::vector<collapse::Blas>* blas4)
{
    const auto& [prims, nPrims, mats, nMats, textures, nTexels, lights, nLights, bvhNodes, nNodes, primIdx, nIdx, tlas, nTlas, blas, nBlas] = in;
    // ---- derive.  Layout 1 (pair or quad records, triangle records, encoded roots) only when the encodings fit (rebuild_common.h,
    // shared with rt_rebuild_scene's kernels); in layout 0 the instance records carry root entry 0
    const RtBVHNode2* n2 = (const RtBVHNode2*)bvhNodes; const RtBVHNode4* n4 = (const RtBVHNode4*)bvhNodes;
    std::vector<uint32_t> pairNode, roots((size_t)nBlas, 0u);
    std::vector<RtFloat4> pairs, quads;
    LiveTrees live;
    if (accel == RT_ACCEL_BVH2) {
        uint32_t largestLeaf = 0;
        for (int32_t i = 0; i < nNodes; i++) largestLeaf = std::max(largestLeaf, n2[i].count);
        if (rebuild::takes_layout1(extendVariant != 1, nIdx, largestLeaf)) { pairs = pair_records(n2, nNodes, blas, nBlas, pairNode, roots); facts.layout = 1; }
    } else if (blas4) {
        // (the layout follows from the collapse on the device, below)
    } else if (extendVariant != 1 && nIdx < rebuild::kMaxPackedIdx) {
        bool fits = true;
        for (int32_t i = 0; i < nNodes && fits; i++) for (int k = 0; k < 4; k++) if (n4[i].first[k] != RT_INVALID && n4[i].count[k] > (int32_t)rebuild::kMaxPackedLeaf) fits = false;
        if (fits) { quads = quad_records(n4, nNodes, nIdx, blas, nBlas, roots); facts.layout = 1; facts.nQuads = (int32_t)(quads.size() / 8); }
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
    if (rc == RT_OK && blas4) rc = collapse_uploaded(b, sc, facts, live, extendVariant, in, *blas4, roots);
    else if (rc == RT_OK && facts.layout == 1) {
        rc = accel == RT_ACCEL_BVH4 ? upload(b, &sc.quads, quads) : upload(b, &sc.pairs, pairs);
        if (rc == RT_OK) rc = upload(b, &sc.triRecs, triangle_records(prims, primIdx, nIdx));
        if (rc == RT_OK) rc = upload(b, &sc.rootEntry, roots);
    }
    if (rc == RT_OK) rc = upload(b, &sc.tlasPairs, tlas_records(tlas, nTlas, false));
    if (rc == RT_OK) rc = upload(b, &sc.instRecs, instance_records(blas, nBlas, roots));
    if (rc == RT_OK) rc = upload(b, &sc.tlasPairsP, tlas_records(tlas, nTlas, true));
    if (rc != RT_OK) return rc;
    const bool leafRoot = tlas[0].leftRight == 0;
    sc.tlasRoot = leafRoot ? refit::tlas_leaf_entry(false, tlas[0].BLASidx) : refit::tlas_node_entry(false, 0u);
    sc.tlasRootP = leafRoot ? refit::tlas_leaf_entry(true, tlas[0].BLASidx) : refit::tlas_node_entry(true, 0u);
    sc.nLights = nLights; sc.nPrims = nPrims; sc.nBlas = nBlas; sc.nTex = nTexels; sc.nMats = nMats;
    facts.nInterior = (int)pairNode.size(); facts.singleBlas = leafRoot;
    // ---- bind: what updates and rebuilds need of this upload, then the arrays, the facts and the trees, each assigned once
    b.hMats.assign(mats, mats + nMats); b.texPad = texPad; b.texCap = (size_t)nTexels + (size_t)texPad;   // (rt_update_materials)
    if ((rc = prepare_update(b, live, accel, extendVariant, in, pairNode)) != RT_OK) return rc;
    b.sc = sc; b.facts = facts; b.live = std::move(live);
    return RT_OK;
}

// rt_upload_scene_bvh2 on a BVH4 context, after the wire arrays are on the device: the collapse into sc.bvh4, then the layout, the stack
// size and the layout-1 records (quads, root entries, triangle records) as rt_upload_scene derives them from the host's collapse
static int collapse_uploaded(SceneBag& b, SceneArrays& sc, SceneFacts& facts, LiveTrees& live, int extendVariant, const HostScene& in,
                             const std::vector<collapse::Blas>& blas4, std::vector<uint32_t>& roots)
{
    using namespace collapsedev;
    const char* who = "rt_upload_scene_bvh2";
    const int32_t nNodes = in.nNodes, nIdx = in.nIdx, nBlas = in.nBlas;
    if (const int rc = scene_stream(b, nullptr)) return rc;
    hipStream_t s = b.stream;
    size_t quadCap = 0;   // a live node per interior node and leaf root at most
    for (const collapse::Blas& k : blas4) quadCap += std::max(k.interiors, 1u);
    int rc = dalloc(b.allocs, &sc.bvh4, (size_t)nNodes);
    if (rc == RT_OK) rc = dalloc(b.allocs, &live.newId, (size_t)nNodes);   // the copy's own: RT_REBUILD_REFIT reads them
    if (rc == RT_OK) rc = dalloc(b.allocs, &live.quadNode, quadCap);
    if (rc == RT_OK) rc = collapse_scratch(b, (size_t)nNodes);
    if (rc != RT_OK) return rc;
    Work w = collapse_work(b, live.newId, live.quadNode, quadCap);
    HIPCHK(begin(s, w, sc.bvh2, (uint32_t)nNodes, sc.bvh4));
    for (const collapse::Blas& k : blas4) HIPCHK(collapse_blas(s, w, sc.bvh2, (uint32_t)nNodes, k.root, k.interiors, k.height, sc.bvh4));
    CollapseStatus st;
    HIPCHK(st.read(s, w));
    HIPCHK(hipStreamSynchronize(s));
    if ((rc = st.error(who, "")) != RT_OK) return rc;
    live.nLive = st.live(); live.c4Need = st.need();
    facts.layout = rebuild::takes_layout1(extendVariant != 1, nIdx, st.largest_leaf()) ? 1 : 0;
    facts.stackEntries = rebuild::stack_entries((int)std::max(st.need(), 1u));
    facts.nQuads = facts.layout == 1 ? (int32_t)live.nLive : 0;
    b.keepsBvh2 = true;
    if (facts.layout != 1) return RT_OK;
    rc = dalloc(b.allocs, &sc.quads, (size_t)std::max(live.nLive, 1u) * 8);
    if (rc == RT_OK) rc = dalloc(b.allocs, &sc.rootEntry, (size_t)nBlas);
    if (rc == RT_OK) rc = dalloc(b.allocs, &sc.triRecs, (size_t)nIdx * 3);
    if (rc != RT_OK) return rc;
    w.quadCap = std::min(w.quadCap, std::max(live.nLive, 1u));   // what sc.quads holds
    HIPCHK(finish(s, w, sc.bvh4, (uint32_t)nNodes, (uint32_t)nIdx, (const uint32_t*)sc.blas, (uint32_t)(sizeof(RtBVHInstance) / 4), (uint32_t)nBlas, sc.quads, sc.rootEntry));
    HIPCHK(refitdev::launch_records(s, sc.prims, sc.bvh2, sc.primIdx, (uint32_t)nIdx, sc.lights, (uint32_t)in.nLights, 0u, (uint32_t)in.nPrims, nullptr, 0u, nullptr,
                                    sc.triRecs, sc.shadeRecs, sc.lightRecs));
    HIPCHK(hipMemcpyAsync(roots.data(), sc.rootEntry, sizeof(uint32_t) * (size_t)nBlas, hipMemcpyDeviceToHost, s));   // (the instance records carry them)
    HIPCHK(hipStreamSynchronize(s));
    return RT_OK;
}

// ---- what the upload and the in-place changes share (declared in scene_dev.h, with the rules of the capacities) ------------------------
int scenedev::scene_stream(SceneBag& b, hipEvent_t* ev)
{
    if (!b.stream) HIPCHK(hipStreamCreateWithFlags(&b.stream, hipStreamNonBlocking));
    for (int i = 0; ev && i < 4; i++) if (!ev[i]) HIPCHK(hipEventCreate(&ev[i]));
    return RT_OK;
}
size_t scenedev::rebuild_initial_cap(const SceneBag& b)
{
    if (const char* env = getenv("RT355_REBUILD_INITIAL_CAP")) {
        const long long k = atoll(env);
        if (k > 0) return (size_t)std::min<long long>(k, 1ll << 30);
    }
    return (size_t)std::max(b.sc.nPrims, 1);
}
// (flags / ranks / newId: a word per node, the frontiers: per interior node)
int scenedev::rebuild_scratch(SceneBag& b, size_t nodeNeed)
{
    const size_t cap = (grown_cap(nodeNeed, b.dwFlags.cap, b.dwFlags.p != nullptr) + 1) & ~(size_t)1;
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
int scenedev::flag_scan_result(SceneBag& b, int32_t n, uint32_t* firstBad, int32_t* nLights)
{
    uint32_t lastRank = 0, lastFlag = 0;
    hipStream_t s = b.stream;
    *firstBad = resize::kNoBad;
    HIPCHK(hipMemcpyAsync(firstBad, b.rStatus, sizeof *firstBad, hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(&lastRank, b.dw.ranks + (n - 1), sizeof lastRank, hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(&lastFlag, b.dw.flags + (n - 1), sizeof lastFlag, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    *nLights = (int32_t)(lastRank + lastFlag);
    return RT_OK;
}
// (kernels: collapse.hip, rules: collapse_common.h; the scratch grows as the derivation's does)
int scenedev::collapse_scratch(SceneBag& b, size_t nodeNeed)
{
    const size_t cap = (grown_cap(nodeNeed, b.c4Cap, b.c4Cap != 0) + 1) & ~(size_t)1;
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
collapsedev::Work scenedev::collapse_work(const SceneBag& b, uint32_t* newId, uint32_t* quadNode, size_t quadCap)
{
    collapsedev::Work w = b.c4;
    w.newId = newId; w.quadNode = quadNode; w.quadCap = (uint32_t)std::min<size_t>(quadCap, 0x7fffffffu);
    return w;
}
int scenedev::CollapseStatus::error(const char* who, const char* tail) const
{
    if (walk()) return fail(RT_E_DEVICE, "%s: the BVH4 level walk does not match the BVH2 (inconsistent device result)", who);
    if (rebuild::exceeds_stack(need()))   // validate_scene's rule for a BVH4
        return fail(RT_E_UNSUPPORTED, "%s: a collapsed BLAS: traversal needs %u stack entries, at most %d are supported%s", who, need(), RT_BVH4_STACK, tail);
    return RT_OK;
}
int scenedev::too_many_nodes(const char* who)
{
    return fail(RT_E_UNSUPPORTED, "%s: the new trees have 2^31 nodes or index slots, or more; the scene is unchanged", who);
}
void scenedev::write_blocks(const LiveTrees& t, int32_t* n, int32_t* primFirst, int32_t* primCount, int32_t* nodes, int32_t* idxSlots, int32_t* compact, int32_t cap)
{
    if (n) *n = (int32_t)t.ranges.size();
    for (size_t k = 0; k < t.ranges.size() && (int64_t)k < (int64_t)cap; k++) {
        if (primFirst) primFirst[k] = (int32_t)t.ranges[k].first;
        if (primCount) primCount[k] = (int32_t)t.ranges[k].count;
        if (nodes) nodes[k] = (int32_t)t.block[k].nodes;
        if (idxSlots) idxSlots[k] = (int32_t)t.block[k].idxSlots;
        if (compact) compact[k] = t.block[k].compact;
    }
}

// ---- queries: the bound trees' blocks, the allocation count, and (no device needed) the ranges and blocks of host arrays ---------------

int scenedev::blas_blocks(const SceneBag& b, int32_t* n, int32_t* primFirst, int32_t* primCount, int32_t* nodes, int32_t* idxSlots, int32_t* compact, int32_t cap)
{
    if (b.rebuildRefusal) return fail(RT_E_UNSUPPORTED, "rt_scene_blas_blocks: %s", b.rebuildRefusal);
    if (b.live.block.size() != b.live.ranges.size()) return fail(RT_E_UNSUPPORTED, "rt_scene_blas_blocks: %s", b.refitRefusal ? b.refitRefusal : "the scene's BLAS ranges are not known");
    write_blocks(b.live, n, primFirst, primCount, nodes, idxSlots, compact, cap);
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
    LiveTrees t;
    if (const char* why = rebuild::find_blas_ranges(nodes, nNodes, primIdx, nIdx, nPrims, blas, nBlas, t.ranges, t.instBlas))
        return fail(why == std::string("missing array") ? RT_E_INVALID : RT_E_UNSUPPORTED, "rt_blas_blocks: %s", why);
    rebuild::find_blas_blocks(nodes, t.ranges, t.block);
    write_blocks(t, n, primFirst, primCount, nodesOut, idxSlots, compact, cap);
    return RT_OK;
}
int scenedev::scene_array(const SceneBag& b, int32_t which, const void** src, size_t* n)
{
    const SceneArrays& sc = b.sc;
    const LiveTrees& t = b.live;
    switch (which) {
    case RT_SCENE_PRIMS:        *src = sc.prims; *n = sizeof(RtPrimitive) * (size_t)sc.nPrims; break;
    case RT_SCENE_BVH:          *src = b.accel == RT_ACCEL_BVH4 ? (const void*)sc.bvh4 : (const void*)sc.bvh2;
                                *n = (b.accel == RT_ACCEL_BVH4 ? sizeof(RtBVHNode4) : sizeof(RtBVHNode2)) * (size_t)t.nNodes; break;
    case RT_SCENE_TLAS:         *src = sc.tlas; *n = sizeof(RtTLASNode) * (size_t)t.nTlas; break;
    case RT_SCENE_INSTANCES:    *src = sc.blas; *n = sizeof(RtBVHInstance) * (size_t)sc.nBlas; break;
    case RT_SCENE_PAIRS:        *src = sc.pairs; *n = sc.pairs ? sizeof(RtFloat4) * 4 * (size_t)t.nPairs : 0; break;
    case RT_SCENE_TRI_RECS:     *src = sc.triRecs; *n = sc.triRecs ? sizeof(RtFloat4) * 3 * (size_t)t.nIdx : 0; break;
    case RT_SCENE_SHADE_RECS:   *src = sc.shadeRecs; *n = sizeof(RtFloat4) * (size_t)sc.nPrims; break;
    case RT_SCENE_LIGHT_RECS:   *src = sc.lightRecs; *n = sizeof(RtFloat4) * 8 * (size_t)sc.nLights; break;
    case RT_SCENE_TLAS_PAIRS:   *src = sc.tlasPairs; *n = sizeof(RtFloat4) * 4 * (size_t)t.nTlas; break;
    case RT_SCENE_TLAS_PAIRS_P: *src = sc.tlasPairsP; *n = sizeof(RtFloat4) * 4 * (size_t)t.nTlas; break;
    case RT_SCENE_INST_RECS:    *src = sc.instRecs; *n = sizeof(RtFloat4) * 4 * (size_t)sc.nBlas; break;
    case RT_SCENE_QUADS:        *src = sc.quads; *n = sc.quads ? sizeof(RtFloat4) * 8 * (size_t)std::max(b.facts.nQuads, 1) : 0; break;
    case RT_SCENE_ROOT_ENTRY:   *src = sc.rootEntry; *n = sc.rootEntry ? sizeof(uint32_t) * (size_t)sc.nBlas : 0; break;
    case RT_SCENE_LIGHTS:       *src = sc.lights; *n = sizeof(uint32_t) * (size_t)sc.nLights; break;
    case RT_SCENE_MATERIALS:    *src = sc.mats; *n = sizeof(RtMaterial) * (size_t)sc.nMats; break;
    case RT_SCENE_TEXTURES:     *src = sc.tex; *n = sizeof(RtFloat4) * ((size_t)sc.nTex + (size_t)b.texPad); break;
    case RT_SCENE_BVH2_KEPT:    *src = sc.bvh2; *n = b.keepsBvh2 ? sizeof(RtBVHNode2) * (size_t)t.nNodes : 0; break;
    default: return fail(RT_E_INVALID, "rt_debug_get_scene_array: unknown array %d", which);
    }
    return RT_OK;
}

// host_capi.cpp — extern "C" wrappers (include/rt355_host.h) over the C++ host classes.
#include <cstring>
#include <exception>
#include <memory>
#include <string>
#include "../../include/rt355.h"
#include "../../include/rt355_host.h"
#include "../csrc/collapse_common.h"
#include "../csrc/resize_common.h"
#include "../csrc/geometry_common.h"
#include "rt_host.h"

using namespace rt355;

static thread_local std::string g_herr;
struct RthScene { Scene scene; TLAS* tlas = nullptr; ~RthScene() { delete tlas; } };
struct RthRenderer { Renderer* r = nullptr; RthScene* adopted = nullptr; };

#define GUARD(...) try { __VA_ARGS__; return 0; } catch (const std::exception& e) { g_herr = e.what(); return -1; }
static float3 f3(const float* p) { return float3(p[0], p[1], p[2]); }
static float2 f2(const float* p) { float2 r; if (p) { r.x = p[0]; r.y = p[1]; } return r; }

// rth_build_blas_<builder>: the start index checked, then the BVH2 method; an LbvhError carries its RT_E_* code
template <class Build> static int build_blas(const char* who, RthScene* s, int startIdx, Build build)
{
    if (!s || startIdx < 0 || startIdx >= (int)s->scene.primitives.size()) { g_herr = std::string(who) + ": bad start index"; return RT_E_INVALID; }
    try { build(); return 0; }
    catch (const LbvhError& e) { g_herr = e.what(); return e.code; }
    catch (const std::exception& e) { g_herr = e.what(); return RT_E_NOMEM; }
}
// rth_build_bvh2_<builder>: the host restatement's message goes to rth_last_error() when it refuses
template <class Build> static int build_bvh2(Build build)
{
    std::string err;
    const int rc = build(err);
    if (rc != RT_OK) g_herr = err;
    return rc;
}
// The host restatement of rt_update_materials: the Scene methods' message goes to rth_last_error() when they refuse
template <class Set> static int set_materials(const char* who, RthScene* s, Set set)
{
    if (!s) { g_herr = std::string(who) + ": null scene"; return RT_E_INVALID; }
    try {
        std::string err;
        const int rc = set(err);
        if (rc != RT_OK) g_herr = err;
        return rc;
    } catch (const std::exception& e) { g_herr = e.what(); return RT_E_NOMEM; }
}

extern "C" {

const char* rth_last_error(void) { return g_herr.c_str(); }

RthScene* rth_scene_create(void) { try { return new RthScene(); } catch (...) { return nullptr; } }
void rth_scene_destroy(RthScene* s) { delete s; }

int rth_add_material(RthScene* s, const char* name, const RtMaterial* init)
{
    if (!s || !name) { g_herr = "rth_add_material: null argument"; return -1; }
    try {
        RtMaterial& m = s->scene.AddMaterial(name);
        if (init) m = *init;
        return (int)s->scene.materials.size() - 1;
    } catch (const std::exception& e) { g_herr = e.what(); return -1; }
}
int rth_add_texture(RthScene* s, const char* name, const RtFloat4* texels, int w, int h)
{
    if (!s || !name || !texels || w <= 0 || h <= 0) { g_herr = "rth_add_texture: bad argument"; return -1; }
    try { return s->scene.AddTexture(texels, w, h, name); } catch (const std::exception& e) { g_herr = e.what(); return -1; }
}
int rth_load_texture(RthScene* s, const char* filename, const char* name)
{
    if (!s || !filename || !name) { g_herr = "rth_load_texture: null argument"; return -1; }
    try { return s->scene.LoadTexture(filename, name); } catch (const std::exception& e) { g_herr = e.what(); return -1; }
}
int rth_add_sphere(RthScene* s, const float pos[3], float radius, const char* material) { GUARD(s->scene.AddSphere(f3(pos), radius, material)) }
int rth_add_plane(RthScene* s, const float N[3], float d, const char* material) { GUARD(s->scene.AddPlane(f3(N), d, material)) }
int rth_add_triangle(RthScene* s, const float v0[3], const float v1[3], const float v2[3], const float uv0[2], const float uv1[2],
                     const float uv2[2], const char* material, int flip)
{
    GUARD(s->scene.AddTriangle(f3(v0), f3(v1), f3(v2), f2(uv0), f2(uv1), f2(uv2), material, flip != 0))
}
int rth_add_quad(RthScene* s, const float v0[3], const float v1[3], const float v2[3], const float v3[3], const char* material, int flip)
{
    GUARD(s->scene.AddQuad(f3(v0), f3(v1), f3(v2), f3(v3), material, flip != 0))
}
int rth_add_triangles(RthScene* s, const float* verts, const float* uvs, int n, const char* material, int flip)
{
    if (!s || !verts || n < 0 || !material) { g_herr = "rth_add_triangles: bad argument"; return -1; }
    try {
        const std::string mat(material);
        s->scene.primitives.reserve(s->scene.primitives.size() + (size_t)n);
        for (int i = 0; i < n; i++) {
            const float* v = verts + (size_t)i * 9;
            const float* t = uvs ? uvs + (size_t)i * 6 : nullptr;
            s->scene.AddTriangle(f3(v), f3(v + 3), f3(v + 6), f2(t), f2(t ? t + 2 : nullptr), f2(t ? t + 4 : nullptr), mat, flip != 0);
        }
        return 0;
    } catch (const std::exception& e) { g_herr = e.what(); return -1; }
}
int rth_build_blas(RthScene* s, int startIdx, float alpha)
{
    if (!s || startIdx < 0 || startIdx >= (int)s->scene.primitives.size()) { g_herr = "rth_build_blas: bad start index"; return -1; }
    GUARD(s->scene.bvh2->alpha = alpha; s->scene.bvh2->BuildBLAS(true, startIdx))
}
int rth_build_blas_lbvh(RthScene* s, int startIdx, int device, const RtBuildOptions* opts)
{
    return build_blas("rth_build_blas_lbvh", s, startIdx, [&] { s->scene.bvh2->BuildBLASLBVH(startIdx, device, opts); });
}
int rth_build_bvh2_lbvh(const RtBuildOptions* opts, const RtPrimitive* prims, int32_t nPrims, int32_t first, int32_t count, uint32_t nodeBase,
                        uint32_t idxBase, RtBVHNode2* nodes, int32_t nodeCap, int32_t* nNodes, uint32_t* primIdx, RtBuildStats* stats)
{
    return build_bvh2([&](std::string& err) { return LbvhBuildHost(opts, prims, nPrims, first, count, nodeBase, idxBase, nodes, nodeCap, nNodes, primIdx, stats, err); });
}
int rth_lbvh_stats(RthScene* s, RtBuildStats* out) { if (!s || !out) return -1; *out = s->scene.bvh2->lastLbvh; return 0; }
int rth_build_blas_sah_gpu(RthScene* s, int startIdx, int device)
{
    return build_blas("rth_build_blas_sah_gpu", s, startIdx, [&] { s->scene.bvh2->BuildBLASSAHGPU(startIdx, device); });
}
int rth_build_bvh2_sah(const RtPrimitive* prims, int32_t nPrims, int32_t first, int32_t count, uint32_t nodeBase, uint32_t idxBase,
                       RtBVHNode2* nodes, int32_t nodeCap, int32_t* nNodes, uint32_t* primIdx, RtBuildStats* stats)
{
    return build_bvh2([&](std::string& err) { return SahBuildHost(prims, nPrims, first, count, nodeBase, idxBase, nodes, nodeCap, nNodes, primIdx, stats, err); });
}
int rth_build_blas_sbvh_gpu(RthScene* s, int startIdx, float alpha, int device)
{
    return build_blas("rth_build_blas_sbvh_gpu", s, startIdx, [&] { s->scene.bvh2->BuildBLASSBVHGPU(startIdx, alpha, device); });
}
int rth_build_bvh2_sbvh(float alpha, const RtPrimitive* prims, int32_t nPrims, int32_t first, int32_t count, uint32_t nodeBase, uint32_t idxBase,
                        RtBVHNode2* nodes, int32_t nodeCap, int32_t* nNodes, uint32_t* primIdx, int32_t idxCap, int32_t* nIdx, RtSbvhStats* stats)
{
    return build_bvh2([&](std::string& err) {
        return SbvhBuildHost(alpha, prims, nPrims, first, count, nodeBase, idxBase, nodes, nodeCap, nNodes, primIdx, idxCap, nIdx, stats, err);
    });
}
int rth_set_build_threads(RthScene* s, int threads) { if (!s) return -1; s->scene.bvh2->buildThreads = threads < 1 ? 1 : threads; return 0; }
int rth_build_bvh4(RthScene* s) { GUARD(s->scene.BuildBVH4()) }
int rth_build_bvh4_gpu(RthScene* s, int device)
{
    if (!s || !s->scene.bvh2) { g_herr = "rth_build_bvh4_gpu: null scene"; return RT_E_INVALID; }
    try {
        Scene& sc = s->scene;
        const std::vector<RtBVHNode2>& n2 = sc.bvh2->bvhNodes;
        std::vector<RtBVHNode4> out(n2.size());
        std::vector<uint32_t> roots;
        for (const RtBVHInstance& inst : sc.blasNodes) roots.push_back(inst.bvhIdx);
        std::string err;
        const int rc = device < 0
            ? Bvh4LevelsHost(n2.data(), (int32_t)n2.size(), (int32_t)sc.bvh2->primIdx.size(), roots.data(), (int32_t)roots.size(), out.data(), nullptr, nullptr,
                             nullptr, nullptr, err)
            : rt_build_bvh4(device, n2.data(), (int32_t)n2.size(), (int32_t)sc.bvh2->primIdx.size(), roots.data(), (int32_t)roots.size(), out.data(), nullptr);
        if (rc != RT_OK) { g_herr = device < 0 ? err : std::string(rt_last_error()); return rc; }   // (the scene keeps the BVH4 it had)
        delete sc.bvh4; sc.bvh4 = new BVH4(*sc.bvh2, std::move(out));
        return 0;
    } catch (const std::exception& e) { g_herr = e.what(); return RT_E_NOMEM; }
}
int rth_build_bvh4_levels(const RtBVHNode2* nodes2, int32_t nNodes, int32_t nIdx, const uint32_t* roots, int32_t nRoots, RtBVHNode4* out4,
                          RtBvh4Stats* stats, RtFloat4* quads, uint32_t* rootEntry, uint32_t* quadNode)
{
    return build_bvh2([&](std::string& err) { return Bvh4LevelsHost(nodes2, nNodes, nIdx, roots, nRoots, out4, stats, quads, rootEntry, quadNode, err); });
}
int rth_bvh4_refit(const RtBVHNode2* refit2, int32_t nNodes, int32_t nIdx, const uint32_t* roots, int32_t nRoots, RtBVHNode4* inout4,
                   const uint32_t* quadNode, int32_t nLive, int32_t* changedNodes)
{
    return build_bvh2([&](std::string& err) { return Bvh4RefitHost(refit2, nNodes, nIdx, roots, nRoots, inout4, quadNode, nLive, changedNodes, err); });
}
// rth_bvh4_refit on the scene's own arrays: its BVH4 is the collapse of the BVH2 as it was before rth_refit.  The live nodes of that
// collapse are numbered as the upload numbers them: breadth-first, BLAS by BLAS in the order in which the instances first name them.
int rth_refit_bvh4(RthScene* s, int32_t* changedNodes)
{
    if (!s || !s->scene.bvh2 || !s->scene.bvh4) { g_herr = "rth_refit_bvh4: a scene with a BVH2 and the BVH4 collapsed from it is required"; return RT_E_INVALID; }
    try {
        Scene& sc = s->scene;
        const std::vector<RtBVHNode2>& n2 = sc.bvh2->bvhNodes;
        std::vector<RtBVHNode4>& n4 = sc.bvh4->Nodes();
        if (n4.size() != n2.size() || n2.empty()) { g_herr = "rth_refit_bvh4: the BVH4 is not the collapse of the scene's BVH2"; return RT_E_INVALID; }
        std::vector<uint32_t> roots, order;
        std::vector<uint8_t> seen(n2.size(), 0);
        for (const RtBVHInstance& inst : sc.blasNodes) roots.push_back(inst.bvhIdx);
        for (const uint32_t root : roots) {
            if (root >= n4.size()) { g_herr = "rth_refit_bvh4: an instance's bvhIdx is out of range"; return RT_E_INVALID; }
            if (seen[root]) continue;
            size_t head = order.size();
            seen[root] = 1; order.push_back(root);
            for (; head < order.size(); head++)
                for (int k = 0; k < 4; k++) if (collapse::is_child(n4[order[head]], k)) {
                    const uint32_t c = (uint32_t)n4[order[head]].first[k];
                    if (c >= n4.size() || seen[c]) { g_herr = "rth_refit_bvh4: the BVH4 is malformed (a child out of range or reachable twice)"; return RT_E_INVALID; }
                    seen[c] = 1; order.push_back(c);
                }
        }
        std::string err;
        const int rc = Bvh4RefitHost(n2.data(), (int32_t)n2.size(), (int32_t)sc.bvh2->primIdx.size(), roots.data(), (int32_t)roots.size(), n4.data(), order.data(),
                                     (int32_t)order.size(), changedNodes, err);
        if (rc != RT_OK) g_herr = err;
        return rc;
    } catch (const std::exception& e) { g_herr = e.what(); return RT_E_NOMEM; }
}
// BVH4::Convert + Collapse (bvh.cpp:695-787) on a caller-provided BVH2 node array with ONE BLAS rooted at node 0: how the tests feed
// the reference's own hand-built 13-node tree (bvh.cpp:615-674) through the collapse.
int rth_bvh4_from_nodes(const RtBVHNode2* nodes, int n, RtBVHNode4* out)
{
    if (!nodes || !out || n <= 0) { g_herr = "rth_bvh4_from_nodes: bad argument"; return -1; }
    {   // Convert / Collapse index children unchecked and recurse: refuse child ids out of range and nodes reachable twice (a cycle)
        std::vector<uint32_t> st{ 0u };
        size_t visited = 0;
        while (!st.empty()) {
            const uint32_t i = st.back(); st.pop_back();
            if (i >= (uint32_t)n || ++visited > (size_t)n) { g_herr = "rth_bvh4_from_nodes: child index out of range or a node reachable twice"; return -1; }
            if (nodes[i].count == 0) { st.push_back(nodes[i].first); st.push_back(nodes[i].first + 1); }
        }
        // ... and Convert reads both children of EVERY interior record of the array, reachable from node 0 or not
        for (int i = 0; i < n; i++) if (nodes[i].count == 0 && (uint64_t)nodes[i].first + 1 >= (uint64_t)n) {
            g_herr = "rth_bvh4_from_nodes: node " + std::to_string(i) + ": child index out of range (an unreachable interior record is converted too)";
            return -1;
        }
    }
    try {
        std::vector<RtPrimitive> prims; std::vector<RtBVHInstance> blas(1);
        memset(&blas[0], 0, sizeof blas[0]);
        blas[0].bvhIdx = 0;
        BVH2 b2(prims, blas);
        b2.bvhNodes.assign(nodes, nodes + n);
        BVH4 b4(b2);
        memcpy(out, b4.Nodes().data(), sizeof(RtBVHNode4) * (size_t)n);
        return 0;
    } catch (const std::exception& e) { g_herr = e.what(); return -1; }
}
int rth_set_primitives(RthScene* s, int first, int count, const RtPrimitive* prims)
{
    if (!s) { g_herr = "rth_set_primitives: null scene"; return RT_E_INVALID; }
    std::string err;
    const int rc = SetPrimitivesHost(s->scene.primitives, first, count, prims, err);
    if (rc != RT_OK) g_herr = err;
    return rc;
}
int rth_set_vertices(RthScene* s, int first, int count, const float* positions, int64_t strideBytes, int64_t nVertices, const uint32_t* indices)
{
    if (!s) { g_herr = "rth_set_vertices: null scene"; return RT_E_INVALID; }
    std::vector<RtPrimitive>& prims = s->scene.primitives;
    try {
        RtGeometry g{};
        g.first = first; g.count = count; g.positions = positions; g.positionStride = strideBytes; g.nVertices = nVertices; g.indices = indices;
        std::vector<int32_t> types(prims.size());
        for (size_t i = 0; i < prims.size(); i++) types[i] = prims[i].objType;
        std::string err;
        if (const int rc = geometry::check_args(&g, (int64_t)prims.size(), types.data(), err)) { g_herr = "rth_set_vertices: " + err; return rc; }
        // every index before any record: a refusal changes nothing
        for (int64_t i = 0; indices && i < count; i++) {
            const uint32_t* t = indices + 3 * i;
            if (t[0] >= nVertices || t[1] >= nVertices || t[2] >= nVertices) { g_herr = "rth_set_vertices: indices: " + geometry::bad_index_message(i, t, nVertices); return RT_E_INVALID; }
        }
        for (int64_t i = 0; i < count; i++) {
            const uint64_t j0 = indices ? indices[3 * i] : 3 * (uint64_t)i, j1 = indices ? indices[3 * i + 1] : j0 + 1, j2 = indices ? indices[3 * i + 2] : j0 + 2;
            geometry::set_triangle(prims[(size_t)first + (size_t)i], geometry::vertex(positions, strideBytes, j0), geometry::vertex(positions, strideBytes, j1),
                                   geometry::vertex(positions, strideBytes, j2));
        }
        return RT_OK;
    } catch (const std::exception& e) { g_herr = e.what(); return RT_E_NOMEM; }
}
int rth_refit(RthScene* s)
{
    if (!s || !s->scene.bvh2) { g_herr = "rth_refit: null scene"; return RT_E_INVALID; }
    std::string err;
    const int rc = RefitHost(s->scene.bvh2->bvhNodes, s->scene.bvh2->primIdx, s->scene.primitives, s->scene.blasNodes, err);
    if (rc != RT_OK) g_herr = err;
    return rc;
}
int rth_rebuild(RthScene* s, int builder, const RtBuildOptions* opts)
{
    if (!s || !s->scene.bvh2) { g_herr = "rth_rebuild: null scene"; return RT_E_INVALID; }
    try { s->scene.bvh2->Rebuild(builder, opts); return 0; }
    catch (const LbvhError& e) { g_herr = e.what(); return e.code; }
    catch (const std::exception& e) { g_herr = e.what(); return RT_E_NOMEM; }
}
int rth_rebuild_ranges(RthScene* s, const int32_t* plan, int nRanges, const RtBuildOptions* opts)
{
    if (!s || !s->scene.bvh2) { g_herr = "rth_rebuild_ranges: null scene"; return RT_E_INVALID; }
    try { s->scene.bvh2->RebuildRanges(plan, nRanges, opts); return 0; }
    catch (const LbvhError& e) { g_herr = e.what(); return e.code; }
    catch (const std::exception& e) { g_herr = e.what(); return RT_E_NOMEM; }
}
int rth_blas_ranges(RthScene* s, int32_t* firstOut, int32_t* countOut)
{
    if (!s || !s->scene.bvh2) { g_herr = "rth_blas_ranges: null scene"; return RT_E_INVALID; }
    const BVH2& b = *s->scene.bvh2;
    return rt_blas_ranges(b.bvhNodes.data(), (int32_t)b.bvhNodes.size(), b.primIdx.data(), (int32_t)b.primIdx.size(), (int32_t)s->scene.primitives.size(),
                          s->scene.blasNodes.data(), (int32_t)s->scene.blasNodes.size(), firstOut, countOut);
}
// (a refused build - too many instances, a singular transform, no partner - leaves the TLAS the scene had)
int rth_build_tlas(RthScene* s) { GUARD(std::unique_ptr<TLAS> t(new TLAS(*s->scene.bvh2)); t->Build(); delete s->tlas; s->tlas = t.release()) }
int rth_set_instance_transform(RthScene* s, int blas, const float invT[16])
{
    if (!s || blas < 0 || blas >= (int)s->scene.blasNodes.size()) { g_herr = "rth_set_instance_transform: bad index"; return -1; }
    memcpy(s->scene.blasNodes[blas].invT, invT, sizeof(float) * 16);
    return 0;
}
int rth_add_instance(RthScene* s, int blas, const float invT[16])
{
    if (!s || blas < 0 || blas >= (int)s->scene.blasNodes.size()) { g_herr = "rth_add_instance: bad index"; return -1; }
    if (s->scene.blasNodes.size() >= (size_t)refit::kMaxInstances) { g_herr = "rth_add_instance: TLAS::Build takes at most 256 instances"; return -1; }
    RtBVHInstance inst;
    memset(&inst, 0, sizeof inst);
    inst.bvhIdx = s->scene.blasNodes[(size_t)blas].bvhIdx;
    inst.invT[0] = inst.invT[5] = inst.invT[10] = inst.invT[15] = 1.0f;   // BuildBLAS's identity
    if (invT) {
        if (refit::singular(invT)) { g_herr = "rth_add_instance: the transform is singular"; return -1; }
        memcpy(inst.invT, invT, sizeof(float) * 16);
    }
    try { s->scene.blasNodes.push_back(inst); } catch (const std::exception& e) { g_herr = e.what(); return -1; }
    return (int)s->scene.blasNodes.size() - 1;
}
int rth_swap_instances(RthScene* s, int a, int b)
{
    const int n = s ? (int)s->scene.blasNodes.size() : 0;
    if (a < 0 || b < 0 || a >= n || b >= n) { g_herr = "rth_swap_instances: bad index"; return -1; }
    std::swap(s->scene.blasNodes[(size_t)a], s->scene.blasNodes[(size_t)b]);
    return 0;
}
int rth_light_list(const RtPrimitive* prims, int32_t nPrims, const RtMaterial* mats, int32_t nMats, uint32_t* out)
{
    if (!prims || !mats || !out || nPrims <= 0 || nMats <= 0) { g_herr = "rth_light_list: missing array"; return RT_E_INVALID; }
    for (int32_t i = 0; i < nPrims; i++) if (!resize::prim_ok(prims[i].objType, prims[i].matIdx, nMats)) {
        g_herr = "rth_light_list: primitive " + std::to_string(i) + ": objType " + std::to_string(prims[i].objType) + " / matIdx " + std::to_string(prims[i].matIdx) + " out of range";
        return RT_E_INVALID;
    }
    try {
        std::vector<uint32_t> lights;
        resize::light_list(prims, nPrims, mats, lights);
        if (!lights.empty()) memcpy(out, lights.data(), sizeof(uint32_t) * lights.size());
        return (int)lights.size();
    } catch (const std::exception& e) { g_herr = e.what(); return RT_E_NOMEM; }
}
int rth_set_materials(RthScene* s, const RtMaterial* mats, int32_t nMats)
{
    return set_materials("rth_set_materials", s, [&](std::string& err) { return s->scene.SetMaterials(mats, nMats, err); });
}
int rth_set_texels(RthScene* s, const RtFloat4* texels, int32_t first, int32_t count, int32_t nTexels)
{
    return set_materials("rth_set_texels", s, [&](std::string& err) { return s->scene.SetTexels(texels, first, count, nTexels, err); });
}
int rth_set_prim_materials(RthScene* s, int32_t first, int32_t count, const int32_t* matIdx)
{
    return set_materials("rth_set_prim_materials", s, [&](std::string& err) { return s->scene.SetPrimMaterials(first, count, matIdx, err); });
}

#define VIEW(vec) do { if (n) *n = (int)(vec).size(); return (vec).data(); } while (0)
const RtPrimitive*   rth_primitives(RthScene* s, int* n) { VIEW(s->scene.primitives); }
const RtMaterial*    rth_materials(RthScene* s, int* n) { VIEW(s->scene.materials); }
const RtFloat4*      rth_textures(RthScene* s, int* n) { VIEW(s->scene.textures); }
const uint32_t*      rth_lights(RthScene* s, int* n) { VIEW(s->scene.lights); }
const RtBVHNode2*    rth_bvh2_nodes(RthScene* s, int* n) { VIEW(s->scene.bvh2->bvhNodes); }
const RtBVHNode4*    rth_bvh4_nodes(RthScene* s, int* n) { if (!s->scene.bvh4) { if (n) *n = 0; return nullptr; } VIEW(s->scene.bvh4->Nodes()); }
const uint32_t*      rth_prim_idx(RthScene* s, int* n) { VIEW(s->scene.bvh2->primIdx); }
const RtTLASNode*    rth_tlas_nodes(RthScene* s, int* n) { if (!s->tlas) { if (n) *n = 0; return nullptr; } VIEW(s->tlas->tlasNodes); }
const RtBVHInstance* rth_blas_nodes(RthScene* s, int* n) { VIEW(s->scene.blasNodes); }

int rth_bvh_stats(RthScene* s, uint32_t u[5], float f[2])
{
    if (!s) return -1;
    const BVH2& b = *s->scene.bvh2;
    u[0] = b.stat_depth; u[1] = b.stat_node_count; u[2] = b.stat_spatial_splits; u[3] = b.stat_prims_clipped; u[4] = b.stat_prim_count;
    f[0] = b.stat_sah_cost; f[1] = b.stat_build_time;
    return 0;
}

int rth_camera(int width, int height, float vfov, int type, const float origin[3], const float forward[3], float aperture,
               float focalLength, RtCamera* out)
{
    if (!out || width <= 0 || height <= 0) { g_herr = "rth_camera: bad argument"; return -1; }
    CameraManager cm(width, height, vfov, type);
    if (origin) cm.cam.origin = RtFloat4{ origin[0], origin[1], origin[2], 0 };
    if (forward) cm.cam.forward = RtFloat4{ forward[0], forward[1], forward[2], 0 };
    cm.cam.aperture = aperture; cm.cam.focalLength = focalLength;
    cm.UpdateCamVec();
    *out = cm.cam;
    return 0;
}

// Renderer mirror: the scene handed in is adopted (its arrays are moved into Renderer::scene).
RthRenderer* rth_renderer_create(RthScene* scene, int width, int height, int device, int y0, int y1, int shading, int sampling,
                                 int bvh, int rr, int fireflies)
{
    if (!scene) { g_herr = "rth_renderer_create: null scene"; return nullptr; }
    try {
        RthRenderer* h = new RthRenderer();
        h->r = new Renderer(width, height, device, y0, y1);
        Scene& dst = h->r->scene; Scene& src = scene->scene;
        dst.primitives = src.primitives; dst.materials = src.materials; dst.lights = src.lights; dst.textures = src.textures;
        dst.blasNodes = src.blasNodes;
        dst.bvh2->bvhNodes = src.bvh2->bvhNodes; dst.bvh2->primIdx = src.bvh2->primIdx; dst.bvh2->alpha = src.bvh2->alpha;
        h->r->imgui.shading = shading; h->r->imgui.sampling = sampling; h->r->imgui.bvh = bvh;
        h->r->imgui.use_russian_roulette = rr != 0; h->r->imgui.filter_fireflies = fireflies != 0;
        return h;
    } catch (const std::exception& e) { g_herr = e.what(); return nullptr; }
}
void rth_renderer_destroy(RthRenderer* r) { if (r) { delete r->r; delete r; } }
int rth_renderer_init(RthRenderer* r) { GUARD(r->r->Init()) }
int rth_renderer_set_camera(RthRenderer* r, const float origin[3], const float forward[3], float fov, float aperture)
{
    try {
        CameraManager& c = r->r->camera;
        if (origin) c.cam.origin = RtFloat4{ origin[0], origin[1], origin[2], 0 };
        if (forward) c.cam.forward = RtFloat4{ forward[0], forward[1], forward[2], 0 };
        c.cam.fov = fov; c.cam.aperture = aperture; c.moved = true; c.UpdateCamVec();
        return 0;
    } catch (const std::exception& e) { g_herr = e.what(); return -1; }
}
int rth_renderer_tick(RthRenderer* r, int frames) { GUARD(for (int i = 0; i < frames; i++) r->r->Tick(0.0f)) }
int rth_renderer_read(RthRenderer* r, RtFloat4* out, float* energy)
{
    GUARD(if (out) r->r->ReadAccum(out); if (energy) { r->r->ComputeEnergy(); *energy = r->r->energy_total; })
}
int rth_renderer_camera(RthRenderer* r, RtCamera* out) { GUARD(*out = r->r->camera.cam) }

} // extern "C"

extern "C" int rth_load_model(RthScene* s, const char* filename, const char* defaultMaterial, const float pos[3], int forceDefaultMat)
{
    if (!s || !filename || !defaultMaterial) { g_herr = "rth_load_model: null argument"; return -1; }
    try { return s->scene.LoadModel(filename, defaultMaterial, pos ? f3(pos) : float3(0, 0, 0), forceDefaultMat != 0); }
    catch (const std::exception& e) { g_herr = e.what(); return -1; }
}
extern "C" int rth_save_png(const char* file, int w, int h, const RtFloat4* data)
{
    if (!file || !data || w <= 0 || h <= 0) { g_herr = "rth_save_png: bad argument"; return -1; }
    GUARD(SavePNG(file, w, h, data))
}
// Renderer input half that touches the path (renderer.cpp:310-365): camera controller, then Tick() resets the accumulator
extern "C" int rth_renderer_camera_move(RthRenderer* r, int camdir) { GUARD(r->r->camera.Move(camdir, 0.0f)) }
extern "C" int rth_renderer_camera_mouse(RthRenderer* r, float dx, float dy) { GUARD(r->r->camera.MouseMove(dx, dy)) }
extern "C" int rth_renderer_camera_zoom(RthRenderer* r, float offset) { GUARD(r->r->camera.Zoom(offset)) }
// sample streams behind the Renderer (before Init): Tick() then renders `lanes` frames whose kernels overlap (include/rt355.h, rt_group_*)
extern "C" int rth_renderer_set_lanes(RthRenderer* r, int lanes) { if (!r || lanes < 1 || lanes > 8) { g_herr = "rth_renderer_set_lanes: lanes must be 1..8"; return -1; } r->r->lanes = lanes; return 0; }
// arithmetic of the contexts Init() creates (before Init): RT_BUILTINS_* of include/rt355.h; anything else is refused here
extern "C" int rth_renderer_set_builtins(RthRenderer* r, int builtins)
{
    if (!r || (builtins != RT_BUILTINS_DEFAULT && builtins != RT_BUILTINS_IEEE && builtins != RT_BUILTINS_REFERENCE)) {
        g_herr = "rth_renderer_set_builtins: builtins must be RT_BUILTINS_DEFAULT (0), RT_BUILTINS_IEEE (1) or RT_BUILTINS_REFERENCE (2)";
        return -1;
    }
    r->r->builtins = builtins;
    return 0;
}
extern "C" int rth_renderer_builtins(RthRenderer* r) { return r ? r->r->builtins : -1; }
extern "C" int rth_renderer_frames(RthRenderer* r) { return r && r->r->settings ? r->r->settings->frames : -1; }
extern "C" int rth_renderer_save_frame(RthRenderer* r, const char* file) { GUARD(r->r->SaveFrame(file)) }

// seeds[i] = (first+i+1)-th xorshift32 output from 0x12345678 — the reference's host seed loop
// (src/renderer.cpp:195-196 over template/template.cpp:711,724-730).
extern "C" int rth_seed_stream(uint32_t* out, int64_t first, int64_t n)
{
    if (!out || first < 0 || n < 0) return -1;
    uint32_t s = 0x12345678u;
    auto next = [&s]() { s ^= s << 13; s ^= s >> 17; s ^= s << 5; return s; };
    for (int64_t i = 0; i < first; i++) next();
    for (int64_t i = 0; i < n; i++) out[i] = next();
    return 0;
}

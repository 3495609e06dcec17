// scene_rebuild.hip — the in-place changes of a bound scene copy that move its trees: rt_update_scene (refit, committed in place) and the
// one body of rt_rebuild_scene, rt_rebuild_ranges and rt_resize_scene, which builds into the set that is not live and commits by a
// pointer swap.  Host code only: the kernels are refit.hip's, rebuild.hip's, collapse.hip's and the builders' (sah.hip / lbvh.hip /
// sbvh.hip), the rules rebuild_common.h's; what it shares with the upload and the material updates is scene_dev.h's.
#include <cstdlib>
#include <string>
#include "scene_dev.h"
#include "resize_common.h"
#include "geometry_common.h"

using namespace scenedev;

// What an update and a rebuild refuse alike, before anything is written: `geo` replaces the primitives [first, first + count), `blas`
// (may be NULL) the instances.  typeSuffix ends the message about a changed objType / matIdx.
static int changed_type(const char* who, const SceneBag& b, size_t g, int32_t objType, int32_t matIdx, const char* typeSuffix)
{
    return fail(RT_E_INVALID, "%s: primitive %zu changes its objType / matIdx (%d / %d -> %d / %d)%s", who, g, b.primType[g], b.primMat[g], objType, matIdx, typeSuffix);
}
static int check_change(const char* who, const SceneBag& b, const Geometry& geo, const RtBVHInstance* blas, int32_t nBlas, const char* typeSuffix)
{
    // the geometry: what needs no device (geometry_common.h; a vertex form moves triangles only), then host records against the shadow
    // of objType / matIdx (records on the device are checked there: stage_geometry)
    std::string msg;
    if (const int rc = geometry::check_args(&geo.g, b.sc.nPrims, b.primType.data(), msg)) return fail(rc, "%s: %s", who, msg.c_str());
    const RtPrimitive* prims = geo.primsOnDevice ? nullptr : (const RtPrimitive*)geo.g.prims;
    for (int32_t i = 0; prims && i < geo.g.count; i++) {
        const size_t g = (size_t)geo.g.first + (size_t)i;
        if (prims[i].objType != b.primType[g] || prims[i].matIdx != b.primMat[g]) return changed_type(who, b, g, prims[i].objType, prims[i].matIdx, typeSuffix);
    }
    if (blas) {
        if (nBlas != b.sc.nBlas) return fail(RT_E_INVALID, "%s: %d instances given, %d uploaded", who, nBlas, b.sc.nBlas);
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

// The one place a call's replacement geometry reaches the device: fills the window of the staged primitives `dst` (the whole array; the
// device-to-device copy of the bound primitives into it has been queued on the copy's stream) from geo, which has passed check_change.
//   host records     the copy rt_update_scene has always queued, and nothing else
//   device records   a copy where they lie, then k_window_check against the bound records
//   vertices         k_tri_from_vertices over the staged records; host positions / indices go through scratch first
// The two device forms wait for their status word: a refusal found there returns before anything is derived from the window (dst is
// staging or the set that is not live: nothing bound has changed).
static int stage_geometry(const char* who, SceneBag& b, const Geometry& geo, RtPrimitive* dst, const char* typeSuffix)
{
    const RtGeometry& g = geo.g;
    if (g.count == 0) return RT_OK;
    hipStream_t s = b.stream;
    const size_t count = (size_t)g.count;
    RtPrimitive* const win = dst + g.first;
    if (g.prims && !geo.primsOnDevice) {
        HIPCHK(hipMemcpyAsync(win, g.prims, sizeof(RtPrimitive) * count, hipMemcpyHostToDevice, s));
        return RT_OK;
    }
    if (const int rc = rebuild_fit(b, b.gStatus, 1, "the geometry status word")) return rc;
    uint32_t bad = geometrydev::kNoBad;
    if (g.prims) {
        HIPCHK(hipMemcpyAsync(win, g.prims, sizeof(RtPrimitive) * count, hipMemcpyDefault, s));
        HIPCHK(geometrydev::window_check(s, win, b.sc.prims + g.first, (uint32_t)g.count, b.gStatus.p));
        HIPCHK(hipMemcpyAsync(&bad, b.gStatus.p, sizeof bad, hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));
        if (bad == geometrydev::kNoBad) return RT_OK;
        int32_t tm[2] = { 0, 0 };   // the one record's objType, matIdx
        HIPCHK(hipMemcpy(tm, &win[bad].objType, sizeof tm, hipMemcpyDeviceToHost));
        return changed_type(who, b, (size_t)g.first + bad, tm[0], tm[1], typeSuffix);
    }
    // the vertex form
    const float* positions = (const float*)g.positions;
    const uint32_t* indices = (const uint32_t*)g.indices;
    if (indices && !geo.indicesOnDevice) {
        if (const int rc = rebuild_fit(b, b.gIdx, 3 * count, "the geometry indices")) return rc;
        HIPCHK(hipMemcpyAsync(b.gIdx.p, indices, sizeof(uint32_t) * 3 * count, hipMemcpyHostToDevice, s));
        indices = b.gIdx.p;
    }
    if (!geo.positionsOnDevice && g.nVertices > 0) {
        const size_t bytes = (size_t)(g.nVertices - 1) * (size_t)g.positionStride + 12;   // to the last vertex's z
        if (const int rc = rebuild_fit(b, b.gPos, bytes, "the geometry positions")) return rc;
        HIPCHK(hipMemcpyAsync(b.gPos.p, positions, bytes, hipMemcpyHostToDevice, s));
        positions = (const float*)b.gPos.p;
    }
    HIPCHK(geometrydev::tri_from_vertices(s, win, (uint32_t)g.count, positions, g.positionStride, g.nVertices, indices, b.gStatus.p));
    HIPCHK(hipMemcpyAsync(&bad, b.gStatus.p, sizeof bad, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    if (bad == geometrydev::kNoBad) return RT_OK;
    uint32_t idx[3] = { 0, 0, 0 };   // (only a triangle with indices can be refused: check_change has counted the vertices otherwise)
    if (indices) HIPCHK(hipMemcpy(idx, indices + 3 * (size_t)bad, sizeof idx, hipMemcpyDefault));
    return fail(RT_E_INVALID, "%s: indices: %s", who, geometry::bad_index_message((int64_t)bad, idx, g.nVertices).c_str());
}

int scenedev::update_scene(SceneBag& b, const char* who, const Geometry& geo, const RtBVHInstance* blas, int32_t nBlas, RtUpdateStats* stats)
{
    const int32_t first = geo.g.first, count = geo.g.count;
    const SceneArrays& sc = b.sc;
    const LiveTrees& lt = b.live;
    const bool layout1 = b.facts.layout == 1;
    // ---- refusals: before anything is written
    if (b.refitRefusal) return fail(RT_E_UNSUPPORTED, "%s: %s", who, b.refitRefusal);
    if (const int rc = check_change(who, b, geo, blas, nBlas, ": topology must not change")) return rc;
    HIPCHK(hipSetDevice(b.device));
    // ---- staging buffers (the first update makes them; one after a resize that outgrew them replaces them)
    if (const int rc = scene_stream(b, b.ev)) return rc;   // (a rebuild may have made the stream already)
    {
        int rc = rebuild_fit(b, b.sPrims, (size_t)sc.nPrims, "the staging primitives");
        if (rc == RT_OK) rc = rebuild_fit(b, b.sInst, (size_t)sc.nBlas, "the staging instances");
        if (rc == RT_OK) rc = rebuild_fit(b, b.sTlas, (size_t)lt.nTlas, "the staging TLAS");
        if (rc == RT_OK) rc = rebuild_fit(b, b.sTp, (size_t)lt.nTlas * 4, "the staging TLAS records");
        if (rc == RT_OK) rc = rebuild_fit(b, b.sTpP, (size_t)lt.nTlas * 4, "the staging TLAS records");
        if (rc == RT_OK) rc = rebuild_fit(b, b.sIr, (size_t)sc.nBlas * 4, "the staging instance records");
        if (rc == RT_OK && !b.sStatus) { rc = dalloc(b.allocs, &b.sStatus, 2); if (rc == RT_OK) b.rallocs++; }
        if (rc != RT_OK) return rc;
    }
    if (!b.sNodes.p || (size_t)lt.nNodes > b.sNodes.cap) {
        // the staging nodes: at first room for every tree the SAH and the linear builder can bind later; an SBVH rebuild may bind more
        // nodes than that, then the array grows as the rebuild's sets do (nothing in it outlives a call)
        const size_t n = (size_t)lt.nNodes, cap = b.sNodes.p ? with_headroom(n) : std::max(n, 2 * rebuild_initial_cap(b));
        if (const int rc = rebuild_grow(b, b.sNodes, cap, 0, "the staging nodes", "rt_update_scene: %zu staging nodes")) return rc;
    }
    hipStream_t s = b.stream;
    // ---- stage: the new primitives, the refit tree and the rebuilt TLAS in scratch
    HIPCHK(hipEventRecord(b.ev[0], s));
    HIPCHK(hipMemcpyAsync(b.sPrims.p, sc.prims, sizeof(RtPrimitive) * (size_t)sc.nPrims, hipMemcpyDeviceToDevice, s));
    if (const int rc = stage_geometry(who, b, geo, b.sPrims.p, ": topology must not change")) return rc;
    HIPCHK(hipMemcpyAsync(b.sNodes.p, sc.bvh2, sizeof(RtBVHNode2) * (size_t)lt.nNodes, hipMemcpyDeviceToDevice, s));
    if (blas) HIPCHK(hipMemcpyAsync(b.sInst.p, blas, sizeof(RtBVHInstance) * (size_t)sc.nBlas, hipMemcpyHostToDevice, s));
    else HIPCHK(hipMemcpyAsync(b.sInst.p, sc.blas, sizeof(RtBVHInstance) * (size_t)sc.nBlas, hipMemcpyDeviceToDevice, s));
    HIPCHK(refitdev::launch_refit(s, b.sNodes.p, lt.nNodes, b.sPrims.p, sc.primIdx, lt.leaves, lt.nLeaves, lt.parent, lt.tickets));
    HIPCHK(refitdev::launch_tlas(s, b.sNodes.p, b.sInst.p, sc.nBlas, layout1 ? sc.rootEntry : nullptr, b.sTlas.p, b.sTp.p, b.sTpP.p, b.sIr.p, b.sStatus));
    int32_t status[2] = { 0, 0 };
    HIPCHK(hipEventRecord(b.ev[1], s));
    HIPCHK(hipMemcpyAsync(status, b.sStatus, sizeof status, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    if (const int rc = tlas_status_error(who, status)) return rc;
    // ---- commit: no kernel of a context holding this copy may read the arrays while they are rewritten
    if (const int rc = b.wait_holders()) return rc;
    HIPCHK(hipEventRecord(b.ev[2], s));
    if (count) HIPCHK(hipMemcpyAsync(sc.prims + first, b.sPrims.p + first, sizeof(RtPrimitive) * (size_t)count, hipMemcpyDeviceToDevice, s));
    HIPCHK(hipMemcpyAsync(sc.bvh2, b.sNodes.p, sizeof(RtBVHNode2) * (size_t)lt.nNodes, hipMemcpyDeviceToDevice, s));
    HIPCHK(hipMemcpyAsync(sc.blas, b.sInst.p, sizeof(RtBVHInstance) * (size_t)sc.nBlas, hipMemcpyDeviceToDevice, s));
    HIPCHK(hipMemcpyAsync(sc.tlas, b.sTlas.p, sizeof(RtTLASNode) * (size_t)lt.nTlas, hipMemcpyDeviceToDevice, s));
    HIPCHK(hipMemcpyAsync(sc.tlasPairs, b.sTp.p, sizeof(RtFloat4) * 4 * (size_t)lt.nTlas, hipMemcpyDeviceToDevice, s));
    HIPCHK(hipMemcpyAsync(sc.tlasPairsP, b.sTpP.p, sizeof(RtFloat4) * 4 * (size_t)lt.nTlas, hipMemcpyDeviceToDevice, s));
    HIPCHK(hipMemcpyAsync(sc.instRecs, b.sIr.p, sizeof(RtFloat4) * 4 * (size_t)sc.nBlas, hipMemcpyDeviceToDevice, s));
    HIPCHK(refitdev::launch_records(s, sc.prims, sc.bvh2, sc.primIdx, lt.nIdx, sc.lights, (uint32_t)sc.nLights, (uint32_t)std::max(first, 0), (uint32_t)count,
                                    lt.pairNode, lt.nPairs, layout1 ? sc.pairs : nullptr, layout1 ? sc.triRecs : nullptr, sc.shadeRecs, sc.lightRecs));
    HIPCHK(hipEventRecord(b.ev[3], s));
    HIPCHK(hipStreamSynchronize(s));
    if (blas) b.inst.assign(blas, blas + nBlas);
    const bool reconfigure = status[1] != b.facts.tlasDepth;
    if (reconfigure) { b.facts.tlasDepth = status[1]; b.generation++; }
    if (stats) {
        float ms = 0, ms2 = 0;   // GPU time of both phases (not the wait for the holders in between)
        (void)hipEventElapsedTime(&ms, b.ev[0], b.ev[1]); (void)hipEventElapsedTime(&ms2, b.ev[2], b.ev[3]);
        ms += ms2;
        *stats = RtUpdateStats{};
        stats->gpu_ms = ms; stats->prims = count; stats->nodes = (int32_t)lt.nReach; stats->tlas_nodes = lt.nTlas; stats->tlas_depth = status[1];
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
    const size_t idxCap = grown_cap(idxNeed, t.primIdx.cap, have), nodeCap = (grown_cap(nodeNeed, t.nodes.cap, have) + 1) & ~(size_t)1;
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
// The lights' arrays of the set `t` (not live): one record at least, as at upload
static int reserve_lights(SceneBag& b, SceneBag::RebuildSet& t, size_t nLights)
{
    const int rc = rebuild_fit(b, t.lights, nLights, "the light list");
    return rc != RT_OK ? rc : rebuild_fit(b, t.lightRecs, std::max<size_t>(nLights, 1) * 8, "light records");
}
// Room in the set `t` (not live) for a scene of nPrims primitives, nBlas instances and the trees `next` describes so far (its ranges, its TLAS)
static int rebuild_alloc(SceneBag& b, SceneBag::RebuildSet& t, int32_t nPrims, int32_t nBlas, const LiveTrees& next, bool resize)
{
    const size_t nP = (size_t)nPrims, nB = (size_t)nBlas, nT = next.nTlas, nL = (size_t)b.sc.nLights;
    int rc = RT_OK;
    // every piece is made on its own: a call that ran out of memory half way is taken up where it stopped
    auto need = [&](auto** p, size_t count) { if (rc == RT_OK && !*p) { rc = dalloc(b.allocs, p, count); if (rc == RT_OK) b.rallocs++; } };
    if ((rc = scene_stream(b, b.rev)) != RT_OK) return rc;
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
    if (rc == RT_OK && !resize) rc = rebuild_fit(b, t.lightRecs, std::max<size_t>(nL, 1) * 8, "light records");
    if (rc == RT_OK && !resize && b.lightsInSet) rc = rebuild_fit(b, t.lights, nL, "the light list");
    // ... and with the trees (the first allocation: the initial capacity)
    if (rc == RT_OK && !t.nodes.p) rc = rebuild_reserve(b, t, next.ranges.size(), std::max(cap0, t.primIdx.cap), std::max(2 * cap0, t.nodes.cap), 0, 0);
    return rc;
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
// The builders' own argument checks, BLAS by BLAS under plan[k], one RT_REBUILD_SAH / LBVH / SBVH / KEEP / REFIT_RANGE per range (node and index
// ids as the host appends BLAS after BLAS: a kept or refit BLAS takes its block's - blocks NULL: a SAH tree's at most - and the ids behind an SBVH tree
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

// ---- the one body of rt_rebuild_scene, rt_rebuild_ranges and rt_resize_scene, phase by phase ----------------------------------------------
// What a call asks for; it has passed the checks that need no device.  A rebuild (newPrims NULL) keeps the bound counts and ranges and takes
// the replacement geometry geo and blas as rt_update_scene does; a resize builds the caller's shape - nPrims records at
// newPrims (host or device memory), nBlas instances, newRanges, newInstBlas - with blas (NULL: identity) carrying the transforms.  plan[k]
// says what becomes of range k: built with RT_REBUILD_SAH / LBVH / SBVH, or (RT_REBUILD_KEEP, a rebuild of a compact bound tree only) its
// bound tree moved to where the new scene numbers it, or (RT_REBUILD_REFIT_RANGE, likewise) moved and then given new boxes; an empty plan is
// RT_REBUILD_REFIT of the whole scene (no builder runs, opts is ignored).  perRange: the call is rt_rebuild_ranges (rt_ranges_info describes it).
namespace {
struct Request {
    const char* who;
    int32_t nPrims, nBlas;
    const void* newPrims;
    Geometry geo;
    const RtBVHInstance* blas;
    std::vector<int32_t> plan;
    const RtBuildOptions* opts;
    lbvh::Params P;
    bool perRange = false;
    std::vector<rebuild::BlasRange> newRanges;   // a resize: the primitive range of every distinct BLAS, in increasing order ...
    std::vector<int32_t> newInstBlas;            // ... and instance -> its range
};
// One call: the trees (`next`), the facts and the host shadows of the scene it builds in the set that is not live - everything commit moves
// into the bag - and the phases that build them, in the order rebuild_body calls them
struct Pending {
    SceneBag& b;
    const Request& rq;
    const char* const who = rq.who;
    const int32_t nPrims = rq.nPrims, nBlas = rq.nBlas;
    const bool resize = rq.newPrims != nullptr, refit = rq.plan.empty(), bvh4 = b.accel == RT_ACCEL_BVH4, layout1 = b.facts.layout == 1;
    SceneBag::RebuildSet& t = b.rset[b.rnext];
    // The next live trees: a rebuild starts from the bound ones (a whole-scene refit leaves all but the pointers), a resize from the
    // caller's ranges.  place() writes the roots and the blocks, derive_ids() the runs, read_back() the set's pointers and the collapse's
    LiveTrees next = start();
    const size_t nR = next.ranges.size();
    SceneFacts facts = b.facts;                  // (the layout stays: read_back refuses a change)
    std::vector<int32_t> primType, primMat;      // a resize: the host's shadow of objType / matIdx, the only per-primitive data that comes back
    std::vector<RtBVHInstance> inst;
    LiveTrees start() const
    {
        LiveTrees n;
        if (!resize) n = b.live;
        else { n.ranges = rq.newRanges; n.instBlas = rq.newInstBlas; n.nTlas = 2 * (uint32_t)nBlas; }   // (TLAS::Build's node count)
        if (!refit) { n.nNodes = n.nIdx = n.nPairs = 0; n.block.assign(n.ranges.size(), rebuild::BlasBlock{}); }
        return n;
    }
    int size();                  // 1. room for what the plan is known to need, the builders' workspace
    int stage();                 // 2. the primitives and the lights
    int trees();                 // 3. refit copy, kept segments, builders
    int derive();                // 4. numbering, collapse, records, TLAS
    int read_back(bool timed);   // 5. ... and refuse: walk, collapse, TLAS, layout
    void commit();               // 6. host memory only
    struct KeptSegment { uint32_t srcNode = 0, dstNode = 0, nNodes = 0, nodeDelta = 0, srcIdx = 0, dstIdx = 0, nIdx = 0, idxDelta = 0; };
    int stage_resize(), stage_rebuild(), refit_trees(), flush_kept(KeptSegment& seg), keep_tree(size_t k, KeptSegment& seg), build_tree(size_t k);
    int derive_ids(), derive_records();
    // range k keeps its bound tree as a block: kept, or refit (new boxes afterwards)
    bool refits(size_t k) const { return !refit && rq.plan[k] == RT_REBUILD_REFIT_RANGE; }
    bool moves(size_t k) const { return !refit && (rq.plan[k] == RT_REBUILD_KEEP || rq.plan[k] == RT_REBUILD_REFIT_RANGE); }
    // A BVH2 copy with a block that moves takes the derived data of such blocks from the bound arrays and derives the built ranges'
    // alone.  (Not a copy bound in layout 0 that could take layout 1: the layout check needs every leaf's size, which only the leaf scan
    // over all ranges gives.  Not a BVH4 copy: its collapse is derived over all ranges.)
    bool blockwise = false;
    std::vector<uint32_t> hostRoots;                    // per instance: its root entry
    RtRangesInfo info{};                                // counted as the launches are queued

    using clock = std::chrono::steady_clock;
    clock::time_point t0 = clock::now(), t1, t2, t3;   // the call, staged, trees built, read back
    // size: what the ranges behind range k need that is known beforehand, and the BLAS in the order the instances first name them
    std::vector<size_t> restIdx, restNodes, order;
    bool anyKnown = false;
    // the lights of the new scene, and where their list lies
    int32_t nLights = 0;
    const uint32_t* lights = nullptr;
    uint32_t maxDepth = 0;
    int32_t nBuilt = 0;
    uint64_t spatialSplits = 0, primsClipped = 0;
    // read back: k_tlas_build's status, the derivation's walk status and largest leaf, the collapse's status
    int32_t tlas[2] = { 0, 0 };
    uint32_t walk[2] = { 0, 0 }, changed = 0;
    CollapseStatus c4;
    int32_t refitPath = 0;
    int stackNeed = 0;
    float gpuMs = 0, fitMs = 0, deriveMs = 0, tlasMs = 0;   // between the events (read for stats only)
    bool reconfigured = false;
    // range k has a tree of `nodes` nodes, height `height`, over `slots` index slots: behind the trees placed so far, one block
    void place(size_t k, uint32_t nodes, uint32_t height, uint32_t slots)
    {
        next.ranges[k].root = next.nNodes;
        next.block[k] = rebuild::BlasBlock{ nodes, next.nIdx, slots, 1, height };
        maxDepth = std::max(maxDepth, height);
        next.nNodes += nodes; next.nIdx += slots;
    }
};
} // namespace

// 1. Size: room in the set that is not live for what the plan is known to need, and the builders' workspace
int Pending::size()
{
    // a kept or refit tree needs its block, a SAH or LBVH tree count slots and 2 * count - 1 nodes at most (an SBVH tree is sized when it is
    // built: size, then place)
    restIdx.assign(nR + 1, 0); restNodes.assign(nR + 1, 0);
    for (size_t k = nR; k-- > 0 && !refit;) {
        const bool keep = moves(k), known = keep || rq.plan[k] != RT_REBUILD_SBVH;
        restIdx[k] = restIdx[k + 1] + (keep ? b.live.block[k].idxSlots : known ? next.ranges[k].count : 0u);
        restNodes[k] = restNodes[k + 1] + (keep ? b.live.block[k].nodes : known ? 2 * (size_t)next.ranges[k].count - 1 : 0u);
        anyKnown = anyKnown || known;
    }
    std::vector<uint8_t> named(nR, 0);
    for (const int32_t k : next.instBlas) if (!named[(size_t)k]) { named[(size_t)k] = 1; order.push_back((size_t)k); }
    HIPCHK(hipSetDevice(b.device));
    if (const int rc = rebuild_alloc(b, t, nPrims, nBlas, next, resize)) return rc;
    if (refit) return rebuild_reserve(b, t, nR, (size_t)next.nIdx, (size_t)next.nNodes + nR, 0, 0);   // the bound trees (nR spare nodes: see build_tree)
    if (!anyKnown) return RT_OK;
    // room for the kept trees and for every tree the SAH and the linear builder can make (a set or the scratch that started smaller, or
    // has only held SBVH trees so far); nR spare nodes: see build_tree.  With every range built by those two this is nPrims slots and
    // 2 * nPrims nodes for ranges that tile the primitives
    if (restIdx[0] > 0x7fffffffull || restNodes[0] + nR > 0x7fffffffull) return too_many_nodes(who);
    if (const int rc = rebuild_reserve(b, t, nR, restIdx[0], restNodes[0] + nR, 0, 0)) return rc;
    size_t need = 0;   // the builders' workspace, over the ranges they build
    for (size_t k = 0; k < nR; k++) {
        if (rq.plan[k] != RT_REBUILD_SAH && rq.plan[k] != RT_REBUILD_LBVH) continue;
        size_t bytes = 0;
        const int rc = rq.plan[k] == RT_REBUILD_SAH ? sahdev::work_bytes(who, next.ranges[k].count, b.stream, &bytes) : lbvhdev::work_bytes(who, next.ranges[k].count, b.stream, &bytes);
        if (rc != RT_OK) return rc;
        need = std::max(need, bytes);
    }
    if (need > b.rwork.cap) return rebuild_grow(b, b.rwork, need, 0, "the builders' workspace", "in-place scene change: %zu bytes of builder workspace");
    return RT_OK;
}

// 2. Stage: the new primitives and the lights into the set that is not live
int Pending::stage() { return resize ? stage_resize() : stage_rebuild(); }
// A resize: check, scan, emit - one path for host and device input: copied first (the set is not live, so checking after the copy is
// safe), then checked where it lies; the light list and the light records come from the same pass
int Pending::stage_resize()
{
    const SceneArrays& sc = b.sc;
    hipStream_t s = b.stream;
    if (const int rc = rebuild_scratch(b, (size_t)nPrims)) return rc;   // (flags and ranks: a word per primitive)
    if (const int rc = rebuild_fit(b, b.rPacked, (size_t)nPrims, "the packed objType / matIdx pairs")) return rc;
    HIPCHK(hipMemcpyAsync(t.prims.p, rq.newPrims, sizeof(RtPrimitive) * (size_t)nPrims, hipMemcpyDefault, s));
    HIPCHK(rebuilddev::resize_check(s, b.dw, t.prims.p, (uint32_t)nPrims, sc.mats, sc.nMats, b.rPacked.p, (uint32_t*)b.rStatus));
    uint32_t firstBad = resize::kNoBad;
    if (const int rc = flag_scan_result(b, nPrims, &firstBad, &nLights)) return rc;
    if (firstBad != resize::kNoBad) {
        int2 pm{ 0, 0 };
        HIPCHK(hipMemcpy(&pm, b.rPacked.p + firstBad, sizeof pm, hipMemcpyDeviceToHost));
        return fail(RT_E_INVALID, "%s: primitive %u: objType %d / matIdx %d out of range (objType: one of RT_PRIM_*, matIdx: [0, %d)); the scene is unchanged", who,
                    firstBad, pm.x, pm.y, sc.nMats);
    }
    if (const int rc = reserve_lights(b, t, (size_t)nLights)) return rc;
    HIPCHK(rebuilddev::light_emit(s, b.dw, t.prims.p, (uint32_t)nPrims, sc.mats, (uint32_t)nLights, t.lights.p, t.lightRecs.p));
    lights = t.lights.p;
    return RT_OK;
}
// A rebuild: copy, window, carry the lights
int Pending::stage_rebuild()
{
    const SceneArrays& sc = b.sc;
    hipStream_t s = b.stream;
    HIPCHK(hipMemcpyAsync(t.prims.p, sc.prims, sizeof(RtPrimitive) * (size_t)sc.nPrims, hipMemcpyDeviceToDevice, s));
    if (const int rc = stage_geometry(who, b, rq.geo, t.prims.p, "")) return rc;
    HIPCHK(hipMemcpyAsync(t.lightRecs.p, sc.lightRecs, sizeof(RtFloat4) * 8 * std::max<size_t>((size_t)sc.nLights, 1), hipMemcpyDeviceToDevice, s));   // (the emittance words stay)
    nLights = sc.nLights; lights = sc.lights;
    if (b.lightsInSet) {   // the light list lives in a set since a resize: it moves on with the arrays
        if (nLights) HIPCHK(hipMemcpyAsync(t.lights.p, sc.lights, sizeof(uint32_t) * (size_t)nLights, hipMemcpyDeviceToDevice, s));
        lights = t.lights.p;
    }
    return RT_OK;
}

// 3. The trees, in the order of the ranges.  A refit of the whole scene: the bound trees and their refit topology into the set, then the boxes anew: no BLAS
// is built, so node ids, leaf ranges, primIdx and pair ids stay
int Pending::refit_trees()
{
    const SceneArrays& sc = b.sc;
    hipStream_t s = b.stream;
    HIPCHK(hipMemcpyAsync(t.nodes.p, sc.bvh2, sizeof(RtBVHNode2) * (size_t)next.nNodes, hipMemcpyDeviceToDevice, s));
    HIPCHK(hipMemcpyAsync(t.primIdx.p, sc.primIdx, sizeof(uint32_t) * (size_t)next.nIdx, hipMemcpyDeviceToDevice, s));
    HIPCHK(hipMemcpyAsync(t.parent.p, b.live.parent, sizeof(uint32_t) * (size_t)next.nNodes, hipMemcpyDeviceToDevice, s));
    if (next.nLeaves) HIPCHK(hipMemcpyAsync(t.leaves.p, b.live.leaves, sizeof(uint32_t) * (size_t)next.nLeaves, hipMemcpyDeviceToDevice, s));
    if (next.nPairs) HIPCHK(hipMemcpyAsync(t.pairNode.p, b.live.pairNode, sizeof(uint32_t) * (size_t)next.nPairs, hipMemcpyDeviceToDevice, s));
    HIPCHK(refitdev::launch_refit(s, t.nodes.p, next.nNodes, t.prims.p, t.primIdx.p, t.leaves.p, next.nLeaves, t.parent.p, t.tickets.p));
    for (const rebuild::BlasBlock& blk : next.block) maxDepth = std::max(maxDepth, blk.height);
    return RT_OK;
}
// Kept trees move as segments: adjacent kept BLAS whose node and index offsets agree are one (rebuilddev::relocate), and their primIdx
// slots, whose values are global primitive ids of a range that did not move, one plain copy.  A segment is queued when the next range
// does not extend it, so before anything else touches the set.
int Pending::flush_kept(KeptSegment& seg)
{
    if (!seg.nNodes) return RT_OK;
    HIPCHK(rebuilddev::relocate(b.stream, b.sc.bvh2 + seg.srcNode, t.nodes.p + seg.dstNode, seg.nNodes, seg.nodeDelta, seg.idxDelta));
    HIPCHK(hipMemcpyAsync(t.primIdx.p + seg.dstIdx, b.sc.primIdx + seg.srcIdx, sizeof(uint32_t) * (size_t)seg.nIdx, hipMemcpyDeviceToDevice, b.stream));
    seg = KeptSegment{};
    return RT_OK;
}
// range k keeps its bound tree, to stay as it is or to be refit once its leaves and parent links are in the set (derive): room is
// reserved by size(); the bound values stand for the builder's
int Pending::keep_tree(size_t k, KeptSegment& seg)
{
    const rebuild::BlasBlock& blk = b.live.block[k];
    const uint32_t root = b.live.ranges[k].root, nodeDelta = next.nNodes - root, idxDelta = next.nIdx - blk.idxLo;
    if (seg.nNodes && seg.nodeDelta == nodeDelta && seg.idxDelta == idxDelta && seg.srcNode + seg.nNodes == root && seg.srcIdx + seg.nIdx == blk.idxLo) {
        seg.nNodes += blk.nodes; seg.nIdx += blk.idxSlots;
    } else {
        if (const int rc = flush_kept(seg)) return rc;
        seg = KeptSegment{ root, next.nNodes, blk.nodes, nodeDelta, blk.idxLo, next.nIdx, blk.idxSlots, idxDelta };
    }
    place(k, blk.nodes, blk.height, blk.idxSlots);
    if (!refits(k)) info.kept++;
    return RT_OK;
}
// range k is built by plan[k], behind the trees placed so far
int Pending::build_tree(size_t k)
{
    const rebuild::BlasRange& r = next.ranges[k];
    const bool sbvh = rq.plan[k] == RT_REBUILD_SBVH;
    hipStream_t s = b.stream;
    Built built{};
    uint32_t slots = r.count;
    if (sbvh) {
        // size, then place: the tree stays in the builder's own memory until the set has room for it (one tree at a time)
        struct TreeGuard { sbvhdev::Tree* p = nullptr; ~TreeGuard() { sbvhdev::destroy(p); } } tree;
        SbvhBuilt sb{};
        const float alpha = rq.opts ? rq.opts->alpha : 0.0f;   // (check_builder has seen it)
        if (const int rc = sbvhdev::build(who, s, alpha, t.prims.p + r.first, r.count, r.first, next.nNodes, next.nIdx, nullptr, nullptr, b.spool, &tree.p, &sb)) return rc;
        // room for this tree and for what the ranges behind it are known to need (nR spare nodes: the leaf and pair arrays hold half the
        // node capacity, and k trees have k leaves more than interior nodes)
        const uint64_t nodeNeed = (uint64_t)next.nNodes + sb.nodes + restNodes[k + 1] + nR, idxNeed = (uint64_t)next.nIdx + sb.nIdx + restIdx[k + 1];
        if (sb.nIdx == 0 || nodeNeed > 0x7fffffffull || idxNeed > 0x7fffffffull) return too_many_nodes(who);
        if (const int rc = rebuild_reserve(b, t, nR, (size_t)idxNeed, (size_t)nodeNeed, next.nIdx, next.nNodes)) return rc;
        if (const int rc = sbvhdev::emit(who, s, tree.p, t.nodes.p + next.nNodes, t.primIdx.p + next.nIdx)) return rc;
        built.nodes = sb.nodes; built.depth = sb.depth; slots = sb.nIdx;
        spatialSplits += sb.spatialSplits; primsClipped += sb.primsClipped;
    } else {
        const int rc = rq.plan[k] == RT_REBUILD_SAH
            ? sahdev::build(who, s, b.rwork.p, t.prims.p + r.first, r.count, r.first, next.nNodes, next.nIdx, t.nodes.p + next.nNodes, t.primIdx.p + next.nIdx, nullptr, nullptr, &built)
            : lbvhdev::build(who, s, b.rwork.p, rq.P, t.prims.p + r.first, r.count, r.first, next.nNodes, next.nIdx, t.nodes.p + next.nNodes, t.primIdx.p + next.nIdx, nullptr, nullptr, &built);
        if (rc != RT_OK) return rc;
    }
    if (built.nodes == 0 || (built.nodes & 1u) == 0 || (!sbvh && built.nodes > 2 * r.count - 1))
        return fail(RT_E_DEVICE, "%s: inconsistent builder result (%u nodes for %u primitives)", who, built.nodes, r.count);
    if ((built.depth == 0) != (built.nodes == 1))
        return fail(RT_E_DEVICE, "%s: inconsistent builder result (height %u with %u nodes)", who, built.depth, built.nodes);
    if (rebuild::exceeds_stack(built.depth))   // validate_scene's rule
        return fail(RT_E_UNSUPPORTED, "%s: the new BLAS %zu needs %u stack entries, at most %d are supported; the scene is unchanged", who, k,
                    built.depth, RT_BVH4_STACK);
    nBuilt++;
    place(k, built.nodes, built.depth, slots);
    return RT_OK;
}
int Pending::trees()
{
    if (refit) {
        if (const int rc = refit_trees()) return rc;
    } else {
        KeptSegment seg;
        for (size_t k = 0; k < nR; k++) {
            if (moves(k)) { if (const int rc = keep_tree(k, seg)) return rc; blockwise = !bvh4 && (layout1 || !b.variantLayout1); continue; }
            if (const int rc = flush_kept(seg)) return rc;
            if (const int rc = build_tree(k)) return rc;
        }
        if (const int rc = flush_kept(seg)) return rc;
        if (const int rc = rebuild_scratch(b, (size_t)next.nNodes + nR)) return rc;
    }
    return bvh4 ? collapse_scratch(b, (size_t)next.nNodes + nR) : RT_OK;
}

// 4. Derive: the instances (host: at most 256 records), then everything upload derives: numbering, collapse, records, TLAS
int Pending::derive()
{
    const SceneArrays& sc = b.sc;
    hipStream_t s = b.stream;
    if (rq.blas) inst.assign(rq.blas, rq.blas + nBlas);
    else if (!resize) inst = b.inst;
    else {   // a resize without transforms: BuildBLAS's identity
        inst.assign((size_t)nBlas, RtBVHInstance{});
        for (RtBVHInstance& r : inst) r.invT[0] = r.invT[5] = r.invT[10] = r.invT[15] = 1.0f;
    }
    for (int32_t i = 0; i < nBlas; i++) inst[(size_t)i].bvhIdx = next.ranges[(size_t)next.instBlas[(size_t)i]].root;
    HIPCHK(hipMemcpyAsync(t.blas.p, inst.data(), sizeof(RtBVHInstance) * (size_t)nBlas, hipMemcpyHostToDevice, s));
    HIPCHK(hipEventRecord(b.rev[1], s));
    if (refit) {   // the pair records (launch_records rewrites their boxes) and the root entries as they are bound
        if (layout1 && !bvh4) {
            HIPCHK(hipMemcpyAsync(t.pairs.p, sc.pairs, sizeof(RtFloat4) * 4 * std::max<size_t>(next.nPairs, 1), hipMemcpyDeviceToDevice, s));
            HIPCHK(hipMemcpyAsync(t.rootEntry.p, sc.rootEntry, sizeof(uint32_t) * (size_t)b.sc.nBlas, hipMemcpyDeviceToDevice, s));
        }
    } else if (const int rc = derive_ids()) return rc;
    if (layout1 && !bvh4 && next.nPairs == 0) HIPCHK(hipMemsetAsync(t.pairs.p, 0, sizeof(RtFloat4) * 4, s));   // no interior node: one zero record, as at upload
    if (!refit) { next.nLeaves = next.nNodes - next.nPairs; next.nReach = next.nNodes; }
    refitPath = refit ? 1 : 0;
    if (bvh4) {   // the collapse into the set's bvh4, BLAS by BLAS in the same order; quad records and root entries (layout 1)
        const collapsedev::Work w = collapse_work(b, t.newId.p, t.quadNode.p, std::min(t.quadNode.cap, t.quads.cap / 8));
        HIPCHK(collapsedev::begin(s, w, t.nodes.p, next.nNodes, t.bvh4.p));
        if (refit) {
            // in place: the live records anew under the bound live ids (the set takes the bound tables over); if no slot of any of
            // them changed, they are the collapse of the refit trees and the level loop is skipped
            HIPCHK(hipMemcpyAsync(t.newId.p, b.live.newId, sizeof(uint32_t) * (size_t)next.nNodes, hipMemcpyDeviceToDevice, s));
            HIPCHK(hipMemcpyAsync(t.quadNode.p, b.live.quadNode, sizeof(uint32_t) * (size_t)b.live.nLive, hipMemcpyDeviceToDevice, s));
            HIPCHK(collapsedev::refit_records(s, w, t.nodes.p, next.nNodes, sc.bvh4, t.quadNode.p, b.live.nLive, t.bvh4.p));
            HIPCHK(c4.read(s, w));
            HIPCHK(hipStreamSynchronize(s));
            if (const int rc = c4.error(who, "; the scene is unchanged")) return rc;
            changed = c4.changed();
            const char* env = getenv("RT355_REFIT_RECOLLAPSE");
            refitPath = env && atoi(env) == 1 ? 3 : changed ? 2 : 1;
            if (refitPath != 1) HIPCHK(collapsedev::begin(s, w, t.nodes.p, next.nNodes, t.bvh4.p));   // the fallback: the rebuild's collapse
        }
        if (refitPath != 1)
            for (const size_t k : order) HIPCHK(collapsedev::collapse_blas(s, w, t.nodes.p, next.nNodes, next.ranges[k].root, next.interiors(k), next.block[k].height, t.bvh4.p));
        HIPCHK(collapsedev::finish(s, w, t.bvh4.p, next.nNodes, next.nIdx, (const uint32_t*)t.blas.p, (uint32_t)(sizeof(RtBVHInstance) / 4), (uint32_t)nBlas,
                                   layout1 ? t.quads.p : nullptr, t.rootEntry.p));
    }
    if (const int rc = derive_records()) return rc;
    HIPCHK(hipEventRecord(b.rev[2], s));
    HIPCHK(refitdev::launch_tlas(s, t.nodes.p, t.blas.p, nBlas, layout1 ? t.rootEntry.p : nullptr, t.tlas.p, t.tp.p, t.tpP.p, t.ir.p, b.rStatus));
    HIPCHK(hipEventRecord(b.rev[3], s));
    return RT_OK;
}

// The pair ids, the refit topology and the pair records of a call that is no whole-scene refit.  Pair ids go BLAS by BLAS in the order in
// which the instances first name them, the leaf list range by range (node order).  Without a block that moves (rt_rebuild_scene,
// rt_resize_scene, an all-built plan) and on the copies `blockwise` leaves out: number every BLAS, then one finish over all ranges.
// Otherwise a BLAS that moves has its runs taken from the bound arrays by the offsets of its block, a built one is numbered and finished
// on its own, and the root entries are host arithmetic.  Then the refit ranges' boxes, once their leaves and parent links are in the set.
int Pending::derive_ids()
{
    const SceneArrays& sc = b.sc;
    hipStream_t s = b.stream;
    RtFloat4* const pairs = layout1 && !bvh4 ? t.pairs.p : nullptr;
    next.pairLo.assign(nR, 0u); next.leafLo.assign(nR, 0u);
    for (size_t k = 0, at = 0; k < nR; k++) { next.leafLo[k] = (uint32_t)at; at += next.interiors(k) + 1; }
    HIPCHK(rebuilddev::begin(s, b.dw, t.parent.p, next.nNodes));
    for (const size_t k : order) {
        const uint32_t m = 2 * next.interiors(k) + 1;
        next.pairLo[k] = next.nPairs;
        if (blockwise && moves(k)) {
            const uint32_t oldRoot = b.live.ranges[k].root, oldPair = b.live.pairLo[k];
            HIPCHK(rebuilddev::relocate_ids(s, b.live.parent + oldRoot, t.parent.p + next.ranges[k].root, m, b.live.pairNode + oldPair, t.pairNode.p + next.nPairs, pairs ? next.interiors(k) : 0u,
                                            b.live.leaves + b.live.leafLo[k], t.leaves.p + next.leafLo[k], next.interiors(k) + 1, next.ranges[k].root - oldRoot));
            if (pairs) {
                HIPCHK(rebuilddev::relocate_pairs(s, sc.pairs + (size_t)oldPair * 4, pairs + (size_t)next.nPairs * 4, next.interiors(k), next.nPairs - oldPair, next.block[k].idxLo - b.live.block[k].idxLo));
                info.pairs_relocated += (int32_t)next.interiors(k);
            }
        } else {
            HIPCHK(rebuilddev::number_blas(s, b.dw, t.nodes.p, next.nNodes, next.ranges[k].root, next.interiors(k), next.block[k].height, next.nPairs, (uint32_t)t.pairNode.cap, t.pairNode.p, t.parent.p));
            info.nodes_numbered += (int32_t)m;
            if (blockwise) {
                HIPCHK(rebuilddev::finish_blas(s, b.dw, t.nodes.p, next.ranges[k].root, m, next.nPairs, next.interiors(k), t.pairNode.p, pairs, t.leaves.p + next.leafLo[k]));
                if (pairs) info.pairs_derived += (int32_t)next.interiors(k);
            }
        }
        next.nPairs += next.interiors(k);
    }
    if (!blockwise) {
        HIPCHK(rebuilddev::finish(s, b.dw, t.nodes.p, next.nNodes, next.nPairs, next.nNodes - next.nPairs, t.blas.p, (uint32_t)nBlas, t.pairNode.p, pairs, t.rootEntry.p, t.leaves.p));
        if (pairs) info.pairs_derived += (int32_t)next.nPairs;
    } else if (pairs) {   // a leaf root: the leaf entry at its index base; otherwise the start of its run of pair ids (the root is the walk's first node)
        hostRoots.resize((size_t)nBlas);
        for (int32_t i = 0; i < nBlas; i++) {
            const size_t k = (size_t)next.instBlas[(size_t)i];
            hostRoots[(size_t)i] = rebuild::child_entry(next.block[k].idxLo, next.interiors(k) ? 0u : next.block[k].idxSlots, next.pairLo[k]);
        }
        HIPCHK(hipMemcpyAsync(t.rootEntry.p, hostRoots.data(), sizeof(uint32_t) * hostRoots.size(), hipMemcpyHostToDevice, s));
    }
    for (size_t k = 0; k < nR; k++) {   // (before anything reads a box: the collapse, the pair boxes below, the TLAS)
        if (!refits(k)) continue;
        HIPCHK(refitdev::launch_refit_blas(s, t.nodes.p, next.ranges[k].root, 2 * next.interiors(k) + 1, t.prims.p, t.primIdx.p, t.leaves.p + next.leafLo[k], next.interiors(k) + 1, t.parent.p,
                                           t.tickets.p));
        info.refit++; info.leaves_refit += (int32_t)next.interiors(k) + 1;
    }
    return RT_OK;
}
// The records that follow the primitives.  Over everything as at upload; with blocks that move: the shade records as bound and the
// window's anew (the light records: stage_rebuild's copy, anew when there is a window), and BLAS by BLAS the triangle records - a kept
// BLAS's are a copy of its slot run, a refit BLAS also gets the boxes of its pair records rewritten
int Pending::derive_records()
{
    const SceneArrays& sc = b.sc;
    hipStream_t s = b.stream;
    if (!blockwise) {
        const bool boxes = refit && layout1 && !bvh4;
        HIPCHK(refitdev::launch_records(s, t.prims.p, t.nodes.p, t.primIdx.p, next.nIdx, lights, (uint32_t)nLights, 0u, (uint32_t)nPrims,
                                        boxes ? t.pairNode.p : nullptr, boxes ? next.nPairs : 0u, boxes ? t.pairs.p : nullptr, layout1 ? t.triRecs.p : nullptr,
                                        t.shadeRecs.p, t.lightRecs.p));
        if (layout1) info.slots_derived += (int32_t)next.nIdx;
        return RT_OK;
    }
    HIPCHK(hipMemcpyAsync(t.shadeRecs.p, sc.shadeRecs, sizeof(RtFloat4) * (size_t)nPrims, hipMemcpyDeviceToDevice, s));
    HIPCHK(refitdev::launch_records(s, t.prims.p, t.nodes.p, t.primIdx.p, 0u, lights, (uint32_t)nLights, (uint32_t)std::max(rq.geo.g.first, 0), (uint32_t)rq.geo.g.count,
                                    nullptr, 0u, nullptr, nullptr, t.shadeRecs.p, t.lightRecs.p));
    if (!layout1) return RT_OK;
    for (size_t k = 0; k < nR; k++) {
        RtFloat4* const recs = t.triRecs.p + (size_t)next.block[k].idxLo * 3;
        if (moves(k) && !refits(k)) {
            HIPCHK(hipMemcpyAsync(recs, sc.triRecs + (size_t)b.live.block[k].idxLo * 3, sizeof(RtFloat4) * 3 * (size_t)next.block[k].idxSlots, hipMemcpyDeviceToDevice, s));
            info.slots_relocated += (int32_t)next.block[k].idxSlots;
            continue;
        }
        const uint32_t boxes = refits(k) ? next.interiors(k) : 0u;   // (a built BLAS: k_rb_pairs wrote them)
        HIPCHK(refitdev::launch_blas_records(s, t.prims.p, t.nodes.p, t.pairNode.p + next.pairLo[k], boxes, boxes ? t.pairs.p + (size_t)next.pairLo[k] * 4 : nullptr,
                                             t.primIdx.p + next.block[k].idxLo, next.block[k].idxSlots, recs));
        info.slots_derived += (int32_t)next.block[k].idxSlots;
    }
    return RT_OK;
}

// 5. Read back and refuse: the walk, the collapse, the TLAS, the layout; then whatever commit and the stats need of the device
int Pending::read_back(bool timed)
{
    hipStream_t s = b.stream;
    HIPCHK(hipMemcpyAsync(tlas, b.rStatus, sizeof tlas, hipMemcpyDeviceToHost, s));
    if (!refit) HIPCHK(hipMemcpyAsync(walk, b.dw.ctr + rebuilddev::kStatus, sizeof walk, hipMemcpyDeviceToHost, s));
    if (bvh4 && refitPath != 1) HIPCHK(c4.read(s, b.c4));
    HIPCHK(hipStreamSynchronize(s));
    if (bvh4 && refitPath == 1) c4.at(collapsedev::kNeed) = b.live.c4Need;   // (a top-down figure: carried over with the live ids)
    if (walk[0]) return fail(RT_E_DEVICE, "%s: the breadth-first walk does not match the builder's tree (inconsistent device result)", who);
    if (bvh4) {
        if (const int rc = c4.error(who, "; the scene is unchanged")) return rc;
        walk[1] = c4.largest_leaf();   // the layout rule of a BVH4 looks at the collapsed records
    }
    if (const int rc = tlas_status_error(who, tlas)) return rc;
    stackNeed = bvh4 ? (int)c4.need() : (int)maxDepth;
    // (a refit moves no leaf size: a BVH2 copy keeps its layout, a BVH4 copy's check cannot fail)
    if (!(refit && !bvh4) && rebuild::takes_layout1(b.variantLayout1, (int32_t)next.nIdx, std::max(walk[1], 1u)) != layout1)
        return fail(RT_E_UNSUPPORTED, "%s: the new trees would change the scene's derived layout (largest leaf %u primitives, %u index slots; "
                    "layout %d is bound): upload the rebuilt scene instead; the scene is unchanged", who, walk[1], next.nIdx, b.facts.layout);
    if (resize) {
        std::vector<int2> packed((size_t)nPrims);
        HIPCHK(hipMemcpy(packed.data(), b.rPacked.p, sizeof(int2) * packed.size(), hipMemcpyDeviceToHost));
        primType.resize(packed.size()); primMat.resize(packed.size());
        for (size_t i = 0; i < packed.size(); i++) { primType[i] = packed[i].x; primMat[i] = packed[i].y; }
    }
    // the trees and the facts are complete: the set's arrays lie where they will stay, the collapse has counted
    next.parent = t.parent.p; next.leaves = t.leaves.p; next.tickets = t.tickets.p; next.pairNode = t.pairNode.p;
    if (!(layout1 && !bvh4)) next.nPairs = 0;   // (no pair table is bound)
    if (bvh4) { next.newId = t.newId.p; next.quadNode = t.quadNode.p; next.nLive = c4.live(); next.c4Need = c4.need(); }
    facts.stackEntries = rebuild::stack_entries(std::max(stackNeed, 1));   // (a BVH4: the collapsed trees' need, as validate_scene replays it)
    facts.tlasDepth = tlas[1]; facts.nInterior = (int)next.nPairs; facts.nQuads = layout1 && bvh4 ? (int32_t)c4.live() : 0;
    if (resize) facts.singleBlas = nBlas == 1;   // (the TLAS root is a leaf iff there is one instance: TLAS::Build copies it to node 0)
    if (timed) {   // (the events have passed: the stream is idle)
        (void)hipEventElapsedTime(&gpuMs, b.rev[0], b.rev[3]); (void)hipEventElapsedTime(&fitMs, b.rev[0], b.rev[1]);
        (void)hipEventElapsedTime(&deriveMs, b.rev[1], b.rev[2]); (void)hipEventElapsedTime(&tlasMs, b.rev[2], b.rev[3]);
    }
    return RT_OK;
}

// 6. Commit: the holders have been waited for.  Swap the arrays, assign the facts, move the trees and the host shadows in.  Host memory
// only: no device call
void Pending::commit()
{
    SceneArrays n = b.sc;
    n.prims = t.prims.p; n.bvh2 = t.nodes.p; n.primIdx = t.primIdx.p; n.blas = t.blas.p; n.tlas = t.tlas.p;
    n.tlasPairs = t.tp.p; n.tlasPairsP = t.tpP.p; n.instRecs = t.ir.p;
    n.shadeRecs = t.shadeRecs.p; n.lightRecs = t.lightRecs.p;
    if (resize || b.lightsInSet) n.lights = t.lights.p;
    if (layout1 && !bvh4) n.pairs = t.pairs.p;
    if (layout1) { n.triRecs = t.triRecs.p; n.rootEntry = t.rootEntry.p; }
    if (bvh4) { n.bvh4 = t.bvh4.p; if (layout1) n.quads = t.quads.p; }
    if (resize) {   // the new shape: the counts, the TLAS root (instance 0, or TLAS node 0)
        n.nPrims = nPrims; n.nLights = nLights; n.nBlas = nBlas;
        n.tlasRoot = facts.singleBlas ? refit::tlas_leaf_entry(false, 0u) : refit::tlas_node_entry(false, 0u);
        n.tlasRootP = facts.singleBlas ? refit::tlas_leaf_entry(true, 0u) : refit::tlas_node_entry(true, 0u);
    }
    reconfigured = facts.tlasDepth != b.facts.tlasDepth || facts.stackEntries != b.facts.stackEntries;
    b.sc = n; b.facts = facts; b.live = std::move(next);
    if (resize) { b.primType = std::move(primType); b.primMat = std::move(primMat); b.lightsInSet = true; }
    b.inst = std::move(inst);
    if (rq.perRange) { info.built = nBuilt; b.rangesInfo = info; }
    if (refit) b.refitInfo = RtRefitInfo{ refitPath, bvh4 ? (int32_t)b.live.nLive : 0, (int32_t)changed, stackNeed };
    b.generation++;   // every holder takes the new arrays (and re-derives its traversal kernels) before its next launch
    b.rnext ^= 1;
}

static int rebuild_body(SceneBag& b, const Request& rq, RtRebuildStats* stats)
{
    Pending pd{ b, rq };
    if (const int rc = pd.size()) return rc;
    HIPCHK(hipEventRecord(b.rev[0], b.stream));
    if (const int rc = pd.stage()) return rc;
    pd.t1 = Pending::clock::now();
    if (const int rc = pd.trees()) return rc;
    pd.t2 = Pending::clock::now();
    if (const int rc = pd.derive()) return rc;
    if (const int rc = pd.read_back(stats != nullptr)) return rc;
    pd.t3 = Pending::clock::now();
    if (const int rc = b.wait_holders()) return rc;   // no kernel of a holder reads the old arrays any more
    pd.commit();
    const auto t4 = Pending::clock::now();
    if (stats) {
        *stats = RtRebuildStats{};
        stats->gpu_ms = pd.gpuMs; stats->wall_ms = ms_between(pd.t0, t4);
        stats->stage_ms = ms_between(pd.t0, pd.t1); stats->derive_ms = pd.deriveMs; stats->tlas_ms = pd.tlasMs;
        stats->build_ms = pd.refit ? pd.fitMs : ms_between(pd.t1, pd.t2);   // (a refit: GPU time of the staging copies and the refit)
        stats->commit_ms = ms_between(pd.t3, t4);
        stats->prims = pd.resize ? rq.nPrims : rq.geo.g.count; stats->blas_built = pd.nBuilt; stats->nodes = (int32_t)b.live.nNodes; stats->n_idx = (int32_t)b.live.nIdx;
        stats->max_depth = (int32_t)pd.maxDepth; stats->tlas_nodes = b.live.nTlas; stats->tlas_depth = pd.tlas[1]; stats->reconfigured = pd.reconfigured ? 1 : 0;
        stats->spatial_splits = (int32_t)std::min<uint64_t>(pd.spatialSplits, 0x7fffffffu); stats->prims_clipped = (int32_t)std::min<uint64_t>(pd.primsClipped, 0x7fffffffu);
    }
    return RT_OK;
}
int scenedev::rebuild_scene(SceneBag& b, const char* who, const Geometry& geo, const RtBVHInstance* blas, int32_t nBlas,
                            int32_t builder, const RtBuildOptions* opts, RtRebuildStats* stats)
{
    // ---- refusals that need no device work
    if (b.refitRefusal) return fail(RT_E_UNSUPPORTED, "%s: %s", who, b.refitRefusal);
    if (b.rebuildRefusal) return fail(RT_E_UNSUPPORTED, "%s: %s", who, b.rebuildRefusal);
    if (const int rc = check_builder(who, builder, opts, true)) return rc;
    if (const int rc = check_change(who, b, geo, blas, nBlas, "")) return rc;
    lbvh::Params P{};
    const std::vector<int32_t> plan(builder == RT_REBUILD_REFIT ? 0 : b.live.ranges.size(), builder);   // every range: `builder`
    if (!plan.empty()) if (const int rc = check_ranges(who, plan.data(), opts, b.sc.nPrims, b.live.ranges, nullptr, P)) return rc;
    return rebuild_body(b, Request{ who, b.sc.nPrims, b.sc.nBlas, nullptr, geo, blas, plan, opts, P }, stats);
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
        blocks[(size_t)k] = rebuild::BlasBlock{ 2 * (uint32_t)rangeCount[k] - 1, 0u, (uint32_t)rangeCount[k], (uint8_t)(!compact || compact[k] ? 1 : 0), 0u };
    }
    if (count < 0 || (count > 0 && (first < 0 || (int64_t)first + count > (int64_t)nPrims)))
        return fail(RT_E_INVALID, "%s: primitive range [%d, %lld) outside the %d uploaded", who, first, (long long)first + count, nPrims);
    lbvh::Params P{};
    return plan_check_args(who, nPrims, ranges, blocks.data(), plan, nRanges, first, count, opts, P);
}
int scenedev::rebuild_ranges(SceneBag& b, const char* who, const Geometry& geo, const RtBVHInstance* blas, int32_t nBlas,
                             const int32_t* plan, int32_t nRanges, const RtBuildOptions* opts, RtRebuildStats* stats)
{
    // ---- refusals that need no device work
    if (b.refitRefusal) return fail(RT_E_UNSUPPORTED, "%s: %s", who, b.refitRefusal);
    if (b.rebuildRefusal) return fail(RT_E_UNSUPPORTED, "%s: %s", who, b.rebuildRefusal);
    if (const int rc = check_change(who, b, geo, blas, nBlas, "")) return rc;
    lbvh::Params P{};
    if (const int rc = plan_check_args(who, b.sc.nPrims, b.live.ranges, b.live.block.data(), plan, nRanges, geo.g.first, geo.g.count, opts, P)) return rc;
    return rebuild_body(b, Request{ who, b.sc.nPrims, b.sc.nBlas, nullptr, geo, blas, std::vector<int32_t>(plan, plan + nRanges), opts, P, true }, stats);
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
        for (const rebuild::BlasRange& r : b.live.ranges) {
            if (r.first != next) return fail(RT_E_UNSUPPORTED, "rt_resize_scene: the bound scene's BLAS ranges leave a gap: primitives [%u, %u) belong to no BLAS", next, r.first);
            next = r.first + r.count;
        }
        if (next != (uint32_t)b.sc.nPrims)
            return fail(RT_E_UNSUPPORTED, "rt_resize_scene: the bound scene's BLAS ranges leave a gap: primitives [%u, %d) belong to no BLAS", next, b.sc.nPrims);
    }
    const std::vector<int32_t> plan(ranges.size(), builder);   // (never RT_REBUILD_KEEP)
    return rebuild_body(b, Request{ who, nPrims, shape->nBlas, prims, Geometry{}, shape->blas, plan, opts, P, false, std::move(ranges),
                                    std::vector<int32_t>(shape->instRange, shape->instRange + shape->nBlas) }, stats);
}

// scene_dev.h — the device copy of a scene as the contexts of rt355.hip hold it, what the files of the C-ABI share (error reporting and
// the allocation helper) and what the three files that own a copy share: scene.hip (checks, upload, views), scene_rebuild.hip (update,
// rebuild, ranges, resize) and scene_materials.hip.  They know nothing of a context (RtCtx) but that the holders of a copy can be made
// to wait.
#pragma once
#include <hip/hip_runtime.h>
#include <algorithm>
#include <chrono>
#include <cstdarg>
#include <cstdio>
#include <vector>
#include "../../include/rt355.h"
#include "refit_common.h"
#include "rebuild_common.h"
#include "rebuild_dev.h"
#include "collapse_dev.h"
#include "build_cores.h"
#include "geometry_dev.h"

int rt355_set_error(int code, const char* msg);   // rt355.hip: sets the text rt_last_error() returns
static int fail(int code, const char* fmt, ...)
{
    char buf[512];
    va_list ap; va_start(ap, fmt); vsnprintf(buf, sizeof buf, fmt, ap); va_end(ap);
    return rt355_set_error(code, buf);
}
#define HIPCHK(expr) do { hipError_t e_ = (expr); if (e_ != hipSuccess) \
    return fail(RT_E_DEVICE, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), __FILE__, __LINE__); } while (0)

template <class T> static int dalloc(std::vector<void*>& bag, T** p, size_t count)
{
    void* v = nullptr;
    size_t bytes = std::max<size_t>(count, 1) * sizeof(T);
    hipError_t e = hipMalloc(&v, bytes);
    if (e != hipSuccess) return fail(RT_E_NOMEM, "hipMalloc(%zu) failed: %s", bytes, hipGetErrorString(e));
    bag.push_back(v);
    *p = (T*)v;
    return RT_OK;
}

namespace refitdev {   // refit.hip's kernels (rules: refit_common.h)
hipError_t launch_refit(hipStream_t s, RtBVHNode2* nodes, uint32_t nNodes, const RtPrimitive* prims, const uint32_t* primIdx, const uint32_t* leaves,
                        uint32_t nLeaves, const uint32_t* parent, uint32_t* tickets);
hipError_t launch_refit_blas(hipStream_t s, RtBVHNode2* nodes, uint32_t root, uint32_t nBlasNodes, const RtPrimitive* prims, const uint32_t* primIdx,
                             const uint32_t* leafRun, uint32_t nLeaves, const uint32_t* parent, uint32_t* tickets);
hipError_t launch_blas_records(hipStream_t s, const RtPrimitive* prims, const RtBVHNode2* nodes, const uint32_t* pairNode, uint32_t nPairs, RtFloat4* pairs,
                               const uint32_t* primIdx, uint32_t nSlots, RtFloat4* triRecs);
hipError_t launch_tlas(hipStream_t s, const RtBVHNode2* nodes, const RtBVHInstance* inst, int n, const uint32_t* rootEntry, RtTLASNode* tlas, RtFloat4* tp,
                       RtFloat4* tpP, RtFloat4* ir, int32_t* status);
hipError_t launch_records(hipStream_t s, const RtPrimitive* prims, const RtBVHNode2* nodes, const uint32_t* primIdx, uint32_t nIdx, const uint32_t* lights,
                          uint32_t nLights, uint32_t first, uint32_t count, const uint32_t* pairNode, uint32_t nPairs, RtFloat4* pairs, RtFloat4* triRecs,
                          RtFloat4* shadeRecs, RtFloat4* lightRecs);
}

struct RtCtx;
namespace scenedev __attribute__((visibility("hidden"))) {   // (nothing of this interface is exported from the library)

// The arrays of a copy as their owner writes them: DevScene (rt355_dev.h) field for field and in its order, writable and in the wire types.
// A context turns them into the kernels' read-only view when it takes the copy over (rt355.hip, adopt_scene).
struct SceneArrays {
    RtPrimitive* prims; RtMaterial* mats; RtFloat4* tex; uint32_t* lights; RtBVHNode2* bvh2; RtBVHNode4* bvh4; uint32_t* primIdx;
    RtTLASNode* tlas; RtBVHInstance* blas;
    RtFloat4 *pairs, *triRecs; uint32_t* rootEntry; RtFloat4 *shadeRecs, *tlasPairs, *instRecs; uint32_t tlasRoot;
    RtFloat4* tlasPairsP; uint32_t tlasRootP; RtFloat4 *lightRecs, *quads;
    int32_t nLights, nPrims, nBlas, nTex, nMats;
};
// What a holder plans its traversal from (trav_common.h): the bag has one, a context (RtCtx) the one it adopted
struct SceneFacts {
    int layout = 0;                           // 0 = traverse the reference arrays as uploaded, 1 = derived pair/triangle-record layout
    int stackEntries = RT_BVH2_STACK, tlasDepth = 0, nInterior = 0;   // LDS stack entries the trees need; TLAS height; records of the dense pair table
    int32_t nQuads = 0; bool singleBlas = false;   // quad records (the surviving nodes of a BVH4 in layout 1); the TLAS root is a leaf
};
// The trees a copy renders from: found at upload, built anew by a rebuild (Pending::next, scene_rebuild.hip) and committed whole
struct LiveTrees {
    uint32_t nNodes = 0, nIdx = 0, nPairs = 0, nTlas = 0, nLeaves = 0, nReach = 0;   // (nPairs: of the bound pair table; nReach: nodes a refit visits)
    uint32_t *parent = nullptr, *leaves = nullptr, *pairNode = nullptr, *tickets = nullptr;   // refit topology (walked from the BLAS roots)
    // One record per bound BLAS, in two halves of rebuild_common.h's types (check_plan and check_ranges take them): ranges[k] its
    // primitives (in increasing order) and its root, block[k] the nodes and index slots the live tree occupies (an SBVH tree has more
    // slots than primitives), whether it can move as one (RT_REBUILD_KEEP) and its height.  A refit leaves them.
    std::vector<rebuild::BlasRange> ranges; std::vector<rebuild::BlasBlock> block;
    std::vector<int32_t> instBlas;            // instance -> its range
    uint32_t interiors(size_t k) const { return (block[k].nodes - 1) / 2; }   // interior nodes of BLAS k
    // ... and beside it where the derived data of BLAS k lie: the start of its run of pair ids (interiors of them; BLAS by BLAS in the order
    // in which the instances first name them) and the start of its run in the leaf list (interiors + 1 of them; after an upload the
    // runs come in that same order, after a rebuild in range order - the order inside a run is no contract).  rt_rebuild_ranges moves a
    // kept or refit BLAS's derived data by them.
    std::vector<uint32_t> pairLo, leafLo;
    // The live collapse of a BVH4 copy that keeps its BVH2: node -> live id and live id -> node (the upload's own arrays or the live
    // set's, never scratch: a refused call in between must leave them), the live nodes and the stack need as the collapse counted it
    uint32_t *newId = nullptr, *quadNode = nullptr, nLive = 0, c4Need = 0;
};
// The device copy of a scene (uploaded arrays + derived layouts).  Contexts that render the same scene - sample-stream lanes, the
// row bands of one frame - can hold ONE copy (rt_share_scene): less HBM, and one working set in the L2s / Infinity Cache instead of one per context.
struct SceneBag {
    std::vector<void*> allocs; int device = 0;   // what is made once and lives as long as the copy; the device it lies on
    // What a holder renders with, each written whole by upload and by the commits of update, rebuild and material update only; a context
    // takes sc and facts over in adopt_scene (rt355.hip)
    SceneArrays sc{};                         // the device arrays and their counts (an update rewrites them in place, a rebuild swaps them)
    SceneFacts facts; LiveTrees live;
    uint64_t generation = 0;                  // bumped when an update or a rebuild changes any of them
    std::vector<RtCtx*> holders;              // the contexts rendering from this copy
    int wait_holders() const;                 // rt355.hip: until `stream` and `home` of every holder are idle (before a commit)
    // rt_update_scene: what an in-place update needs of the upload, kept beside the device copy
    const char* refitRefusal = nullptr;       // why this scene cannot be updated in place (NULL: it can)
    int32_t accel = 0; bool keepsBvh2 = false;   // a BVH4 copy bound with its BVH2 (rt_upload_scene_bvh2): sc.bvh2 is kept, the copy can be rebuilt
    std::vector<int32_t> primType, primMat;   // host shadow of every primitive's objType / matIdx (the light list and materials depend on them)
    std::vector<RtBVHInstance> inst;          // the instances as last uploaded or updated
    // A device array that is replaced during the copy's life (rebuild_grow, below, is the one place that does) and freed with it
    template <class T> struct Grown {
        T* p = nullptr; size_t cap = 0;
        Grown() = default; Grown(const Grown&) = delete; Grown& operator=(const Grown&) = delete;
        ~Grown() { if (p) (void)hipFree(p); }
    };
    // staging of an update (allocated by the first one, grown when a resize has changed the counts): nothing live is written before the
    // new TLAS has passed
    Grown<RtPrimitive> sPrims; Grown<RtBVHInstance> sInst; Grown<RtTLASNode> sTlas;
    Grown<RtFloat4> sTp, sTpP, sIr; int32_t* sStatus = nullptr;
    Grown<RtBVHNode2> sNodes;                 // (a rebuild changes the node count)
    hipStream_t stream = nullptr;             // where updates run
    hipEvent_t ev[4] = { nullptr, nullptr, nullptr, nullptr };   // brackets of the staging and of the commit
    // rt_rebuild_scene: what it needs of the upload, and its device memory (allocated by the first rebuilds, then reused)
    const char* rebuildRefusal = nullptr;     // why this scene cannot be rebuilt in place (NULL: it can)
    bool variantLayout1 = false;              // the holders' extend_variant admits the derived layout 1
    RtRangesInfo rangesInfo{};                // the last successful rt_rebuild_ranges (rt_ranges_info)
    RtRefitInfo refitInfo{};                  // the last successful RT_REBUILD_REFIT (rt_refit_info)
    // Everything a rebuild changes, twice: a rebuild writes the set that is not live and the commit swaps the pointers; the upload's own
    // arrays stay behind until the copy is freed.  The arrays that scale with the primitives, the instances and the lights fit the bound
    // shape exactly at first; rt_resize_scene changes those counts, and an array of the set that is not live that the new shape outgrows
    // goes to the need plus a quarter (rebuild_fit).  Those that scale with the
    // trees have capacities of their own: nPrims index slots and 2 * nPrims nodes at first, which bounds every tree of the SAH
    // and the linear builder; an SBVH tree has no such bound, so the set that is not live grows to what the finished trees need plus a
    // quarter (kRebuildHeadroomDiv, rebuild_reserve), what was emitted so far is kept and the arrays it replaces are freed at once.
    struct RebuildSet {
        Grown<RtPrimitive> prims; Grown<RtFloat4> shadeRecs;                                 // primitives
        Grown<RtBVHInstance> blas; Grown<RtTLASNode> tlas; Grown<RtFloat4> tp, tpP, ir;      // instances (tlas: 2 per instance; tp, tpP, ir: 4 rows per record)
        Grown<uint32_t> rootEntry;
        Grown<uint32_t> lights; Grown<RtFloat4> lightRecs;                                   // lights (lightRecs: 8 rows each, one record at least)
        Grown<uint32_t> primIdx; Grown<RtFloat4> triRecs;                                    // index slots (triRecs: 3 per slot)
        Grown<RtBVHNode2> nodes; Grown<uint32_t> parent, tickets;                            // nodes
        Grown<RtFloat4> pairs; Grown<uint32_t> leaves, pairNode;                             // nodes / 2 (pairs: 4 per interior node)
        Grown<RtBVHNode4> bvh4; Grown<RtFloat4> quads;                                       // a BVH4 copy: nodes; nodes / 2 + one per BLAS (8 per live node)
        Grown<uint32_t> newId, quadNode;                                                     // a BVH4 copy: the collapse's tables (nodes; nodes / 2 + one per BLAS)
    } rset[2];
    Grown<uint32_t> dwFlags, dwRanks, dwNewId, dwFrontA, dwFrontB; Grown<char> dwScan;   // the derivation's scratch, grown likewise
    // the collapse's scratch (a BVH4 copy that keeps its BVH2), grown likewise: frontiers, flags / ranks / kids, scan, counters.  The
    // tables a collapse leaves (newId, quadNode) are not scratch: they belong to the arrays collapsed (the upload's, a set's)
    Grown<uint2> c4FrontA, c4FrontB; Grown<uint32_t> c4Flags, c4Ranks, c4Kids, c4Ctr; Grown<char> c4Scan;
    size_t c4Cap = 0;                         // the nodes the scratch was sized for
    collapsedev::Work c4{};                   // (newId / quadNode / quadCap: filled in by the caller)
    sbvhdev::Pool* spool = nullptr;           // the SBVH builder's device blocks, kept from rebuild to rebuild
    uint64_t rallocs = 0;                     // device allocations by updates and rebuilds of this copy (rt_debug_rebuild_allocations)
    int rnext = 0;                            // the set the next rebuild writes
    Grown<char> rwork;                        // the builders' workspace (bytes)
    rebuilddev::Work dw{};                    // scratch of the derivation
    int32_t* rStatus = nullptr;               // k_tlas_build's status words (word 0, before that: k_resize_check's lowest refused primitive)
    // RtGeometry: the status word of its kernels (the lowest refused index of the window), and host positions / host indices of the vertex
    // form on their way to k_tri_from_vertices; made by the first call that needs them and grown as the staging arrays are
    Grown<uint32_t> gStatus, gIdx; Grown<char> gPos;
    Grown<int2> rPacked;                      // rt_resize_scene: (objType, matIdx) per new primitive, what the host reads back for primType / primMat
    bool lightsInSet = false;                 // a resize or a material update has bound a light list of its own: rebuilds carry it from set to set from then on
    hipEvent_t rev[4] = { nullptr, nullptr, nullptr, nullptr };
    // rt_update_materials: the host shadow of the bound table (a shrinking atlas is checked against it), the pad behind the atlas and
    // the capacity of the live atlas in texels, the pad included.  What depends on the materials exists twice, as the rebuild's sets do:
    // an update writes the set that is not live and the commit swaps the pointers (the upload's arrays, or a rebuild set's light list and
    // records, stay behind).  An atlas that outgrows its array moves to the texture array that is not live.
    std::vector<RtMaterial> hMats;
    int64_t texPad = 2; size_t texCap = 0;
    Grown<RtMaterial> mmats[2];
    struct LightSet { Grown<uint32_t> lights; Grown<RtFloat4> lightRecs; } mlights[2];
    Grown<RtFloat4> mtex[2];
    int mmatsNext = 0, mlightsNext = 0, mtexNext = 0;   // which of each the next update writes (flipped when a commit has made it live)
    Grown<int32_t> mAssign;                   // the new matIdx values of an update's range, host or device input alike
    ~SceneBag()
    {
        (void)hipSetDevice(device);
        if (stream) (void)hipStreamDestroy(stream);
        for (hipEvent_t e : ev) if (e) (void)hipEventDestroy(e);
        for (hipEvent_t e : rev) if (e) (void)hipEventDestroy(e);
        sbvhdev::pool_destroy(spool);
        for (void* p : allocs) (void)hipFree(p);
    }
};

// ---- scene.hip; messages go to rt_last_error()
struct HostScene {   // the host arrays of rt_upload_scene (include/rt355.h), in its order
    const RtPrimitive* prims; int32_t nPrims; const RtMaterial* mats; int32_t nMats; const RtFloat4* textures; int32_t nTexels; const uint32_t* lights; int32_t nLights;
    const void* bvhNodes; int32_t nNodes; const uint32_t* primIdx; int32_t nIdx; const RtTLASNode* tlas; int32_t nTlas; const RtBVHInstance* blas; int32_t nBlas;
};
int validate_scene(int accel, const HostScene& in, SceneFacts* factsOut, int64_t* texPadOut);   // (of the facts: stackEntries and tlasDepth)
// fills a fresh copy on the current device from arrays that have passed validate_scene, which began `facts` and gave texPad
// blas4 != NULL (a BVH4 context, in.bvhNodes is the BVH2; collapse::check_args gave the BLAS): the BVH2 is kept and collapsed on the device
int upload_scene(SceneBag& b, int accel, int extendVariant, const HostScene& in, SceneFacts facts, int64_t texPad, const std::vector<collapse::Blas>* blas4 = nullptr);
// ---- scene_rebuild.hip
// The replacement geometry of an update or a rebuild (RtGeometry, include/rt355.h) and where each of its sources lies: on the host, or
// in memory the copy's device reaches (the caller has applied the pointer rule).  `who` names the entry point in every message.
struct Geometry {
    RtGeometry g{};
    bool primsOnDevice = false, positionsOnDevice = false, indicesOnDevice = false;
    // what rt_update_scene, rt_rebuild_scene and rt_rebuild_ranges take: records in host memory (a window without records keeps `first`
    // out of the checks, as those calls always have)
    static Geometry host_records(const RtPrimitive* prims, int32_t first, int32_t count)
    {
        Geometry G;
        G.g.first = count != 0 ? first : 0; G.g.count = count; G.g.prims = prims;
        return G;
    }
};
int update_scene(SceneBag& b, const char* who, const Geometry& geo, const RtBVHInstance* blas, int32_t nBlas, RtUpdateStats* stats);
int rebuild_scene(SceneBag& b, const char* who, const Geometry& geo, const RtBVHInstance* blas, int32_t nBlas,
                  int32_t builder, const RtBuildOptions* opts, RtRebuildStats* stats);
// rt_rebuild_ranges (include/rt355.h): plan[nRanges], one RT_REBUILD_SAH / LBVH / SBVH / KEEP / REFIT_RANGE per distinct BLAS in the order of b.live.ranges
int rebuild_ranges(SceneBag& b, const char* who, const Geometry& geo, const RtBVHInstance* blas, int32_t nBlas,
                   const int32_t* plan, int32_t nRanges, const RtBuildOptions* opts, RtRebuildStats* stats);
// rt_scene_blas_blocks: the ranges and blocks of the bound trees (any output may be NULL; at most cap entries are written)
int blas_blocks(const SceneBag& b, int32_t* n, int32_t* primFirst, int32_t* primCount, int32_t* nodes, int32_t* idxSlots, int32_t* compact, int32_t cap);
// rt_resize_scene (include/rt355.h): the caller's shape, checked by resize::check_shape; prims may be host or device memory
int resize_scene(SceneBag& b, const void* prims, int32_t nPrims, const RtSceneShape* shape, int32_t builder, const RtBuildOptions* opts, RtRebuildStats* stats);
// ---- scene_materials.hip
// rt_update_materials (include/rt355.h): texels / primMat may be host or device memory (the caller has applied the pointer rule)
int update_materials(SceneBag& b, const RtMaterialUpdate& u, RtMaterialStats* stats);

// ---- what the three files share, each written once (scene.hip defines what is not defined here) ---------------------------------------
// b.stream, and the four events `ev` (b.ev, b.rev; NULL: none), made by the first call that needs them
int scene_stream(SceneBag& b, hipEvent_t* ev);
// Capacities of what scales with the trees (SceneBag::RebuildSet, the derivation's and the collapse's scratch, rt_update_scene's staging
// nodes): index slots at first, twice as many nodes; RT355_REBUILD_INITIAL_CAP=k (read per call; tests, A/B runs) starts smaller or
// larger.  An array that a finished tree outgrows goes to the need plus need / kRebuildHeadroomDiv: a quarter covers the frame-to-frame
// drift of an animated SBVH scene (its slot count moved by a few percent between the deformations tried), so a per-frame rebuild stops
// allocating once both sets have grown, and costs at most that much idle memory.
constexpr size_t kRebuildHeadroomDiv = 4;
inline size_t with_headroom(size_t need) { return need + need / kRebuildHeadroomDiv; }
// what an array of `cap` records becomes when `need` are asked of it (have: it exists; the first allocation is exact)
inline size_t grown_cap(size_t need, size_t cap, bool have) { return need <= cap ? cap : have ? with_headroom(need) : need; }
size_t rebuild_initial_cap(const SceneBag& b);
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
// once a resize outgrows it replaced by one of the need plus headroom.  Nothing in it is kept.
template <class T> static int rebuild_fit(SceneBag& b, SceneBag::Grown<T>& a, size_t need, const char* what)
{
    need = std::max<size_t>(need, 1);
    if (a.p && need <= a.cap) return RT_OK;
    return rebuild_grow(b, a, a.p ? with_headroom(need) : need, 0, what);
}
// The derivation's scratch (b.dw) for trees of nodeNeed nodes in all, or for a flag scan over as many primitives
int rebuild_scratch(SceneBag& b, size_t nodeNeed);
// After a flag scan over n primitives (rebuilddev::resize_check, mat_flags; `bad` word: b.rStatus): the lowest refused primitive
// (resize::kNoBad: none) and the lights the scan counted.  Waits for the stream.
int flag_scan_result(SceneBag& b, int32_t n, uint32_t* firstBad, int32_t* nLights);
// The collapse's scratch (b.c4) for trees of nodeNeed nodes in all; b.c4 lacks the tables a collapse leaves behind (newId, quadNode and
// their capacity): collapse_work adds those of the arrays that are collapsed.
int collapse_scratch(SceneBag& b, size_t nodeNeed);
collapsedev::Work collapse_work(const SceneBag& b, uint32_t* newId, uint32_t* quadNode, size_t quadCap);
// The status words a collapse leaves in its counters (collapse_dev.h), by name
struct CollapseStatus {
    uint32_t w[collapsedev::kStatusWords] = { 0 };
    uint32_t& at(uint32_t word) { return w[word - collapsedev::kStatus]; }
    uint32_t at(uint32_t word) const { return w[word - collapsedev::kStatus]; }
    uint32_t walk() const { return at(collapsedev::kWalkWord); }      // a failed walk
    uint32_t live() const { return at(collapsedev::kLive); }          // live nodes
    uint32_t need() const { return at(collapsedev::kNeed); }          // stack entries of the deepest BLAS
    uint32_t changed() const { return at(collapsedev::kChanged); }    // refit_records: live records whose slots differ
    uint32_t largest_leaf() const { return std::max(std::max(at(collapsedev::kLeaf), at(collapsedev::kLeafAny)), 1u); }
    hipError_t read(hipStream_t s, const collapsedev::Work& work) { return hipMemcpyAsync(w, work.ctr + collapsedev::kStatus, sizeof w, hipMemcpyDeviceToHost, s); }
    // a failed walk, a BLAS that needs more stack than there is, as the error of the call `who`; `tail` ends the stack message
    int error(const char* who, const char* tail) const;
};
// "the new trees have 2^31 nodes or index slots, or more": the refusal of a rebuild whose trees outgrow the 31-bit ids
int too_many_nodes(const char* who);
// the outputs of rt_blas_blocks / rt_scene_blas_blocks (any may be NULL; at most cap entries are written)
void write_blocks(const LiveTrees& t, int32_t* n, int32_t* primFirst, int32_t* primCount, int32_t* nodes, int32_t* idxSlots, int32_t* compact, int32_t cap);
inline double ms_between(std::chrono::steady_clock::time_point a, std::chrono::steady_clock::time_point b)
{
    return std::chrono::duration<double, std::milli>(b - a).count();
}
int64_t rebuild_allocations(const SceneBag& b);
int scene_array(const SceneBag& b, int32_t which, const void** src, size_t* bytes);   // where RT_SCENE_* lies on the device and how long it is

} // namespace scenedev

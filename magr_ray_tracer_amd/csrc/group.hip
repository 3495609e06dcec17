// group.hip — lane groups (rt_group_*, include/rt355.h): several contexts of rt355.hip behind one handle, their frames routed to the
// streams that really run side by side, their accumulators summed in lane order.  A group drives its lanes through the public rt_* calls;
// what it touches of a context beyond them is listed in ctx.h.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <string>
#include <vector>
#include "../../include/rt355.h"
#include "rt355_math.h"   // add4
#include "ctx.h"

using namespace rt355dev;

// ---- lanes: several sample streams of one accumulation behind ONE handle -------------------------------------------------------
// Every launch of a frame ends in a tail of a few long rays during which most of the chip idles, and the frames of ONE seed stream cannot
// overlap (each continues the RNG state of the one before).  A group renders the accumulation as `lanes` independent sample streams
// instead - own context, HIP stream, queues and seed slice each, ONE device copy of the scene - and interleaves their frames, so the
// tails of one lane's launches are filled by the others' kernels.  The group's accumulator is the sum of its lanes' accumulators in
// lane order.  (Reference: one Renderer, one in-order queue, renderer.cpp:26-94; the group is what stands behind Renderer::Tick here.)
//
// HIP maps a process's streams onto GPU_MAX_HW_QUEUES hardware queues per stream priority (default 4; the normal pool holds the null
// stream too) and runs kernels of streams that share one after the other.  The library leaves that setting to the process that loads
// it; rt_group_create MEASURES how many of its streams really run side by side - per priority class, choose_streams - so a caller is
// told instead of silently serialised.
//
// Fewer concurrent streams than lanes must not leave a lane's frames queued behind another's: two lanes on one queue render twice
// as many frames in series as the rest, which finish at half-time and leave the chip to one context (4 lanes on 3 queues: 41 % of
// the bench's timed region, profiles/r04_group_streams.txt).  So the group keeps a lane's SAMPLES where they are (frame j is
// lane j mod L's, with its seeds, accumulator and counters) but issues frame j on worker stream j mod S, the S lane streams found to
// run side by side.  A lane's `stream` is then the worker that ran its last frame, and everything else it queues (reset, seeds, sum,
// reads, synchronize, stage events) lands behind that frame.  A move to another worker waits on an event recorded right after the
// lane's last frame - not on the other lanes' frames queued behind it there - or, when the lane has queued more work since, after that.

__global__ void k_spin(long long ticks, int* sink)
{
    const long long t0 = wall_clock64();
    while (wall_clock64() - t0 < ticks) __builtin_amdgcn_s_sleep(8);
    if (ticks < 0) *sink = 1;
}
__global__ __launch_bounds__(kBlock) void k_sum_lanes(float4* out, const float4* a0, const float4* a1, const float4* a2, const float4* a3,
                                                       const float4* a4, const float4* a5, const float4* a6, const float4* a7, int lanes, int first, int n)
{
    // only the group's own rows [first, first + n): the bands of one frame can be summed into one buffer without touching each other
    int i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    i += first;
    const float4* a[8] = { a0, a1, a2, a3, a4, a5, a6, a7 };
    float4 s = a[0][i];
    for (int m = 1; m < lanes; m++) s = add4(s, a[m][i]);   // lane order, left to right
    out[i] = s;
}

// The stream classes of a group: HIP's stream priorities.  rt_group_stream_class reports one of these, or kClassMixed.
enum { kClassLow = -1, kClassNormal = 0, kClassHigh = 1, kClassMixed = 2 };
// Between the two classes beside normal, at equal S: the lower one, so that a renderer embedded in an application yields to that
// application's other GPU work (the bench tells them apart by no more than its spread, EXPERIMENTS.md (62))
static constexpr int kPreferClass = kClassLow;
// Lanes that no single class runs side by side take streams of the other classes only on request (RT355_GROUP_PRIORITY=mixed): workers
// of unequal priority finish their equal shares of frames at different times
static constexpr bool kMixedByDefault = false;

struct RtGroup {
    std::vector<RtCtx*> lane;
    std::vector<int> laneClass;         // one per lane: the class of its home stream
    int seen[3] = { -1, -1, -1 };       // S as measured per class (low, normal, high) at creation; -1: not measured
    float4* sum = nullptr;              // lane-ordered sum of the lanes' accumulators (own buffer)
    std::vector<hipEvent_t> done;       // one per lane: "this lane's queued frames are finished", for the sum on lane 0's stream
    uint64_t frames = 0;                // frames rendered by all lanes since the last reset (= the divisor of prep())
    int concurrent = 0;                 // S = worker.size(): streams measured to run side by side at creation
    std::vector<int> worker;            // the lanes whose home streams run side by side: frames are issued on these
    std::vector<hipEvent_t> moved;      // one per lane: the end of its last frame (or of work queued since), waited on by the worker it moves to
    int nextLane = 0;                   // round-robin position, so that successive one-frame calls visit all lanes
    int nextWorker = 0;                 // the same over the workers
};
static constexpr int kMaxLanes = 8;

static void group_free(RtGroup* g)
{
    if (!g) return;
    for (RtCtx* c : g->lane) { (void)hipStreamSynchronize(c->stream); c->stream = c->home; }   // a lane may sit on another's stream
    for (RtCtx* c : g->lane) ctx_free(c);
    for (hipEvent_t e : g->done) (void)hipEventDestroy(e);
    for (hipEvent_t e : g->moved) (void)hipEventDestroy(e);
    if (g->sum) (void)hipFree(g->sum);
    delete g;
}
// Which streams execute concurrently: one single-wave kernel that naps for ~1 ms, on one stream alone and then on every stream of a
// candidate set at once, both timed on the host.  Streams that share a hardware queue run their naps one after the other, so a set
// whose naps take about as long as one nap runs side by side.  Greedy: `set` (its first stream, when empty: the first candidate) grows
// by each candidate that keeps it concurrent; returns which candidates were taken.  Measured, not predicted: which queue a stream
// lands on is the runtime's business.
static std::vector<int> grow_concurrent(RtGroup* g, std::vector<hipStream_t>& set, const std::vector<hipStream_t>& cand)
{
    std::vector<int> taken;
    size_t first = 0;
    if (set.empty() && !cand.empty()) { set.push_back(cand[0]); taken.push_back(0); first = 1; }
    if (first >= cand.size()) return taken;
    int rate = 0;
    if (hipDeviceGetAttribute(&rate, hipDeviceAttributeWallClockRate, g->lane[0]->cfg.device) != hipSuccess || rate <= 0) rate = 100000;   // kHz
    const long long ticks = (long long)rate;        // 1 ms
    int* sink = (int*)g->sum;                        // never written (ticks >= 0); the group's own memory, allocated before any measurement
    auto run = [&](const std::vector<hipStream_t>& on) {
        const auto t0 = std::chrono::steady_clock::now();
        for (hipStream_t s : on) hipLaunchKernelGGL(k_spin, dim3(1), dim3(64), 0, s, ticks, sink);
        for (hipStream_t s : on) (void)hipStreamSynchronize(s);
        return std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count();
    };
    // the best of three each: a host thread that is descheduled for a millisecond must not read as a serialised stream
    auto best = [&](const std::vector<hipStream_t>& on) { float t = run(on); for (int k = 0; k < 2; k++) t = std::min(t, run(on)); return t; };
    std::vector<hipStream_t> all = set;
    all.insert(all.end(), cand.begin() + (ptrdiff_t)first, cand.end());
    (void)run(all);                                  // warms the code object up on every stream
    const float one = best({ set[0] });
    if (one <= 0) return taken;
    for (size_t k = first; k < cand.size(); k++) {
        std::vector<hipStream_t> with = set; with.push_back(cand[k]);
        if (best(with) < 1.5f * one) { set = with; taken.push_back((int)k); }   // serialised: >= 2 naps
    }
    return taken;
}

// Which streams the lanes' frames are issued on.  HIP keeps one pool of hardware queues PER STREAM PRIORITY, each up to the process's
// limit, and the process's other streams (the null stream, a framework's) sit in the normal pool: lane streams of another priority
// class can have that class's queues to themselves.  All lanes of a class have equal priority among themselves, and nothing
// process-wide changes.  Which class gives the most concurrent workers is measured like everything else here:
//   normal   the streams of rt_create, as for a single context
//   low/high every lane's stream replaced by one of that priority
//   auto     (unset) normal when every lane runs side by side there - no other stream is ever created then - or when no other class
//            holds more workers; else the class with the most, kPreferClass at a tie
//   mixed    auto, then the lanes left over try a stream of each other class (kMixedByDefault: auto does the same)
// A lane's stream is replaced before anything but its creation work was queued: rt_create has synchronised that, and nothing else of
// a context is bound to its stream (the stage events are recorded on ctx->stream at use).
static int choose_streams(RtGroup* g, int want, bool mixed)
{
    const int n = (int)g->lane.size();
    int least = 0, greatest = 0;
    HIPCHK(hipDeviceGetStreamPriorityRange(&least, &greatest));
    const bool classes = least != greatest;   // (numerically, a lower value is a higher priority)
    if (!classes && (want == kClassLow || want == kClassHigh)) return fail(RT_E_INVALID, "rt_group_create: RT355_GROUP_PRIORITY asks for a priority class, but this device has one stream priority only");
    std::vector<hipStream_t> cls[3];           // [class + 1][lane]; normal: the lanes' own
    for (RtCtx* c : g->lane) cls[1].push_back(c->home);
    auto drop = [&](int k) { for (hipStream_t s : cls[k + 1]) if (s) (void)hipStreamDestroy(s); cls[k + 1].clear(); };
    auto make = [&](int k) {
        for (int m = 0; m < n; m++) {
            hipStream_t s = nullptr;
            const hipError_t e = hipStreamCreateWithPriority(&s, hipStreamNonBlocking, k == kClassLow ? least : greatest);
            if (e != hipSuccess) { drop(k); return fail(RT_E_DEVICE, "rt_group_create: hipStreamCreateWithPriority failed: %s", hipGetErrorString(e)); }
            cls[k + 1].push_back(s);
        }
        return (int)RT_OK;
    };
    std::vector<hipStream_t> set;              // the concurrent streams
    std::vector<int> worker;                   // and whose they are
    int bestClass = kClassNormal;
    auto measure = [&](int k) {
        std::vector<hipStream_t> s;
        std::vector<int> w = grow_concurrent(g, s, cls[k + 1]);
        g->seen[k + 1] = (int)w.size();
        // a tie with normal keeps normal; between the other two, kPreferClass
        if (set.empty() || w.size() > set.size() || (w.size() == set.size() && bestClass != kClassNormal && k == kPreferClass)) { set = s; worker = w; bestClass = k; }
    };
    if (want == kClassLow || want == kClassHigh) {
        const int rc = make(want); if (rc != RT_OK) return rc;
        measure(want);
    } else {
        measure(kClassNormal);
        if (want != kClassNormal && classes && (int)set.size() < n)
            for (int k : { kClassLow, kClassHigh }) {
                const int rc = make(k); if (rc != RT_OK) { drop(kClassLow); return rc; }
                measure(k);
            }
    }
    std::vector<hipStream_t> home = cls[bestClass + 1];
    g->laneClass.assign((size_t)n, bestClass);
    if (mixed && classes && (int)set.size() < n) {   // (only the measured choice is extended, and it has tried every class by now)
        for (int m = 0; m < n; m++) {
            if (std::find(worker.begin(), worker.end(), m) != worker.end()) continue;
            for (int k : { kClassNormal, kClassLow, kClassHigh }) {
                if (k == bestClass) continue;
                if (grow_concurrent(g, set, { cls[k + 1][(size_t)m] }).empty()) continue;
                worker.push_back(m); home[(size_t)m] = cls[k + 1][(size_t)m]; g->laneClass[(size_t)m] = k;
                break;
            }
        }
    }
    // every lane its stream; the streams of the classes not kept go, so that their hardware queues are released
    for (int m = 0; m < n; m++) {
        RtCtx* c = g->lane[(size_t)m];
        for (int k = 0; k < 3; k++) if (!cls[k].empty() && cls[k][(size_t)m] == home[(size_t)m]) cls[k][(size_t)m] = nullptr;
        if (c->home == home[(size_t)m]) continue;
        cls[1][(size_t)m] = nullptr;
        HIPCHK(hipStreamSynchronize(c->home));   // the naps
        HIPCHK(hipStreamDestroy(c->home));
        c->home = c->stream = home[(size_t)m];
    }
    cls[1].clear();                            // (what is left there is some lane's home)
    drop(kClassLow); drop(kClassHigh);
    g->worker = worker;
    return RT_OK;
}

extern "C" int rt_group_create(const RtConfig* cfg, int32_t lanes, RtGroup** out)
{
    if (!cfg || !out) return fail(RT_E_INVALID, "rt_group_create: null argument");
    if (lanes < 1 || lanes > kMaxLanes) return fail(RT_E_INVALID, "rt_group_create: lanes must be 1..%d", kMaxLanes);
    int want = kClassNormal;
    bool any = true, mixed = kMixedByDefault;   // any: the class is the measurement's choice
    if (const char* t = getenv("RT355_GROUP_PRIORITY")) {   // forces a class (tests, A/B runs)
        const std::string v(t);
        if (v == "normal") any = false;
        else if (v == "low") { any = false; want = kClassLow; }
        else if (v == "high") { any = false; want = kClassHigh; }
        else if (v == "mixed") mixed = true;
        else if (v != "auto" && !v.empty()) return fail(RT_E_INVALID, "rt_group_create: RT355_GROUP_PRIORITY=%s is none of normal, low, high, auto, mixed", t);
    }
    if (!any) mixed = false;
    std::unique_ptr<RtGroup, void (*)(RtGroup*)> guard(new RtGroup(), group_free);
    RtGroup* g = guard.get();
    for (int m = 0; m < lanes; m++) {
        RtConfig c = *cfg;
        if (lanes > 1) {   // contexts that share the GPU get the footprints that fit BESIDE each other
            if (c.shade_blocks_per_cu == 0) c.shade_blocks_per_cu = 1;
        }
        if (m > 0) c.profile = 0;   // HIP-event brackets on the first lane only
        RtCtx* ctx = nullptr;
        const int rc = rt_create(&c, &ctx);
        if (rc != RT_OK) return rc;
        g->lane.push_back(ctx);
        for (auto* ev : { &g->done, &g->moved }) {
            hipEvent_t e;
            if (hipEventCreateWithFlags(&e, hipEventDisableTiming) != hipSuccess) return fail(RT_E_DEVICE, "rt_group_create: hipEventCreate failed");
            ev->push_back(e);
        }
    }
    const size_t px = (size_t)cfg->width * cfg->height;
    if (hipMalloc((void**)&g->sum, px * sizeof(float4)) != hipSuccess) return fail(RT_E_NOMEM, "rt_group_create: hipMalloc of the group accumulator failed");
    HIPCHK(hipMemset(g->sum, 0, px * sizeof(float4)));
    {
        const int rc = choose_streams(g, any ? kClassMixed : want, mixed);
        if (rc != RT_OK) return rc;
    }
    if (const char* t = getenv("RT355_GROUP_STREAMS")) {   // at most this many workers (tests of the routing; A/B runs)
        const int k = atoi(t);
        if (k >= 1 && k < (int)g->worker.size()) g->worker.resize((size_t)k);
    }
    g->concurrent = (int)g->worker.size();
    // the persistent traversal grids (sized at scene upload) of S concurrent lanes: S grids beside each other.  2 per CU was tuned
    // for four; 3 for three or fewer (profiles/r04_group_streams.txt; at S = 4 on today's kernels 2 and 3 are equal, r08_group_priority.txt)
    if (lanes > 1 && cfg->persist_blocks_per_cu == 0)
        for (RtCtx* c : g->lane) c->cfg.persist_blocks_per_cu = g->concurrent >= 4 ? 2 : 3;
    if (g->concurrent < lanes) {
        static bool warned = false;
        if (!warned) {
            warned = true;
            static const char* const name[] = { "low", "normal", "high", "mixed" };
            const char* q = getenv("GPU_MAX_HW_QUEUES");
            fprintf(stderr, "librt355: %d lanes requested but only %d of their HIP streams run concurrently (stream priority class: %s; measured per class: "
                            "low %d, normal %d, high %d, -1 = not tried; HIP serialises streams that share a hardware queue and keeps up to "
                            "GPU_MAX_HW_QUEUES=%s of them per priority class, the normal class's shared with the process's other streams)\n",
                    lanes, g->concurrent, name[rt_group_stream_class(g) + 1], g->seen[0], g->seen[1], g->seen[2], q ? q : "4 (unset)");
        }
    }
    {   // lane m starts on sample stream m, as rt_group_seed(g, 0) leaves it
        const int rc = rt_group_seed(g, 0);
        if (rc != RT_OK) return rc;
    }
    *out = guard.release();
    return RT_OK;
}
extern "C" int rt_group_destroy(RtGroup* g) { group_free(g); return RT_OK; }
extern "C" int rt_group_lanes(RtGroup* g) { return g ? (int)g->lane.size() : 0; }
extern "C" int rt_group_concurrency(RtGroup* g) { return g ? g->concurrent : 0; }
extern "C" int rt_group_stream_class(RtGroup* g)
{
    if (!g || g->laneClass.empty()) return kClassNormal;
    for (int k : g->laneClass) if (k != g->laneClass[0]) return kClassMixed;
    return g->laneClass[0];
}
extern "C" int rt_group_class_concurrency(RtGroup* g, int32_t cls) { return g && cls >= kClassLow && cls <= kClassHigh ? g->seen[cls + 1] : -1; }
extern "C" RtCtx* rt_group_lane(RtGroup* g, int32_t m) { return g && m >= 0 && m < (int)g->lane.size() ? g->lane[(size_t)m] : nullptr; }
extern "C" uint64_t rt_group_frames(RtGroup* g) { return g ? g->frames : 0; }

static int share_lane0(RtGroup* g, int rc)   // the other lanes take the copy lane 0 has bound; rc: what lane 0's upload returned
{
    for (size_t m = 1; m < g->lane.size() && rc == RT_OK; m++) rc = rt_share_scene(g->lane[m], g->lane[0]);   // ONE device copy
    return rc;
}
extern "C" int rt_group_upload_scene(RtGroup* g, const RtPrimitive* prims, int32_t nPrims, const RtMaterial* mats, int32_t nMats,
                                     const RtFloat4* textures, int32_t nTexels, const uint32_t* lights, int32_t nLights,
                                     const void* bvhNodes, int32_t nNodes, const uint32_t* primIdx, int32_t nIdx,
                                     const RtTLASNode* tlas, int32_t nTlas, const RtBVHInstance* blas, int32_t nBlas)
{
    if (!g) return fail(RT_E_INVALID, "rt_group_upload_scene: null group");
    return share_lane0(g, rt_upload_scene(g->lane[0], prims, nPrims, mats, nMats, textures, nTexels, lights, nLights, bvhNodes, nNodes, primIdx, nIdx, tlas, nTlas, blas, nBlas));
}
extern "C" int rt_group_upload_scene_bvh2(RtGroup* g, const RtPrimitive* prims, int32_t nPrims, const RtMaterial* mats, int32_t nMats,
                                          const RtFloat4* textures, int32_t nTexels, const uint32_t* lights, int32_t nLights,
                                          const RtBVHNode2* bvhNodes, int32_t nNodes, const uint32_t* primIdx, int32_t nIdx,
                                          const RtTLASNode* tlas, int32_t nTlas, const RtBVHInstance* blas, int32_t nBlas)
{
    if (!g) return fail(RT_E_INVALID, "rt_group_upload_scene_bvh2: null group");
    return share_lane0(g, rt_upload_scene_bvh2(g->lane[0], prims, nPrims, mats, nMats, textures, nTexels, lights, nLights, bvhNodes, nNodes, primIdx, nIdx, tlas, nTlas, blas, nBlas));
}
// Another group on the same device (e.g. another row band of the frame) renders from the device copy `from` holds.
extern "C" int rt_group_share_scene(RtGroup* g, RtGroup* from)
{
    if (!g || !from) return fail(RT_E_INVALID, "rt_group_share_scene: null group");
    for (RtCtx* c : g->lane) { const int rc = rt_share_scene(c, from->lane[0]); if (rc != RT_OK) return rc; }
    return RT_OK;
}
extern "C" int rt_group_update_scene(RtGroup* g, const RtPrimitive* prims, int32_t first, int32_t count, const RtBVHInstance* blas, int32_t nBlas,
                                     RtUpdateStats* stats)
{
    if (!g) return fail(RT_E_INVALID, "rt_group_update_scene: null group");
    return rt_update_scene(rt_group_lane(g, 0), prims, first, count, blas, nBlas, stats);   // every lane holds lane 0's copy
}
extern "C" int rt_group_rebuild_scene(RtGroup* g, const RtPrimitive* prims, int32_t first, int32_t count, const RtBVHInstance* blas, int32_t nBlas,
                                      int32_t builder, const RtBuildOptions* opts, RtRebuildStats* stats)
{
    if (!g) return fail(RT_E_INVALID, "rt_group_rebuild_scene: null group");
    return rt_rebuild_scene(rt_group_lane(g, 0), prims, first, count, blas, nBlas, builder, opts, stats);   // every lane holds lane 0's copy
}
extern "C" int rt_group_rebuild_ranges(RtGroup* g, const RtPrimitive* prims, int32_t first, int32_t count, const RtBVHInstance* blas, int32_t nBlas,
                                       const int32_t* plan, int32_t nRanges, const RtBuildOptions* opts, RtRebuildStats* stats)
{
    if (!g) return fail(RT_E_INVALID, "rt_group_rebuild_ranges: null group");
    return rt_rebuild_ranges(rt_group_lane(g, 0), prims, first, count, blas, nBlas, plan, nRanges, opts, stats);   // every lane holds lane 0's copy
}
extern "C" int rt_group_update_geometry(RtGroup* g, const RtGeometry* geometry, const RtBVHInstance* blas, int32_t nBlas, RtUpdateStats* stats)
{
    if (!g) return fail(RT_E_INVALID, "rt_group_update_geometry: null group");
    return rt_update_geometry(rt_group_lane(g, 0), geometry, blas, nBlas, stats);   // every lane holds lane 0's copy
}
extern "C" int rt_group_rebuild_geometry(RtGroup* g, const RtGeometry* geometry, const RtBVHInstance* blas, int32_t nBlas, int32_t builder, const RtBuildOptions* opts,
                                         RtRebuildStats* stats)
{
    if (!g) return fail(RT_E_INVALID, "rt_group_rebuild_geometry: null group");
    return rt_rebuild_geometry(rt_group_lane(g, 0), geometry, blas, nBlas, builder, opts, stats);   // every lane holds lane 0's copy
}
extern "C" int rt_group_rebuild_geometry_ranges(RtGroup* g, const RtGeometry* geometry, const RtBVHInstance* blas, int32_t nBlas, const int32_t* plan, int32_t nRanges,
                                                const RtBuildOptions* opts, RtRebuildStats* stats)
{
    if (!g) return fail(RT_E_INVALID, "rt_group_rebuild_geometry_ranges: null group");
    return rt_rebuild_geometry_ranges(rt_group_lane(g, 0), geometry, blas, nBlas, plan, nRanges, opts, stats);   // every lane holds lane 0's copy
}
extern "C" int rt_group_resize_scene(RtGroup* g, const void* prims, int32_t nPrims, const RtSceneShape* shape, int32_t builder, const RtBuildOptions* opts,
                                     RtRebuildStats* stats)
{
    if (!g) return fail(RT_E_INVALID, "rt_group_resize_scene: null group");
    return rt_resize_scene(rt_group_lane(g, 0), prims, nPrims, shape, builder, opts, stats);   // every lane holds lane 0's copy
}
extern "C" int rt_group_update_materials(RtGroup* g, const RtMaterialUpdate* update, RtMaterialStats* stats)
{
    if (!g) return fail(RT_E_INVALID, "rt_group_update_materials: null group");
    return rt_update_materials(rt_group_lane(g, 0), update, stats);   // every lane holds lane 0's copy
}

// Lane m renders sample stream `firstStream + m`: its seeds are outputs (firstStream + m) * W*H + firstPixel + i + 1 of the reference's
// host xorshift32 stream (renderer.cpp:195-196).  A single Renderer has firstStream 0; rank r of a sample-partitioned job r * lanes.
extern "C" int rt_group_seed(RtGroup* g, uint64_t firstStream)
{
    if (!g) return fail(RT_E_INVALID, "rt_group_seed: null group");
    const RtCtx* c0 = g->lane[0];
    const uint64_t P = (uint64_t)c0->cfg.width * (uint64_t)c0->cfg.height;
    uint32_t x = 0x12345678u; // template/template.cpp:711
    auto next = [&x]() { x ^= x << 13; x ^= x >> 17; x ^= x << 5; return x; };
    uint64_t pos = 0;
    std::vector<uint32_t> s((size_t)c0->nPix);
    for (size_t m = 0; m < g->lane.size(); m++) {
        const uint64_t first = (firstStream + m) * P + (uint64_t)c0->firstPixel;
        for (; pos < first; pos++) next();
        for (auto& v : s) v = next();
        pos += s.size();
        const int rc = rt_set_seeds(g->lane[m], s.data(), (int64_t)s.size());
        if (rc != RT_OK) return rc;
    }
    return RT_OK;
}
extern "C" int rt_group_reset(RtGroup* g)
{
    if (!g) return fail(RT_E_INVALID, "rt_group_reset: null group");
    for (RtCtx* c : g->lane) { const int rc = rt_reset(c); if (rc != RT_OK) return rc; }
    g->frames = 0; g->nextLane = 0; g->nextWorker = 0;
    return RT_OK;
}
// `frames` frames in all, dealt to the lanes round-robin (continuing where the last call stopped) and queued interleaved, so that the
// lanes' kernels overlap on the GPU.  Asynchronous.  After k frames in total the group accumulator holds the sum of k samples per
// pixel: prep() divides by k (postproc.cl:71), exactly as with one stream.
extern "C" int rt_group_render(RtGroup* g, const RtCamera* cam, const RtSettings* settings, int32_t frames)
{
    if (!g || !cam) return fail(RT_E_INVALID, "rt_group_render: null argument");
    if (frames <= 0) return fail(RT_E_INVALID, "rt_group_render: frames must be > 0");
    const int n = (int)g->lane.size(), S = (int)g->worker.size();
    HIPCHK(hipSetDevice(g->lane[0]->cfg.device));
    for (int f = 0; f < frames; f++) {
        RtCtx* c = g->lane[(size_t)g->nextLane];
        hipEvent_t moved = g->moved[(size_t)g->nextLane];
        const hipStream_t w = g->lane[(size_t)g->worker[(size_t)g->nextWorker]]->home;
        if (S == n) {   // frame j's worker is lane j's own stream
            const int rc = rt_render(c, cam, settings, 1);
            if (rc != RT_OK) return rc;
        } else {
            if (c->stream != w) {
                // `moved` marks the end of the lane's last frame; the frames of other lanes queued behind it on that stream must not
                // be waited for.  Work the lane queued after its frame (a reset, the group sum) sits behind them and must be.
                if (c->queued) HIPCHK(hipEventRecord(moved, c->stream));
                HIPCHK(hipStreamWaitEvent(w, moved, 0));
                c->stream = w;
            }
            const int rc = rt_render(c, cam, settings, 1);
            if (rc != RT_OK) return rc;
            HIPCHK(hipEventRecord(moved, w));
            c->queued = false;
        }
        g->nextLane = (g->nextLane + 1) % n;
        g->nextWorker = (g->nextWorker + 1) % S;
    }
    g->frames += (uint64_t)frames;
    return RT_OK;
}
extern "C" int rt_group_synchronize(RtGroup* g)
{
    if (!g) return fail(RT_E_INVALID, "rt_group_synchronize: null group");
    for (RtCtx* c : g->lane) { const int rc = rt_synchronize(c); if (rc != RT_OK) return rc; }
    return RT_OK;
}
// The lane-ordered sum of the lanes' accumulators, on the device: into `devicePtr` (float4[width*height], e.g. the tensor a
// torch.distributed all_reduce then works on) or, when NULL, into the group's own buffer.  Queued on lane 0's stream behind every
// lane's pending frames; rt_group_synchronize (or rt_group_read_accum) waits for it.
extern "C" int rt_group_sum(RtGroup* g, void* devicePtr)
{
    if (!g) return fail(RT_E_INVALID, "rt_group_sum: null group");
    RtCtx* c0 = g->lane[0];
    HIPCHK(hipSetDevice(c0->cfg.device));
    const int n = (int)g->lane.size();
    for (int m = 1; m < n; m++) { HIPCHK(hipEventRecord(g->done[(size_t)m], g->lane[(size_t)m]->stream)); HIPCHK(hipStreamWaitEvent(c0->stream, g->done[(size_t)m], 0)); }
    const float4* a[kMaxLanes];
    for (int m = 0; m < kMaxLanes; m++) a[m] = g->lane[(size_t)std::min(m, n - 1)]->q.accum;
    hipLaunchKernelGGL(k_sum_lanes, grid_for(c0->nPix), dim3(kBlock), 0, c0->stream, devicePtr ? (float4*)devicePtr : g->sum,
                       a[0], a[1], a[2], a[3], a[4], a[5], a[6], a[7], n, c0->firstPixel, c0->nPix);
    HIPCHK(hipGetLastError());
    // the lanes must not start overwriting their accumulators before the sum has read them
    HIPCHK(hipEventRecord(g->done[0], c0->stream));
    for (int m = 1; m < n; m++) HIPCHK(hipStreamWaitEvent(g->lane[(size_t)m]->stream, g->done[0], 0));
    for (RtCtx* c : g->lane) c->queued = true;
    return RT_OK;
}
extern "C" int rt_group_read_accum(RtGroup* g, RtFloat4* out)
{
    if (!g || !out) return fail(RT_E_INVALID, "rt_group_read_accum: null argument");
    int rc = rt_group_sum(g, nullptr); if (rc != RT_OK) return rc;
    rc = rt_group_synchronize(g); if (rc != RT_OK) return rc;
    const RtCtx* c0 = g->lane[0];
    HIPCHK(hipMemcpy(out, g->sum, sizeof(float4) * (size_t)c0->cfg.width * c0->cfg.height, hipMemcpyDeviceToHost));
    return RT_OK;
}
extern "C" int rt_group_focus(RtGroup* g, int32_t x, int32_t y, const RtCamera* cam, float* t) { return g ? rt_focus(g->lane[0], x, y, cam, t) : fail(RT_E_INVALID, "rt_group_focus: null group"); }
// Renderer::PostProc + SaveFrame over the group's accumulator; `frames` is the group's frame count (rt_group_frames) unless > 0.
extern "C" int rt_group_postproc(RtGroup* g, int32_t frames, float vignette, float gamma, float chromatic, RtFloat4* outF32, uint8_t* outRGBA8)
{
    if (!g) return fail(RT_E_INVALID, "rt_group_postproc: null group");
    RtCtx* c0 = g->lane[0];
    const float4* accum = c0->q.accum;   // one lane: its accumulator is the group's
    if (g->lane.size() > 1) { const int rc = rt_group_sum(g, nullptr); if (rc != RT_OK) return rc; accum = g->sum; }
    return postproc(c0, accum, frames > 0 ? frames : (int32_t)std::max<uint64_t>(g->frames, 1), vignette, gamma, chromatic, outF32, outRGBA8);
}

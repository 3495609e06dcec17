// rt355.hip — the rendering context of the C-ABI (include/rt355.h; RtCtx, ctx.h): its device memory and stream, the traversal
// configuration it derives from the scene copy it holds (scene.hip) and trace_launch, which maps a stage to a kernel launch; the stages
// and rt_render, rt_trace, the read-backs and debug exports, post-processing.  Every kernel of a frame is compiled here
// (rt355_kernels.h).  This is the replacement for the reference's OpenCL Kernel/Buffer dispatch in Renderer
// (src/renderer.cpp:64-94,142-263,289-301).  No CPU fallback exists here.  Lane groups live in group.hip, the math probes in math_debug.hip.
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>
#include <algorithm>
#include <cstdio>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <atomic>
#include <string>
#include <vector>
#include "../../include/rt355.h"
#include "rt355_kernels.h"
#include "ctx.h"
#include "geometry_common.h"

using namespace rt355dev;
using namespace scenedev;

// (the Traversal kinds, their constants and the column arithmetic: trav_common.h, which cannot see the kernels' own sizes)
static_assert(kColumnLanes == kBlock && kTopLevelsMax == kTopMaxLevels && sizeof(float4) * 4 == 64, "trav_common.h computes with the kernels' sizes");
static thread_local std::string g_err;
int rt355_set_error(int code, const char* msg) { g_err = msg; return code; }   // for every source file of this library (fail, build_fail)

template <bool REFB> static void choose_builtin_kernels_of(RtCtx* ctx)
{
    const bool nee = ctx->cfg.shading == RT_SHADING_NEE, small = ctx->shadeTile == 256;
    ctx->kGenerate = k_generate<REFB>;
    ctx->kShade = nee ? (small ? k_shade<true, 256, REFB> : k_shade<true, kTile, REFB>) : (small ? k_shade<false, 256, REFB> : k_shade<false, kTile, REFB>);
    ctx->kFocus = ctx->cfg.accel == RT_ACCEL_BVH4 ? k_focus<RT_ACCEL_BVH4, REFB> : k_focus<RT_ACCEL_BVH2, REFB>;
    ctx->kTracePrimary[RtCtx::PRIMARY_PLAIN] = k_trace_primary<REFB, false, false>;
    ctx->kTracePrimary[RtCtx::PRIMARY_COHERENT] = k_trace_primary<REFB, true, false>;
    ctx->kTracePrimary[RtCtx::PRIMARY_BVH4] = k_trace_primary<REFB, false, true>;
    ctx->kShadePrimary = nee ? (small ? k_shade<true, 256, REFB, true> : k_shade<true, kTile, REFB, true>) : (small ? k_shade<false, 256, REFB, true> : k_shade<false, kTile, REFB, true>);
}
static void choose_builtin_kernels(RtCtx* ctx)   // needs cfg (builtins resolved) and shadeTile
{
    if (ctx->cfg.builtins == RT_BUILTINS_REFERENCE) choose_builtin_kernels_of<true>(ctx);
    else choose_builtin_kernels_of<false>(ctx);
}
enum { ST_GENERATE, ST_EXTEND, ST_SHADE, ST_COMPACT, ST_CONNECT, ST_ACCUM };

extern "C" const char* rt_last_error(void) { return g_err.c_str(); }
extern "C" int rt_device_count(void) { int n = 0; if (hipGetDeviceCount(&n) != hipSuccess) return 0; return n; }
static int sync_scene_config(RtCtx* ctx);
extern "C" int rt_builtins(RtCtx* ctx)
{
    if (!ctx) return fail(RT_E_INVALID, "rt_builtins: null context");
    return ctx->cfg.builtins;
}
extern "C" int rt_kernel_info(RtCtx* ctx, RtKernelInfo* out)
{
    if (!ctx || !out) return fail(RT_E_INVALID, "rt_kernel_info: null argument");
    if (!ctx->sceneLoaded) return fail(RT_E_INVALID, "rt_kernel_info: no scene uploaded");
    if (const int rc = sync_scene_config(ctx)) return rc;
    const int persist = ctx->trav <= TRAV_TLAS_SPILL ? ctx->trav : 0;
    const int persist4 = ctx->trav == TRAV_BVH4 ? 1 : (ctx->trav == TRAV_BVH4_TLAS ? 2 : (ctx->trav == TRAV_BVH4_TLAS_SPILL ? 3 : 0));
    *out = RtKernelInfo{ ctx->facts.layout, persist, persist4, spill_trav(ctx->trav) ? ctx->spillCap : ctx->facts.stackEntries, ctx->persistGrid, ctx->persistGridConnect,
                         ctx->shadeGrid, ctx->sc.nBlas };
    return RT_OK;
}

extern "C" int rt_top_levels(RtCtx* ctx, int32_t* extend, int32_t* connect)
{
    if (!ctx || !extend || !connect) return fail(RT_E_INVALID, "rt_top_levels: null argument");
    if (!ctx->sceneLoaded) return fail(RT_E_INVALID, "rt_top_levels: no scene uploaded");
    if (const int rc = sync_scene_config(ctx)) return rc;
    *extend = ctx->tune.topLevels; *connect = ctx->tuneConnect.topLevels;
    return RT_OK;
}

static int beside_shade(const RtCtx* c, int stage, int topLevels, int* perCU, int* shadeLds);
extern "C" int rt_shade_footprint(RtCtx* ctx, int32_t* ldsBytes, int32_t* traversalBeside)
{
    if (!ctx || !ldsBytes || !traversalBeside) return fail(RT_E_INVALID, "rt_shade_footprint: null argument");
    if (!ctx->sceneLoaded) return fail(RT_E_INVALID, "rt_shade_footprint: no scene uploaded");
    if (const int rc = sync_scene_config(ctx)) return rc;
    *ldsBytes = 0; *traversalBeside = 0;
    if (!persistent(ctx->trav)) {   // no persistent grid to count: the footprint alone
        hipFuncAttributes a{};
        HIPCHK(hipFuncGetAttributes(&a, (const void*)ctx->kShade));
        *ldsBytes = (int32_t)a.sharedSizeBytes;
        return RT_OK;
    }
    int lds = 0, beside = 0;
    if (const int rc = beside_shade(ctx, ST_EXTEND, 0, &beside, &lds)) return rc;
    *ldsBytes = lds; *traversalBeside = beside;
    return RT_OK;
}

extern "C" int rt_shade_tables(RtCtx* ctx, int32_t* capacityRows, int32_t* staged)
{
    if (!ctx || !capacityRows || !staged) return fail(RT_E_INVALID, "rt_shade_tables: null argument");
    if (!ctx->sceneLoaded) return fail(RT_E_INVALID, "rt_shade_tables: no scene uploaded");
    if (const int rc = sync_scene_config(ctx)) return rc;
    *capacityRows = kShadeTableRows;
    *staged = ctx->var.shadeTables != 0 && shade_tables_fit(ctx->sc.nLights, ctx->sc.nMats);   // k_shade's own rule, from the arguments it is launched with
    return RT_OK;
}

extern "C" int rt_primary_fused(RtCtx* ctx, int32_t* fused)
{
    if (!ctx || !fused) return fail(RT_E_INVALID, "rt_primary_fused: null argument");
    if (!ctx->sceneLoaded) return fail(RT_E_INVALID, "rt_primary_fused: no scene uploaded");
    if (const int rc = sync_scene_config(ctx)) return rc;
    *fused = ctx->fusePrimary ? 1 : 0;   // what rt_render reads
    return RT_OK;
}

static void free_bag(std::vector<void*>& bag) { for (void* p : bag) (void)hipFree(p); bag.clear(); }

// A context holds at most one device copy of a scene; the copy knows its holders (rt_update_scene waits for them and reconfigures them).
static void scene_release(RtCtx* ctx)
{
    if (!ctx->scene) return;
    auto& h = ctx->scene->holders;
    h.erase(std::remove(h.begin(), h.end(), ctx), h.end());
    ctx->scene.reset();
}
static void scene_hold(RtCtx* ctx, const std::shared_ptr<SceneBag>& bag)
{
    scene_release(ctx);
    ctx->scene = bag;
    bag->holders.push_back(ctx);
}
// What scene.hip needs of the holders before it commits an update or a rebuild: no kernel of theirs reads the arrays any more
int SceneBag::wait_holders() const
{
    for (const RtCtx* h : holders) {
        HIPCHK(hipStreamSynchronize(h->stream));
        if (h->home != h->stream) HIPCHK(hipStreamSynchronize(h->home));
    }
    return RT_OK;
}

// The dynamic LDS of a context's TLAS kernels: its column entries (trav_common.h) with the world-ray backup behind them
static int tlas_lds_entries(const RtCtx* c) { return tlas_lds_entries(c->trav, c->spillCap, c->facts.stackEntries, c->facts.tlasDepth); }
static size_t tlas_stack_bytes(const RtCtx* c) { return tlas_column_bytes(tlas_lds_entries(c)); }

// The traversal launch of a stage: the one place that maps (stage, bounce, steps wanted) to a kernel instantiation, its grid, its dynamic
// LDS and its PersistTune.  A persistent kernel takes (scene, queues, b0, b1, renderBVH, tune); where none runs, the nested one-ray-per-lane
// kernel takes (scene, queues, bounce, renderBVH) for extend and (scene, queues, b0, b1) for connect.  `rays`: the stage's queue capacity.
using PersistKernel = void (*)(DevScene, DevQueues, int, int, int, PersistTune);
using NestedKernel = void (*)(DevScene, DevQueues, int, int);
using PrimaryKernel = void (*)(DevScene, DevQueues, RtCamera, int, int, PersistTune);   // (scene, queues, camera, antiAliasing, renderBVH, tune)
struct TraceLaunch {
    PersistKernel persist = nullptr;
    NestedKernel nested = nullptr;
    PrimaryKernel primary = nullptr;   // set INSTEAD of `persist`, only where asked for (`primary`) and the context fuses (RtCtx.fusePrimary)
    dim3 grid;
    size_t lds = 0;
    PersistTune tune{};
};
static TraceLaunch trace_launch(const RtCtx* c, int stage, int bounce, bool steps, int rays, int topLevels = -1 /* >= 0: as if the stage's PersistTune.topLevels were this */,
                                bool primary = false /* rt_render's extend(0): the launch that computes the primary rays, where the context fuses */)
{
    TraceLaunch L;
    L.grid = grid_for(rays);
    L.lds = stack_bytes(c->facts.stackEntries);
    const bool connect = stage == ST_CONNECT;
    const bool bvh4 = c->cfg.accel == RT_ACCEL_BVH4, l1 = c->facts.layout == 1;
    bool top = false;
    switch (c->trav) {
    case TRAV_NESTED:
        if (connect) L.nested = bvh4 ? (l1 ? k_connect<RT_ACCEL_BVH4, 1> : k_connect<RT_ACCEL_BVH4, 0>) : (l1 ? k_connect<RT_ACCEL_BVH2, 1> : k_connect<RT_ACCEL_BVH2, 0>);
        else L.nested = bvh4 ? (l1 ? k_extend<RT_ACCEL_BVH4, 1> : k_extend<RT_ACCEL_BVH4, 0>) : (l1 ? k_extend<RT_ACCEL_BVH2, 1> : k_extend<RT_ACCEL_BVH2, 0>);
        break;
    case TRAV_BVH2:
        L.tune = connect ? c->tuneConnect : c->tune;
        if (topLevels >= 0) L.tune.topLevels = topLevels;
        // (topLevels > 0: the TOP instantiations of the launches whose long queues run the event loop; the table lies behind the stack columns)
        if (connect) { top = L.tune.topLevels > 0; L.persist = top ? k_trace_persist<true, false, false, true> : k_trace_persist<true>; L.grid = dim3(c->persistGridConnect); }
        else if (bounce > 0 || c->cfg.extend_variant == 3) {
            top = L.tune.topLevels > 0;
            if (top) L.persist = steps ? k_trace_persist<false, false, true, true> : k_trace_persist<false, false, false, true>;
            else L.persist = steps ? k_trace_persist<false, false, true> : k_trace_persist<false>;
            L.grid = dim3(c->persistGrid);
        }
        else if (c->cfg.extend_variant == 5) L.nested = k_extend<RT_ACCEL_BVH2, 1>;
        // bounce 0 through the same kernel with one workgroup per 256 rays: its "queue not longer than the grid" branch is the plain
        // one-ray-per-lane loop without the TLAS code of k_extend (60 instead of 86 VGPRs: 8 instead of 5 waves per SIMD)
        else if (primary && c->fusePrimary) L.primary = c->kTracePrimary[c->coherent ? RtCtx::PRIMARY_COHERENT : RtCtx::PRIMARY_PLAIN];   // (the same branch, rays computed)
        else L.persist = c->coherent ? k_trace_persist<false, true> : (steps ? k_trace_persist<false, false, true> : k_trace_persist<false>);
        if (top) { L.tune.topBase = c->facts.stackEntries * kBlock; L.lds += top_bytes(L.tune.topLevels); }
        break;
    case TRAV_BVH4:
        L.tune = connect ? c->tuneConnect : c->tune4;
        L.persist = connect ? k_trace_persist4<true> : k_trace_persist4<false>;
        if (connect || bounce > 0) L.grid = dim3(connect ? c->persistGridConnect : c->persistGrid);
        else if (primary && c->fusePrimary) { L.persist = nullptr; L.primary = c->kTracePrimary[RtCtx::PRIMARY_BVH4]; }
        break;
    case TRAV_TLAS:
    case TRAV_TLAS_SPILL: {
        const bool spill = c->trav == TRAV_TLAS_SPILL;
        L.lds = tlas_stack_bytes(c);
        if (connect) {
            L.tune = c->tuneConnect;
            L.persist = spill ? k_trace_persist_tlas<true, false, true> : k_trace_persist_tlas<true>;
            L.grid = dim3(c->persistGridConnect);
            break;
        }
        L.tune = c->tune;
        // bounce 0 with one workgroup per 256 rays: the kernel's short-queue branch (coherent primary rays); every SPILL launch runs on
        // the persistent grid, which bounds the global stack columns
        if (bounce > 0 || spill) L.grid = dim3(c->persistGrid);
        const bool coh = c->coherent && (bounce == 0 || c->coherent == 2) && (c->tune.flat || !spill);   // (through the one-ray-per-lane branch)
        if (steps) L.persist = spill ? k_trace_persist_tlas<false, true, true> : k_trace_persist_tlas<false, true>;
        else if (coh) L.persist = spill ? k_trace_persist_tlas<false, false, true, true> : k_trace_persist_tlas<false, false, false, true>;
        else L.persist = spill ? k_trace_persist_tlas<false, false, true> : k_trace_persist_tlas<false>;
        break;
    }
    case TRAV_BVH4_TLAS:
    case TRAV_BVH4_TLAS_SPILL: {
        const bool spill = c->trav == TRAV_BVH4_TLAS_SPILL;
        L.lds = tlas_stack_bytes(c);
        if (connect) {
            L.tune = c->tuneConnect;
            L.persist = spill ? k_trace_persist4_tlas<true, false, true> : k_trace_persist4_tlas<true>;
            L.grid = dim3(c->persistGridConnect);
            break;
        }
        L.tune = c->tune4;
        if (bounce > 0 || spill) L.grid = dim3(c->persistGrid);   // (as TRAV_TLAS*: every SPILL launch on the persistent grid)
        if (steps) L.persist = spill ? k_trace_persist4_tlas<false, true, true> : k_trace_persist4_tlas<false, true>;
        else L.persist = spill ? k_trace_persist4_tlas<false, false, true> : k_trace_persist4_tlas<false>;
        break;
    }
    }
    return L;
}

// What the occupancy query says of the kernel a stage runs on its persistent grid (workgroups per CU by VGPRs, LDS and wave slots);
// topLevels >= 0: with a top table of that many levels instead of the stage's own
static int persist_query(const RtCtx* c, int stage, int topLevels, int* perCU)
{
    const TraceLaunch L = trace_launch(c, stage, stage == ST_CONNECT ? 0 : 1, false, c->nPix, topLevels);
    HIPCHK(hipOccupancyMaxActiveBlocksPerMultiprocessor(perCU, L.persist, kBlock, L.lds));
    return RT_OK;
}
// Workgroups per CU of a stage's persistent grid, given that answer.  The closest-hit instantiations use ~90 SGPRs, the any-hit ones ~100:
// the hardware admits 7 resp. 6 workgroups per CU where the query may say more (see rt_create); a surplus workgroup would strand its static
// first chunk until another exits.  Contexts that share the GPU take RtConfig.persist_blocks_per_cu at most; RT355_TUNE's fifth field and,
// for connect, RT355_CONNECT_BLOCKS (lab) override both (the plan's tuneBlocks and connectBlocks).
static int persist_blocks(const RtCtx* c, int stage, int perCU)
{
    const bool connect = stage == ST_CONNECT;
    const int fit = std::max(1, perCU);
    int g = std::max(1, std::min(perCU, connect ? kAdmitAnySgpr : kAdmit96Sgpr));
    if (c->cfg.persist_blocks_per_cu > 0) g = std::min(g, std::min(c->cfg.persist_blocks_per_cu, fit));
    if (c->tuneBlocks > 0) g = std::min(c->tuneBlocks, fit);
    if (connect && c->connectBlocks > 0) g = std::min(c->connectBlocks, fit);
    return g;
}

// What shares a CU when the lanes of a group run side by side: the traversal grids of some lanes with a k_shade workgroup of another
// (its grid is one workgroup per CU; a lane spends about a quarter of its time there, so with three lanes in flight one is resident about
// half the time).  *perCU: the workgroups of the stage's persistent kernel, with a top table of `topLevels` levels, that fit a CU beside ONE
// k_shade workgroup of this context's instantiation - by LDS, by the VGPR file (512 per lane and SIMD, allocated in eights; a workgroup of
// 256 threads puts one wave on each SIMD) and by the eight wave slots of a SIMD, capped at what the hardware admits of the kernel anyway.
// *shadeLds: k_shade's static LDS.  Footprints come from the code objects, not from constants; a CU hands its LDS out in blocks of 320
// dwords, which decides at these sizes (measured, tools/lab/lds_census.hip: beside 26,688 B five workgroups of 22,528 B, beside 24,908 B six).
static constexpr size_t kLdsBlock = 1280;
static int beside_shade(const RtCtx* c, int stage, int topLevels, int* perCU, int* shadeLds)
{
    const TraceLaunch L = trace_launch(c, stage, stage == ST_CONNECT ? 0 : 1, false, c->nPix, topLevels);
    hipFuncAttributes shade{}, trav{};
    HIPCHK(hipFuncGetAttributes(&shade, (const void*)c->kShade));
    HIPCHK(hipFuncGetAttributes(&trav, (const void*)L.persist));
    auto alloc = [](int regs) { return std::max(8, (regs + 7) / 8 * 8); };
    const size_t ldsCU = std::max(c->ldsPerCU, c->ldsPerBlock);
    auto blocks = [](size_t bytes) { return (bytes + kLdsBlock - 1) / kLdsBlock * kLdsBlock; };
    const size_t travLds = blocks(trav.sharedSizeBytes + L.lds), shadeLdsCU = blocks(shade.sharedSizeBytes);
    const int shadeWaves = std::max(1, c->shadeTile / kBlock);   // per SIMD
    const int byLds = ldsCU > shadeLdsCU && travLds > 0 ? (int)((ldsCU - shadeLdsCU) / travLds) : 0;
    const int byVgpr = (512 - shadeWaves * alloc(shade.numRegs)) / alloc(trav.numRegs);
    const int bySlots = 8 - shadeWaves;
    *perCU = std::max(0, std::min(std::min(byLds, byVgpr), std::min(bySlots, stage == ST_CONNECT ? kAdmitAnySgpr : kAdmit96Sgpr)));
    *shadeLds = (int)shade.sharedSizeBytes;
    return RT_OK;
}

// ---- profiling brackets --------------------------------------------------------------
// Stage timing: a fixed ring of HIP event pairs on the context's stream.  Recording never forces a device sync: when the ring
// wraps, the oldest pair is harvested (it completed thousands of launches ago; if not, the HOST waits on that one event while the
// GPU keeps draining its queue).
static constexpr size_t kEvRing = 4096;
static void ev_account(RtCtx* c, RtCtx::Ev& e)
{
    float ms = 0;
    if (hipEventElapsedTime(&ms, e.a, e.b) != hipSuccess) { (void)hipEventSynchronize(e.b); (void)hipEventElapsedTime(&ms, e.a, e.b); }
    switch (e.stage) {
    case ST_GENERATE: c->times.generate_ms += ms; c->times.generate_launches++; break;
    case ST_EXTEND:   c->times.extend_ms += ms; c->times.extend_launches++; break;
    case ST_SHADE:    c->times.shade_ms += ms; c->times.shade_launches++; break;
    case ST_COMPACT:  c->times.compact_ms += ms; c->times.compact_launches++; break;
    case ST_CONNECT:  c->times.connect_ms += ms; c->times.connect_launches++; break;
    case ST_ACCUM:    c->times.accumulate_ms += ms; c->times.accumulate_launches++; break;
    }
    e.stage = -1;
}
static void ev_init(RtCtx* c)   // rt_create, so that no event is created inside a timed region
{
    if (!c->cfg.profile || !c->evPool.empty()) return;
    c->evPool.resize(kEvRing);
    for (auto& e : c->evPool) { (void)hipEventCreate(&e.a); (void)hipEventCreate(&e.b); e.stage = -1; }
}
static inline bool ev_on(const RtCtx* c, int stage) { return c->cfg.profile >= 2 || (c->cfg.profile == 1 && stage == ST_EXTEND); }
static void ev_begin(RtCtx* c, int stage)
{
    if (!ev_on(c, stage)) return;
    ev_init(c);
    RtCtx::Ev& e = c->evPool[c->evUsed % kEvRing];
    if (e.stage >= 0) ev_account(c, e);   // ring wrapped: harvest the oldest pair first
    e.stage = stage;
    (void)hipEventRecord(e.a, c->stream);
}
static void ev_end(RtCtx* c, int stage)
{
    if (!ev_on(c, stage)) return;
    (void)hipEventRecord(c->evPool[c->evUsed % kEvRing].b, c->stream);
    c->evUsed++;
}
// A single launch is timed by the events the dispatch itself carries (hipExtLaunchKernelGGL: start/stop are the kernel's own begin/end
// timestamps, no marker packets on the stream - bracketing a launch with hipEventRecord costs ~2 % of a frame at 24 launches).
static RtCtx::Ev& ev_slot(RtCtx* c, int stage)
{
    ev_init(c);
    RtCtx::Ev& e = c->evPool[c->evUsed % kEvRing];
    if (e.stage >= 0) ev_account(c, e);   // ring wrapped: harvest the oldest pair first
    e.stage = stage;
    c->evUsed++;
    return e;
}
#define LAUNCHB(ctx, stage, kernel, grid, block, shmem, ...) do { \
        if (ev_on(ctx, stage)) { RtCtx::Ev& e_ = ev_slot(ctx, stage); hipExtLaunchKernelGGL(kernel, grid, dim3(block), (uint32_t)(shmem), (ctx)->stream, e_.a, e_.b, 0, __VA_ARGS__); } \
        else hipLaunchKernelGGL(kernel, grid, dim3(block), shmem, (ctx)->stream, __VA_ARGS__); \
    } while (0)
#define LAUNCH(ctx, stage, kernel, grid, shmem, ...) LAUNCHB(ctx, stage, kernel, grid, kBlock, shmem, __VA_ARGS__)
static void ev_collect(RtCtx* c) // call after a stream sync
{
    for (auto& e : c->evPool) if (e.stage >= 0) ev_account(c, e);
}

// ---- create / destroy ----------------------------------------------------------------
extern "C" int rt_create(const RtConfig* cfg, RtCtx** out)
{
    if (!cfg || !out) return fail(RT_E_INVALID, "rt_create: null argument");
    if (cfg->width <= 0 || cfg->height <= 0) return fail(RT_E_INVALID, "rt_create: bad resolution %dx%d", cfg->width, cfg->height);
    RtConfig c = *cfg;
    if (c.y1 <= 0) c.y1 = c.height;
    if (c.y0 < 0 || c.y0 >= c.y1 || c.y1 > c.height) return fail(RT_E_INVALID, "rt_create: bad row band [%d,%d)", c.y0, c.y1);
    if (c.max_bounces <= 0) c.max_bounces = RT_MAX_BOUNCES;
    if (c.max_bounces > RT_MAX_BOUNCES) return fail(RT_E_INVALID, "rt_create: max_bounces %d > %d", c.max_bounces, RT_MAX_BOUNCES);
    if ((c.shading != RT_SHADING_SIMPLE && c.shading != RT_SHADING_NEE) || (c.sampling != RT_SAMPLING_HEMISPHERE && c.sampling != RT_SAMPLING_COSINE) ||
        (c.accel != RT_ACCEL_BVH2 && c.accel != RT_ACCEL_BVH4))
        return fail(RT_E_INVALID, "rt_create: unknown kernel variant");
    if (!resolve_builtins(c.builtins, &c.builtins))
        return fail(RT_E_INVALID, "rt_create: RtConfig.builtins = %d is none of RT_BUILTINS_DEFAULT (0), RT_BUILTINS_IEEE (1), RT_BUILTINS_REFERENCE (2)", cfg->builtins);
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0)
        return fail(RT_E_DEVICE, "rt_create: no HIP device visible (this library has no CPU path)");
    if (c.device < 0 || c.device >= ndev) return fail(RT_E_INVALID, "rt_create: device %d out of range (%d visible)", c.device, ndev);
    HIPCHK(hipSetDevice(c.device));
    std::unique_ptr<RtCtx, void (*)(RtCtx*)> guard(new RtCtx(), ctx_free);   // released on success; any early return frees it
    RtCtx* ctx = guard.get();
    ctx->cfg = c;
    ctx->nPix = (c.y1 - c.y0) * c.width;
    ctx->firstPixel = c.y0 * c.width;
    ctx->gridMax = (ctx->nPix * std::max(1, c.max_bounces) + kBlock - 1) / kBlock; // connect may cover max_bounces*nPix shadow rays
    ctx->gridMax = std::max(ctx->gridMax, 4096);                                    // and the persistent grid (<= 256 CUs x 8 blocks)
    ctx->var = DevVariant{ c.shading, c.sampling, c.accel, c.russian_roulette ? 1 : 0, c.filter_fireflies ? 1 : 0, c.max_bounces, 1 };
    const ShadeKnobs knobs = read_shade_knobs();
    if (knobs.tablesSet) ctx->var.shadeTables = knobs.tables;   // 0: k_shade reads lights and materials from global memory (A/B runs)
    {   // k_shade: as many workgroups as the CUs hold at once.  Its ordered scan does not depend on that (tiles go by ticket to
        // running workgroups), so the size only matters for speed.  The occupancy query knows the VGPR, LDS and wave-slot limits
        // but not the SGPR file: 256-thread workgroups are admitted up to min(query, 8, 800 / (ceil16(sgprs) + 16)) per CU
        // (MI355X_MICROARCH.md, residency) = 6 for any kernel (<= 112 SGPRs), 7 up to 96 SGPRs.  k_shade: 2 workgroups of 512 threads (registers; 49.8 KB of LDS each).
        hipDeviceProp_t prop; int perCU = 0;
        HIPCHK(hipGetDeviceProperties(&prop, c.device));
        // (what this file needs of the device, asked once: a reconfiguration reads it from here)
        ctx->cuCount = prop.multiProcessorCount; ctx->ldsPerBlock = prop.sharedMemPerBlock; ctx->ldsPerCU = prop.maxSharedMemoryPerMultiProcessor;
        ctx->shadeTile = c.shade_blocks_per_cu > 0 ? 256 : kTile;
        if (knobs.tile) ctx->shadeTile = knobs.tile;
        choose_builtin_kernels(ctx);
        HIPCHK(hipOccupancyMaxActiveBlocksPerMultiprocessor(&perCU, ctx->kShade, ctx->shadeTile, 0));
        perCU = std::min(perCU, kAdmitAnySgpr);
        ctx->shadeGrid = ctx->cuCount * std::max(1, perCU);
        if (c.shade_blocks_per_cu > 0 && c.shade_blocks_per_cu <= 16) ctx->shadeGrid = ctx->cuCount * c.shade_blocks_per_cu;
        if (knobs.perCU) ctx->shadeGrid = ctx->cuCount * knobs.perCU;   // tuning / over-subscription tests
    }
    hipError_t e = hipStreamCreateWithFlags(&ctx->home, hipStreamNonBlocking);
    if (e != hipSuccess) return fail(RT_E_DEVICE, "hipStreamCreate failed: %s", hipGetErrorString(e));
    ctx->stream = ctx->home;
    DevQueues& q = ctx->q;
    const size_t n = (size_t)ctx->nPix, nS = n * (size_t)c.max_bounces;
    int rc = RT_OK;
    auto& bag = ctx->queueAllocs;
#define QA(field, count) if (rc == RT_OK) rc = dalloc(bag, &q.field, count)
    const size_t nTiles = (n + kBlock - 1) / kBlock;
    for (int k = 0; k < 2; k++) { QA(O[k], n); QA(D[k], n); QA(inten[k], n); QA(meta[k], n); QA(tile[k], nTiles + 2); QA(super[k], nTiles / 64 + 2); QA(supAcc[k], nTiles / 64 + 2); }
    QA(hit, n);
    QA(sA, nS); QA(sB, nS); QA(sC, nS);
    QA(nRays, RT_MAX_BOUNCES + 2); QA(nShadow, RT_MAX_BOUNCES + 2); QA(cursor, kCursorWords); QA(shadeTicket, (size_t)(RT_MAX_BOUNCES + 1) * kTicketClasses * kTicketStride); QA(fault, 1);
    QA(seeds, n); QA(accum, (size_t)c.width * c.height);
    if (rc == RT_OK) rc = dalloc(bag, &ctx->dSteps, n);
    q.steps = nullptr;
    QA(ctrExtend, (size_t)ctx->gridMax * kCtrCols); QA(ctrConnect, (size_t)ctx->gridMax * kCtrCols);
#undef QA
    if (rc == RT_OK) rc = dalloc(bag, &ctx->dFocus, 1);
    if (rc != RT_OK) return rc;
    q.nPix = ctx->nPix; q.firstPixel = ctx->firstPixel; q.width = c.width; q.height = c.height;
    (void)hipMemsetAsync(q.accum, 0, sizeof(float4) * (size_t)c.width * c.height, ctx->stream);
    (void)hipMemsetAsync(q.nRays, 0, sizeof(int32_t) * (RT_MAX_BOUNCES + 2), ctx->stream);
    (void)hipMemsetAsync(q.nShadow, 0, sizeof(int32_t) * (RT_MAX_BOUNCES + 2), ctx->stream);
    (void)hipMemsetAsync(q.cursor, 0, sizeof(int32_t) * kCursorWords, ctx->stream);
    (void)hipMemsetAsync(q.shadeTicket, 0, sizeof(int32_t) * (size_t)(RT_MAX_BOUNCES + 1) * kTicketClasses * kTicketStride, ctx->stream);
    (void)hipMemsetAsync(q.fault, 0, sizeof(int32_t), ctx->stream);
    (void)hipMemsetAsync(q.ctrExtend, 0, sizeof(unsigned long long) * (size_t)ctx->gridMax * kCtrCols, ctx->stream);
    (void)hipMemsetAsync(q.ctrConnect, 0, sizeof(unsigned long long) * (size_t)ctx->gridMax * kCtrCols, ctx->stream);
    for (int k = 0; k < 2; k++) {
        (void)hipMemsetAsync(q.tile[k], 0, sizeof(unsigned long long) * (nTiles + 2), ctx->stream);
        (void)hipMemsetAsync(q.super[k], 0, sizeof(unsigned long long) * (nTiles / 64 + 2), ctx->stream);
        (void)hipMemsetAsync(q.supAcc[k], 0, sizeof(unsigned long long) * (nTiles / 64 + 2), ctx->stream);
    }
    (void)hipMemsetAsync(q.hit, 0, sizeof(float4) * n, ctx->stream);
    HIPCHK(hipStreamSynchronize(ctx->stream));
    // never an unseeded context: state 0 is the RNG's fixed point, and k_shade's sample_ball would not return from it (rt_set_seeds)
    rc = rt_seed_default(ctx);
    if (rc != RT_OK) return rc;
    ev_init(ctx);
    *out = guard.release();
    return RT_OK;
}

void ctx_free(RtCtx* ctx)   // every owned resource; safe on a partially constructed context (ctx.h: group.hip frees its lanes with it)
{
    if (!ctx) return;
    (void)hipSetDevice(ctx->cfg.device);
    if (ctx->stream) (void)hipStreamSynchronize(ctx->stream);
    scene_release(ctx); free_bag(ctx->queueAllocs);
    if (ctx->dRayIO) (void)hipFree(ctx->dRayIO);
    free_bag(ctx->tv.words);
    for (float4* p : ctx->tv.rays) if (p) (void)hipFree(p);
    if (ctx->dSpill) (void)hipFree(ctx->dSpill);
    if (ctx->dPostF) (void)hipFree(ctx->dPostF);
    if (ctx->dPostB) (void)hipFree(ctx->dPostB);
    for (auto& e : ctx->evPool) { if (e.a) (void)hipEventDestroy(e.a); if (e.b) (void)hipEventDestroy(e.b); }
    if (ctx->home) (void)hipStreamDestroy(ctx->home);
    delete ctx;
}
extern "C" int rt_destroy(RtCtx* ctx)
{
    ctx_free(ctx);
    return RT_OK;
}

// ---- the scene: a context holds a device copy (scene.hip) and renders from what it took over of it ------------------------------
// What the traversal plan of a context is a function of (trav_common.h): its configuration, the facts of the copy it holds, its device
static TravFacts traversal_facts(const RtCtx* ctx)
{
    const SceneFacts& s = ctx->facts;   // (what the context adopted, never the live bag's)
    return TravFacts{ ctx->cfg.accel, ctx->cfg.extend_variant, ctx->cfg.persist_blocks_per_cu, s.layout, s.singleBlas, s.tlasDepth, s.nInterior, s.nQuads, s.stackEntries,
                      (int)ctx->ldsPerBlock, ctx->xcdFirst };
}
static void adopt_plan(RtCtx* ctx, const TravPlan& p)
{
    ctx->trav = p.trav; ctx->spillCap = p.spillCap; ctx->coherent = p.coherent;
    ctx->tune = p.tune; ctx->tuneConnect = p.tuneConnect; ctx->tune4 = p.tune4;
    ctx->tuneBlocks = p.tuneBlocks; ctx->connectBlocks = p.connectBlocks;
    ctx->fusePrimary = p.fusePrimary;
}
// The top tables against the device.  One that would not fit behind the stack columns of a very deep tree is left out: no launch the
// runtime would reject.  Then, where no knob named the depth (topAuto):
// The table's LDS can cost a resident workgroup, and on the one scene this was measured on (the bench scene, EXPERIMENTS.md (59):
// alone, 22 KB of stack columns x 7 workgroups leave room for three levels) that costs more than the deeper levels give, while
// contexts that share the GPU run fewer workgroups per CU and lose none with six.  So without the knob each stage gets the
// deepest table with which it keeps the workgroups per CU it has without one.
// The lanes of a group (persist_blocks_per_cu > 0) do not have the CU to themselves: their few workgroups sit there with those of
// the other lanes and, about half the time, with a k_shade workgroup.  What the table must not cost them is a place beside that
// workgroup (beside_shade; EXPERIMENTS.md (60)): the deepest table with which as many fit there as with none.
static int fit_top_tables(RtCtx* ctx, bool topAuto)
{
    for (PersistTune* t : { &ctx->tune, &ctx->tuneConnect }) if (stack_bytes(ctx->facts.stackEntries) + top_bytes(t->topLevels) > ctx->ldsPerBlock) t->topLevels = 0;
    if (topAuto) for (int stage : { ST_EXTEND, ST_CONNECT }) {
        PersistTune& t = stage == ST_CONNECT ? ctx->tuneConnect : ctx->tune;
        int q = 0, lv = t.topLevels, beside = 0, shadeLds = 0;
        const bool shared = ctx->cfg.persist_blocks_per_cu > 0;
        if (const int rc = persist_query(ctx, stage, 0, &q)) return rc;
        const int base = persist_blocks(ctx, stage, q);
        if (shared) { if (const int rc = beside_shade(ctx, stage, 0, &beside, &shadeLds)) return rc; }
        for (; lv > 0; lv--) {
            if (const int rc = persist_query(ctx, stage, lv, &q)) return rc;
            if (persist_blocks(ctx, stage, q) != base) continue;
            if (!shared) break;
            int fit = 0;
            if (const int rc = beside_shade(ctx, stage, lv, &fit, &shadeLds)) return rc;
            if (fit >= beside) break;
        }
        t.topLevels = lv;
    }
    return RT_OK;
}
static int size_persistent_grids(RtCtx* ctx)
{
    int perCU = 0;
    if (const int rc = persist_query(ctx, ST_EXTEND, -1, &perCU)) return rc;   // what extend runs on the persistent grid
    // (k_trace_persist4_tlas: its any-hit instantiations need more registers than its closest-hit ones and admit a workgroup fewer, so
    // connect's grid goes by connect's own kernel; so does k_trace_persist's with a top table for connect: its own LDS size)
    int perCUc = perCU;
    if (bvh4_tlas_trav(ctx->trav) || ctx->tuneConnect.topLevels > 0) { if (const int rc = persist_query(ctx, ST_CONNECT, -1, &perCUc)) return rc; }
    ctx->persistGrid = std::min(ctx->gridMax, persist_blocks(ctx, ST_EXTEND, perCU) * ctx->cuCount);
    ctx->persistGridConnect = std::min(ctx->gridMax, persist_blocks(ctx, ST_CONNECT, perCUc) * ctx->cuCount);
    return RT_OK;
}
// The global columns of the SPILL kinds, grown to what the grids need, and what the kernels are told of the columns
static int bind_spill_columns(RtCtx* ctx)
{
    ctx->q.spill = nullptr; ctx->q.spillStride = 0; ctx->q.stackCap = 0;
    ctx->q.tlasLdsEntries = tlas_trav(ctx->trav) ? (uint32_t)tlas_lds_entries(ctx) : 0u;
    if (!spill_trav(ctx->trav)) return RT_OK;
    // every SPILL launch runs on a persistent grid (bounce 0 too), so the global columns are bounded by the grids
    const size_t stride = (size_t)std::max(ctx->persistGrid, ctx->persistGridConnect) * kBlock;
    const size_t words = stride * (size_t)(tlas_stack_entries(ctx->facts.stackEntries, ctx->facts.tlasDepth) - ctx->spillCap);
    if (words > ctx->spillWords) {
        if (ctx->dSpill) (void)hipFree(ctx->dSpill);
        ctx->dSpill = nullptr; ctx->spillWords = 0;
        if (hipMalloc((void**)&ctx->dSpill, words * sizeof(uint32_t)) != hipSuccess) return fail(RT_E_NOMEM, "hipMalloc of the spill stacks (%zu bytes) failed", words * sizeof(uint32_t));
        ctx->spillWords = words;
    }
    ctx->q.spill = ctx->dSpill; ctx->q.spillStride = (uint32_t)stride; ctx->q.stackCap = (uint32_t)ctx->spillCap;
    return RT_OK;
}
// What a context derives from its configuration once it has a scene: which traversal kernels run, with which launch parameters
// (plan_traversal, trav_common.h: the rules, and every RT355_* knob of the traversal), and how their persistent grids are sized.
static int configure_traversal(RtCtx* ctx)
{
    static std::atomic<int> serial{ 0 };   // contexts start their sparse queues on different XCDs
    if (ctx->xcdFirst < 0) ctx->xcdFirst = serial.fetch_add(1) & 7;
    const TravPlan plan = plan_traversal(traversal_facts(ctx), read_trav_knobs());
    adopt_plan(ctx, plan);
    if (persistent(ctx->trav)) {
        if (const int rc = fit_top_tables(ctx, plan.topAuto)) return rc;
        if (const int rc = size_persistent_grids(ctx)) return rc;
    } else ctx->persistGrid = ctx->persistGridConnect = 0;   // (a resize took the persistent kernels away: rt_kernel_info reports what a fresh context does)
    return bind_spill_columns(ctx);
}

// A context takes over the facts of the copy it holds - the arrays, the layout, the stack sizes - and derives its traversal
// configuration from them: after an upload, on sharing, and before the first launch after an update or a rebuild (sync_scene_config).
// Nothing else assigns them.
static void frame_state_reset(RtCtx* ctx);
static int adopt_scene(RtCtx* ctx)
{
    const SceneBag& b = *ctx->scene;
    const SceneArrays& a = b.sc;
    // A resize changed the primitive count under a holder: its hit queue may name primitives the new array lacks, and k_shade and
    // k_export_rays index the primitives by it.  So the queues are emptied on the holder's stream before its next launch, to what a
    // new context has: every ray and shadow count, dequeue head and ticket zero and every hit record zero (primitive 0, which every
    // scene has).  rt_stage_begin_frame's own state would not do: it sets the count of bounce 0 to the band's pixels, which hands the
    // old hit records to rt_debug_get_rays.  (A frame of rt_render never spans the resize: the commit waited for this stream.)
    if (ctx->sceneLoaded && ctx->sc.nPrims != a.nPrims) {
        const DevQueues& q = ctx->q;
        HIPCHK(hipMemsetAsync(q.nRays, 0, sizeof(int32_t) * (RT_MAX_BOUNCES + 2), ctx->stream));
        HIPCHK(hipMemsetAsync(q.nShadow, 0, sizeof(int32_t) * (RT_MAX_BOUNCES + 2), ctx->stream));
        HIPCHK(hipMemsetAsync(q.cursor, 0, sizeof(int32_t) * kCursorWords, ctx->stream));
        HIPCHK(hipMemsetAsync(q.shadeTicket, 0, sizeof(int32_t) * (size_t)(RT_MAX_BOUNCES + 1) * kTicketClasses * kTicketStride, ctx->stream));
        HIPCHK(hipMemsetAsync(q.hit, 0, sizeof(float4) * (size_t)ctx->nPix, ctx->stream));
        ctx->queued = true;
        frame_state_reset(ctx);
    }
    auto f4 = [](const RtFloat4* p) { return (const float4*)p; };
    ctx->sc = DevScene{ a.prims, a.mats, f4(a.tex), a.lights, a.bvh2, a.bvh4, a.primIdx, a.tlas, a.blas, f4(a.pairs), f4(a.triRecs), a.rootEntry, f4(a.shadeRecs),
                        f4(a.tlasPairs), f4(a.instRecs), a.tlasRoot, f4(a.tlasPairsP), a.tlasRootP, f4(a.lightRecs), f4(a.quads), a.nLights, a.nPrims, a.nBlas, a.nTex, a.nMats };
    ctx->facts = b.facts;
    const int rc = configure_traversal(ctx);
    if (rc == RT_OK) ctx->sceneGen = b.generation;
    return rc;
}
// A holder of a scene copy that an update or a rebuild has changed takes it over again before its next launch
static int sync_scene_config(RtCtx* ctx)
{
    if (!ctx->scene || ctx->sceneGen == ctx->scene->generation) return RT_OK;
    return adopt_scene(ctx);
}
// The plan's rules from outside (tests): the facts a context plans from, and the plan of any facts under the knobs of the environment
static_assert(sizeof(PersistTune) == sizeof(int32_t) * RT_TUNE_FIELDS, "RtTraversalPlan mirrors PersistTune field by field");
extern "C" int rt_debug_traversal_facts(RtCtx* ctx, RtTraversalFacts* out)
{
    if (!ctx || !out) return fail(RT_E_INVALID, "rt_debug_traversal_facts: null argument");
    if (!ctx->sceneLoaded) return fail(RT_E_INVALID, "rt_debug_traversal_facts: no scene uploaded");
    if (const int rc = sync_scene_config(ctx)) return rc;
    const TravFacts f = traversal_facts(ctx);
    *out = RtTraversalFacts{ f.accel, f.extend_variant, f.persist_blocks_per_cu, f.layout, f.singleBlas, f.tlasDepth, f.nInterior, f.nQuads, f.stackEntries,
                             f.sharedMemPerBlock, f.xcdFirst };
    return RT_OK;
}
extern "C" int rt_debug_traversal_plan(const RtTraversalFacts* facts, RtTraversalPlan* out)
{
    if (!facts || !out) return fail(RT_E_INVALID, "rt_debug_traversal_plan: null argument");
    TravFacts f;
    f.accel = facts->accel; f.extend_variant = facts->extend_variant; f.persist_blocks_per_cu = facts->persist_blocks_per_cu;
    f.layout = facts->layout; f.singleBlas = facts->singleBlas; f.tlasDepth = facts->tlasDepth; f.nInterior = facts->nInterior;
    f.nQuads = facts->nQuads; f.stackEntries = facts->stackEntries; f.sharedMemPerBlock = facts->sharedMemPerBlock; f.xcdFirst = facts->xcdFirst;
    const TravPlan p = plan_traversal(f, read_trav_knobs());
    *out = RtTraversalPlan{ p.trav, p.spillCap, p.coherent, p.topAuto ? 1 : 0, p.tuneBlocks, p.connectBlocks, {}, {}, {} };
    memcpy(out->tune, &p.tune, sizeof p.tune); memcpy(out->tuneConnect, &p.tuneConnect, sizeof p.tuneConnect); memcpy(out->tune4, &p.tune4, sizeof p.tune4);
    return RT_OK;
}
// The last step of every way to a scene: the context holds `bag` and is usable again once it has taken the copy over
static int bind_scene(RtCtx* ctx, const std::shared_ptr<SceneBag>& bag)
{
    scene_hold(ctx, bag);
    ctx->sceneLoaded = false; ctx->trav = TRAV_NESTED;
    const int rc = adopt_scene(ctx);
    if (rc != RT_OK) { scene_release(ctx); return rc; }
    ctx->sceneLoaded = true;
    return RT_OK;
}

extern "C" int rt_upload_scene(RtCtx* ctx, const RtPrimitive* prims, int32_t nPrims, const RtMaterial* mats, int32_t nMats,
                               const RtFloat4* textures, int32_t nTexels, const uint32_t* lights, int32_t nLights,
                               const void* bvhNodes, int32_t nNodes, const uint32_t* primIdx, int32_t nIdx,
                               const RtTLASNode* tlas, int32_t nTlas, const RtBVHInstance* blas, int32_t nBlas)
{
    if (!ctx) return fail(RT_E_INVALID, "rt_upload_scene: null context");
    const HostScene in{ prims, nPrims, mats, nMats, textures, nTexels, lights, nLights, bvhNodes, nNodes, primIdx, nIdx, tlas, nTlas, blas, nBlas };
    SceneFacts facts; int64_t texPad = 2;   // (validate_scene begins the facts: the stack entries, the TLAS height)
    // nothing of the context changes until the arrays have passed (a failed upload leaves the bound scene usable)
    if (const int rc = validate_scene(ctx->cfg.accel, in, &facts, &texPad)) return rc;
    HIPCHK(hipSetDevice(ctx->cfg.device));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    scene_release(ctx);   // the bound copy goes before the new one is made (one shared with other contexts lives on with them)
    ctx->sceneLoaded = false; ctx->trav = TRAV_NESTED;   // nothing usable until this upload has succeeded
    auto bag = std::make_shared<SceneBag>();
    bag->device = ctx->cfg.device;
    if (const int rc = upload_scene(*bag, ctx->cfg.accel, ctx->cfg.extend_variant, in, facts, texPad)) return rc;
    return bind_scene(ctx, bag);
}

// rt_upload_scene with the BVH2 given for any context.  A BVH4 context collapses it on the device (scene.hip, collapse.hip) and keeps it,
// so the copy can be rebuilt in place.  The new copy is made beside the bound one, which stays in use when the call is refused.
extern "C" int rt_upload_scene_bvh2(RtCtx* ctx, const RtPrimitive* prims, int32_t nPrims, const RtMaterial* mats, int32_t nMats,
                                    const RtFloat4* textures, int32_t nTexels, const uint32_t* lights, int32_t nLights,
                                    const RtBVHNode2* bvhNodes, int32_t nNodes, const uint32_t* primIdx, int32_t nIdx,
                                    const RtTLASNode* tlas, int32_t nTlas, const RtBVHInstance* blas, int32_t nBlas)
{
    if (!ctx) return fail(RT_E_INVALID, "rt_upload_scene_bvh2: null context");
    if (ctx->cfg.accel == RT_ACCEL_BVH2)
        return rt_upload_scene(ctx, prims, nPrims, mats, nMats, textures, nTexels, lights, nLights, bvhNodes, nNodes, primIdx, nIdx, tlas, nTlas, blas, nBlas);
    const HostScene in{ prims, nPrims, mats, nMats, textures, nTexels, lights, nLights, bvhNodes, nNodes, primIdx, nIdx, tlas, nTlas, blas, nBlas };
    SceneFacts facts; int64_t texPad = 2;   // (validate_scene begins the facts: the stack entries, the TLAS height)
    if (const int rc = validate_scene(RT_ACCEL_BVH2, in, &facts, &texPad)) return rc;   // the BVH2 rules ...
    std::vector<uint32_t> roots((size_t)nBlas);
    for (int32_t b = 0; b < nBlas; b++) roots[(size_t)b] = blas[b].bvhIdx;
    std::vector<collapse::Blas> blas4;
    std::string why;
    if (const int rc = collapse::check_args(bvhNodes, nNodes, nIdx, roots.data(), nBlas, blas4, why))   // ... and every record the collapse reads
        return fail(rc, "rt_upload_scene_bvh2: %s", why.c_str());
    HIPCHK(hipSetDevice(ctx->cfg.device));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    auto bag = std::make_shared<SceneBag>();
    bag->device = ctx->cfg.device;
    if (const int rc = upload_scene(*bag, ctx->cfg.accel, ctx->cfg.extend_variant, in, facts, texPad, &blas4)) return rc;
    return bind_scene(ctx, bag);
}

// A second context on the same device renders the scene `from` holds: it takes the device copy (uploaded arrays and derived layouts)
// instead of uploading its own.  Both contexts must agree on what the derived layout depends on (accel, extend_variant).
extern "C" int rt_share_scene(RtCtx* ctx, RtCtx* from)
{
    if (!ctx || !from) return fail(RT_E_INVALID, "rt_share_scene: null context");
    if (ctx == from) return RT_OK;
    if (!from->sceneLoaded) return fail(RT_E_INVALID, "rt_share_scene: the source context has no scene");
    if (const int rc = sync_scene_config(from)) return rc;   // (a rebuild may have swapped the arrays since `from` last launched)
    if (ctx->cfg.device != from->cfg.device) return fail(RT_E_INVALID, "rt_share_scene: contexts on different devices (%d, %d)", ctx->cfg.device, from->cfg.device);
    if (ctx->cfg.accel != from->cfg.accel || ctx->cfg.extend_variant != from->cfg.extend_variant)
        return fail(RT_E_INVALID, "rt_share_scene: the contexts differ in accel / extend_variant, which the derived layout depends on");
    HIPCHK(hipSetDevice(ctx->cfg.device));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    return bind_scene(ctx, from->scene);
}

// ---- in-place updates and rebuilds of the copy a context holds (scene_rebuild.hip, scene_materials.hip) ---------------------------
// What the entry points that change or inspect a bound copy ask first: a context (entry points that name their other required
// arguments in that message have asked already), a copy, and - lostBvh2 != NULL - its BVH2, which a BVH4 copy bound through
// rt_upload_scene has not kept; lostBvh2 ends that message.
static int bound_scene(const RtCtx* ctx, const char* who, const char* lostBvh2 = nullptr)
{
    if (!ctx) return fail(RT_E_INVALID, "%s: null context", who);
    if (!ctx->sceneLoaded || !ctx->scene) return fail(RT_E_INVALID, "%s: no scene uploaded", who);
    if (lostBvh2 && ctx->cfg.accel != RT_ACCEL_BVH2 && !ctx->scene->keepsBvh2)
        return fail(RT_E_UNSUPPORTED, "%s: a BVH4 copy bound through rt_upload_scene has lost its BVH2%s", who, lostBvh2);
    return RT_OK;
}
static const char* const kCannotRebuild = " and cannot rebuild in place (bind the BVH2 with rt_upload_scene_bvh2, or build on the host and upload)";
extern "C" int rt_update_scene(RtCtx* ctx, const RtPrimitive* prims, int32_t first, int32_t count, const RtBVHInstance* blas, int32_t nBlas,
                               RtUpdateStats* stats)
{
    if (const int rc = bound_scene(ctx, "rt_update_scene")) return rc;
    if (ctx->cfg.accel != RT_ACCEL_BVH2)
        return fail(RT_E_UNSUPPORTED, "rt_update_scene: BVH4 contexts cannot refit (rt_rebuild_scene a copy bound with rt_upload_scene_bvh2, or rebuild and upload)");
    return update_scene(*ctx->scene, "rt_update_scene", Geometry::host_records(prims, first, count), blas, nBlas, stats);
}
extern "C" int rt_rebuild_scene(RtCtx* ctx, const RtPrimitive* prims, int32_t first, int32_t count, const RtBVHInstance* blas, int32_t nBlas,
                                int32_t builder, const RtBuildOptions* opts, RtRebuildStats* stats)
{
    if (const int rc = bound_scene(ctx, "rt_rebuild_scene", kCannotRebuild)) return rc;
    return rebuild_scene(*ctx->scene, "rt_rebuild_scene", Geometry::host_records(prims, first, count), blas, nBlas, builder, opts, stats);
}
extern "C" int rt_rebuild_ranges(RtCtx* ctx, const RtPrimitive* prims, int32_t first, int32_t count, const RtBVHInstance* blas, int32_t nBlas,
                                 const int32_t* plan, int32_t nRanges, const RtBuildOptions* opts, RtRebuildStats* stats)
{
    if (const int rc = bound_scene(ctx, "rt_rebuild_ranges", kCannotRebuild)) return rc;
    return rebuild_ranges(*ctx->scene, "rt_rebuild_ranges", Geometry::host_records(prims, first, count), blas, nBlas, plan, nRanges, opts, stats);
}
extern "C" int rt_scene_blas_blocks(RtCtx* ctx, int32_t* n, int32_t* primFirst, int32_t* primCount, int32_t* nodes, int32_t* idxSlots, int32_t* compact, int32_t cap)
{
    if (const int rc = bound_scene(ctx, "rt_scene_blas_blocks", "")) return rc;
    return blas_blocks(*ctx->scene, n, primFirst, primCount, nodes, idxSlots, compact, cap);
}
static int device_pointer(const RtCtx* ctx, const char* who, const char* name, const void* p, int64_t bytes, int align, bool hostAllowed, bool* onDevice = nullptr);   // (below, with rt_trace)
extern "C" int rt_resize_scene(RtCtx* ctx, const void* prims, int32_t nPrims, const RtSceneShape* shape, int32_t builder, const RtBuildOptions* opts,
                               RtRebuildStats* stats)
{
    if (!ctx || !prims || !shape) return fail(RT_E_INVALID, "rt_resize_scene: null argument (context, prims and shape are required)");
    if (const int rc = bound_scene(ctx, "rt_resize_scene")) return rc;
    if (nPrims <= 0) return fail(RT_E_INVALID, "rt_resize_scene: nPrims must be positive (%d given)", nPrims);
    HIPCHK(hipSetDevice(ctx->cfg.device));
    // rt_trace's pointer rule, with host memory allowed: the records are copied, not followed by a kernel
    if (const int rc = device_pointer(ctx, "rt_resize_scene", "prims", prims, (int64_t)sizeof(RtPrimitive) * nPrims, 4, true)) return rc;
    if (const int rc = bound_scene(ctx, "rt_resize_scene", " and cannot be rebuilt in place (bind the BVH2 with rt_upload_scene_bvh2, or build on the host and upload)")) return rc;
    return resize_scene(*ctx->scene, prims, nPrims, shape, builder, opts, stats);
}
extern "C" int rt_update_materials(RtCtx* ctx, const RtMaterialUpdate* update, RtMaterialStats* stats)
{
    if (!ctx || !update) return fail(RT_E_INVALID, "rt_update_materials: null argument (context and update are required)");
    if (const int rc = bound_scene(ctx, "rt_update_materials")) return rc;
    HIPCHK(hipSetDevice(ctx->cfg.device));
    // rt_resize_scene's pointer rule: both arrays are copied, not followed by a kernel, so host memory passes as well
    if (update->texels && update->texCount > 0)
        if (const int rc = device_pointer(ctx, "rt_update_materials", "texels", update->texels, (int64_t)sizeof(RtFloat4) * update->texCount, 4, true)) return rc;
    if (update->primMat && update->primCount > 0)
        if (const int rc = device_pointer(ctx, "rt_update_materials", "primMat", update->primMat, (int64_t)sizeof(int32_t) * update->primCount, 4, true)) return rc;
    SceneBag& b = *ctx->scene;
    const bool stagedBefore = ctx->var.shadeTables != 0 && shade_tables_fit(b.sc.nLights, b.sc.nMats);
    if (const int rc = update_materials(b, *update, stats)) return rc;
    if (stats) stats->tables_staged_changed = (ctx->var.shadeTables != 0 && shade_tables_fit(b.sc.nLights, b.sc.nMats)) != stagedBefore ? 1 : 0;   // k_shade's own rule
    return RT_OK;
}
// ---- rt_update_geometry / rt_rebuild_geometry / rt_rebuild_geometry_ranges: the same three calls fed from an RtGeometry ------------
// The checks of an RtGeometry that need no device, then rt_resize_scene's pointer rule for every source it names (host memory passes:
// it is copied; 4-byte alignment and the end of a known allocation are rt_trace's rule); out: the geometry with where its sources lie
static int locate_geometry(const RtCtx* ctx, const char* who, const RtGeometry* g, Geometry& out)
{
    const SceneBag& b = *ctx->scene;
    std::string msg;
    if (b.refitRefusal) return fail(RT_E_UNSUPPORTED, "%s: %s", who, b.refitRefusal);   // (such a copy has no shadow of the types)
    if (const int rc = geometry::check_args(g, b.sc.nPrims, b.primType.data(), msg)) return fail(rc, "%s: %s", who, msg.c_str());
    out.g = *g;
    if (g->count == 0) return RT_OK;
    HIPCHK(hipSetDevice(ctx->cfg.device));
    if (g->prims) return device_pointer(ctx, who, "prims", g->prims, (int64_t)sizeof(RtPrimitive) * g->count, 4, true, &out.primsOnDevice);
    if (g->indices)
        if (const int rc = device_pointer(ctx, who, "indices", g->indices, (int64_t)sizeof(uint32_t) * 3 * g->count, 4, true, &out.indicesOnDevice)) return rc;
    const int64_t bytes = g->nVertices > 0 ? (g->nVertices - 1) * g->positionStride + 12 : 0;   // to the last vertex's z
    return device_pointer(ctx, who, "positions", g->positions, bytes, 4, true, &out.positionsOnDevice);
}
extern "C" int rt_geometry_check(const RtGeometry* geometry, int32_t nPrims, const int32_t* objType)
{
    std::string msg;
    if (nPrims < 0) return fail(RT_E_INVALID, "rt_geometry_check: nPrims %d is negative", nPrims);
    if (const int rc = geometry::check_args(geometry, nPrims, objType, msg)) return fail(rc, "rt_geometry_check: %s", msg.c_str());
    return RT_OK;
}
extern "C" int rt_update_geometry(RtCtx* ctx, const RtGeometry* geometry, const RtBVHInstance* blas, int32_t nBlas, RtUpdateStats* stats)
{
    const char* who = "rt_update_geometry";
    if (const int rc = bound_scene(ctx, who)) return rc;
    if (ctx->cfg.accel != RT_ACCEL_BVH2)
        return fail(RT_E_UNSUPPORTED, "%s: BVH4 contexts cannot refit (rt_rebuild_geometry a copy bound with rt_upload_scene_bvh2, or rebuild and upload)", who);
    Geometry geo;
    if (const int rc = locate_geometry(ctx, who, geometry, geo)) return rc;
    return update_scene(*ctx->scene, who, geo, blas, nBlas, stats);
}
extern "C" int rt_rebuild_geometry(RtCtx* ctx, const RtGeometry* geometry, const RtBVHInstance* blas, int32_t nBlas, int32_t builder, const RtBuildOptions* opts,
                                   RtRebuildStats* stats)
{
    const char* who = "rt_rebuild_geometry";
    if (const int rc = bound_scene(ctx, who, kCannotRebuild)) return rc;
    Geometry geo;
    if (const int rc = locate_geometry(ctx, who, geometry, geo)) return rc;
    return rebuild_scene(*ctx->scene, who, geo, blas, nBlas, builder, opts, stats);
}
extern "C" int rt_rebuild_geometry_ranges(RtCtx* ctx, const RtGeometry* geometry, const RtBVHInstance* blas, int32_t nBlas, const int32_t* plan, int32_t nRanges,
                                          const RtBuildOptions* opts, RtRebuildStats* stats)
{
    const char* who = "rt_rebuild_geometry_ranges";
    if (const int rc = bound_scene(ctx, who, kCannotRebuild)) return rc;
    Geometry geo;
    if (const int rc = locate_geometry(ctx, who, geometry, geo)) return rc;
    return rebuild_ranges(*ctx->scene, who, geo, blas, nBlas, plan, nRanges, opts, stats);
}
extern "C" int rt_refit_info(RtCtx* ctx, RtRefitInfo* out)
{
    if (!ctx || !out) return fail(RT_E_INVALID, "rt_refit_info: null argument");
    if (const int rc = bound_scene(ctx, "rt_refit_info")) return rc;
    *out = ctx->scene->refitInfo;
    return RT_OK;
}
extern "C" int rt_ranges_info(RtCtx* ctx, RtRangesInfo* out)
{
    if (!ctx || !out) return fail(RT_E_INVALID, "rt_ranges_info: null argument");
    if (const int rc = bound_scene(ctx, "rt_ranges_info")) return rc;
    *out = ctx->scene->rangesInfo;
    return RT_OK;
}
extern "C" int rt_debug_rebuild_allocations(RtCtx* ctx, int64_t* count)
{
    if (!ctx || !count) return fail(RT_E_INVALID, "rt_debug_rebuild_allocations: null argument");
    if (const int rc = bound_scene(ctx, "rt_debug_rebuild_allocations")) return rc;
    *count = rebuild_allocations(*ctx->scene);
    return RT_OK;
}
extern "C" int rt_debug_get_scene_array(RtCtx* ctx, int32_t which, void* out, int64_t capacityBytes, int64_t* bytes)
{
    if (!ctx || !bytes) return fail(RT_E_INVALID, "rt_debug_get_scene_array: null argument");
    if (const int rc = bound_scene(ctx, "rt_debug_get_scene_array")) return rc;
    const void* src = nullptr; size_t n = 0;
    if (const int rc = scene_array(*ctx->scene, which, &src, &n)) return rc;
    *bytes = (int64_t)n;
    if (!out || n == 0) return RT_OK;
    if (capacityBytes < (int64_t)n) return fail(RT_E_INVALID, "rt_debug_get_scene_array: %zu bytes needed, capacity %lld", n, (long long)capacityBytes);
    HIPCHK(hipSetDevice(ctx->cfg.device));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    HIPCHK(hipMemcpy(out, src, n, hipMemcpyDeviceToHost));
    return RT_OK;
}

// ---- seeds / accumulator ---------------------------------------------------------------
extern "C" int rt_set_seeds(RtCtx* ctx, const uint32_t* seeds, int64_t n)
{
    if (!ctx || !seeds) return fail(RT_E_INVALID, "rt_set_seeds: null argument");
    if (n != ctx->nPix) return fail(RT_E_INVALID, "rt_set_seeds: expected %d seeds (band pixels), got %lld", ctx->nPix, (long long)n);
    // The RNG step is a bijection of the 32-bit states that fixes only 0: a nonzero state never becomes 0, and from 0
    // every draw is 0.0f, with which sample_ball's rejection loop never ends.  So 0 is refused here, before anything is copied.
    for (int64_t i = 0; i < n; i++)
        if (seeds[i] == 0) return fail(RT_E_INVALID, "rt_set_seeds: seeds[%lld] is 0, the fixed point of the RNG: every seed must be nonzero", (long long)i);
    HIPCHK(hipSetDevice(ctx->cfg.device));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    HIPCHK(hipMemcpy(ctx->q.seeds, seeds, sizeof(uint32_t) * (size_t)n, hipMemcpyHostToDevice));
    return RT_OK;
}
extern "C" int rt_seed_default(RtCtx* ctx)
{
    if (!ctx) return fail(RT_E_INVALID, "rt_seed_default: null context");
    std::vector<uint32_t> s((size_t)ctx->nPix);
    uint32_t x = 0x12345678u; // template/template.cpp:711
    auto next = [&x]() { x ^= x << 13; x ^= x >> 17; x ^= x << 5; return x; };
    for (int64_t i = 0; i < ctx->firstPixel; i++) next();
    for (auto& v : s) v = next();
    return rt_set_seeds(ctx, s.data(), (int64_t)s.size());
}
extern "C" int rt_get_seeds(RtCtx* ctx, uint32_t* out, int64_t n)
{
    if (!ctx || !out || n != ctx->nPix) return fail(RT_E_INVALID, "rt_get_seeds: bad argument");
    HIPCHK(hipSetDevice(ctx->cfg.device));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    HIPCHK(hipMemcpy(out, ctx->q.seeds, sizeof(uint32_t) * (size_t)n, hipMemcpyDeviceToHost));
    return RT_OK;
}
extern "C" int rt_bind_accum(RtCtx* ctx, void* devicePtr)
{
    if (!ctx) return fail(RT_E_INVALID, "rt_bind_accum: null context");
    HIPCHK(hipSetDevice(ctx->cfg.device));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    if (devicePtr) { ctx->q.accum = (float4*)devicePtr; ctx->ownAccum = false; }
    else if (!ctx->ownAccum) {
        float4* a = nullptr;
        int rc = dalloc(ctx->queueAllocs, &a, (size_t)ctx->cfg.width * ctx->cfg.height);
        if (rc != RT_OK) return rc;
        HIPCHK(hipMemset(a, 0, sizeof(float4) * (size_t)ctx->cfg.width * ctx->cfg.height));
        ctx->q.accum = a; ctx->ownAccum = true;
    }
    return RT_OK;
}
extern "C" void* rt_accum_device_ptr(RtCtx* ctx) { return ctx ? (void*)ctx->q.accum : nullptr; }
extern "C" void* rt_stream(RtCtx* ctx) { if (ctx) ctx->queued = true; return ctx ? (void*)ctx->stream : nullptr; }   // (the caller may queue work there)

extern "C" int rt_reset(RtCtx* ctx)
{
    if (!ctx) return fail(RT_E_INVALID, "rt_reset: null context");
    HIPCHK(hipSetDevice(ctx->cfg.device));
    ctx->queued = true;
    hipLaunchKernelGGL(k_reset, dim3((ctx->nPix + kBlock - 1) / kBlock), dim3(kBlock), 0, ctx->stream, ctx->q.accum, ctx->firstPixel, ctx->nPix);
    HIPCHK(hipGetLastError());
    return RT_OK;
}

// ---- stages --------------------------------------------------------------------------------
static int need_scene(RtCtx* ctx, const char* who)
{
    if (!ctx) return fail(RT_E_INVALID, "%s: null context", who);
    if (!ctx->sceneLoaded) return fail(RT_E_INVALID, "%s: no scene uploaded", who);
    return sync_scene_config(ctx);
}

static void frame_state_reset(RtCtx* ctx)
{
    memset(ctx->cursorUsed, 0, sizeof ctx->cursorUsed);
    memset(ctx->shadeRun, 0, sizeof ctx->shadeRun);
    ctx->generated = false;
}
extern "C" int rt_stage_begin_frame(RtCtx* ctx)
{
    if (!ctx) return fail(RT_E_INVALID, "rt_stage_begin_frame: null context");
    ctx->queued = true;
    hipLaunchKernelGGL(k_begin_frame, dim3(1), dim3(256), 0, ctx->stream, ctx->q);
    HIPCHK(hipGetLastError());
    frame_state_reset(ctx);
    return RT_OK;
}
static int generate(RtCtx* ctx, const RtCamera* cam, const RtSettings* s, int beginFrame)
{
    if (beginFrame) frame_state_reset(ctx);
    ctx->queued = true;
    LAUNCH(ctx, ST_GENERATE, ctx->kGenerate, grid_for(ctx->nPix), 0, ctx->q, *cam, s ? s->antiAliasing : 1, beginFrame);
    HIPCHK(hipGetLastError());
    ctx->primaryRays += (uint64_t)ctx->nPix;
    ctx->generated = true;
    return RT_OK;
}
extern "C" int rt_stage_generate(RtCtx* ctx, const RtCamera* cam, const RtSettings* s)
{
    if (!ctx || !cam) return fail(RT_E_INVALID, "rt_stage_generate: null argument");
    return generate(ctx, cam, s, 0);
}
extern "C" int rt_stage_extend(RtCtx* ctx, int32_t bounce, int32_t renderBVH)
{
    int rc = need_scene(ctx, "rt_stage_extend"); if (rc) return rc;
    ctx->queued = true;
    if (bounce < 0 || bounce > ctx->cfg.max_bounces) return fail(RT_E_INVALID, "rt_stage_extend: bounce %d outside [0, %d]", bounce, ctx->cfg.max_bounces);
    if (persistent(ctx->trav)) { // a queue head is good for one launch per frame; re-arm it if this stage is run again
        if (ctx->cursorUsed[bounce]) HIPCHK(hipMemsetAsync(ctx->q.cursor + bounce, 0, sizeof(int32_t), ctx->stream));
        ctx->cursorUsed[bounce] = true;
    }
    const bool wantSteps = renderBVH != 0 || ctx->q.steps != nullptr;   // only then does the event loop keep the per-ray `steps`
    const TraceLaunch L = trace_launch(ctx, ST_EXTEND, bounce, wantSteps, ctx->nPix);
    if (L.persist) LAUNCH(ctx, ST_EXTEND, L.persist, L.grid, L.lds, ctx->sc, ctx->q, bounce, bounce, renderBVH, L.tune);
    else LAUNCH(ctx, ST_EXTEND, L.nested, L.grid, L.lds, ctx->sc, ctx->q, bounce, renderBVH);
    HIPCHK(hipGetLastError());
    return RT_OK;
}
// The first launch of a fused frame of rt_render: generate, the frame's counter reset and extend(0) in one (k_trace_primary).  The
// host's frame state is what generate(.., 1) and rt_stage_extend(0) leave: to every later stage the frame looks the same.
static int extend_primary(RtCtx* ctx, const RtCamera* cam, const RtSettings* s, int renderBVH)
{
    frame_state_reset(ctx);
    ctx->queued = true;
    const TraceLaunch L = trace_launch(ctx, ST_EXTEND, 0, false, ctx->nPix, -1, true);
    if (!L.primary) return fail(RT_E_INVALID, "rt_render: no fused primary launch for this context's traversal");
    LAUNCH(ctx, ST_EXTEND, L.primary, L.grid, L.lds, ctx->sc, ctx->q, *cam, s ? s->antiAliasing : 1, renderBVH, L.tune);
    HIPCHK(hipGetLastError());
    ctx->primaryRays += (uint64_t)ctx->nPix;
    ctx->generated = true;
    ctx->cursorUsed[0] = true;
    return RT_OK;
}
static int stage_shade(RtCtx* ctx, int32_t bounce, const RtCamera* primaryCam, int aa);
extern "C" int rt_stage_shade(RtCtx* ctx, int32_t bounce) { return stage_shade(ctx, bounce, nullptr, 0); }
// primaryCam: bounce 0 of a fused frame - the launch computes its queue entries from the camera (k_shade<.., PRIMARY>)
static int stage_shade(RtCtx* ctx, int32_t bounce, const RtCamera* primaryCam, int aa)
{
    int rc = need_scene(ctx, "rt_stage_shade"); if (rc) return rc;
    ctx->queued = true;
    // the shadow queue and the counter rows are sized by cfg.max_bounces, not by the compile-time maximum
    if (bounce < 0 || bounce >= ctx->cfg.max_bounces) return fail(RT_E_INVALID, "rt_stage_shade: bounce %d outside [0, %d)", bounce, ctx->cfg.max_bounces);
    // The scan state of bounce b is armed by generate (b = 0) or by shade(b-1); re-arm it by hand when this
    // stage is run out of sequence (stage-level API used by the tests) or twice for the same bounce.
    if (ctx->shadeRun[bounce] || (bounce > 0 && !ctx->shadeRun[bounce - 1]) || (bounce == 0 && !ctx->generated)) {
        const size_t nTiles = ((size_t)ctx->nPix + kBlock - 1) / kBlock;
        HIPCHK(hipMemsetAsync(ctx->q.tile[bounce & 1], 0, sizeof(unsigned long long) * (nTiles + 2), ctx->stream));
        HIPCHK(hipMemsetAsync(ctx->q.super[bounce & 1], 0, sizeof(unsigned long long) * (nTiles / 64 + 2), ctx->stream));
        HIPCHK(hipMemsetAsync(ctx->q.supAcc[bounce & 1], 0, sizeof(unsigned long long) * (nTiles / 64 + 2), ctx->stream));
        HIPCHK(hipMemsetAsync(ctx->q.shadeTicket + (size_t)bounce * kTicketClasses * kTicketStride, 0, sizeof(int32_t) * (size_t)kTicketClasses * kTicketStride, ctx->stream));
    }
    const int tileSz = ctx->shadeTile;
    const dim3 sg((unsigned)std::max(1, std::min(ctx->shadeGrid, (ctx->nPix + tileSz - 1) / tileSz)));
    if (primaryCam) LAUNCHB(ctx, ST_SHADE, ctx->kShadePrimary, sg, tileSz, 0, ctx->sc, ctx->q, ctx->var, ShadeArg<true>{ { *primaryCam, aa } });
    else LAUNCHB(ctx, ST_SHADE, ctx->kShade, sg, tileSz, 0, ctx->sc, ctx->q, ctx->var, ShadeArg<false>{ bounce });
    ctx->shadeRun[bounce] = true;
    HIPCHK(hipGetLastError());
    return RT_OK;
}
extern "C" int rt_stage_connect(RtCtx* ctx, int32_t b0, int32_t b1)
{
    int rc = need_scene(ctx, "rt_stage_connect"); if (rc) return rc;
    ctx->queued = true;
    if (b0 < 0 || b1 < b0 || b1 >= ctx->cfg.max_bounces) return fail(RT_E_INVALID, "rt_stage_connect: bounce range [%d,%d] outside [0, %d)", b0, b1, ctx->cfg.max_bounces);
    if (persistent(ctx->trav)) {
        const int ci = (RT_MAX_BOUNCES + 2) + b0;
        if (ctx->cursorUsed[ci]) HIPCHK(hipMemsetAsync(ctx->q.cursor + ci, 0, sizeof(int32_t), ctx->stream));
        ctx->cursorUsed[ci] = true;
    }
    const TraceLaunch L = trace_launch(ctx, ST_CONNECT, b0, false, ctx->nPix * (b1 - b0 + 1));
    if (L.persist) LAUNCH(ctx, ST_CONNECT, L.persist, L.grid, L.lds, ctx->sc, ctx->q, b0, b1, 0, L.tune);
    else LAUNCH(ctx, ST_CONNECT, L.nested, L.grid, L.lds, ctx->sc, ctx->q, b0, b1);
    ev_begin(ctx, ST_ACCUM);
    for (int b = b0; b <= b1; b++)
        hipLaunchKernelGGL(k_accumulate, dim3(std::min(grid_for(ctx->nPix).x, 2048u)), dim3(kBlock), 0, ctx->stream, ctx->q, b);
    ev_end(ctx, ST_ACCUM);
    HIPCHK(hipGetLastError());
    return RT_OK;
}

// ---- rt_trace: the caller's rays through the context's traversal kernels ------------------------------------------------------------
// The kernels take DevQueues by value, so a query hands them a view of its own: the caller's arrays where their layout is the queue's
// (in place: the batch costs the traversal launches and a one-thread arming launch per pass), else the view's arrays between
// k_trace_load and k_trace_store.  Nothing the frame owns is written: counts, cursors, the fault word and the counter rows are the
// view's; the spill columns are the context's - scratch that no launch expects to survive the one before it, and every SPILL launch
// runs on a persistent grid, which is what they are sized for.  The launches carry no profiling events: stage times stay the frame's.
// A pass takes at most trace_window() rays: the counter rows (gridMax, one per workgroup of the nested kernels' 256-ray grid) bound it,
// and 2^22 rays caps what the view's arrays can grow to (48 bytes per ray: 192 MB) while a 1080p queue still goes in one pass.
static constexpr int64_t kTraceWindowMax = (int64_t)1 << 22;
static int64_t trace_window(const RtCtx* ctx)
{
    int64_t w = std::min<int64_t>((int64_t)ctx->gridMax * kBlock, kTraceWindowMax);
    if (const char* t = getenv("RT355_TRACE_WINDOW")) { const long long k = atoll(t); if (k > 0) w = std::min<int64_t>(w, k); }
    return w;
}
extern "C" int64_t rt_trace_window(RtCtx* ctx)
{
    if (!ctx) return fail(RT_E_INVALID, "rt_trace_window: null context");
    return trace_window(ctx);
}
// A pointer the kernels will follow for `bytes` bytes: it must be memory the context's device can reach (a host pointer passed by
// mistake is an error message here, not a fault there), aligned for the accesses, and - where the runtime knows the allocation - inside it.
// hostAllowed (rt_resize_scene, which copies from it): memory the runtime does not know, or knows as host memory, passes as well.
// onDevice (may be NULL) receives whether a kernel can follow the pointer.
static int device_pointer(const RtCtx* ctx, const char* who, const char* name, const void* p, int64_t bytes, int align, bool hostAllowed, bool* onDevice)
{
    if ((uintptr_t)p % (uintptr_t)align) return fail(RT_E_INVALID, "%s: %s (%p) is not aligned to %d bytes", who, name, p, align);
    hipPointerAttribute_t a{};
    const hipError_t e = hipPointerGetAttributes(&a, p);
    if (e != hipSuccess) (void)hipGetLastError();
    const bool device = e == hipSuccess && a.type == hipMemoryTypeDevice && a.device == ctx->cfg.device;
    const bool shared = e == hipSuccess && (a.type == hipMemoryTypeManaged || (a.type == hipMemoryTypeHost && a.devicePointer == p));
    const bool host = e != hipSuccess || a.type == hipMemoryTypeUnregistered || a.type == hipMemoryTypeHost;
    if (!device && !shared && !(hostAllowed && host))
        return fail(RT_E_INVALID, "%s: %s (%p) is not memory accessible from device %d (a host pointer? memory of another GPU?)", who, name, p, ctx->cfg.device);
    if (device) {
        hipDeviceptr_t base = nullptr; size_t size = 0;
        if (hipMemGetAddressRange(&base, &size, (hipDeviceptr_t)p) != hipSuccess) (void)hipGetLastError();   // (not every allocator's memory has one)
        else if ((const char*)p + bytes > (const char*)base + size)
            return fail(RT_E_INVALID, "%s: %s needs %lld bytes from %p, its allocation ends %lld bytes earlier", who, name, (long long)bytes, p,
                        (long long)(((const char*)p + bytes) - ((const char*)base + size)));
    }
    if (onDevice) *onDevice = device || shared;
    return RT_OK;
}
static int trace_pointer(const RtCtx* ctx, const char* name, const void* p, int64_t bytes, int align) { return device_pointer(ctx, "rt_trace", name, p, bytes, align, false); }
static int trace_view(RtCtx* ctx, size_t ownRays)
{
    RtCtx::TraceView& v = ctx->tv;
    if (!v.ready) {
        DevQueues q{};
        unsigned long long* ctr = nullptr;
        int rc = dalloc(v.words, &q.nRays, RT_MAX_BOUNCES + 2);
        if (rc == RT_OK) rc = dalloc(v.words, &q.nShadow, RT_MAX_BOUNCES + 2);
        if (rc == RT_OK) rc = dalloc(v.words, &q.cursor, kCursorWords);
        if (rc == RT_OK) rc = dalloc(v.words, &q.fault, 1);
        if (rc == RT_OK) rc = dalloc(v.words, &ctr, (size_t)ctx->gridMax * kCtrCols);   // nobody sums a query's work: one table takes both stages' rows
        if (rc != RT_OK) { free_bag(v.words); return rc; }
        HIPCHK(hipMemsetAsync(q.nRays, 0, sizeof(int32_t) * (RT_MAX_BOUNCES + 2), ctx->stream));
        HIPCHK(hipMemsetAsync(q.nShadow, 0, sizeof(int32_t) * (RT_MAX_BOUNCES + 2), ctx->stream));
        HIPCHK(hipMemsetAsync(q.cursor, 0, sizeof(int32_t) * kCursorWords, ctx->stream));
        HIPCHK(hipMemsetAsync(q.fault, 0, sizeof(int32_t), ctx->stream));
        HIPCHK(hipMemsetAsync(ctr, 0, sizeof(unsigned long long) * (size_t)ctx->gridMax * kCtrCols, ctx->stream));
        q.ctrExtend = q.ctrConnect = ctr;
        q.nPix = ctx->nPix; q.firstPixel = ctx->firstPixel; q.width = ctx->cfg.width; q.height = ctx->cfg.height;
        v.q = q; v.ready = true;
    }
    if (ownRays > v.cap) {
        HIPCHK(hipStreamSynchronize(ctx->stream));   // an earlier query may still be reading the arrays this one replaces
        for (float4*& p : v.rays) { if (p) (void)hipFree(p); p = nullptr; }
        v.cap = 0;
        for (float4*& p : v.rays)
            if (hipMalloc((void**)&p, ownRays * sizeof(float4)) != hipSuccess) {
                (void)hipGetLastError();
                for (float4*& r : v.rays) { if (r) (void)hipFree(r); r = nullptr; }
                return fail(RT_E_NOMEM, "rt_trace: hipMalloc of the query's ray arrays (3 x %zu bytes) failed", ownRays * sizeof(float4));
            }
        v.cap = ownRays;
    }
    return RT_OK;
}
extern "C" int rt_trace(RtCtx* ctx, int32_t mode, const RtRayBatch* rays, const RtTraceOut* out)
{
    if (!ctx) return fail(RT_E_INVALID, "rt_trace: null ctx");
    if (!rays) return fail(RT_E_INVALID, "rt_trace: null rays");
    if (!out) return fail(RT_E_INVALID, "rt_trace: null out");
    int rc = need_scene(ctx, "rt_trace"); if (rc) return rc;
    if (mode != RT_TRACE_CLOSEST && mode != RT_TRACE_ANY) return fail(RT_E_INVALID, "rt_trace: mode %d is neither RT_TRACE_CLOSEST (0) nor RT_TRACE_ANY (1)", mode);
    const bool any = mode == RT_TRACE_ANY;
    const int64_t n = rays->n;
    if (n < 0) return fail(RT_E_INVALID, "rt_trace: rays->n = %lld is negative", (long long)n);
    if (rays->originStride < 12 || rays->originStride % 4) return fail(RT_E_INVALID, "rt_trace: rays->originStride = %lld must be >= 12 and a multiple of 4", (long long)rays->originStride);
    if (rays->dirStride < 12 || rays->dirStride % 4) return fail(RT_E_INVALID, "rt_trace: rays->dirStride = %lld must be >= 12 and a multiple of 4", (long long)rays->dirStride);
    if (any) {
        if (out->hit || out->point || out->normal) return fail(RT_E_INVALID, "rt_trace: out->%s is not produced by RT_TRACE_ANY", out->hit ? "hit" : (out->point ? "point" : "normal"));
    } else if (out->occluded) return fail(RT_E_INVALID, "rt_trace: out->occluded is not produced by RT_TRACE_CLOSEST");
    if (n == 0) return RT_OK;
    if (any ? !out->occluded : !out->hit) return fail(RT_E_INVALID, "rt_trace: out->%s is required by %s", any ? "occluded" : "hit", any ? "RT_TRACE_ANY" : "RT_TRACE_CLOSEST");
    if (!rays->origin) return fail(RT_E_INVALID, "rt_trace: null rays->origin");
    if (!rays->dir) return fail(RT_E_INVALID, "rt_trace: null rays->dir");
    HIPCHK(hipSetDevice(ctx->cfg.device));
    if ((rc = trace_pointer(ctx, "rays->origin", rays->origin, (n - 1) * rays->originStride + 12, 4))) return rc;
    if ((rc = trace_pointer(ctx, "rays->dir", rays->dir, (n - 1) * rays->dirStride + 12, 4))) return rc;
    if (rays->tmax) if ((rc = trace_pointer(ctx, "rays->tmax", rays->tmax, n * 4, 4))) return rc;
    if (out->hit) if ((rc = trace_pointer(ctx, "out->hit", out->hit, n * 16, 16))) return rc;
    if (out->point) if ((rc = trace_pointer(ctx, "out->point", out->point, n * 16, 16))) return rc;
    if (out->normal) if ((rc = trace_pointer(ctx, "out->normal", out->normal, n * 16, 16))) return rc;
    if (out->occluded) if ((rc = trace_pointer(ctx, "out->occluded", out->occluded, n, 1))) return rc;
    const bool vecO = rays->originStride == 16 && (uintptr_t)rays->origin % 16 == 0, vecD = rays->dirStride == 16 && (uintptr_t)rays->dir % 16 == 0;
    const bool inPlace = !any && vecO && vecD && !rays->tmax && !out->point && !out->normal;   // the queue's own layout, nothing but the hit record wanted
    const int64_t window = trace_window(ctx);
    if ((rc = trace_view(ctx, inPlace ? 0 : (size_t)std::min(n, window)))) return rc;
    ctx->queued = true;
    DevQueues q = ctx->tv.q;
    q.spill = ctx->q.spill; q.spillStride = ctx->q.spillStride; q.stackCap = ctx->q.stackCap; q.tlasLdsEntries = ctx->q.tlasLdsEntries;
    for (int64_t off = 0; off < n; off += window) {
        const int m = (int)std::min(window, n - off);
        TraceIO io{ (const char*)rays->origin + off * rays->originStride, (const char*)rays->dir + off * rays->dirStride, rays->originStride, rays->dirStride,
                    rays->tmax ? rays->tmax + off : nullptr, out->hit ? (float4*)out->hit + off : nullptr, out->point ? (float4*)out->point + off : nullptr,
                    out->normal ? (float4*)out->normal + off : nullptr, out->occluded ? out->occluded + off : nullptr };
        float4* const* own = ctx->tv.rays;
        q.O[kTraceBounce & 1] = q.sA = inPlace ? (float4*)io.origin : own[0];
        q.D[kTraceBounce & 1] = q.sB = inPlace ? (float4*)io.dir : own[1];
        q.hit = q.sC = inPlace ? io.hit : own[2];
        hipLaunchKernelGGL(k_trace_arm, dim3(1), dim3(1), 0, ctx->stream, q, m, (int)any);
        if (!inPlace) hipLaunchKernelGGL(k_trace_load, grid_for(m), dim3(kBlock), 0, ctx->stream, q, io, m, (int)any, (int)vecO, (int)vecD);
        const TraceLaunch L = trace_launch(ctx, any ? ST_CONNECT : ST_EXTEND, kTraceBounce, false, m);
        if (L.persist) hipLaunchKernelGGL(L.persist, L.grid, dim3(kBlock), L.lds, ctx->stream, ctx->sc, q, kTraceBounce, kTraceBounce, 0, L.tune);
        else if (any) hipLaunchKernelGGL(L.nested, L.grid, dim3(kBlock), L.lds, ctx->stream, ctx->sc, q, kTraceBounce, kTraceBounce);
        else hipLaunchKernelGGL(L.nested, L.grid, dim3(kBlock), L.lds, ctx->stream, ctx->sc, q, kTraceBounce, 0);
        if (!inPlace) hipLaunchKernelGGL(k_trace_store, grid_for(m), dim3(kBlock), 0, ctx->stream, ctx->sc, q, io, m, (int)any);
        HIPCHK(hipGetLastError());
    }
    return RT_OK;
}

// Renderer::RayTrace() (renderer.cpp:64-94), `frames` times.
extern "C" int rt_render(RtCtx* ctx, const RtCamera* cam, const RtSettings* settings, int32_t frames)
{
    int rc = need_scene(ctx, "rt_render"); if (rc) return rc;
    if (!cam) return fail(RT_E_INVALID, "rt_render: null camera");
    if (frames <= 0) return fail(RT_E_INVALID, "rt_render: frames must be > 0");
    HIPCHK(hipSetDevice(ctx->cfg.device));
    const bool nee = ctx->cfg.shading == RT_SHADING_NEE, rr = ctx->cfg.russian_roulette != 0;
    const int renderBVH = settings ? settings->renderBVH : 0;
    const bool fused = ctx->fusePrimary;   // decided with the traversal (plan_traversal): bounce 0's two launches compute the primary rays, no k_generate
    const int aa = settings ? settings->antiAliasing : 1;
    for (int f = 0; f < frames; f++) {
        // the frame's counter reset rides in the first workgroup of its first launch
        if ((rc = fused ? extend_primary(ctx, cam, settings, renderBVH) : generate(ctx, cam, settings, 1))) return rc;
        for (int b = 0; b < ctx->cfg.max_bounces; b++) {
            if (b > 0 || !fused) if ((rc = rt_stage_extend(ctx, b, renderBVH))) return rc;
            if (renderBVH) break;                                  // renderer.cpp:79
            if ((rc = stage_shade(ctx, b, fused && b == 0 ? cam : nullptr, aa))) return rc;
            if (!rr && nee) if ((rc = rt_stage_connect(ctx, b, b))) return rc;   // renderer.cpp:85-87
        }
        if (rr && nee && !renderBVH) if ((rc = rt_stage_connect(ctx, 0, ctx->cfg.max_bounces - 1))) return rc; // renderer.cpp:91-92
        ctx->frames++;
    }
    return RT_OK;
}
static int check_fault(RtCtx* ctx) // after a stream sync: did a bounded device-side wait expire?
{
    int32_t f = 0;
    HIPCHK(hipMemcpy(&f, ctx->q.fault, sizeof f, hipMemcpyDeviceToHost));
    if (f) {
        (void)hipMemset(ctx->q.fault, 0, sizeof f);
        return fail(RT_E_DEVICE, "device fault 0x%08x: a bounded wait of the ordered scan in k_shade expired (results of this render are invalid)", (unsigned)f);
    }
    return RT_OK;
}
extern "C" int rt_synchronize(RtCtx* ctx)
{
    if (!ctx) return fail(RT_E_INVALID, "rt_synchronize: null context");
    HIPCHK(hipSetDevice(ctx->cfg.device));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    ev_collect(ctx);
    return check_fault(ctx);
}

extern "C" int rt_focus(RtCtx* ctx, int32_t x, int32_t y, const RtCamera* cam, float* t)
{
    int rc = need_scene(ctx, "rt_focus"); if (rc) return rc;
    if (!cam || !t) return fail(RT_E_INVALID, "rt_focus: null argument");
    HIPCHK(hipSetDevice(ctx->cfg.device));
    hipLaunchKernelGGL(ctx->kFocus, dim3(1), dim3(kBlock), stack_bytes(ctx->facts.stackEntries), ctx->stream, ctx->sc, *cam, x, y, ctx->cfg.width, ctx->cfg.height, ctx->dFocus);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(t, ctx->dFocus, sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    return RT_OK;
}

extern "C" int rt_read_accum(RtCtx* ctx, RtFloat4* out)
{
    if (!ctx || !out) return fail(RT_E_INVALID, "rt_read_accum: null argument");
    HIPCHK(hipSetDevice(ctx->cfg.device));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    ev_collect(ctx);
    int rc = check_fault(ctx); if (rc) return rc;
    HIPCHK(hipMemcpy(out, ctx->q.accum, sizeof(float4) * (size_t)ctx->cfg.width * ctx->cfg.height, hipMemcpyDeviceToHost));
    return RT_OK;
}
// Restore half of a checkpoint: the running-sum accumulator (SURVEY.md §5 "Checkpoint / resume": the state a render
// carries across frames is {accum, seeds, frames}; seeds go through rt_set_seeds, frames live in the caller's Settings).
extern "C" int rt_write_accum(RtCtx* ctx, const RtFloat4* in)
{
    if (!ctx || !in) return fail(RT_E_INVALID, "rt_write_accum: null argument");
    HIPCHK(hipSetDevice(ctx->cfg.device));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    HIPCHK(hipMemcpy(ctx->q.accum, in, sizeof(float4) * (size_t)ctx->cfg.width * ctx->cfg.height, hipMemcpyHostToDevice));
    return RT_OK;
}
static int sum_table(RtCtx* ctx, const unsigned long long* dev, uint64_t out[kCtrCols])
{
    std::vector<unsigned long long> h((size_t)ctx->gridMax * kCtrCols);
    HIPCHK(hipMemcpy(h.data(), dev, h.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    for (int k = 0; k < kCtrCols; k++) out[k] = 0;
    for (size_t b = 0; b < (size_t)ctx->gridMax; b++) for (int k = 0; k < kCtrCols; k++) out[k] += h[b * kCtrCols + k];
    return RT_OK;
}
extern "C" int rt_read_counters(RtCtx* ctx, RtCounters* out)
{
    if (!ctx || !out) return fail(RT_E_INVALID, "rt_read_counters: null argument");
    HIPCHK(hipSetDevice(ctx->cfg.device));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    ev_collect(ctx);
    uint64_t e[kCtrCols], c[kCtrCols];
    int rc = sum_table(ctx, ctx->q.ctrExtend, e); if (rc) return rc;
    rc = sum_table(ctx, ctx->q.ctrConnect, c); if (rc) return rc;
    memset(out, 0, sizeof *out);
    out->extend_rays = e[0]; out->extend_tlas_visits = e[1]; out->extend_inst_visits = e[2]; out->extend_node_visits = e[3]; out->extend_prim_tests = e[4];
    out->connect_rays = c[0]; out->connect_tlas_visits = c[1]; out->connect_inst_visits = c[2]; out->connect_node_visits = c[3]; out->connect_prim_tests = c[4];
    out->primary_rays = ctx->primaryRays; out->shadow_rays = c[0]; out->frames = ctx->frames;
    out->extend_node_issues = e[5]; out->extend_leaf_issues = e[6]; out->connect_node_issues = c[5]; out->connect_leaf_issues = c[6];
    out->extend_loop_node_events = e[7]; out->extend_loop_leaf_events = e[8]; out->connect_loop_node_events = c[7]; out->connect_loop_leaf_events = c[8];
    return RT_OK;
}
extern "C" int rt_reset_counters(RtCtx* ctx)
{
    if (!ctx) return fail(RT_E_INVALID, "rt_reset_counters: null context");
    HIPCHK(hipSetDevice(ctx->cfg.device));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    HIPCHK(hipMemset(ctx->q.ctrExtend, 0, sizeof(unsigned long long) * (size_t)ctx->gridMax * kCtrCols));
    HIPCHK(hipMemset(ctx->q.ctrConnect, 0, sizeof(unsigned long long) * (size_t)ctx->gridMax * kCtrCols));
    ctx->frames = 0; ctx->primaryRays = 0;
    return RT_OK;
}
extern "C" int rt_read_stage_times(RtCtx* ctx, RtStageTimes* out)
{
    if (!ctx || !out) return fail(RT_E_INVALID, "rt_read_stage_times: null argument");
    HIPCHK(hipSetDevice(ctx->cfg.device));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    ev_collect(ctx);
    *out = ctx->times;
    return RT_OK;
}
extern "C" int rt_set_profile(RtCtx* ctx, int32_t level)
{
    if (!ctx || level < 0 || level > 2) return fail(RT_E_INVALID, "rt_set_profile: level must be 0, 1 or 2");
    HIPCHK(hipSetDevice(ctx->cfg.device));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    ev_collect(ctx);
    ctx->cfg.profile = level;
    ev_init(ctx);
    return RT_OK;
}
extern "C" int rt_reset_stage_times(RtCtx* ctx)
{
    if (!ctx) return fail(RT_E_INVALID, "rt_reset_stage_times: null context");
    HIPCHK(hipStreamSynchronize(ctx->stream));
    ev_collect(ctx);
    memset(&ctx->times, 0, sizeof ctx->times);
    return RT_OK;
}

// ---- debug import/export ----------------------------------------------------------------------
static int ray_io(RtCtx* ctx)
{
    if (!ctx->dRayIO) HIPCHK(hipMalloc((void**)&ctx->dRayIO, sizeof(RtRay) * (size_t)ctx->nPix));
    return RT_OK;
}
static int read_count(RtCtx* ctx, const int32_t* dev, int32_t* out)
{
    HIPCHK(hipMemcpyAsync(out, dev, sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    return RT_OK;
}
extern "C" int rt_debug_get_rays(RtCtx* ctx, int32_t bounce, RtRay* out, int32_t capacity, int32_t* n)
{
    int rc = need_scene(ctx, "rt_debug_get_rays"); if (rc) return rc;
    if (!n || bounce < 0 || bounce > ctx->cfg.max_bounces) return fail(RT_E_INVALID, "rt_debug_get_rays: bad argument");
    HIPCHK(hipSetDevice(ctx->cfg.device));
    if ((rc = read_count(ctx, ctx->q.nRays + bounce, n))) return rc;
    if (!out) return RT_OK;
    if (*n > capacity) return fail(RT_E_INVALID, "rt_debug_get_rays: capacity %d < %d rays", capacity, *n);
    if ((rc = ray_io(ctx))) return rc;
    if (*n > 0) {
        hipLaunchKernelGGL(k_export_rays, grid_for(*n), dim3(kBlock), 0, ctx->stream, ctx->sc, ctx->q, bounce, ctx->dRayIO);
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemcpyAsync(out, ctx->dRayIO, sizeof(RtRay) * (size_t)*n, hipMemcpyDeviceToHost, ctx->stream));
        HIPCHK(hipStreamSynchronize(ctx->stream));
    }
    return RT_OK;
}
extern "C" int rt_debug_set_rays(RtCtx* ctx, int32_t bounce, const RtRay* in, int32_t n)
{
    if (!ctx || !in || n < 0 || n > ctx->nPix || bounce < 0 || bounce > ctx->cfg.max_bounces) return fail(RT_E_INVALID, "rt_debug_set_rays: bad argument");
    // the kernels index the accumulator by pixelIdx and the primitives by primIdx: refuse what lies outside before anything is written
    // (a resize may have changed the copy since this holder's last launch: it is taken over first - its queues are emptied then, not
    // after the injection - and the count is the new one)
    if (ctx->sceneLoaded) if (const int rc = sync_scene_config(ctx)) return rc;
    const int32_t nPrims = ctx->sceneLoaded ? ctx->sc.nPrims : 0;
    for (int32_t i = 0; i < n; i++) {
        if (in[i].pixelIdx < ctx->firstPixel || in[i].pixelIdx >= ctx->firstPixel + ctx->nPix)
            return fail(RT_E_INVALID, "rt_debug_set_rays: ray %d: pixelIdx %d outside the context's band [%d, %d)", i, in[i].pixelIdx, ctx->firstPixel, ctx->firstPixel + ctx->nPix);
        if (in[i].primIdx < -1 || in[i].primIdx >= nPrims)
            return fail(RT_E_INVALID, "rt_debug_set_rays: ray %d: primIdx %d outside [-1, %d)", i, in[i].primIdx, nPrims);
    }
    HIPCHK(hipSetDevice(ctx->cfg.device));
    int rc = ray_io(ctx); if (rc) return rc;
    HIPCHK(hipStreamSynchronize(ctx->stream));
    if (n > 0) {
        HIPCHK(hipMemcpy(ctx->dRayIO, in, sizeof(RtRay) * (size_t)n, hipMemcpyHostToDevice));
        hipLaunchKernelGGL(k_import_rays, grid_for(n), dim3(kBlock), 0, ctx->stream, ctx->q, ctx->dRayIO, n, bounce & 1);
    }
    hipLaunchKernelGGL(k_set_count, dim3(1), dim3(1), 0, ctx->stream, ctx->q.nRays + bounce, n);
    memset(ctx->shadeRun, 0, sizeof ctx->shadeRun); ctx->generated = false;   // injected queue: scan state must be re-armed
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(ctx->stream));
    return RT_OK;
}
extern "C" int rt_debug_get_shadow(RtCtx* ctx, int32_t b0, int32_t b1, RtShadowRecord* out, int32_t capacity, int32_t* n)
{
    if (!ctx || !n || b0 < 0 || b1 < b0 || b1 >= ctx->cfg.max_bounces) return fail(RT_E_INVALID, "rt_debug_get_shadow: bad argument");
    if (ctx->sceneLoaded) if (const int rc = sync_scene_config(ctx)) return rc;   // (a holder of a resized copy: its queues are emptied first)
    HIPCHK(hipSetDevice(ctx->cfg.device));
    int32_t lo = 0, hi = 0, rc;
    if ((rc = read_count(ctx, ctx->q.nShadow + b0, &lo))) return rc;
    if ((rc = read_count(ctx, ctx->q.nShadow + b1 + 1, &hi))) return rc;
    *n = hi - lo;
    if (!out) return RT_OK;
    if (*n > capacity) return fail(RT_E_INVALID, "rt_debug_get_shadow: capacity %d < %d", capacity, *n);
    std::vector<float4> a((size_t)*n), b((size_t)*n), c((size_t)*n);
    if (*n > 0) {
        HIPCHK(hipMemcpy(a.data(), ctx->q.sA + lo, sizeof(float4) * a.size(), hipMemcpyDeviceToHost));
        HIPCHK(hipMemcpy(b.data(), ctx->q.sB + lo, sizeof(float4) * b.size(), hipMemcpyDeviceToHost));
        HIPCHK(hipMemcpy(c.data(), ctx->q.sC + lo, sizeof(float4) * c.size(), hipMemcpyDeviceToHost));
    }
    for (int32_t i = 0; i < *n; i++) {
        RtShadowRecord r;
        r.ox = a[i].x; r.oy = a[i].y; r.oz = a[i].z; r.tmax = a[i].w;
        r.lx = b[i].x; r.ly = b[i].y; r.lz = b[i].z; memcpy(&r.pixelIdx, &b[i].w, 4);
        r.radiance = RtFloat4{ c[i].x, c[i].y, c[i].z, c[i].w };
        out[i] = r;
    }
    return RT_OK;
}
extern "C" int rt_debug_enable_steps(RtCtx* ctx, int32_t on)
{
    if (!ctx) return fail(RT_E_INVALID, "rt_debug_enable_steps: null context");
    HIPCHK(hipStreamSynchronize(ctx->stream));
    ctx->q.steps = on ? ctx->dSteps : nullptr;
    return RT_OK;
}
extern "C" int rt_debug_get_steps(RtCtx* ctx, int32_t* out, int32_t capacity, int32_t* n)
{
    if (!ctx || !n) return fail(RT_E_INVALID, "rt_debug_get_steps: bad argument");
    if (!ctx->q.steps) return fail(RT_E_INVALID, "rt_debug_get_steps: call rt_debug_enable_steps(ctx, 1) before the extend stage");
    HIPCHK(hipSetDevice(ctx->cfg.device));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    *n = ctx->nPix;
    if (!out) return RT_OK;
    if (capacity < ctx->nPix) return fail(RT_E_INVALID, "rt_debug_get_steps: capacity too small");
    HIPCHK(hipMemcpy(out, ctx->dSteps, sizeof(int32_t) * (size_t)ctx->nPix, hipMemcpyDeviceToHost));
    return RT_OK;
}

// ---- post-processing chain (renderer.cpp:95-124 PostProc, :303-308 SaveFrame) ----------------------------------------
extern "C" int rt_postproc(RtCtx* ctx, int32_t frames, float vignette, float gamma, float chromatic, RtFloat4* outF32, uint8_t* outRGBA8)
{
    if (!ctx) return fail(RT_E_INVALID, "rt_postproc: null context");
    if (frames <= 0) return fail(RT_E_INVALID, "rt_postproc: frames must be > 0 (it is the divisor of prep())");
    return postproc(ctx, ctx->q.accum, frames, vignette, gamma, chromatic, outF32, outRGBA8);
}
int postproc(RtCtx* ctx, const float4* accum, int32_t frames, float vignette, float gamma, float chromatic, RtFloat4* outF32, uint8_t* outRGBA8)
{
    HIPCHK(hipSetDevice(ctx->cfg.device));
    const size_t px = (size_t)ctx->cfg.width * ctx->cfg.height;
    if (!ctx->dPostF) { HIPCHK(hipMalloc((void**)&ctx->dPostF, px * sizeof(float4))); HIPCHK(hipMalloc((void**)&ctx->dPostB, px * 4)); }
    PostParams pp{ 1 / (float)frames, vignette, gamma, chromatic, ctx->cfg.width, ctx->cfg.height };
    hipLaunchKernelGGL(k_postproc, grid_for((int)px), dim3(kBlock), 0, ctx->stream, accum, ctx->dPostF, ctx->dPostB, pp);
    HIPCHK(hipGetLastError());
    if (outF32) HIPCHK(hipMemcpyAsync(outF32, ctx->dPostF, px * sizeof(float4), hipMemcpyDeviceToHost, ctx->stream));
    if (outRGBA8) HIPCHK(hipMemcpyAsync(outRGBA8, ctx->dPostB, px * 4, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    ev_collect(ctx);
    return RT_OK;
}

#ifdef RT355_TAIL_PROBE
// lab build only: copies the per-wave probe records of the last persistent launches out (9 x 8192 x 4 uint64, see rt355_kernels.h)
extern "C" int rt_lab_tail_probe(void* out) { return hipMemcpyFromSymbol(out, HIP_SYMBOL(rt355dev::g_tp), sizeof(rt355dev::g_tp)) == hipSuccess ? 0 : 1; }
#endif

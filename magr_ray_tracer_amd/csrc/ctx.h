// ctx.h — a rendering context (RtCtx, include/rt355.h) as rt355.hip, which owns it, and group.hip, which runs several of them as the
// lanes of a group, both see it.  group.hip goes through the public rt_* calls; of the struct it reads and writes `stream`, `home`,
// `queued`, `cfg`, `nPix`, `firstPixel` and `q.accum`, and of rt355.hip's internals it calls what is declared at the end of this file.
#pragma once
#include <algorithm>
#include <memory>
#include <vector>
#include "rt355_dev.h"
#include "scene_dev.h"

struct RtCtx {
    RtConfig cfg{};
    hipStream_t stream = nullptr;         // where this context's work is queued: `home`, unless a group has moved its frames (rt_group_render)
    hipStream_t home = nullptr;           // the context's own stream
    bool queued = true;                   // asynchronous work queued since a group marked the end of this context's last frame
    rt355dev::DevScene sc{};
    rt355dev::DevQueues q{};
    rt355dev::DevVariant var{};
    int nPix = 0, firstPixel = 0, gridMax = 0;
    int cuCount = 0; size_t ldsPerBlock = 0, ldsPerCU = 0;   // of cfg.device, asked once by rt_create: CUs, the LDS a workgroup may ask for, the LDS of a CU
    bool sceneLoaded = false, ownAccum = true;
    std::shared_ptr<scenedev::SceneBag> scene;   // shared by the contexts of rt_share_scene, freed with the last of them
    uint64_t sceneGen = 0;                // the SceneBag generation this context's traversal configuration was derived for
    scenedev::SceneFacts facts;           // what the traversal is planned from (this and sc: the copy's, assigned whole by adopt_scene only)
    std::vector<void*> queueAllocs;
    float* dFocus = nullptr;
    RtRay* dRayIO = nullptr; // debug import/export staging (lazy)
    uint64_t frames = 0, primaryRays = 0;
    // profiling
    struct Ev { hipEvent_t a, b; int stage; };
    std::vector<Ev> evPool; size_t evUsed = 0;
    RtStageTimes times{};
    int trav = 0;           // the traversal kernels (Traversal, set by configure_traversal)
    int coherent = 1;       // RT355_COHERENT: wave-uniform node records through the scalar cache on bounce 0 (1), every bounce of the TLAS kernel (2, lab), off (0)
    uint32_t* dSpill = nullptr; size_t spillWords = 0;
    int xcdFirst = -1;      // the XCD this context's sparse queues start on (PersistTune.xcdFirst)
    int spillCap = 0;       // LDS stack entries per lane of a spilling kernel, set by configure_traversal (RT355_SPILL_CAP: tests force the spill path with a tiny cap, >= 6)
    bool cursorUsed[2 * (RT_MAX_BOUNCES + 2)] = {};   // work-queue heads consumed since the last k_begin_frame
    bool shadeRun[RT_MAX_BOUNCES + 1] = {};           // shade(b) launched since the last k_begin_frame
    bool generated = false;                           // generate launched since the last k_begin_frame
    int persistGrid = 0, persistGridConnect = 0;
    rt355dev::PersistTune tune{}, tuneConnect{}, tune4{};   // extend (BVH2), connect, extend (BVH4): set by configure_traversal
    int tuneBlocks = 0, connectBlocks = 0;   // workgroups per CU the knobs ask of the persistent grids (TravPlan; persist_blocks)
    float4* dPostF = nullptr; uchar4* dPostB = nullptr;   // post-processing outputs (lazy)
    int32_t* dSteps = nullptr;   // per-ray `steps` buffer, only bound while rt_debug_enable_steps is on
    // rt_trace's own DevQueues view (lazy): count, cursor and fault words and a counter table that no frame reads or writes, and queue
    // arrays for the batches that are not traced in the caller's arrays, grown to the largest pass so far
    struct TraceView { rt355dev::DevQueues q{}; bool ready = false; std::vector<void*> words; float4* rays[3] = {}; size_t cap = 0; } tv;
    int shadeTile = rt355dev::kTile;   // k_shade tile = workgroup size: kTile (512), or 256 for contexts that share the GPU (RtConfig.shade_blocks_per_cu > 0)
    int shadeGrid = 1024;   // workgroups of k_shade (what the CUs hold at once; the kernel does not depend on it); set in rt_create
    // The instantiations of the kernels that reach one of the seven builtins, for this context's arithmetic (cfg.builtins, resolved to
    // RT_BUILTINS_IEEE or RT_BUILTINS_REFERENCE), shading, tile and accel: chosen once by choose_builtin_kernels (rt_create)
    void (*kGenerate)(rt355dev::DevQueues, RtCamera, int, int) = nullptr;
    void (*kShade)(rt355dev::DevScene, rt355dev::DevQueues, rt355dev::DevVariant, rt355dev::ShadeArg<false>) = nullptr;
    void (*kFocus)(rt355dev::DevScene, RtCamera, int, int, int, int, float*) = nullptr;
    // ... and of the fused primary path of rt_render (fusePrimary, set by configure_traversal from the plan): bounce 0's traversal launch
    // that computes its rays - plain, coherent, BVH4 - and bounce 0's shade launch that computes them again
    enum { PRIMARY_PLAIN, PRIMARY_COHERENT, PRIMARY_BVH4, PRIMARY_KINDS };
    void (*kTracePrimary[PRIMARY_KINDS])(rt355dev::DevScene, rt355dev::DevQueues, RtCamera, int, int, rt355dev::PersistTune) = {};
    void (*kShadePrimary)(rt355dev::DevScene, rt355dev::DevQueues, rt355dev::DevVariant, rt355dev::ShadeArg<true>) = nullptr;
    bool fusePrimary = false;   // rt_render runs no k_generate: bounce 0's extend and shade launches make the primary rays themselves
};

static inline dim3 grid_for(int n) { return dim3((unsigned)std::max(1, (n + rt355dev::kBlock - 1) / rt355dev::kBlock)); }
// rt355.hip, for group.hip (hidden: neither is exported from the library)
__attribute__((visibility("hidden"))) void ctx_free(RtCtx* ctx);   // every owned resource; safe on a partially constructed context
// rt_postproc's work on the accumulator it is handed: the context's own, or a group's sum of its lanes'
__attribute__((visibility("hidden"))) int postproc(RtCtx* ctx, const float4* accum, int32_t frames, float vignette, float gamma, float chromatic,
                                                    RtFloat4* outF32, uint8_t* outRGBA8);

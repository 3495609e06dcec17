/* rt355.h — C-ABI of the MI355X device path (librt355.so).
 *
 * The reference has no FFI: its "operator API" is the Kernel/Buffer call sequence that
 * Renderer issues (reference: src/renderer.cpp:64-94 RayTrace, :142-209 InitBuffers,
 * :211-263 InitWavefrontKernels, :289-301 FocusCamera, :126-140 ComputeEnergy) plus the
 * POD arrays of src/common.h.  Each entry point below replaces the cited piece of that
 * sequence; INTEGRATION.md shows the Renderer-side binding.
 *
 * Conventions: every function returns 0 on success and a negative RT_E_* code on
 * failure; rt_last_error() returns a thread-local message (the reference aborts through
 * FatalError(), template/template.cpp:949-962 — this library never aborts).  Host
 * pointers are copied during the call and never retained (the reference's Buffer keeps
 * a non-owning alias and copies in CopyToDevice(), template.cpp:1133-1137).  A context
 * is bound to one GPU and is not re-entrant: one host thread (or process) per GPU.
 * There is NO CPU fallback: without a HIP device rt_create() fails.
 */
#ifndef RT355_H
#define RT355_H
#include "rt355_types.h"

#ifdef __cplusplus
extern "C" {
#endif

#define RT_OK            0
#define RT_E_INVALID    (-1)   /* bad argument / call order                       */
#define RT_E_DEVICE     (-2)   /* HIP error (message in rt_last_error)            */
#define RT_E_NOMEM      (-3)
#define RT_E_UNSUPPORTED (-4)

/* Kernel variants — the reference's prepended #defines (renderer.h:6-19, renderer.cpp:213-215). */
#define RT_SHADING_SIMPLE       0   /* SHADING_SIMPLE ("Kajiya")  */
#define RT_SHADING_NEE          1   /* SHADING_NEE (default)      */
#define RT_SAMPLING_HEMISPHERE  0   /* SAMPLING_HEMISPHERE        */
#define RT_SAMPLING_COSINE      1   /* SAMPLING_COSINE (default)  */
#define RT_ACCEL_BVH2           0   /* USE_BVH2 (default)         */
#define RT_ACCEL_BVH4           1   /* USE_BVH4                   */

typedef struct RtCtx RtCtx;

/* Replaces the compile-time macros of src/constants.h:3-7,28-31 and the ImGuiData
 * variant selection (renderer.h:23-36) with run-time values. */
typedef struct RtConfig {
    int32_t width, height;      /* SCRWIDTH, SCRHEIGHT                                        */
    int32_t y0, y1;             /* row band [y0,y1) this context renders; 0,height = all rows  */
    int32_t max_bounces;        /* MAX_BOUNCES host loop count (7); must be 1..RT_MAX_BOUNCES  */
    int32_t shading, sampling, accel;
    int32_t russian_roulette;   /* RUSSIAN_ROULETTE                                           */
    int32_t filter_fireflies;   /* FILTER_FIREFLIES                                           */
    int32_t device;             /* HIP device ordinal                                         */
    int32_t extend_variant;     /* traversal kernels: 0 = best available (derived node/triangle layout + persistent
                                 * wavefronts when the TLAS has one BLAS), 1 = traverse the reference arrays as uploaded,
                                 * one ray per lane, 2 = derived layout, one ray per lane, 4 = as 0 but multi-BLAS scenes keep the
                                 * one-ray-per-lane nested TLAS loops instead of k_trace_persist_tlas (A/B runs),
                                 * 6 = as 0, and a BVH4 context whose scene has several BLAS (layout 1, a TLAS of at most 8
                                 * levels, fewer than 2^29 quad records) traces through k_trace_persist4_tlas instead of the
                                 * one-ray-per-lane nested loops (opt-in until it has been measured as the default)   */
    int32_t profile;            /* HIP-event brackets on the context's stream: 0 none, 1 extend launches only
                                 * (what the roofline needs; ~1 % overhead), 2 every stage launch (~3.5 %)        */
    int32_t shade_blocks_per_cu;/* k_shade workgroups per CU: 0 = what the CUs hold (2, best for one context with the GPU to itself);
                                 * > 0 also selects 256-slot tiles (24.9 KB of LDS instead of 49.8; rt_shade_footprint): 1 leaves room for the kernels of
                                 * other contexts (best when several sample streams share the GPU)                               */
    int32_t persist_blocks_per_cu; /* workgroups per CU of the persistent traversal grids: 0 = what the hardware admits (7 extend / 6 connect);
                                 * 4 is best when three contexts share the GPU (their workgroups then fit beside each other);
                                 * a group of several lanes picks 2 when four or more of its streams run side by side, else 3       */
    int32_t builtins;           /* RT_BUILTINS_*: how normalize / length / exp / sin / cos / acospi / atan2pi are evaluated (see below);
                                 * any other value: RT_E_INVALID                                                             */
} RtConfig;

/* RtConfig.builtins.  IEEE: sequences of IEEE + - * / sqrt that a CPU reproduces bit for bit (what the oracle checks).  REFERENCE: the
 * instruction sequences ROCm's OpenCL library gives the reference's own kernels (hardware rsq / sqrt, the ocml functions): the
 * reference's image from the reference's seeds.  DEFAULT (what a zero-filled struct asks for) is IEEE. */
#define RT_BUILTINS_DEFAULT    0
#define RT_BUILTINS_IEEE       1
#define RT_BUILTINS_REFERENCE  2

/* Device-side work counters (per-kernel-family totals since the last rt_reset_counters).
 * They define the algorithmic bytes of SURVEY.md §8(d). */
typedef struct RtCounters {
    uint64_t extend_rays, extend_tlas_visits, extend_inst_visits, extend_node_visits, extend_prim_tests;
    uint64_t connect_rays, connect_tlas_visits, connect_inst_visits, connect_node_visits, connect_prim_tests;
    uint64_t primary_rays;       /* pixels generated                     */
    uint64_t shadow_rays;        /* shadow rays appended by shade        */
    uint64_t frames;
    /* how often the persistent event loops issued their two code paths (wave level) and how many events those issues carried:
     * loop_node_events / (64 * node_issues) is the share of the lanes that had a box pair to test when the node path ran,
     * loop_leaf_events / (64 * leaf_issues) the same for the triangle path.  Counted by the extend instantiation that also keeps the
     * per-ray `steps` (rt_debug_enable_steps(ctx, 1) or renderBVH): the production kernel does not pay for them; launches that ran one
     * ray per lane count nothing here.  An iteration of the top descent (a node event whose record comes from the LDS top table,
     * rt_top_levels) is an issue of the node path and its events are node events */
    uint64_t extend_node_issues, extend_leaf_issues, connect_node_issues, connect_leaf_issues;
    uint64_t extend_loop_node_events, extend_loop_leaf_events, connect_loop_node_events, connect_loop_leaf_events;   /* the events those issues carried */
} RtCounters;

/* Accumulated stage times in milliseconds (HIP events on the context's stream) and
 * launch counts; only filled when RtConfig.profile != 0. */
typedef struct RtStageTimes {
    double  generate_ms, extend_ms, shade_ms, compact_ms, connect_ms, accumulate_ms;
    int64_t generate_launches, extend_launches, shade_launches, compact_launches, connect_launches, accumulate_launches;
} RtStageTimes;

/* Which kernels a context runs for the uploaded scene (chosen at rt_upload_scene; bench.py names the roofline's kernel from it). */
typedef struct RtKernelInfo {
    int32_t layout;               /* 0 = the reference arrays as uploaded, 1 = derived pair / quad / triangle records */
    int32_t persist, persist4;    /* persistent-wavefront traversal over the BVH2 (1: one BLAS, 2: through a multi-BLAS
                                   * TLAS, k_trace_persist_tlas, 3: the same with the deep end of the traversal stacks
                                   * spilled to global memory) / over the BVH4 (1: one BLAS, k_trace_persist4; with
                                   * extend_variant 6 also 2: through a multi-BLAS TLAS, k_trace_persist4_tlas, 3: the
                                   * same with the deep end of the stacks in global memory).  At most one is non-zero  */
    int32_t stack_entries;        /* LDS traversal stack entries per lane (a spilling kernel: the part kept in LDS)   */
    int32_t persist_grid, persist_grid_connect, shade_grid;   /* workgroups of the persistent launches                */
    int32_t n_blas;
} RtKernelInfo;

const char* rt_last_error(void);
int rt_device_count(void);
int rt_kernel_info(RtCtx* ctx, RtKernelInfo* out);
int rt_builtins(RtCtx* ctx);   /* the context's arithmetic, resolved: RT_BUILTINS_IEEE or RT_BUILTINS_REFERENCE */
/* Levels of the BLAS that the event loops of extend and of connect descend from a table in LDS when a lane takes a new ray (0..6; 0: no
 * table.  Single-BLAS BVH2 scenes under persistent wavefronts only, else 0; RT355_TOP_LEVELS overrides the defaults) */
int rt_top_levels(RtCtx* ctx, int32_t* extend, int32_t* connect);
/* How a context chooses its traversal, for tests (the rules: csrc/trav_common.h, free of the device).  The plan is a function of these
 * facts and of the RT355_* traversal knobs in the environment. */
typedef struct RtTraversalFacts {
    int32_t accel, extend_variant, persist_blocks_per_cu;   /* of RtConfig                                                          */
    int32_t layout;              /* of the scene copy: RtKernelInfo.layout                                                            */
    int32_t singleBlas;          /* the TLAS root is a leaf (0 / 1)                                                                    */
    int32_t tlasDepth;           /* levels of the TLAS                                                                                 */
    int32_t nInterior, nQuads;   /* records of the pair table (BVH2) and of the quad table (BVH4) in layout 1: ids must fit 29 bits    */
    int32_t stackEntries;        /* traversal stack entries the deepest BLAS needs                                                     */
    int32_t sharedMemPerBlock;   /* of the device: bytes of LDS a workgroup may ask for                                                */
    int32_t xcdFirst;            /* the XCD (0..7) this context's sparse queues start on; handed out per context, passed through       */
} RtTraversalFacts;
#define RT_TUNE_FIELDS 11   /* a launch tune as integers: chunk, refill, inner, leafK, fixedChunks, flat, xcdRays, xcdFirst, thin, topLevels, topBase */
typedef struct RtTraversalPlan {
    int32_t trav;                /* 0 nested loops, 1 BVH2, 2 TLAS, 3 TLAS with spilling stacks, 4 BVH4, 5 BVH4 TLAS, 6 BVH4 TLAS with spilling stacks */
    int32_t spillCap;            /* LDS stack entries per lane of a spilling kernel (12, or RT355_SPILL_CAP)                           */
    int32_t coherent;            /* RT355_COHERENT, default 1                                                                          */
    int32_t topAuto;             /* 1: no knob named the LDS top table's depth, the context fits it to the device (rt_top_levels)      */
    int32_t tuneBlocks, connectBlocks;   /* workgroups per CU asked of the persistent grids by RT355_TUNE's fifth field / RT355_CONNECT_BLOCKS, else 0 */
    int32_t tune[RT_TUNE_FIELDS], tuneConnect[RT_TUNE_FIELDS], tune4[RT_TUNE_FIELDS];   /* extend (BVH2), connect, extend (BVH4), before
                                  * the context fits topLevels to the device; topBase is set per launch and 0 here                      */
} RtTraversalPlan;
/* The plan of `facts` under the knobs as the environment holds them now.  Needs no device and no context. */
int rt_debug_traversal_plan(const RtTraversalFacts* facts, RtTraversalPlan* out);
/* The facts this context's configuration is planned from (it takes over a changed scene copy first, as rt_kernel_info does). */
int rt_debug_traversal_facts(RtCtx* ctx, RtTraversalFacts* out);
/* What shares a CU when contexts run side by side.  *ldsBytes: the static LDS of a workgroup of this context's k_shade instantiation
 * (256 slots for the lanes of a group, 512 for a context alone).  *traversalBeside: how many workgroups of the context's persistent
 * extend kernel, without a top table, fit a CU beside one such workgroup - by LDS, VGPRs and wave slots, from the kernels' own
 * attributes (0 where no persistent kernel runs).  For a context that shares the GPU (RtConfig.persist_blocks_per_cu > 0) the automatic
 * rt_top_levels are the deepest tables that keep this number. */
int rt_shade_footprint(RtCtx* ctx, int32_t* ldsBytes, int32_t* traversalBeside);
/* k_shade's staged tables.  *capacityRows: the 16-byte LDS rows reserved for them; a light takes six, a material three.  *staged: 1 if
 * this context's k_shade launches read the uploaded scene's light records and materials from LDS - all of both fit the rows - and 0 if
 * they read them from global memory (the scene needs more rows, or RT355_SHADE_TABLES=0).  The results are the same bits either way. */
int rt_shade_tables(RtCtx* ctx, int32_t* capacityRows, int32_t* staged);
/* The fused primary path of rt_render.  *fused: 1 if this context's frames launch no k_generate - bounce 0's extend launch computes each
 * pixel's primary ray from the camera and the pixel's seed instead of loading it, bounce 0's shade launch computes it again, and the
 * primary queue (origin, direction, intensity, meta) is never stored; 0 if they generate and store it first.  Fused are single-BLAS
 * scenes under persistent wavefronts, BVH2 (not with extend_variant 3 or 5) and BVH4; multi-BLAS scenes and the nested kernels are not;
 * RT355_FUSE_PRIMARY=0 keeps every context on k_generate.  The results are the same bits either way: accumulators, seeds, queue lengths,
 * counters.  The stage-level calls never fuse: rt_stage_generate stores the queue that rt_stage_extend(0) and rt_stage_shade(0) read, and
 * after a fused frame the stored queue of bounce 0 is NOT that frame's - generate before running bounce 0's stages by hand. */
int rt_primary_fused(RtCtx* ctx, int32_t* fused);

/* new Buffer(...) x11 + new Kernel(...) x6 (renderer.cpp:145-157, :218-223). */
int rt_create(const RtConfig* cfg, RtCtx** out);
int rt_destroy(RtCtx* ctx);

/* primBuffer/matBuffer/texBuffer/lightBuffer/bvhNodeBuffer/bvhIdxBuffer/tlasNodeBuffer/
 * blasNodeBuffer ->CopyToDevice() (renderer.cpp:160-208).  bvhNodes is RtBVHNode2[nNodes]
 * for RT_ACCEL_BVH2 and RtBVHNode4[nNodes] for RT_ACCEL_BVH4, uploaded unchanged. */
int rt_upload_scene(RtCtx* ctx,
                    const RtPrimitive* prims, int32_t nPrims,
                    const RtMaterial* mats, int32_t nMats,
                    const RtFloat4* textures, int32_t nTexels,
                    const uint32_t* lights, int32_t nLights,
                    const void* bvhNodes, int32_t nNodes,
                    const uint32_t* primIdx, int32_t nIdx,
                    const RtTLASNode* tlas, int32_t nTlas,
                    const RtBVHInstance* blas, int32_t nBlas);

/* rt_upload_scene with bvhNodes always RtBVHNode2[nNodes].  On a BVH2 context it is rt_upload_scene.  On a BVH4 context the BVH2 is
 * validated by the BVH2 rules (plus rt_build_bvh4's check of every interior record), uploaded and collapsed on the device
 * (rt_build_bvh4's kernels); quad records, triangle records and root entries are derived there too.  Afterwards every device array
 * and rt_kernel_info equal those of rt_upload_scene of the same scene collapsed on the host.  The copy keeps the BVH2 on the device
 * (RT_SCENE_BVH2_KEPT) and the primitive range of every BLAS, so rt_rebuild_scene works on it (a copy bound through rt_upload_scene
 * on a BVH4 context has lost the BVH2 and refuses).  A refusal - the checks, a collapsed BLAS that needs more than RT_BVH4_STACK
 * stack entries (RT_E_UNSUPPORTED) - leaves the bound scene and its stack size untouched. */
int rt_upload_scene_bvh2(RtCtx* ctx,
                         const RtPrimitive* prims, int32_t nPrims, const RtMaterial* mats, int32_t nMats,
                         const RtFloat4* textures, int32_t nTexels, const uint32_t* lights, int32_t nLights,
                         const RtBVHNode2* bvhNodes, int32_t nNodes, const uint32_t* primIdx, int32_t nIdx,
                         const RtTLASNode* tlas, int32_t nTlas, const RtBVHInstance* blas, int32_t nBlas);

/* The host-side shape checks rt_upload_scene runs before it touches the device (index ranges, tree cycles and depths, stack needs,
 * the 32768-node / instance bound of the TLAS encodings), callable without a GPU.  `accel` says how bvhNodes is to be read.  What it
 * accepts, every kernel and every derivation of rt_upload_scene can walk inside the arrays, within the stacks and in finite time, with
 * the reference arrays and with the derived records alike; anything else is RT_E_INVALID or RT_E_UNSUPPORTED with a message.
 *   BVH4 slots   slot k of a node is unused iff first[k] == -1 (RT_INVALID); a used slot needs count[k] >= 0 and first[k] >= 0:
 *                count > 0 is a leaf with first + count <= nIdx, count == 0 a child with first < nNodes.  Every slot of every record
 *                is held to this, reachable or not; a violation is RT_E_INVALID naming the node and the slot.  (The collapse writes
 *                first = count = -1 into an unused slot and leaves absorbed nodes behind: both pass.)
 *   sharing      instances may share a BLAS root.  A BVH2 subtree named by two parents is accepted as long as the walk over every
 *                path from the root stays within 2 * nNodes + 2 node visits (each level of fully shared children doubles the visits:
 *                a ladder of 3 such levels - 7 nodes, 15 visits - passes, one of 4 - 9 nodes, 31 visits - is refused as malformed),
 *                a BVH4 one within nNodes + 1; such a scene renders but can neither be refit nor rebuilt in place.  A TLAS node
 *                reachable twice is always refused.
 *   unreachable  records no root leads to may hold zeros; their leaf ranges (BVH2) and slots (BVH4) are still checked.
 * Counts below zero are RT_E_INVALID. */
int rt_validate_scene(int32_t accel,
                      const RtPrimitive* prims, int32_t nPrims, const RtMaterial* mats, int32_t nMats,
                      const RtFloat4* textures, int32_t nTexels, const uint32_t* lights, int32_t nLights,
                      const void* bvhNodes, int32_t nNodes, const uint32_t* primIdx, int32_t nIdx,
                      const RtTLASNode* tlas, int32_t nTlas, const RtBVHInstance* blas, int32_t nBlas);

/* A second context on the same device renders the scene `from` holds: it takes `from`'s device copy (uploaded arrays + derived
 * layouts) instead of uploading its own - one copy in HBM and in the caches for the sample streams of a GPU or the row bands of a
 * frame.  The contexts must agree in accel and extend_variant; the copy lives until the last context holding it is destroyed or
 * uploads another scene.  (The reference has one Renderer and one set of buffers, renderer.cpp:160-208; several contexts per device
 * are this library's way to keep a GPU full.) */
int rt_share_scene(RtCtx* ctx, RtCtx* from);

/* ---- acceleration structures on the GPU ----------------------------------------------------------------------------------------
 * Linear BVH (Karras radix tree over 63-bit Morton | index keys, then a bottom-up SAH collapse) over the primitives
 * [first, first + count) of prims[nPrims], built on `device` (a HIP ordinal) and written in the wire format BVH2::BuildBLAS writes:
 * the root is node nodeBase, children are adjacent (first, first + 1), a leaf indexes primIdx at idxBase + (start of its range in key
 * order), primIdx[0, count) receives global primitive ids.  nodes[] needs room for 2 * count - 1 records (nodeCap); *nNodes receives
 * the number written (2 * leaves - 1).  Node and index ids are global, so the arrays can be appended behind the BLASes of either
 * builder.  The tree is a pure function of the primitives and the options: identical on every call and equal, array for array, to
 * the host restatement rth_build_bvh2_lbvh (rt355_host.h).  Its height is <= 63 (rt_validate_scene accepts it).  Synchronous, on a
 * stream of its own; opts NULL = defaults (max_leaf 8, C_t = C_i = 1).  Errors (count <= 0, range outside nPrims, nodeCap too small,
 * bad options, a bad device) return RT_E_* before anything is launched or written.  stats may be NULL. */
int rt_build_bvh2(int32_t device, const RtBuildOptions* opts, const RtPrimitive* prims, int32_t nPrims, int32_t first, int32_t count,
                  uint32_t nodeBase, uint32_t idxBase, RtBVHNode2* nodes, int32_t nodeCap, int32_t* nNodes, uint32_t* primIdx,
                  RtBuildStats* stats);
/* The default SAH BLAS on the GPU: BVH2::BuildBLAS with alpha = 1 (binned SAH, object splits only; rt355_host.h rth_build_blas)
 * over the primitives [first, first + count) of prims[nPrims], on `device`.  Its nodes and primIdx equal, byte for byte, what
 * BuildBLAS(startIdx = first) appends when first + count == nPrims and nodeBase / idxBase are the scene's node and primIdx counts:
 * the root is node nodeBase, the r-th interior node in BuildBLAS's LIFO pop order (right child popped first) has its children at
 * nodeBase + 1 + 2r and nodeBase + 2 + 2r, leaves take primIdx[idxBase + o, + count) in pop order, at most 2 * count - 1 nodes.
 * The rules live in csrc/sah_common.h; the host restatement rth_build_bvh2_sah (rt355_host.h) gives the same arrays.  Any depth.
 * Synchronous, on a stream of its own; the caller's device is restored.  stats: nodes, leaves, depth (BVH2::Depth), sah_cost
 * (BVH2::TotalCost, identical), morton_bits 0, device_ms, wall_ms; may be NULL.
 * Refusals write nothing to the caller's arrays:
 *   RT_E_INVALID      the argument checks of rt_build_bvh2 (count <= 0 or > 2^30, range outside nPrims, nodeCap < 2 * count - 1,
 *                     ids overflowing 32 bits, a missing array, a bad device);
 *   RT_E_UNSUPPORTED  inputs on which BuildBLAS has no defined result: a primitive box or centroid that is not finite; a node
 *                     whose bin index would be computed from a NaN or an infinity (a centroid extent that overflows, or one so
 *                     small that 8 / extent overflows); a node of more than RT_MIN_LEAF_PRIMS refs with no leaf decision and no
 *                     object split below RT_REALLYFAR (node areas near 1e30: coordinates of about 1e15 and beyond). */
int rt_build_bvh2_sah(int32_t device, const RtPrimitive* prims, int32_t nPrims, int32_t first, int32_t count, uint32_t nodeBase,
                      uint32_t idxBase, RtBVHNode2* nodes, int32_t nodeCap, int32_t* nNodes, uint32_t* primIdx, RtBuildStats* stats);
/* Wall-clock split of this process's last successful rt_build_bvh2_sah (measurement aid, tools/sah_gpu_bench.py): out[0] allocation
 * and upload, out[1] the level passes, out[2] numbering and emit, out[3] download (ms), out[4] the number of level passes. */
int rt_debug_sah_phases(float* out);
/* SBVH BLAS trees on the GPU: BVH2::BuildBLAS with bvh2->alpha = alpha in [0, 1] (binned SAH with spatial splits; 0 = full SBVH,
 * 1 = rt_build_bvh2_sah's tree) over the primitives [first, first + count) of prims[nPrims], on `device`.  Nodes and primIdx equal,
 * byte for byte, what BuildBLAS(startIdx = first) appends (see rt_build_bvh2_sah: root at nodeBase, LIFO numbering, leaves index
 * primIdx from idxBase, ids global).  A spatial split duplicates refs, so neither array has a bound known beforehand: when nodeCap
 * or idxCap is too small for the finished tree the call writes nothing to nodes / primIdx, stores the needed sizes in *nNodes /
 * *nIdx and returns RT_E_INVALID with "capacity" in the message; a second call with those sizes succeeds.  The rules live in
 * csrc/sbvh_common.h; the host restatement rth_build_bvh2_sbvh (rt355_host.h) gives the same arrays.  Any depth.  Synchronous, on a
 * stream of its own; the caller's device is restored.  stats may be NULL.  The environment variable RT355_SBVH_INITIAL_REFS=k,
 * read per call, sets the initial capacity of the ref arrays (they grow level by level; for tests and A/B runs).
 * Refusals write nothing to the caller's arrays:
 *   RT_E_INVALID      alpha not in [0, 1] (NaN included); rt_build_bvh2_sah's argument checks except the capacities; capacity (above);
 *   RT_E_NOMEM        device memory (the ref arrays grow with the tree);
 *   RT_E_UNSUPPORTED  what rt_build_bvh2_sah refuses, and a spatial bin index scale * (x - bmin) that is not finite, is <= -1 or is
 *                     >= 2^31 where a spatial split is evaluated (a ref with an empty or inverted box: a plane inside the range, a
 *                     sphere fragment whose clip came out inverted).  BuildBLAS indexes bins[] with it; it throws by the same rule. */
int rt_build_bvh2_sbvh(int32_t device, float alpha, const RtPrimitive* prims, int32_t nPrims, int32_t first, int32_t count,
                       uint32_t nodeBase, uint32_t idxBase, RtBVHNode2* nodes, int32_t nodeCap, int32_t* nNodes, uint32_t* primIdx,
                       int32_t idxCap, int32_t* nIdx, RtSbvhStats* stats);
/* Wall-clock split of this process's last successful rt_build_bvh2_sbvh (tools/sbvh_gpu_bench.py): out[0] allocation and upload,
 * out[1] the level passes, out[2] numbering and emit, out[3] download (ms), out[4] the number of level passes, out[5] scratch bytes
 * per work-item of the spatial-bin kernel, out[6] of the flag kernel, out[7] of the scatter kernel (the three that clip). */
int rt_debug_sbvh_phases(float* out);
/* The BVH2 -> BVH4 collapse on the GPU: BVH4::Convert + Collapse (rt355_host.h rth_build_bvh4) of the BVH2 nodes2[nNodes] whose BLAS
 * roots are roots[nRoots] (the instances' bvhIdx in instance order; a root named before is the same BLAS), on `device`.  out4[nNodes]
 * receives the RtBVHNode4 array byte for byte as BuildBVH4 leaves it: the collapsed records of the surviving nodes, Convert's two-slot
 * records of the absorbed and the unreachable interior nodes, zeros for BVH2 leaves, the one-slot record of a BLAS root that is a
 * leaf.  A surviving node's record is a function of the BVH2 below it alone (csrc/collapse_common.h), so the survivors of one level
 * are collapsed side by side, level by level; the host restatement rth_build_bvh4_levels (rt355_host.h) gives the same arrays.
 * nIdx: the primIdx slots the leaves index.  Synchronous, on a stream of its own; the caller's device is restored.  stats may be NULL.
 * Refusals write nothing to out4:
 *   RT_E_INVALID      a missing array or a count <= 0; a root out of range; any record with count == 0 whose first + 1 is not inside
 *                     the array (every interior record is converted, reachable or not); a leaf range outside nIdx; a node reachable
 *                     twice from the roots; a bad device;
 *   RT_E_UNSUPPORTED  a BLAS whose BVH2 is deeper than RT_BVH4_STACK levels.
 * A result whose stack_need exceeds RT_BVH4_STACK is returned with the figure: it is the upload that refuses it. */
int rt_build_bvh4(int32_t device, const RtBVHNode2* nodes2, int32_t nNodes, int32_t nIdx, const uint32_t* roots, int32_t nRoots,
                  RtBVHNode4* out4, RtBvh4Stats* stats);

/* ---- in-place scene updates (animation) ----------------------------------------------------------------------------------------
 * What Renderer::Tick's disabled animation hook (renderer.cpp:29-37: scene.Animate, tlas->Build, the node buffers' CopyToDevice) needs,
 * without a host rebuild or a re-upload.  The topology stays: primitive count, primIdx, node children and leaf ranges, every
 * primitive's objType and matIdx (the light list and the materials depend on them) and every instance's bvhIdx.
 *   prims: count records replacing [first, first + count) of the uploaded primitives (NULL / 0: geometry unchanged);
 *   blas:  nBlas instances replacing the uploaded ones, of which only invT may differ (NULL: transforms unchanged).
 * Then every BLAS is refit on the device (a leaf's box: the union of its primitives' boxes by BVH2::CreateBVHPrimData's rule, unclipped;
 * an interior node's: the union of its children), the derived records are rewritten on the device and the TLAS is rebuilt on the
 * device by TLAS::Build's rules (at most 256 instances).  The arrays are then bit for bit those of a fresh rt_upload_scene of the
 * scene refit on the host (rth_set_primitives + rth_refit + rth_build_tlas, rt355_host.h).
 * Refusals return before anything is written: RT_E_INVALID for a changed objType / matIdx / bvhIdx, a range outside the upload, a
 * singular invT or a wrong instance count; RT_E_UNSUPPORTED for BVH4 contexts, scenes the update cannot handle (a TLAS not built by
 * TLAS::Build's rules, a node reachable twice), a rebuilt TLAS deeper than RT_TLAS_STACK and a clustering that finds no partner (no two
 * instance boxes with a union area below RT_REALLYFAR; rth_build_tlas refuses it too) (the work is staged: the bound scene then
 * renders exactly as before; a BVH4 context refits through rt_rebuild_scene with RT_REBUILD_REFIT, below, which takes every context).
 * The update waits for the streams of every context holding the scene (rt_share_scene partners, all
 * lanes and worker streams of a group), not for other device work; each of them re-derives its traversal kernels (rt_kernel_info)
 * before its next launch when the TLAS depth changed.  Synchronous; stats may be NULL.  Accumulators are not reset. */
typedef struct RtUpdateStats {
    double  gpu_ms;               /* GPU time of the update (staging + commit)                                                 */
    int32_t prims, nodes;         /* primitives replaced; BVH2 nodes refit (those reachable from the BLAS roots)               */
    int32_t tlas_nodes, tlas_depth;
    int32_t reconfigured;         /* 1: the TLAS depth changed, so the holders re-derive their traversal configuration          */
    int32_t reserved[3];
} RtUpdateStats;
int rt_update_scene(RtCtx* ctx, const RtPrimitive* prims, int32_t first, int32_t count, const RtBVHInstance* blas, int32_t nBlas,
                    RtUpdateStats* stats);
/* ---- in-place rebuilds (a bound scene changes its topology without leaving the device) -------------------------------------------
 * rt_update_scene keeps the trees and only refits their boxes; once the motion outgrows the build-time topology (vertices scrambled
 * across triangles, a BLAS torn apart, SBVH leaves that lose their clipped boxes) the trees are valid but slow.  rt_rebuild_scene
 * takes the same replacement records (prims / first / count and blas / nBlas as for rt_update_scene: objType, matIdx and bvhIdx
 * must stay, only invT of an instance may differ; either may be absent) and then builds every distinct BLAS of the scene anew on
 * the device over its own primitive range, in increasing order of the ranges and numbered the way the host appends BLAS after BLAS
 * (nodeBase of BLAS k = the nodes of BLAS 0..k-1, idxBase likewise), with
 *   RT_REBUILD_SAH   rt_build_bvh2_sah's tree (BVH2::BuildBLAS, alpha 1; opts ignored), or
 *   RT_REBUILD_LBVH  rt_build_bvh2's tree (opts as there, NULL = defaults), or
 *   RT_REBUILD_SBVH  rt_build_bvh2_sbvh's tree (BVH2::BuildBLAS with bvh2->alpha = opts->alpha, spatial splits; opts NULL or
 *                    zero-filled: alpha 0, the full SBVH; the other words of opts are ignored, as alpha is by the other builders):
 *                    the way back to an SBVH for a scene bound as one, whose refits lose the clipped leaf boxes;
 *   RT_REBUILD_REFIT no new tree at all: the bound BVH2 is copied into the set that is not live and refit there as rt_update_scene
 *                    refits it (opts ignored); bvhIdx, node count, primIdx, leaf ranges and pair ids stay, only boxes change.  This
 *                    is the refit of a BVH4 copy that keeps its BVH2 (rt_update_scene refuses every BVH4 context), and one call
 *                    that works on every context: on a BVH2 context the arrays afterwards equal, bit for bit, what
 *                    rt_update_scene leaves for the same arguments; on a BVH4 copy they equal a fresh rt_upload_scene_bvh2 of the
 *                    scene refit on the host (rth_set_primitives + rth_refit + rth_build_tlas), which equals rt_upload_scene of
 *                    that scene collapsed by rth_build_bvh4.  The greedy collapse goes by box areas, so moved boxes can change
 *                    which children a node absorbs.  One flat kernel therefore recomputes the record of every live node from the
 *                    refit BVH2 and counts those whose slots (first, count) differ from the bound record.  None: the bound live
 *                    ids, quad topology and stack need still hold, the records are final and only quad records are rewritten
 *                    (in place).  Otherwise the rebuild's level-by-level collapse runs (the fallback); RT355_REFIT_RECOLLAPSE=1
 *                    in the environment, read per call, forces it (tests, A/B runs).  Both ways end in the same bytes;
 *                    rt_refit_info tells which one ran.  A refit cannot change the derived layout (leaf sizes do not move), and
 *                    the stack need can only change through the fallback, which then sets `reconfigured`.  The stats of a
 *                    refit: blas_built 0, build_ms the GPU time of the staging copies and the refit, nodes / n_idx / max_depth
 *                    those of the bound trees, spatial_splits and prims_clipped 0;
 * every instance's bvhIdx becomes its BLAS's new root, the TLAS is rebuilt by TLAS::Build's rules and every derived array is
 * produced on the device.  No node, index or record array crosses the bus; the host reads the few words per build step the builders
 * read anyway, plus counts, depths and status.  Afterwards the arrays rt_debug_get_scene_array returns, their sizes included, are
 * bit for bit those of a fresh rt_upload_scene of the scene built from scratch on the host from the new primitives with the same
 * builder (rth_rebuild + rth_build_tlas, rt355_host.h), and rt_kernel_info of every holder equals the fresh context's.  The call
 * waits for the streams of every context holding the scene (as rt_update_scene does); each holder takes the new arrays, stack size
 * and traversal kernels before its next launch.  rt_update_scene works on the rebuilt scene (instance records handed to later calls
 * carry the new bvhIdx: RT_SCENE_INSTANCES, or the host restatement's).  Synchronous; accumulators are not
 * reset.  The first two rebuilds of a scene copy allocate two sets of the arrays, which later rebuilds alternate between; the copy
 * uploaded originally stays allocated beside them until the scene copy is freed.  What scales with the trees (nodes, primIdx, pair
 * and triangle records, the refit topology, the derivation's scratch) starts with room for nPrims index slots and 2 * nPrims nodes,
 * which bounds every tree of the first two builders.  A spatial split duplicates refs, so an SBVH tree has no such bound: every BLAS
 * is built in the builder's own memory first (one tree at a time), and when the running totals outgrow the set that is not live its
 * arrays go to the need plus a quarter, device to device, what was emitted so far is kept and the arrays replaced are freed at once;
 * the live set is never touched.  The builder's own memory is kept from rebuild to rebuild, so a scene whose tree sizes are stable is
 * rebuilt without any device allocation once both sets have grown (rt_debug_rebuild_allocations counts them).  rt_update_scene's
 * staging nodes grow the same way.  The environment variable RT355_REBUILD_INITIAL_CAP=k, read per call, makes what is allocated
 * afterwards start at k index slots and 2 * k nodes (for tests and A/B runs: a small k runs every growth path).
 * Refusals change nothing (the work is staged in the set that is not live; the bound scene renders exactly as before):
 *   RT_E_INVALID      what rt_update_scene answers with it, an unknown builder, bad opts (the builder's own argument checks; for
 *                     RT_REBUILD_SBVH an alpha outside [0, 1], NaN included), all before any device work;
 *   RT_E_NOMEM        device memory, for the sets, a grown set or the SBVH builder's ref arrays (a later call takes the allocation
 *                     up where it stopped);
 *   RT_E_UNSUPPORTED  a BVH4 context; a scene whose BLAS do not each cover one contiguous primitive range, ranges disjoint and in the
 *                     order of their roots (found at rt_upload_scene; rt_blas_ranges tells beforehand), more than 256 instances or
 *                     a TLAS not of TLAS::Build's shape; whatever the builder refuses on these primitives (rt_build_bvh2_sah,
 *                     rt_build_bvh2_sbvh: a non-finite box, an undefined spatial bin index, ...);
 *                     a new BLAS that needs more than RT_BVH4_STACK stack entries (the SAH builder makes a tree 65 levels deep
 *                     out of thin triangles on a geometric ladder over 190 octaves; rth_rebuild refuses it by the same rule); a rebuilt TLAS deeper than RT_TLAS_STACK; and
 *                     new trees that would change the scene's derived layout (RtKernelInfo.layout: a leaf of more than 127
 *                     primitives - the SAH builder makes one out of 128 coincident triangles - takes layout 0 at upload, and so
 *                     do 2^24 index slots or more, which an SBVH rebuild can reach with fewer primitives).
 *                     Not following a layout change is a deliberate limit: upload the rebuilt scene in that case. */
#define RT_REBUILD_SAH   0
#define RT_REBUILD_LBVH  1
#define RT_REBUILD_SBVH  2
#define RT_REBUILD_REFIT 3
typedef struct RtRebuildStats {
    double  gpu_ms;               /* from the first to the last GPU operation of the rebuild on its stream                     */
    double  wall_ms;              /* the whole call                                                                            */
    double  stage_ms, build_ms, derive_ms, tlas_ms, commit_ms;   /* split: host time until the staging copies are queued (checks and
                                   * first-use allocation included; the copies run during build_ms), the BLAS builds (wall, their
                                   * per-level host round trips included, as in gpu_ms), the derived arrays and the TLAS (GPU
                                   * events), waiting for the holders and swapping the arrays (wall)                            */
    int32_t prims, blas_built;    /* primitives replaced; BLAS built                                                           */
    int32_t nodes, n_idx;         /* BVH2 nodes and primIdx entries of the rebuilt scene                                       */
    int32_t max_depth;            /* height of the deepest new BLAS (edges)                                                    */
    int32_t tlas_nodes, tlas_depth;
    int32_t reconfigured;         /* 1: the stack size or the TLAS depth changed (the holders always take the new arrays)      */
    int32_t spatial_splits, prims_clipped;   /* RT_REBUILD_SBVH: BVH2::stat_* summed over the BLAS built (0 for the other builders) */
} RtRebuildStats;
int rt_rebuild_scene(RtCtx* ctx, const RtPrimitive* prims, int32_t first, int32_t count, const RtBVHInstance* blas, int32_t nBlas,
                     int32_t builder, const RtBuildOptions* opts, RtRebuildStats* stats);
/* ---- per-range plans: rebuild only the BLAS that changed -----------------------------------------------------------------------------
 * rt_rebuild_scene builds every distinct BLAS anew.  One deforming mesh beside a large static one pays for the static tree again on every
 * call, and one call cannot mix builders.  rt_rebuild_ranges takes a plan: plan[k], one word per distinct BLAS in increasing order of the
 * primitive ranges (the order of rt_scene_blas_blocks and rt_blas_ranges' ranges), is RT_REBUILD_SAH, RT_REBUILD_LBVH or RT_REBUILD_SBVH -
 * that BLAS is built by that builder, as rt_rebuild_scene builds it (one opts for all: the LBVH words go to the LBVH ranges, alpha to the
 * SBVH ranges) -, RT_REBUILD_KEEP: its bound tree stays, or RT_REBUILD_REFIT_RANGE: its bound tree stays and takes new boxes.  prims / first / count / blas / nBlas mean what they mean for
 * rt_rebuild_scene.  Afterwards the scene is numbered the way the host appends BLAS after BLAS: the root of range k is the sum of the
 * node counts of ranges 0..k-1, its first index slot the sum of their slot counts.  A built range holds its builder's tree at that base.
 * A kept range holds its bound tree relocated, by one rule for the device (k_blas_relocate) and the host mirror (rth_rebuild_ranges;
 * csrc/rebuild_common.h, relocated_first): node i of the bound block moves to i - oldRoot + newRoot; an interior record (count == 0) gets
 * first += newRoot - oldRoot, a leaf record first += newIdxBase - oldIdxBase; boxes, counts and pad words are untouched, and its primIdx
 * slots move unchanged (primitive ids are global and the range did not move).  The builders are functions of their primitive range into
 * which the bases enter only as these offsets, so that is byte for byte what the builder that made the tree would write there.  Kept BLAS
 * that are neighbours in both numberings move as one segment, one kernel launch per segment (the node array is read from the live set and
 * written to the set that is not live: they never alias); a segment that does not move at all - the static mesh in front of the moving
 * one - is a plain device-to-device copy, as the primIdx slots always are.  Then rt_rebuild_scene's pipeline runs unchanged over all
 * ranges: bvhIdx from the new roots, pair ids, the collapse of a BVH4 copy that keeps its BVH2, the derived records, TLAS::Build, the
 * layout check and the commit by pointer swap.
 * RT_REBUILD_REFIT_RANGE refits one BLAS: its bound tree stays - node ids relative to its root, leaf ranges, primIdx - and is moved
 * exactly as a kept one is; then its boxes are made anew from the primitives as they are after the replacement window, by
 * rt_update_scene's rules: a leaf is the unclipped union of its primitives, an interior node the union of its children.  A refit SBVH
 * tree therefore loses its clipped boxes, for that BLAS only: its neighbours keep theirs, which a refit of the whole scene does not
 * offer.  The window may intersect refit and built ranges, never a kept one.
 * The derived data of a kept or refit BLAS move as blocks too (BVH2 copies, both layouts): nothing walks such a tree.  Per BLAS the
 * pair records move by one thread per 16-byte vector, the three box vectors copied and the two entries of the fourth patched by
 * rebuild::relocated_entry (a leaf entry moves by the index offset, an interior one by the offset of the BLAS's run of pair ids); the
 * run of pair id -> node id, the parent links and the run of leaves move by the node offset; a kept BLAS's triangle records are a
 * device-to-device copy of its slot run, its instances' root entries host arithmetic; the shade records are copied and recomputed
 * over the window only.  A refit BLAS then runs rt_update_scene's refit kernel over its own leaves, with the tickets of its own block
 * zeroed, and rewrites its pair records' boxes and its triangle records.  Pair ids, the leaf list and the records of the built ranges
 * alone are derived by rt_rebuild_scene's kernels.  A plan without a kept or refit range queues exactly what rt_rebuild_scene queues.
 * (A BVH2 copy bound in layout 0 although its extend_variant admits layout 1 derives over all ranges, as a BVH4 copy does: the layout
 * check needs every leaf's size.)  A BVH4 copy that keeps its BVH2 takes every word: its BVH2 blocks are relocated and refit as
 * above, but its refit topology, the collapse, the quad records and the root entries are derived over all ranges; relocating
 * collapsed records is out of scope.  rt_ranges_info reports what the last successful rt_rebuild_ranges of the scene copy queued.
 * Afterwards every array rt_debug_get_scene_array returns, sizes included, and rt_kernel_info equal those
 * of a fresh upload of the host mirror's scene (rth_rebuild_ranges + rth_build_tlas).  stats as for a rebuild: blas_built counts the
 * ranges a builder built (neither kept nor refit ones), build_ms includes the relocation.
 * Which bound trees can be kept: a BLAS is compact when the nodes reachable from its root are exactly the ids [root, root + m), m odd,
 * and its leaves' primIdx ranges tile one interval without gap or overlap.  Everything BuildBLAS, the GPU builders, rt_rebuild_scene,
 * rt_rebuild_ranges and rt_resize_scene produce is compact; arbitrary arrays handed to rt_upload_scene may not be (found at upload).  A
 * range that is not compact can be built, not kept.  rt_scene_blas_blocks reports, per distinct BLAS in plan order, its primitive range,
 * the nodes and index slots of its bound tree (an SBVH tree has more slots than primitives) and whether it is compact: *n receives the
 * number of distinct BLAS, at most cap entries of each array (any may be NULL) are written.
 * Room: the set that is not live is given the kept trees' sizes plus count slots and 2 * count - 1 nodes for every range the SAH or the
 * linear builder builds, before anything runs; SBVH ranges keep their size-then-place path (and leave room for what lies behind them).
 * The builders' workspace is sized over the built ranges only.
 * Refusals change nothing (rt_rebuild_scene's guarantee):
 *   RT_E_INVALID      before any device work: a null plan; nRanges different from the scene's number of distinct BLAS; a plan word that
 *                     is none of the five; RT_REBUILD_REFIT in a plan (the per-range word is RT_REBUILD_REFIT_RANGE; the whole scene is
 *                     refit with rt_rebuild_scene); a replacement window [first, first + count), count > 0, that intersects a kept range (its boxes
 *                     would go stale); everything rt_rebuild_scene answers with RT_E_INVALID; bad opts for a builder the plan uses;
 *   RT_E_UNSUPPORTED  RT_REBUILD_KEEP or RT_REBUILD_REFIT_RANGE for a range that is not compact (the message names the range); everything rt_rebuild_scene
 *                     refuses (a BVH4 copy without its BVH2, a layout change, ...);
 *   RT_E_NOMEM        as for rebuilds.
 * rt_rebuild_ranges_check runs the plan checks without a device against caller-given ranges: nBound ranges (rangeFirst / rangeCount, in
 * increasing order; compact NULL: all compact), the plan, the window, opts.  RT_OK, or the code and message rt_rebuild_ranges would give. */
#define RT_REBUILD_KEEP  4   /* per-range plans only: the bound tree of this BLAS stays, moved to where the new scene numbers it */
#define RT_REBUILD_REFIT_RANGE 5   /* per-range plans only: ... and its boxes are made anew from the primitives (rt_update_scene's rules) */
int rt_rebuild_ranges(RtCtx* ctx, const RtPrimitive* prims, int32_t first, int32_t count, const RtBVHInstance* blas, int32_t nBlas,
                      const int32_t* plan, int32_t nRanges,   /* HOST: one of RT_REBUILD_SAH / LBVH / SBVH / KEEP / REFIT_RANGE per distinct BLAS */
                      const RtBuildOptions* opts, RtRebuildStats* stats);
int rt_scene_blas_blocks(RtCtx* ctx, int32_t* n, int32_t* primFirst, int32_t* primCount, int32_t* nodes, int32_t* idxSlots, int32_t* compact, int32_t cap);
int rt_rebuild_ranges_check(int32_t nPrims, const int32_t* rangeFirst, const int32_t* rangeCount, const int32_t* compact, int32_t nBound,
                            const int32_t* plan, int32_t nRanges, int32_t first, int32_t count, const RtBuildOptions* opts);
/* ---- in-place resizes (a bound scene changes its shape without leaving the device) ----------------------------------------------------
 * rt_update_scene and rt_rebuild_scene keep the scene's shape: the primitive count, every primitive's objType and matIdx, the number of
 * BLAS and of instances, the light list.  rt_resize_scene replaces all of it but the materials and textures, which stay as bound:
 *   prims   the whole new primitive array, RtPrimitive[nPrims], in host memory or in memory the context's GPU reaches (device memory of
 *           that GPU, managed or pinned host memory: rt_trace's pointer rule - hipPointerGetAttributes decides, and an allocation the
 *           runtime knows must not end before the nPrims-th record), so a simulation that writes primitives on the GPU never crosses the
 *           bus.  The copy runs on the scene copy's own stream, which waits for no other: device work that produces prims must be
 *           complete, or ordered before the call by the caller (Device.resize_scene waits for torch's current stream).  objType and matIdx are free: objType one of RT_PRIM_*, matIdx in [0, nMats) of the bound materials;
 *   shape   nRanges BLAS that cover the new array back to back (rangeCount), and nBlas instances (1..256) that name them (instRange;
 *           every range at least once) under blas[i].invT (blas NULL: identity; bvhIdx is ignored and assigned by the call).
 * The new primitives are copied into the array set that is not live (host to device or device to device: one path from there on).
 * k_resize_check, one thread per primitive, range-checks objType and matIdx, writes the light flag (the material's isLight != 0) and the
 * packed (objType, matIdx) pair - 8 bytes per primitive, the only per-primitive data that returns to the host, which keeps it for the
 * checks of later updates; a scan ranks the flags and k_light_emit writes the light list by the Scene rule (the lights' indices in
 * increasing order) and the complete light records.  Then rt_rebuild_scene's own pipeline runs over the new ranges: every BLAS with
 * RT_REBUILD_SAH, RT_REBUILD_LBVH or RT_REBUILD_SBVH (opts as there; RT_REBUILD_REFIT is RT_E_INVALID: there is no tree to refit), the
 * collapse of a BVH4 copy that keeps its BVH2, the derived records and TLAS::Build, all on the device, and the same commit by pointer
 * swap once the holders' streams are idle.  Afterwards every array rt_debug_get_scene_array returns (RT_SCENE_LIGHTS included), sizes
 * too, is bit for bit that of a fresh rt_upload_scene (a BVH4 copy: rt_upload_scene_bvh2) of the scene made of the new primitives,
 * the bound materials and textures, that light list, each BLAS built on the host over its range with the same builder and appended BLAS
 * after BLAS, instance i carrying invT[i] and the root of BLAS instRange[i], and the TLAS of TLAS::Build; rt_kernel_info and
 * rt_shade_tables of every holder equal the fresh context's (a resize from several instances to one, or back, changes the traversal
 * kernels).  rt_update_scene, rt_rebuild_scene with all four builders, rt_trace, rt_share_scene and further resizes work on the result.
 * Accumulators and seeds are not touched.  A holder whose primitive count changed empties its ray, hit and shadow queues on its own
 * stream before its next launch, to what a new context has: every count, dequeue head and ticket zero, every hit record zero (a queued
 * primIdx may lie outside the new array; rt_debug_get_rays then reports no rays until a stage has made some; rt_render never spans the
 * call), and rt_debug_set_rays checks against the new count.  stats as for a rebuild; prims is nPrims.
 * The arrays of a set that scale with the primitives, the instances and the lights grow like those that scale with the trees: to the
 * need plus a quarter, the replaced array freed at once, the live set never touched, every allocation counted by
 * rt_debug_rebuild_allocations; rt_update_scene's staging arrays likewise.  A scene that alternates between two shapes stops allocating
 * by the third visit to each.
 * Refusals change nothing (everything is staged; the bound scene, its arrays and its next frame are what they were):
 *   RT_E_INVALID      before any device work: a null argument or no scene bound; nPrims <= 0; a range count below 1 or counts that do not
 *                     sum to nPrims; an instRange outside [0, nRanges) or a range no instance names; nBlas outside 1..256; a singular
 *                     invT; an unknown builder or RT_REBUILD_REFIT; bad opts; a prims pointer that is neither host memory nor reachable
 *                     from the context's device for nPrims records.  (rt_resize_check runs the checks of the shape without a device.)
 *                     Found on the device: the first primitive, by lowest index, whose objType or matIdx is out of range;
 *   RT_E_UNSUPPORTED  what rt_rebuild_scene refuses (a BVH4 copy without its BVH2, a bound scene that cannot be rebuilt in place,
 *                     whatever the builder refuses, a tree deeper than RT_BVH4_STACK, a TLAS deeper than RT_TLAS_STACK or one that
 *                     finds no partner, new trees that would change the derived layout), and a bound scene whose BLAS ranges do not
 *                     tile [0, nPrims) without gaps;
 *   RT_E_NOMEM        as for rebuilds (a later call takes the allocation up where it stopped).
 * Deliberately not followed: more than 256 instances, a change of the derived layout, copies without a BVH2.  (Materials and textures
 * change through rt_update_materials, below; a resize checks matIdx and flags its lights against the table that is bound then.) */
typedef struct RtSceneShape {
    int32_t nRanges;              /* distinct BLAS, >= 1 */
    const int32_t* rangeCount;    /* HOST, nRanges entries, each >= 1, sum == nPrims: BLAS k covers primitives
                                     [rangeCount[0] + .. + rangeCount[k-1], + rangeCount[k]) of the new array */
    int32_t nBlas;                /* instances, 1..256 */
    const int32_t* instRange;     /* HOST, nBlas entries in [0, nRanges): the BLAS instance i renders; every range named at least once */
    const RtBVHInstance* blas;    /* HOST, nBlas records of which only invT is read (NULL: identity); bvhIdx is assigned by the call */
} RtSceneShape;
int rt_resize_scene(RtCtx* ctx, const void* prims, int32_t nPrims, const RtSceneShape* shape, int32_t builder, const RtBuildOptions* opts,
                    RtRebuildStats* stats);
/* The checks of rt_resize_scene that need neither a device nor a bound scene: nPrims, the shape, the builder and opts.  RT_OK, or
 * RT_E_INVALID with the message rt_resize_scene would give. */
int rt_resize_check(int32_t nPrims, const RtSceneShape* shape, int32_t builder, const RtBuildOptions* opts);
/* ---- replacement geometry from the GPU (rt_update_geometry, rt_rebuild_geometry, rt_rebuild_geometry_ranges) ---------------------------
 * rt_update_scene, rt_rebuild_scene and rt_rebuild_ranges take RtPrimitive[count] in host memory.  Skinning, cloth or a simulation
 * produce vertex positions on the device; RtGeometry describes the replacement of the window [first, first + count) in either form, and
 * wherever it lies:
 *   records form  (prims)      what the old calls take, in host memory or in memory the context's GPU reaches.  objType and matIdx must
 *                              stay; the rule is checked where the records lie: host records by the old calls' loop, device-reachable
 *                              records by k_window_check (one thread per record against the bound one, the lowest offending index
 *                              found through atomicMin), with the old calls' message from the values read back for that one record.
 *   vertex form   (positions)  every primitive of the window must be a triangle (checked on the host, before any device work).  Triangle
 *                              i of the window takes vertices indices[3i .. 3i+2], or 3i .. 3i+2 without indices.  k_tri_from_vertices,
 *                              one thread per triangle, writes v0, v1, v2, N, centroid and area by Scene::AddTriangle's rule
 *                              (csrc/geometry_common.h, which the host mirror rth_set_vertices compiles too); uv*, objType, matIdx and
 *                              the pad words stay as bound.  AddTriangle's flip is not stored in a record: the new N is negated iff
 *                              dot(bound N, cross(bound v1 - bound v0, bound v2 - bound v0)) < 0, which is false for zero and NaN (a
 *                              bound triangle without a normal counts as not flipped).  An index >= nVertices is never followed: the
 *                              triangle of lowest index that has one is reported, and nothing is bound.
 *                              A triangle whose cross product is zero or not finite gets NaN in N and may get NaN in area; x86 and the
 *                              GPU make NaNs of different sign, so for such a triangle the promise is "NaN where the host has NaN", not
 *                              equal bits.  Every other word is bit for bit the host mirror's.
 * With count > 0 exactly one of prims / positions is given.  Where memory may lie is rt_resize_scene's rule (host memory, or device,
 * managed or pinned memory the context's GPU reaches); alignment (4 bytes) and the end of an allocation the runtime knows are rt_trace's
 * rule.  The copies and kernels run on the scene copy's own stream, which waits for no other: device work that produces the data must be
 * complete, or ordered before the call by the caller (Device.update_geometry waits for torch's current stream).
 * The contract in one sentence: each call leaves the scene copy as its counterpart - rt_update_scene, rt_rebuild_scene,
 * rt_rebuild_ranges - leaves it for host records over the same window: the given ones in records form, the bound ones rewritten by
 * geometry_common.h's rule in vertex form.  That covers every array of rt_debug_get_scene_array with its size, rt_kernel_info, the
 * stats and rt_ranges_info; so everything the counterparts promise carries over: equality with a fresh upload of the host mirror's
 * scene, refusals that change nothing, the window rule of a range plan, the wait for the holders, the allocation counting of
 * rt_debug_rebuild_allocations (index and status scratch grows as the staging arrays do: a repeated call stops allocating).  BVH4
 * contexts answer as their counterparts do.  The old entry points are these with a host-records RtGeometry.
 * Refusals beyond the counterparts', all RT_E_INVALID and before anything is bound: a null geometry, a negative first or count, a window
 * outside the bound primitives, both sources or neither with count > 0, a positionStride below 12 or no multiple of 4, nVertices < 0,
 * nVertices < 3 * count without indices, a non-triangle in the window (vertex form), a pointer that breaks the rules above, and - found
 * on the device - a record that changes objType / matIdx or an index >= nVertices. */
typedef struct RtGeometry {
    int32_t     first, count;     /* the window [first, first + count) of the bound primitives; count 0: geometry unchanged        */
    const void* prims;            /* RtPrimitive[count], host memory or memory the context's GPU reaches; or NULL                  */
    const void* positions;        /* vertex j's x, y, z (float32) at positions + j * positionStride, host or device-reachable; or NULL */
    int64_t     positionStride;   /* bytes, >= 12 and a multiple of 4                                                              */
    int64_t     nVertices;        /* vertices behind `positions`                                                                    */
    const void* indices;          /* uint32[3 * count], host or device-reachable; NULL: triangle i takes vertices 3i, 3i+1, 3i+2   */
} RtGeometry;
int rt_update_geometry(RtCtx* ctx, const RtGeometry* geometry, const RtBVHInstance* blas, int32_t nBlas, RtUpdateStats* stats);
int rt_rebuild_geometry(RtCtx* ctx, const RtGeometry* geometry, const RtBVHInstance* blas, int32_t nBlas, int32_t builder, const RtBuildOptions* opts,
                        RtRebuildStats* stats);
int rt_rebuild_geometry_ranges(RtCtx* ctx, const RtGeometry* geometry, const RtBVHInstance* blas, int32_t nBlas, const int32_t* plan, int32_t nRanges,
                               const RtBuildOptions* opts, RtRebuildStats* stats);
/* The checks of an RtGeometry that need no device: nPrims primitives are bound, objType[nPrims] their types (NULL: all triangles).
 * RT_OK, or the code and message the device calls give. */
int rt_geometry_check(const RtGeometry* geometry, int32_t nPrims, const int32_t* objType);
/* ---- in-place material updates (a bound scene changes its materials, its texture atlas and its primitives' matIdx on the device) ------
 * A lamp switched on, a recoloured object, a video texture played from a device buffer, a repainted part of a mesh: no tree changes and
 * a few hundred bytes do.  The three parts of an update are independent; a part whose pointer is NULL stays as bound, and a call with
 * all three absent succeeds and touches nothing.
 *   mats     the whole new table (HOST), checked as rt_upload_scene checks it against the atlas length that will be bound;
 *   texels   RtFloat4[texCount] in host memory or memory the context's GPU reaches (rt_resize_scene's pointer rule; the copy runs on the
 *            scene copy's own stream, so device work that produces them must be complete): they replace [texFirst, texFirst + texCount)
 *            of the NEW atlas, whose length is nTexels (-1: as bound).  Texels [0, min(old, new)) are kept, [old, new) are zero;
 *   primMat  int32[primCount], host or device-reachable: the new matIdx of primitives [primFirst, primFirst + primCount).
 * The light list depends on the materials (the indices of the primitives whose material has isLight != 0, in increasing order) and a
 * light record carries its material's emittance, so with mats or primMat given the call re-derives both on the device by the pipeline of
 * rt_resize_scene: k_mat_flags (one thread per primitive: matIdx from the new assignment inside the range, from the bound primitive
 * outside; a value outside [0, nMats) of the new table is refused through atomicMin of the lowest index; the light flag), an exclusive
 * scan, k_mat_emit (the list and the complete 8-row records, from the same matIdx source).  All of that is staged in memory no holder
 * reads.  Only then the holders' streams are waited for and the commit writes what is patched in place - k_mat_assign writes
 * prims[i].matIdx and the shade record, the texel range goes into the atlas, the pad behind it is zeroed - and swaps the table, the
 * light list, the light records, the atlas (when it had to grow) and the counts.  With only texels given the light list and the light
 * records stay exactly as bound (a caller's odd but legal list too).  Afterwards every array rt_debug_get_scene_array returns
 * (RT_SCENE_MATERIALS and RT_SCENE_TEXTURES included), sizes too, is bit for bit that of a fresh rt_upload_scene (a BVH4 copy that keeps
 * its BVH2: rt_upload_scene_bvh2) of the bound primitives with the new matIdx values, the new table and atlas, that light list and the
 * bound trees, TLAS and instances; rt_kernel_info and rt_shade_tables of every holder equal the fresh context's (the staged tables of
 * k_shade follow the new counts).  Synchronous; accumulators, seeds, counters and queues are not touched.  Works on every bound scene,
 * whatever rt_update_scene or rt_rebuild_scene answer for it; those, rt_resize_scene, rt_trace, rt_share_scene and further material
 * updates work on the result and check against the new table.
 * Memory: the table, the light list and the light records exist twice (the set that is not live is written, the commit swaps); an atlas
 * that outgrows its array moves to one of the need plus a quarter, the replaced one freed at once; every allocation is counted by
 * rt_debug_rebuild_allocations, and a scene that alternates between two material states stops allocating by the third visit to each.
 * Refusals change nothing:
 *   RT_E_INVALID   a null context or update, no scene bound; mats with nMats <= 0; a texture window outside the new atlas (with mats
 *                  NULL the bound table is checked against a shrinking atlas); nTexels < -1; a negative first or count; a range
 *                  outside the new atlas or the primitives; a count above zero with a null pointer (an absent part has count 0); a
 *                  pointer that is neither host memory nor reachable from the context's device for that many elements.  Found on
 *                  the device: the primitive of lowest index whose matIdx lies outside the new table (the message gives the index,
 *                  the value and nMats);
 *   RT_E_NOMEM     device memory (a later call takes the allocation up where it stopped).
 * stats (may be NULL): gpu_ms the staging and the commit on the device, wall_ms the call; mats, texels, prims: records written; lights:
 * the light count afterwards; tables_staged_changed: k_shade of this context serves its tables from LDS now and did not before, or the
 * reverse; atlas_reallocated: the atlas moved to a new array. */
typedef struct RtMaterialUpdate {
    const RtMaterial* mats; int32_t nMats;   /* HOST. The whole new table; NULL: the table stays (nMats ignored)            */
    const void* texels;                      /* RtFloat4[texCount], host or device-reachable; NULL: no texel is written     */
    int32_t texFirst, texCount;              /* the texels replace [texFirst, texFirst + texCount) of the NEW atlas           */
    int32_t nTexels;                         /* length of the atlas afterwards; -1: as bound                                  */
    const void* primMat;                     /* int32[primCount], host or device-reachable; NULL: the assignment stays        */
    int32_t primFirst, primCount;
} RtMaterialUpdate;
typedef struct RtMaterialStats { double gpu_ms, wall_ms; int32_t mats, texels, prims, lights, tables_staged_changed, atlas_reallocated, reserved[2]; } RtMaterialStats;
int rt_update_materials(RtCtx* ctx, const RtMaterialUpdate* update, RtMaterialStats* stats);
/* The checks of a material table that need no device: validate_scene's material loop against an atlas of nTexels texels.  RT_OK, or
 * RT_E_INVALID with the message rt_update_materials would give. */
int rt_materials_check(const RtMaterial* mats, int32_t nMats, int32_t nTexels);
/* The last successful RT_REBUILD_REFIT of the context's scene copy.  path: 0 no such call yet; 1 the records were rewritten in place
 * (a BVH2 context always reports 1, with live_quads 0); 2 re-collapsed because changed_nodes live records changed a slot; 3
 * re-collapsed because RT355_REFIT_RECOLLAPSE=1 forced it.  live_quads: the live BVH4 nodes afterwards; stack_need: the traversal's
 * stack entries as the collapse counts them (a BVH2 context: the height of the deepest BLAS).  RT_E_INVALID for a null argument or
 * when no scene is bound. */
typedef struct RtRefitInfo { int32_t path, live_quads, changed_nodes, stack_need; } RtRefitInfo;
int rt_refit_info(RtCtx* ctx, RtRefitInfo* out);
/* The last successful rt_rebuild_ranges of the context's scene copy, counted from the arguments of the launches and copies it queued
 * (all zero before any such call): ranges built / kept / refit; pair records derived (k_rb_pairs) and relocated; triangle-record slots
 * derived (k_tri_recs) and relocated (copied); the nodes of the trees the breadth-first numbering walked; the leaves the refit kernel
 * started from.  RT_E_INVALID for a null argument or when no scene is bound. */
typedef struct RtRangesInfo {
    int32_t built, kept, refit, pairs_derived, pairs_relocated, slots_derived, slots_relocated, nodes_numbered, leaves_refit, reserved[3];
} RtRangesInfo;
int rt_ranges_info(RtCtx* ctx, RtRangesInfo* out);
/* Two device-free entries that pin the relocation rule of the derived pair records (no GPU, no context).  rt_debug_derive_pairs: the
 * upload's own host derivation of layout 1 from wire arrays - pairs receives 4 RtFloat4 per interior node reachable (pairCap records of
 * room), pairNode its node id, rootEntry every instance's entry (any may be NULL), *nPairs the count.  rt_debug_relocate_pairs:
 * rebuild::relocated_entry applied to both entries of n records, everything else copied (in and out may be the same array). */
int rt_debug_derive_pairs(const RtBVHNode2* nodes, int32_t nNodes, const RtBVHInstance* blas, int32_t nBlas, RtFloat4* pairs, uint32_t* pairNode,
                          int32_t pairCap, uint32_t* rootEntry, int32_t* nPairs);
int rt_debug_relocate_pairs(const RtFloat4* in, int32_t n, uint32_t pairDelta, uint32_t idxDelta, RtFloat4* out);
/* Device allocations (hipMalloc calls) that rt_update_scene, rt_rebuild_scene, rt_resize_scene and rt_update_materials have made for the
 * context's scene copy so far, the SBVH builder's included: a test can see that a repeated rebuild has stopped allocating. */
int rt_debug_rebuild_allocations(RtCtx* ctx, int64_t* count);
/* The primitive range [first, first + count) of every instance's BLAS in wire arrays, as rt_upload_scene finds them for
 * rt_rebuild_scene (csrc/rebuild_common.h); firstOut / countOut hold nBlas entries (either may be NULL).  RT_E_UNSUPPORTED with the
 * reason in rt_last_error() when the scene is not of the shape rt_rebuild_scene takes.  No device needed. */
int rt_blas_ranges(const RtBVHNode2* nodes, int32_t nNodes, const uint32_t* primIdx, int32_t nIdx, int32_t nPrims,
                   const RtBVHInstance* blas, int32_t nBlas, int32_t* firstOut, int32_t* countOut);
/* rt_scene_blas_blocks for wire arrays, as rt_upload_scene would find the blocks (csrc/rebuild_common.h): per distinct BLAS, in the order
 * a plan of rt_rebuild_ranges names them, the primitive range, the nodes and index slots its tree reaches and whether it is compact (can
 * be kept).  *n receives the number of distinct BLAS; at most cap entries of each array (any may be NULL) are written.  Refused like
 * rt_blas_ranges.  No device needed. */
int rt_blas_blocks(const RtBVHNode2* nodes, int32_t nNodes, const uint32_t* primIdx, int32_t nIdx, int32_t nPrims, const RtBVHInstance* blas, int32_t nBlas,
                   int32_t* n, int32_t* primFirst, int32_t* primCount, int32_t* nodesOut, int32_t* idxSlots, int32_t* compact, int32_t cap);
/* Device arrays of the context's scene copy, for tests: `which` is one of RT_SCENE_*.  *bytes receives the array's size; out NULL:
 * only that.  Waits for the context's stream. */
#define RT_SCENE_PRIMS         0   /* the wire primitives                                  */
#define RT_SCENE_BVH           1   /* the wire BVH2 (or BVH4) nodes                        */
#define RT_SCENE_TLAS          2   /* the wire TLAS nodes                                  */
#define RT_SCENE_INSTANCES     3   /* the wire instances (RtBVHInstance)                   */
#define RT_SCENE_PAIRS         4   /* layout-1 pair records (empty in layout 0 and BVH4)   */
#define RT_SCENE_TRI_RECS      5   /* layout-1 triangle records                            */
#define RT_SCENE_SHADE_RECS    6
#define RT_SCENE_LIGHT_RECS    7
#define RT_SCENE_TLAS_PAIRS    8
#define RT_SCENE_TLAS_PAIRS_P  9
#define RT_SCENE_INST_RECS    10
#define RT_SCENE_QUADS        11   /* layout-1 quad records of a BVH4 (empty otherwise)     */
#define RT_SCENE_ROOT_ENTRY   12   /* layout-1 root entry per instance                      */
#define RT_SCENE_BVH2_KEPT    13   /* the BVH2 a BVH4 copy keeps (rt_upload_scene_bvh2); 0 bytes when the copy holds none */
#define RT_SCENE_LIGHTS       14   /* the light list: uint32 indices of the light primitives, increasing   */
#define RT_SCENE_MATERIALS    15   /* RtMaterial[nMats]                                                    */
#define RT_SCENE_TEXTURES     16   /* RtFloat4[nTexels + texPad], the pad included (zero)                  */
int rt_debug_get_scene_array(RtCtx* ctx, int32_t which, void* out, int64_t capacityBytes, int64_t* bytes);

/* ---- lanes: one accumulation as several interleaved sample streams behind one handle -------------------------------------------
 * What stands behind Renderer::Tick() (renderer.cpp:26-63) when a GPU is to be kept full: `lanes` contexts (own HIP stream, queues,
 * accumulator, seed slice) that share ONE device copy of the scene; their frames are queued interleaved so that the tails of one
 * lane's launches are filled by the others' kernels (1 lane: 733, 4 lanes: 1,000 M samples/s on the bench scene).  Lane m renders
 * sample stream firstStream + m (seeds = that slice of the reference's host xorshift32 stream, renderer.cpp:195-196); the group's
 * accumulator is the sum of the lanes' accumulators in lane order and, after k frames in all, holds k samples per pixel - prep()
 * divides by k exactly as with one stream (postproc.cl:71).  A group of ONE lane is the reference's single Renderer bit for bit.
 * HIP runs kernels of streams that share a hardware queue one after the other, and keeps one pool of up to GPU_MAX_HW_QUEUES queues
 * (the process's own setting, default 4) per stream PRIORITY; the process's other streams - the null stream, a framework's - sit in the
 * normal pool.  rt_group_create measures which of the lanes' streams really run side by side (S of them: rt_group_concurrency), in the
 * normal class first and, when some lanes share a queue there, with the lanes' streams replaced by streams of the lowest and of the
 * highest priority; it keeps the class with the most (normal at a tie, then the lowest: rt_group_stream_class) and writes one line to
 * stderr when S is still fewer than `lanes`.  All lanes of a group have equal priority among themselves; a single context (rt_create)
 * always has a normal stream.  RT355_GROUP_PRIORITY=normal|low|high forces a class, =mixed lets the lanes left over by the best class
 * take streams of the others (rt_group_stream_class: 2), =auto or unset is the above.  Frame j of the group is lane (j mod lanes)'s sample, issued on worker stream j mod S:
 * with S < lanes a lane's frames move between those S streams, strictly in order (each waits on an event recorded behind the lane's
 * last work), so that no queue renders more frames than another.  rt_stream of a lane is the stream its last frame ran on; work the
 * caller queues there lands behind it.  The environment variable RT355_GROUP_STREAMS=k caps S at k (tests, A/B runs). */
typedef struct RtGroup RtGroup;
int rt_group_create(const RtConfig* cfg, int32_t lanes, RtGroup** out);      /* lanes 1..8; cfg as for rt_create (row band included)   */
int rt_group_destroy(RtGroup* g);
int rt_group_lanes(RtGroup* g);
int rt_group_concurrency(RtGroup* g);                                        /* S: streams measured to run concurrently at creation     */
int rt_group_stream_class(RtGroup* g);                                       /* priority class of the lanes' streams: -1 low, 0 normal,
                                                                              * 1 high, 2 mixed                                         */
int rt_group_class_concurrency(RtGroup* g, int32_t cls);                     /* S as measured in class -1, 0 or 1 at creation; -1 when
                                                                              * that class was not tried                                */
RtCtx* rt_group_lane(RtGroup* g, int32_t m);                                 /* lane m's context (counters, stage times, debug stages)  */
uint64_t rt_group_frames(RtGroup* g);                                        /* frames rendered by all lanes since the last reset       */
int rt_group_upload_scene(RtGroup* g,
                          const RtPrimitive* prims, int32_t nPrims, const RtMaterial* mats, int32_t nMats,
                          const RtFloat4* textures, int32_t nTexels, const uint32_t* lights, int32_t nLights,
                          const void* bvhNodes, int32_t nNodes, const uint32_t* primIdx, int32_t nIdx,
                          const RtTLASNode* tlas, int32_t nTlas, const RtBVHInstance* blas, int32_t nBlas);
int rt_group_upload_scene_bvh2(RtGroup* g,
                               const RtPrimitive* prims, int32_t nPrims, const RtMaterial* mats, int32_t nMats,
                               const RtFloat4* textures, int32_t nTexels, const uint32_t* lights, int32_t nLights,
                               const RtBVHNode2* bvhNodes, int32_t nNodes, const uint32_t* primIdx, int32_t nIdx,
                               const RtTLASNode* tlas, int32_t nTlas, const RtBVHInstance* blas, int32_t nBlas);   /* rt_upload_scene_bvh2 */
int rt_group_share_scene(RtGroup* g, RtGroup* from);                         /* e.g. the row bands of one frame: one device copy        */
int rt_group_update_scene(RtGroup* g, const RtPrimitive* prims, int32_t first, int32_t count, const RtBVHInstance* blas, int32_t nBlas,
                          RtUpdateStats* stats);                             /* rt_update_scene for the group's copy (all lanes)        */
int rt_group_rebuild_scene(RtGroup* g, const RtPrimitive* prims, int32_t first, int32_t count, const RtBVHInstance* blas, int32_t nBlas,
                           int32_t builder, const RtBuildOptions* opts, RtRebuildStats* stats);   /* rt_rebuild_scene for the group's copy */
int rt_group_rebuild_ranges(RtGroup* g, const RtPrimitive* prims, int32_t first, int32_t count, const RtBVHInstance* blas, int32_t nBlas,
                            const int32_t* plan, int32_t nRanges, const RtBuildOptions* opts, RtRebuildStats* stats);   /* rt_rebuild_ranges likewise */
int rt_group_resize_scene(RtGroup* g, const void* prims, int32_t nPrims, const RtSceneShape* shape, int32_t builder, const RtBuildOptions* opts,
                          RtRebuildStats* stats);                            /* rt_resize_scene for the group's copy (all lanes)        */
int rt_group_update_materials(RtGroup* g, const RtMaterialUpdate* update, RtMaterialStats* stats);   /* rt_update_materials, likewise  */
int rt_group_update_geometry(RtGroup* g, const RtGeometry* geometry, const RtBVHInstance* blas, int32_t nBlas, RtUpdateStats* stats);   /* rt_update_geometry for the group's copy */
int rt_group_rebuild_geometry(RtGroup* g, const RtGeometry* geometry, const RtBVHInstance* blas, int32_t nBlas, int32_t builder, const RtBuildOptions* opts,
                              RtRebuildStats* stats);                        /* rt_rebuild_geometry likewise                            */
int rt_group_rebuild_geometry_ranges(RtGroup* g, const RtGeometry* geometry, const RtBVHInstance* blas, int32_t nBlas, const int32_t* plan, int32_t nRanges,
                                     const RtBuildOptions* opts, RtRebuildStats* stats);   /* rt_rebuild_geometry_ranges likewise       */
int rt_group_seed(RtGroup* g, uint64_t firstStream);                         /* a single Renderer: 0 (what rt_group_create leaves);
                                                                              * rank r of a sample split: r*lanes                       */
int rt_group_reset(RtGroup* g);                                              /* resetKernel on every lane; frames = 0                   */
int rt_group_render(RtGroup* g, const RtCamera* cam, const RtSettings* settings, int32_t frames);   /* `frames` in all, round-robin   */
int rt_group_synchronize(RtGroup* g);
int rt_group_sum(RtGroup* g, void* devicePtr);                               /* lane-ordered sum of the group's rows into devicePtr (a
                                                                              * full-frame float4 buffer; NULL: the group's own)       */
int rt_group_read_accum(RtGroup* g, RtFloat4* out);
int rt_group_focus(RtGroup* g, int32_t x, int32_t y, const RtCamera* cam, float* t);
int rt_group_postproc(RtGroup* g, int32_t frames, float vignette, float gamma, float chromatic, RtFloat4* outF32, uint8_t* outRGBA8);

/* seedBuffer (renderer.cpp:195-196,200).  rt_set_seeds takes the band's slice
 * (one uint per band pixel); rt_seed_default fills seeds[i] with the (firstPixel+i+1)-th
 * xorshift32 output from 0x12345678 like the reference's host loop.
 * A context is never unseeded: rt_create leaves it as rt_seed_default would, and rt_group_create leaves lane m as
 * rt_group_seed(g, 0) would.  Every seed must be nonzero: rt_set_seeds returns RT_E_INVALID for a 0 (the message names the first
 * such index) before it copies anything, so the seeds on the device stay what they were; rt_group_seed and a checkpoint restore
 * go through it.  State 0 is the fixed point of the RNG step - every draw from it is 0.0f, and the rejection loop that samples a
 * direction at a diffuse hit would never end.  The host check suffices: the step is a bijection of the 32-bit states that fixes
 * only 0, so a nonzero state never becomes 0 on the device, and from a nonzero state that loop makes at most 28 attempts (DESIGN.md
 * section 2). */
int rt_set_seeds(RtCtx* ctx, const uint32_t* seeds, int64_t n);
int rt_seed_default(RtCtx* ctx);
int rt_get_seeds(RtCtx* ctx, uint32_t* out, int64_t n);

/* Optional: render into a caller-owned device accumulator float4[width*height]
 * (e.g. a torch tensor, so that torch.distributed can reduce it). NULL = own buffer. */
int rt_bind_accum(RtCtx* ctx, void* devicePtr);
void* rt_accum_device_ptr(RtCtx* ctx);
void* rt_stream(RtCtx* ctx);

/* resetKernel->Run(PIXELS) (renderer.cpp:41-46): clears this context's band. */
int rt_reset(RtCtx* ctx);

/* Renderer::RayTrace() x frames (renderer.cpp:64-94): generate, then max_bounces x
 * (extend, shade[, connect when RR is off]), then connect.  Uses settings->antiAliasing
 * and settings->renderBVH; asynchronous on the context's stream. */
int rt_render(RtCtx* ctx, const RtCamera* cam, const RtSettings* settings, int32_t frames);
int rt_synchronize(RtCtx* ctx);

/* focusKernel->Run(1) + settingsBuffer->CopyFromDevice() (renderer.cpp:289-301). */
int rt_focus(RtCtx* ctx, int32_t x, int32_t y, const RtCamera* cam, float* t);

/* accumBuffer->CopyFromDevice() (renderer.cpp:128): full frame float4[width*height]. */
int rt_read_accum(RtCtx* ctx, RtFloat4* out);
/* Checkpoint restore: overwrite the accumulator (the state carried across frames is {accum, seeds, settings->frames};
 * the reference has no checkpointing — SURVEY.md §5). */
int rt_write_accum(RtCtx* ctx, const RtFloat4* in);
int rt_read_counters(RtCtx* ctx, RtCounters* out);
int rt_reset_counters(RtCtx* ctx);
int rt_set_profile(RtCtx* ctx, int32_t level);      /* change RtConfig.profile at run time (synchronises) */
int rt_read_stage_times(RtCtx* ctx, RtStageTimes* out);
int rt_reset_stage_times(RtCtx* ctx);

/* Renderer::PostProc() + SaveFrame() (renderer.cpp:95-124,303-308; src/cl/postproc.cl): prep (divide by `frames`, clamp 1),
 * vignetting if vignette > 0, gammaCorr if gamma != 1, chromatic if chromatic > 0, then min(color,1).  Writes the float
 * image (float4[width*height], w = 1) and/or the 8-bit image (RGBA, bytes (uchar)(c*255) as SaveImageF); either may be NULL. */
int rt_postproc(RtCtx* ctx, int32_t frames, float vignette, float gamma, float chromatic, RtFloat4* outF32, uint8_t* outRGBA8);

/* ---- stage-level entry points (one kernel of the reference each), used by the parity
 * tests to feed identical inputs to one stage at a time ------------------------------ */
int rt_stage_begin_frame(RtCtx* ctx);                                           /* renderer.cpp:66-69   */
int rt_stage_generate(RtCtx* ctx, const RtCamera* cam, const RtSettings* s);    /* wavefront.cl:14-34   */
int rt_stage_extend(RtCtx* ctx, int32_t bounce, int32_t renderBVH);             /* wavefront.cl:35-75   */
int rt_stage_shade(RtCtx* ctx, int32_t bounce);                                 /* wavefront.cl:76-142  */
int rt_stage_connect(RtCtx* ctx, int32_t firstBounce, int32_t lastBounce);      /* wavefront.cl:144-201 */
/* ---- queries: the caller's own rays against the bound scene ------------------------------------------------------------------------
 * rt_trace intersects rays->n rays, read from DEVICE memory, with the scene the context holds, through the traversal kernels the
 * context runs for that scene (rt_kernel_info), and writes the results to DEVICE memory.  The reference has no such call: its rays are
 * born in generate and die in shade (wavefront.cl).  Ray i is origin (x, y, z) at rays->origin + i * originStride and direction at
 * rays->dir + i * dirStride (bytes; 12: packed float3, 16: float4 whose w is ignored, 32: every second float4, ...).  Directions are
 * used as given - not normalised, not validated; the sphere test assumes a unit D, as it does in the renderer.
 * A ray with a NaN or infinite component in its origin or direction misses, on every path: CLOSEST reports {RT_REALLYFAR, -1, 0, 0}
 * with zero point and normal, ANY reports 0 whatever tmax (a ray enters an instance before it meets a primitive, in single-BLAS scenes
 * too, and the instance transform - every component times every row, as in the reference - turns one non-finite component into an
 * all-NaN ray, which no box or primitive test accepts).  A zero
 * direction, like a subnormal or a FLT_MAX component, is traced as given: the result is what rt_stage_extend / connect compute for
 * that ray, and a ray with D = 0 can report a sphere it starts inside.
 *   RT_TRACE_CLOSEST, tmax NULL   hit[i] is, bit for bit, what rt_stage_extend leaves in its hit queue for a slot holding
 *                      O = (x, y, z, 0), D = (x, y, z, 0): t, primIdx, u, v of the closest hit, the same on every traversal path
 *                      (the nested loops, k_trace_persist, k_trace_persist_tlas with or without spill, k_trace_persist4,
 *                      k_trace_persist4_tlas); a miss is {RT_REALLYFAR, -1, 0, 0}.  point[i] / normal[i] (optional) are I = O + t * D
 *                      and the primitive's N at I flipped against D, as rt_debug_get_rays reports them - one device function computes
 *                      both; zeros on a miss.
 *   RT_TRACE_CLOSEST, tmax given   a pure function of the above: ray i reports the unbounded hit when its t < tmax[i], else a miss
 *                      (the traversal is NOT started at tmax: at knife edges that would be another float32 function).
 *   RT_TRACE_ANY       occluded[i] = 1 iff the context's connect traversal, given the shadow record {origin, tmax[i]} / {dir},
 *                      accepts a primitive with t < tmax[i] (tmax NULL: RT_REALLYFAR), else 0.  Connect's visit order; the result does
 *                      not depend on it - except for a ray with a direction component so large that the float32 triangle test
 *                      overflows (|D| of the order of FLT_MAX: 1 / det is 0 or the products are infinite, every visited triangle
 *                      then "hits" at t = 0 or NaN).  The verdict for such a ray is what the context's own traversal computes: it
 *                      may differ between a BVH2 and a BVH4 context, and at tmax > RT_REALLYFAR (+inf) a BVH2 context prunes the
 *                      boxes the ray misses, where the reference's loop and a BVH4 context descend into them (their miss value
 *                      1e30 is below such a tmax) and report such a ray occluded.  Every other ray, at every tmax, gets the one
 *                      verdict of the reference's loop ("Non-finite rays").
 * With 16-byte strides on 16-byte boundaries, CLOSEST, no tmax and nothing but `hit` wanted, the kernels read and write the caller's
 * arrays directly; every other form passes through a load and a store kernel that stream the batch once each.
 * A batch runs in passes of at most rt_trace_window(ctx) rays: min(2^22, what the context's per-workgroup tables hold - at least
 * 2^20); the environment variable RT355_TRACE_WINDOW=k, read per call, lowers it (tests).  Only a pass, never n, must fit 32 bits.
 * The call is asynchronous on the context's stream, in order with its renders and stage calls (a lane of a group: as the stage entry
 * points); rt_synchronize waits for it, and the caller's arrays must stay valid until then.  It follows rt_update_scene /
 * rt_rebuild_scene like a render does.  It leaves the frame alone: counters, stage times, accumulator, seeds, the queues behind
 * rt_debug_get_rays / rt_debug_get_shadow and the next rt_render are what they would be without it (the query has count words, dequeue
 * heads, counter rows and ray arrays of its own, allocated on first use - 48 bytes per ray of the largest pass that is not traced in
 * place - and freed with the context).  n == 0 succeeds and touches nothing.
 * RT_E_INVALID, before anything is launched or written: a null ctx / rays / out; no scene bound; an unknown mode; n < 0; a stride below
 * 12 or not a multiple of 4; a missing required output (CLOSEST: hit, ANY: occluded) or origin / dir; an output the mode does not
 * produce; origin / dir / tmax not on a 4-byte, hit / point / normal not on a 16-byte boundary; any pointer that
 * hipPointerGetAttributes does not report as memory accessible from the context's device (device memory of that GPU, managed or
 * pinned host memory), or whose allocation, where the runtime knows it, ends before the n-th element.  The message names the argument. */
#define RT_TRACE_CLOSEST 0      /* the context's extend traversal  */
#define RT_TRACE_ANY     1      /* the context's connect traversal */
typedef struct RtHit { float t; int32_t primIdx; float u, v; } RtHit;   /* the queue's own 16-byte hit record */
typedef struct RtRayBatch {
    const void* origin; const void* dir;   /* DEVICE pointers; ray i's x,y,z at base + i * stride                    */
    int64_t originStride, dirStride;       /* bytes; >= 12 and a multiple of 4 (12: packed float3, 16: float4, ...)   */
    const float* tmax;                     /* DEVICE, n floats; NULL: RT_REALLYFAR for every ray                      */
    int64_t n;
} RtRayBatch;
typedef struct RtTraceOut {                /* DEVICE pointers, n elements each; unused ones NULL                      */
    RtHit*    hit;        /* CLOSEST (required there) */
    RtFloat4* point;      /* CLOSEST, optional: I = O + t * D as extend leaves it in the reference's Ray              */
    RtFloat4* normal;     /* CLOSEST, optional: N of the primitive at I, flipped against D, as extend leaves it       */
    uint8_t*  occluded;   /* ANY (required there): 1 / 0                                                              */
} RtTraceOut;
int     rt_trace(RtCtx* ctx, int32_t mode, const RtRayBatch* rays, const RtTraceOut* out);
int64_t rt_trace_window(RtCtx* ctx);   /* rays one pass takes; never 0 here (0 would mean: any n in one pass) */
/* Ray queue of `bounce` as reference-layout Ray structs (I and N as extend leaves them). */
int rt_debug_get_rays(RtCtx* ctx, int32_t bounce, RtRay* out, int32_t capacity, int32_t* n);
/* Replace the ray queue of `bounce` by n <= (y1 - y0) * width caller records.  The kernels index the accumulator by a record's
 * pixelIdx and the primitive array by its primIdx (a ray that arrives already hit): a pixelIdx outside the context's band
 * [y0 * width, y1 * width) or a primIdx outside [-1, nPrims) of the bound scene (-1 only, without one) is RT_E_INVALID, and the
 * queue stays as it was. */
int rt_debug_set_rays(RtCtx* ctx, int32_t bounce, const RtRay* in, int32_t n);
/* Shadow rays appended by shade() of bounces [firstBounce,lastBounce], in queue order:
 * origin = I + L*EPSILON (xyz), tmax = dist - 2*EPSILON, dir = L (xyz), pixel index and the
 * radiance the ray carries if unoccluded. */
typedef struct RtShadowRecord { float ox, oy, oz, tmax; float lx, ly, lz; int32_t pixelIdx; RtFloat4 radiance; } RtShadowRecord;
int rt_debug_get_shadow(RtCtx* ctx, int32_t firstBounce, int32_t lastBounce, RtShadowRecord* out, int32_t capacity, int32_t* n);
/* Per-ray `steps` (the value the reference's heat map shows, wavefront.cl:66-67) of the last extend; recording is off
 * by default (it costs 4 B written per ray) and is switched on with rt_debug_enable_steps(ctx, 1). */
int rt_debug_enable_steps(RtCtx* ctx, int32_t on);
int rt_debug_get_steps(RtCtx* ctx, int32_t* out, int32_t capacity, int32_t* n);

/* The kernels' math functions on their own (tests/test_gpu_math.py): the very device functions the generate and shade kernels call,
 * evaluated on device 0.  Per element, `in` and `out` hold (32-bit words):
 *   RT_MATH_EXP / SIN / COS / ACOS   x                                  -> float
 *   RT_MATH_ATAN                     x                                  -> float atan2(x, 1), i.e. the atan of atan2
 *   RT_MATH_F2I                      x                                  -> int32 as the GPU converts (NaN -> 0, saturating)
 *   RT_MATH_ATAN2                    y, x                               -> float
 *   RT_MATH_SPHERE_TEXEL             N.x, N.y, N.z, N.w, texW, texH (int32) -> int32 x, y: texel column and row of a sphere hit
 *   RT_MATH_NORMALIZE4               v.x, v.y, v.z, v.w                 -> float4
 *   RT_MATH_LENGTH4                  v.x, v.y, v.z, v.w                 -> float
 * rt_debug_math / rt_debug_math_sweep evaluate the library's default arithmetic (RT_BUILTINS_DEFAULT), the _mode forms the one named
 * (RT_BUILTINS_*; any other value: RT_E_INVALID).  RT_BUILTINS_REFERENCE evaluates the ocml functions; it has no ACOS, ATAN or ATAN2
 * (it calls acospi / atan2pi only inside the texel lookup) and returns RT_E_UNSUPPORTED for them. */
#define RT_MATH_EXP           0
#define RT_MATH_SIN           1
#define RT_MATH_COS           2
#define RT_MATH_ACOS          3
#define RT_MATH_ATAN          4
#define RT_MATH_F2I           5
#define RT_MATH_ATAN2         6
#define RT_MATH_SPHERE_TEXEL  7
#define RT_MATH_NORMALIZE4    8
#define RT_MATH_LENGTH4       9
int rt_debug_math(int32_t fn, const void* in, void* out, int64_t n);
int rt_debug_math_mode(int32_t builtins, int32_t fn, const void* in, void* out, int64_t n);
/* Sweep of a one-argument function (EXP ... F2I) over every float32 bit pattern of blocks [firstBlock, firstBlock + nBlocks) of
 * 2^20 inputs each (block b: bits b<<20 ...; 4096 blocks in all).  hashes[k] = sum mod 2^64 over the block of
 * splitmix64((uint64_t)in_bits << 32 | out_bits), every NaN output counted as 0x7fc00000: independent of evaluation order. */
#define RT_MATH_SWEEP_BLOCK_BITS 20
int rt_debug_math_sweep(int32_t fn, int32_t firstBlock, int32_t nBlocks, uint64_t* hashes);
int rt_debug_math_sweep_mode(int32_t builtins, int32_t fn, int32_t firstBlock, int32_t nBlocks, uint64_t* hashes);

#ifdef __cplusplus
}
#endif
#endif /* RT355_H */

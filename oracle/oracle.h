/* oracle.h — TEST INFRASTRUCTURE ONLY.
 *
 * CPU restatement (plain C) of the reference's wavefront path tracer hot path:
 * generate -> extend -> shade -> connect with TLAS / BVH2 / BVH4 traversal
 * (reference: src/cl/wavefront.cl, tlas.cl, bvh.cl, primitives.cl, ray.cl,
 * shading.cl, camera.cl, glass.cl, skydome.cl, util.cl; launch sequence
 * src/renderer.cpp:64-94).  It is the checker for the HIP path.  Only tests/,
 * __graft_entry__.smoke() and bench.py's cpu_baseline leg may load it; the product
 * library (librt355.so) never links or calls anything in this directory.
 *
 * Pinning: see oracle/README.md — the restatement is checked stage by stage against
 * the reference's own OpenCL kernels, compiled unmodified for gfx950 by
 * oracle/build_ref.sh and run on the MI355X (outputs committed under tests/golden/).
 */
#ifndef ORACLE_H
#define ORACLE_H
#include "../include/rt355_types.h"

#ifdef __cplusplus
extern "C" {
#endif

enum { ORC_SHADING_SIMPLE = 0, ORC_SHADING_NEE = 1 };       /* renderer.h:6-7   */
enum { ORC_SAMPLING_HEMISPHERE = 0, ORC_SAMPLING_COSINE = 1 }; /* renderer.h:12-13 */
enum { ORC_ACCEL_BVH2 = 0, ORC_ACCEL_BVH4 = 1 };            /* renderer.h:15-16 */
/* Schedules (legal executions of the reference's persistent-thread kernels):
 * S1: every work-item claims exactly queue slot g (RNG stream seeds[g]); appends
 *     keep the relative order of their source slots.
 * S0: ONE work-item (global size 1) drains the whole queue: slots are taken in
 *     descending order by atomic_dec, all draws come from seeds[0], appends happen
 *     in processing order.  This is what the reference kernels do when launched
 *     with a global size of 1, and is used to pin shade() against them. */
enum { ORC_SCHED_S1 = 1, ORC_SCHED_S0 = 0 };
/* Order in which an OCCLUSION traversal (connect) visits the two children of a BVH2 BLAS node when the ray hits both:
 * REFERENCE: near child first (bvh.cl:41-52), what a zero-filled config gives.
 * LATER_EXIT: the child with the greater slab exit distance first, ties to child 1 - the order of the HIP path's connect
 *     (rt355_kernels.h slab_any).  Changes nothing else: TLAS nodes, instance entry, BVH4 and every extend / focus traversal keep
 *     the reference's order, and a shadow ray's verdict does not depend on it - only connect's node_visits and prim_tests do.  (The
 *     verdict of a ray whose direction has a component near FLT_MAX can: its primitive tests overflow, see traverse_bvh2_later_exit.) */
enum { ORC_CONNECT_REFERENCE = 0, ORC_CONNECT_LATER_EXIT = 1 };

typedef struct OrcScene {
    const RtPrimitive*   prims;     int32_t nPrims;
    const RtMaterial*    mats;      int32_t nMats;
    const RtFloat4*      tex;       int32_t nTex;
    const uint32_t*      lights;    int32_t nLights;
    const RtBVHNode2*    bvh2;      /* used when accel == ORC_ACCEL_BVH2 */
    const RtBVHNode4*    bvh4;      /* used when accel == ORC_ACCEL_BVH4 */
    int32_t              nNodes;
    const uint32_t*      primIdx;   int32_t nIdx;
    const RtTLASNode*    tlas;      int32_t nTlas;
    const RtBVHInstance* blas;      int32_t nBlas;
} OrcScene;

typedef struct OrcConfig {
    int32_t width, height;
    int32_t max_bounces;            /* host loop count, renderer.cpp:75 (MAX_BOUNCES) */
    int32_t shading, sampling, accel;
    int32_t russian_roulette, filter_fireflies;
    int32_t schedule;               /* ORC_SCHED_S1 / ORC_SCHED_S0 */
    int32_t connect_order;          /* ORC_CONNECT_REFERENCE / ORC_CONNECT_LATER_EXIT */
} OrcConfig;

/* Work counters behind the roofline formula of SURVEY.md §8(d). */
typedef struct OrcCounters {
    uint64_t rays;        /* R      rays traced                       */
    uint64_t tlas_visits; /* V_tlas TLAS interior visits               */
    uint64_t inst_visits; /* L_inst instance (TLAS leaf) visits        */
    uint64_t node_visits; /* V_int  BVH2 interior visits / V4 BVH4 pops */
    uint64_t prim_tests;  /* T_prim primitive tests                    */
} OrcCounters;

uint32_t orc_xorshift32(uint32_t* state);
void     orc_seed_stream(uint32_t* seeds, int64_t first, int64_t n);   /* renderer.cpp:195-196 */

void orc_generate(RtRay* rays, int32_t n, int32_t firstPixel, const OrcConfig* cfg,
                  const RtCamera* cam, int32_t antiAliasing, uint32_t* seeds);
void orc_extend(RtRay* rays, int32_t n, const OrcScene* sc, const OrcConfig* cfg,
                int32_t renderBVH, RtFloat4* accum, int32_t* steps, OrcCounters* ctr);
void orc_shade(RtRay* in, int32_t nIn, RtRay* out, int32_t* nOut,
               RtShadowRay* shadow, int32_t* nShadow, const OrcScene* sc,
               const OrcConfig* cfg, RtFloat4* accum, uint32_t* seeds);
void orc_connect(const RtShadowRay* shadow, int32_t n, const OrcScene* sc,
                 const OrcConfig* cfg, RtFloat4* accum, OrcCounters* ctr);
/* orc_connect's traversal work per shadow ray (work[i] for shadow[i]); accumulates nothing.  Summed, the four counts are what
 * orc_connect adds to its counters for the same queue. */
typedef struct OrcRayWork { uint32_t node_visits, prim_tests, tlas_visits, inst_visits, occluded; } OrcRayWork;
void orc_connect_work(const RtShadowRay* shadow, int32_t n, const OrcScene* sc, const OrcConfig* cfg, OrcRayWork* work);
/* orc_connect's traversal on rays given as they are traced: origin[i], dir[i] (xyz; w is taken as 0), reach tmax[i] (NULL: RT_REALLYFAR);
 * occluded[i] = 1 iff a primitive is accepted with t < tmax[i].  orc_connect's record {I, L, dist} is the ray I + L * eps, L, dist - 2 eps. */
void orc_occluded(const RtFloat4* origin, const RtFloat4* dir, const float* tmax, int32_t n, const OrcScene* sc, const OrcConfig* cfg, uint8_t* occluded);
float orc_focus(int32_t x, int32_t y, const OrcScene* sc, const OrcConfig* cfg, const RtCamera* cam);

/* One Renderer::RayTrace() (renderer.cpp:64-94) over pixels [firstPixel, firstPixel+n).
 * accum is indexed by global pixel index; seeds by band-local slot.  work must hold
 * 2*n RtRay + (max_bounces)*n RtShadowRay (query with orc_frame_work_bytes). */
size_t orc_frame_work_bytes(int32_t n, const OrcConfig* cfg);
void   orc_render_frame(const OrcScene* sc, const OrcConfig* cfg, const RtCamera* cam,
                        int32_t antiAliasing, int32_t firstPixel, int32_t n,
                        RtFloat4* accum, uint32_t* seeds, void* work,
                        OrcCounters* extendCtr, OrcCounters* connectCtr);

/* CPU baseline driver: renders `frames` frames of rows [y0,y1) split into `threads`
 * independent row bands (OpenMP), each band with its own queues and seed slice. */
void orc_render_bands(const OrcScene* sc, const OrcConfig* cfg, const RtCamera* cam,
                      int32_t antiAliasing, int32_t y0, int32_t y1, int32_t frames,
                      int32_t threads, RtFloat4* accum, uint32_t* seeds,
                      OrcCounters* extendCtr, OrcCounters* connectCtr);

/* Template-style CPU tracer (CPU-B of BASELINE.md §3): one primary ray per pixel,
 * nearest hit through the BVH, normal visualisation into out[W*H]. */
void orc_trace_normals(const OrcScene* sc, const OrcConfig* cfg, const RtCamera* cam,
                       int32_t threads, RtFloat4* out);

/* Renderer::PostProc + SaveFrame (renderer.cpp:95-124,303-308; src/cl/postproc.cl:7-86). */
void orc_postproc(const RtFloat4* accum, int32_t W, int32_t H, int32_t frames, float vignette, float gamma, float chromatic,
                  RtFloat4* outF, uint8_t* outRGBA8);

/* Unit hooks for the known-answer tests. */
void     orc_test_random_float3(uint32_t* seed, float out[4]);
void     orc_test_cosine_hemisphere(const float N[4], uint32_t* seed, float out[4]);
void     orc_test_triangle(const float v0[3], const float v1[3], const float v2[3], const float O[3], const float D[3], float out[4]);
uint32_t orc_test_wang_hash(uint32_t s);

/* The math functions of the path on their own: the function ids and in / out layouts of rt_debug_math and the block hash of
 * rt_debug_math_sweep (include/rt355.h).  threads is capped at 16. */
int orc_math(int32_t fn, const void* in, void* out, int64_t n);
int orc_math_sweep(int32_t fn, int32_t firstBlock, int32_t nBlocks, uint64_t* hashes, int32_t threads);
/* Exhaustive error of a one-argument function (EXP ... ATAN; ATAN is atan2(x, 1)) over every float in [lo, hi] against libm double:
 * in ulps of the float spacing at the exact value (subnormal spacing below FLT_MIN), or with `absolute` in units of 2^-24.  A NaN, or an
 * infinity where the exact value does not round to one, counts as an infinite error.  `above` counts the inputs whose error exceeds `bound`; `arg` is the input of the
 * largest error (the smallest in magnitude among ties). */
typedef struct OrcMathError { double max_err; float arg; uint64_t above; uint64_t count; } OrcMathError;
int orc_math_error(int32_t fn, float lo, float hi, int32_t absolute, double bound, int32_t threads, OrcMathError* out);

/* The RNG step is linear over GF(2): `steps` steps from `state` through a power of its 32x32 matrix (a jump-ahead). */
uint32_t orc_xorshift32_jump(uint32_t state, uint64_t steps);
/* sample_ball's rejection loop (ray.cl:49-53 / 62-69) over the RNG's whole cycle, walked once from state 1 in segments reached by
 * jump-ahead (OpenMP; threads is capped at 16).  An attempt takes three draws, each mapped as the kernels map it -
 * (float)u * 2.3283064365387e-10f * 2 - 1 - and is rejected when x*x + y*y + z*z > 1.0f (summed left to right, no contraction).  The
 * loop entered with state s makes the attempts at s, s + 3 draws, s + 6 draws, ...: `longest` is the longest run of consecutively
 * rejected attempts at that stride over every nonzero s; `state` the state the first run of that length on
 * the walk from state 1 starts from, `index` steps after state 1 (the loop entered there makes longest + 1 attempts: 3 * (longest + 1)
 * draws).  `states` is the number of states walked, `rejected` how many of the attempts starting from them are rejected, `closed`
 * whether the segments joined up and the walk returned to state 1 after `states` steps. */
typedef struct OrcRejection { uint64_t states, rejected; uint32_t longest, state, index; int32_t closed; } OrcRejection;
int orc_rejection_cycle(int32_t threads, OrcRejection* out);

#ifdef __cplusplus
}
#endif
#endif

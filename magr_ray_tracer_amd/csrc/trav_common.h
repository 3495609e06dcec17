// trav_common.h — the rules by which a context chooses its traversal (rt355.hip, configure_traversal), free of HIP: which of the seven
// Traversal kinds runs, whether the stack columns spill and at which LDS cap, the three PersistTune records before they are fitted to the
// device, and every RT355_* knob of the traversal, read in one place.  plan_traversal is a pure function of a handful of integers, so a
// test without a GPU pins it (rt_debug_traversal_plan, tests/test_traversal_plan_cpu.py; tools/trav_plan_main.cpp compiles this header
// alone).  What needs the device - occupancy queries, the fitting of the top table, the grids, the spill allocation - stays in rt355.hip.
#pragma once
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include "../../include/rt355.h"

namespace rt355dev {

// What a persistent kernel is handed by value with every launch (rt355_kernels.h)
struct PersistTune {
    int chunk, refill, inner, leafK;   // rays per dequeue, idle lanes that trigger a top-up, events between checks, lanes on a leaf that trigger the triangle path
    int fixedChunks;                   // chunks dealt round-robin instead of dequeued
    int flat = 0;                      // k_trace_persist_tlas runs every queue through its one-ray-per-lane branch, 64 rays per wave and round (short traversals: config 5's open scene)
    int xcdRays = 0, xcdFirst = 0;     // a sparse queue's rays are kept on as few XCDs as hold them at this many rays each (one-ray-per-lane branches; 0 = spread over all eight)
    int thin = 0;                      // a queue of at most `thin` rays per participating wave is spread evenly over the waves (few lanes of each) instead of filling the first waves
    int topLevels = 0, topBase = 0;    // k_trace_persist<.., TOP>: levels of the tree in the LDS top table (1..6) and the table's first word in dynamic LDS (behind the stack columns)
};

// The traversal kernels of a context (layout 1 only; the first four values are RtKernelInfo.persist):
enum Traversal {
    TRAV_NESTED,        // the one-ray-per-lane nested loops (k_extend / k_connect)
    TRAV_BVH2,          // persistent wavefronts over the BVH2 of a single BLAS (k_trace_persist)
    TRAV_TLAS,          // ... through a multi-BLAS TLAS (k_trace_persist_tlas)
    TRAV_TLAS_SPILL,    // ... with the deep end of the traversal stacks in global memory (trees deeper than the LDS share of 7 workgroups per CU)
    TRAV_BVH4,          // ... over the BVH4 of a single BLAS (k_trace_persist4)
    TRAV_BVH4_TLAS,     // ... through a multi-BLAS TLAS over BVH4 instances (k_trace_persist4_tlas; extend_variant 6 only)
    TRAV_BVH4_TLAS_SPILL,   // ... with the deep end of the traversal stacks in global memory
};
static inline bool persistent(int trav) { return trav != TRAV_NESTED; }
static inline bool spill_trav(int trav) { return trav == TRAV_TLAS_SPILL || trav == TRAV_BVH4_TLAS_SPILL; }
static inline bool bvh4_tlas_trav(int trav) { return trav == TRAV_BVH4_TLAS || trav == TRAV_BVH4_TLAS_SPILL; }
static inline bool tlas_trav(int trav) { return trav == TRAV_TLAS || trav == TRAV_TLAS_SPILL || bvh4_tlas_trav(trav); }   // one tagged column per lane, world-ray backup behind it

// workgroups of 256 threads the hardware admits per CU whatever the occupancy query says: any kernel / kernels with <= 96 SGPRs
constexpr int kAdmitAnySgpr = 6, kAdmit96Sgpr = 7;
// LDS words per lane of k_trace_persist_tlas: 22 x 1 KB per workgroup is the most with which seven workgroups share a CU's 160 KB; the
// world ray (O, D, 1/D) and the TLAS level's pruning distance wait in 10 of them while a lane is inside an instance, so a spilling
// kernel keeps 12 stack entries in LDS
constexpr int kFitSeven = 22, kBackupWords = 10, kSpillCap = kFitSeven - kBackupWords;
// levels of the LDS top table of k_trace_persist's event loops, extend and connect, at most: a context takes the deepest table that does
// not cost its persistent grid a resident workgroup (configure_traversal; EXPERIMENTS.md (59)).  0 = the instantiations without it
constexpr int kTopLevelsExtend = 6, kTopLevelsConnect = 6;
// What the kernels fix and the rules compute with (rt355.hip asserts that they agree): the lanes of a workgroup, one stack column each
// (kBlock, rt355_dev.h), and the deepest top table an instantiation takes (kTopMaxLevels, rt355_kernels.h)
constexpr int kColumnLanes = 256, kTopLevelsMax = 6;

// LDS traversal stack: one column per lane; sized at upload to what this scene's trees can need
// (never more than the reference kernels' 32 / 64 entries).
static inline size_t stack_bytes(int stackEntries) { return (size_t)stackEntries * kColumnLanes * sizeof(uint32_t); }
// the top table of k_trace_persist<.., TOP> behind them: 2^levels - 1 pair records of 64 bytes
static inline size_t top_bytes(int levels) { return levels > 0 ? (((size_t)1 << levels) - 1) * 64 : 0; }
// k_trace_persist_tlas keeps its pending TLAS siblings (<= one per level) on the same column; with a SPILL kind only the first spillCap
// entries of a column live in LDS.  The world-ray backup sits behind them.
static inline int tlas_stack_entries(int stackEntries, int tlasDepth) { return stackEntries + tlasDepth + 1; }
static inline int tlas_lds_entries(int trav, int spillCap, int stackEntries, int tlasDepth) { return spill_trav(trav) ? spillCap : tlas_stack_entries(stackEntries, tlasDepth); }
static inline size_t tlas_column_bytes(int entries) { return (size_t)(entries + kBackupWords) * kColumnLanes * sizeof(uint32_t); }

// What the plan is a function of
struct TravFacts {
    int accel = 0, extend_variant = 0, persist_blocks_per_cu = 0;                                         // RtConfig
    int layout = 0, singleBlas = 0, tlasDepth = 0, nInterior = 0, nQuads = 0, stackEntries = 0;           // the scene copy
    int sharedMemPerBlock = 0;   // the device: the LDS a workgroup may ask for
    int xcdFirst = 0;            // the XCD this context's sparse queues start on (handed out per context by rt355.hip)
};

// Every RT355_* knob of the traversal as parsed.  A value outside its range reads as if the knob were unset.
struct TravKnobs {
    bool spillCapSet = false; int spillCap = 0;      // RT355_SPILL_CAP, 6..64: tests force the spill path with a tiny cap
    bool noSpill = false;                            // RT355_NO_SPILL (non-zero)
    bool coherentSet = false; int coherent = 0;      // RT355_COHERENT
    bool tuneSet = false; int tune[4] = {};          // RT355_TUNE="chunk,refill,inner,leafK[,blocksPerCU]" (tuning aid)
    int tuneBlocks = 0;                              // ... its fifth field (> 0), taken whether or not the first four hold
    bool fixedChunksSet = false; int fixedChunks[2] = {};   // RT355_FIXED_CHUNKS="extend,connect" (tuning aid)
    bool tuneConnectSet = false; int tuneConnect[4] = {};   // RT355_TUNE_CONNECT: RT355_TUNE's four fields, connect launches only
    bool topLevelsSet = false; int topLevels[2] = {};       // RT355_TOP_LEVELS="e[,c]" (0..6; one number: both)
    bool flatSet = false; int flat[2] = {};          // RT355_TLAS_FLAT="e,c" (A/B runs)
    bool xcdRaysSet = false; int xcdRays = 0;        // RT355_XCD_RAYS (>= 0)
    bool thinSet = false; int thin = 0;              // RT355_THIN (0..64; 0: off)
    int connectBlocks = 0;                           // RT355_CONNECT_BLOCKS (> 0; lab): workgroups per CU of connect's persistent grid
    bool noFusePrimary = false;                      // RT355_FUSE_PRIMARY=0: rt_render keeps k_generate and the stored primary queue (A/B runs, tests)
};

// The only place that reads them.  Not cached: tests change the environment between a context's uploads.
static inline TravKnobs read_trav_knobs()
{
    TravKnobs k;
    auto tune_ok = [](int a, int b, int c, int l) { return a > 0 && b > 0 && b <= 64 && c > 0 && l > 0 && l <= 64; };
    if (const char* t = getenv("RT355_SPILL_CAP")) { const int v = atoi(t); if (v >= 6 && v <= 64) { k.spillCap = v; k.spillCapSet = true; } }
    if (const char* t = getenv("RT355_NO_SPILL")) k.noSpill = atoi(t) != 0;
    if (const char* t = getenv("RT355_COHERENT")) { k.coherent = atoi(t); k.coherentSet = true; }
    if (const char* t = getenv("RT355_TUNE")) {
        int a = 0, b = 0, c = 0, l = 0, d = 0;
        const int n = sscanf(t, "%d,%d,%d,%d,%d", &a, &b, &c, &l, &d);
        if (n >= 4 && tune_ok(a, b, c, l)) { k.tune[0] = a; k.tune[1] = b; k.tune[2] = c; k.tune[3] = l; k.tuneSet = true; }
        if (n == 5 && d > 0) k.tuneBlocks = d;
    }
    if (const char* t = getenv("RT355_FIXED_CHUNKS")) { int a = 0, b = 0; if (sscanf(t, "%d,%d", &a, &b) == 2) { k.fixedChunks[0] = a; k.fixedChunks[1] = b; k.fixedChunksSet = true; } }
    if (const char* t = getenv("RT355_TUNE_CONNECT")) {
        int a = 0, b = 0, c = 0, l = 0;
        if (sscanf(t, "%d,%d,%d,%d", &a, &b, &c, &l) == 4 && tune_ok(a, b, c, l)) { k.tuneConnect[0] = a; k.tuneConnect[1] = b; k.tuneConnect[2] = c; k.tuneConnect[3] = l; k.tuneConnectSet = true; }
    }
    if (const char* t = getenv("RT355_TOP_LEVELS")) {
        int a = 0, b = 0;
        const int n = sscanf(t, "%d,%d", &a, &b);
        if (n == 1) b = a;
        if (n >= 1 && a >= 0 && a <= kTopLevelsMax && b >= 0 && b <= kTopLevelsMax) { k.topLevels[0] = a; k.topLevels[1] = b; k.topLevelsSet = true; }
    }
    if (const char* t = getenv("RT355_TLAS_FLAT")) { int a = 0, b = 0; if (sscanf(t, "%d,%d", &a, &b) == 2) { k.flat[0] = a; k.flat[1] = b; k.flatSet = true; } }
    if (const char* t = getenv("RT355_XCD_RAYS")) { k.xcdRays = std::max(0, atoi(t)); k.xcdRaysSet = true; }
    if (const char* t = getenv("RT355_THIN")) { k.thin = std::min(64, std::max(0, atoi(t))); k.thinSet = true; }
    if (const char* t = getenv("RT355_CONNECT_BLOCKS")) { const int d = atoi(t); if (d > 0) k.connectBlocks = d; }
    if (const char* t = getenv("RT355_FUSE_PRIMARY")) k.noFusePrimary = atoi(t) == 0;
    return k;
}

// What a context takes over (rt355.hip, configure_traversal)
struct TravPlan {
    int trav = TRAV_NESTED;
    int spillCap = kSpillCap;   // LDS stack entries per lane of a spilling kernel
    int coherent = 1;           // wave-uniform node records through the scalar cache on bounce 0 (1), every bounce of the TLAS kernel (2, lab), off (0)
    PersistTune tune{}, tuneConnect{}, tune4{};   // extend (BVH2), connect, extend (BVH4), before the top table is fitted to the device
    bool topAuto = false;       // no knob named the top table's depth: each stage takes the deepest that costs it no workgroup
    int tuneBlocks = 0, connectBlocks = 0;   // workgroups per CU of the persistent grids that the knobs ask for (0: none asked)
    bool fusePrimary = false;   // rt_render's bounce 0 computes the primary rays in its extend and shade launches: no k_generate, no stored queue
};

static inline TravPlan plan_traversal(const TravFacts& f, const TravKnobs& k)
{
    TravPlan p;
    const int entries = tlas_stack_entries(f.stackEntries, f.tlasDepth);
    // persistent wavefronts need layout 1: over the BVH2 or the BVH4 of a single BLAS (the TLAS root is a leaf), or through a TLAS with
    // several BLAS (BASELINE config 5) - TLAS entries ride on the BLAS stack column, so the TLAS must be shallow (<= 8 levels: <= 256
    // instances in a balanced tree) and the pair-table ids must leave the three tag bits free; extend_variant 4 keeps the one-ray-per-lane
    // nested loops for multi-BLAS scenes (A/B runs)
    p.trav = TRAV_NESTED;
    if (f.layout == 1 && f.extend_variant != 2) {
        if (f.singleBlas) p.trav = f.accel == RT_ACCEL_BVH2 ? TRAV_BVH2 : (f.accel == RT_ACCEL_BVH4 ? TRAV_BVH4 : TRAV_NESTED);
        else if (f.accel == RT_ACCEL_BVH2 && f.extend_variant != 4 && f.tlasDepth <= 8 && f.nInterior < (1 << 29)) p.trav = TRAV_TLAS;
    }
    // extend_variant 6 (opt-in): a multi-BLAS BVH4 scene through k_trace_persist4_tlas, under the TLAS kernel's conditions - quad ids ride on
    // the tagged column, so the copy must hold fewer than 2^29 quad records; everything else under variant 6 is variant 0
    if (f.layout == 1 && f.extend_variant == 6 && f.accel == RT_ACCEL_BVH4 && !f.singleBlas && f.tlasDepth <= 8 && f.nQuads < (1 << 29)) p.trav = TRAV_BVH4_TLAS;
    // deep trees (an SBVH at alpha = 0: config 5's second BLAS has 63 levels): a full LDS column per lane would leave two workgroups per
    // CU, so the column is capped and its deep end spills to global memory (rt355_kernels.h, stk_push / stk_pop)
    p.spillCap = k.spillCapSet ? k.spillCap : kSpillCap;
    const bool forceSpill = k.spillCapSet;
    // (columns of up to 22 entries stay whole in LDS, backup beside them: 5-6 workgroups per CU without the spill branches beat 7 with them,
    // 1,923 against 1,849 and 1,327 against 1,310 M samples/s on two-BLAS scenes of 16 and 22 entries - tools/middepth_tlas.py)
    if (p.trav == TRAV_TLAS && (entries > kFitSeven || forceSpill) && entries > p.spillCap && !k.noSpill) p.trav = TRAV_TLAS_SPILL;
    if (p.trav == TRAV_TLAS && entries > RT_BVH4_STACK + 9) p.trav = TRAV_NESTED;
    if (p.trav == TRAV_BVH4_TLAS) {
        // the BVH2 rule with the BVH2 numbers (kFitSeven was measured on pair records, not on quad records).  A push-all BVH4 needs many
        // more entries than a BVH2 of its depth: a column that, with its backup words, exceeds the LDS a workgroup may ask for takes the
        // spill instantiation too, and the nested loops where RT355_NO_SPILL forbids that - no launch the runtime would reject
        const size_t lds = (size_t)std::max(0, f.sharedMemPerBlock);
        const bool fits = tlas_column_bytes(entries) <= lds;
        const bool canSpill = !k.noSpill && entries > p.spillCap && tlas_column_bytes(p.spillCap) <= lds;
        if ((entries > kFitSeven || forceSpill || !fits) && canSpill) p.trav = TRAV_BVH4_TLAS_SPILL;
        else if (!fits) p.trav = TRAV_NESTED;
    }
    // bounce 0 (RT355_COHERENT=2: every bounce of k_trace_persist_tlas, lab; 0: off for A/B runs): wave-uniform node records come through
    // the scalar cache (traverse_bvh2_packed_coherent, k_trace_persist_tlas<COH>)
    p.coherent = k.coherentSet ? k.coherent : 1;
    // The fused primary path: where bounce 0's extend launch is one workgroup per 256 pixels through the one-ray-per-lane branch of a
    // single-BLAS kernel (trace_short_queue of k_trace_persist, not under extend_variant 3 or 5, and of k_trace_persist4), that launch
    // computes its rays itself (k_trace_primary).  The TLAS kernels' short-queue branches are their own code and the nested kernels have
    // none: those contexts stay on k_generate.  RT355_FUSE_PRIMARY=0 keeps every context there.
    p.fusePrimary = !k.noFusePrimary && ((p.trav == TRAV_BVH2 && f.extend_variant != 3 && f.extend_variant != 5) || p.trav == TRAV_BVH4);

    // extend (BVH2), connect, extend (BVH4): measured optima (tools/tune_extend.sh, tune_connect.sh, tune_persist.sh)
    p.tune = PersistTune{ 112, 24, 6, 8, 0 }; p.tuneConnect = PersistTune{ 128, 32, 6, 16, 0 }; p.tune4 = PersistTune{ 64, 20, 6, 8, 0 };
    if (f.persist_blocks_per_cu > 0) {
        p.tune.leafK = 16;   // contexts sharing the GPU: hold triangle events back until 16 lanes wait on a leaf (+1 % with three lanes, -0.6 % alone)
    } else {
        // a context with the GPU to itself: chunks after the first are dealt round-robin too (no atomic, no round trip per dequeue):
        // 716 -> 725 M samples/s; with three contexts sharing the GPU the dynamic queue is 0.9 % better (profiles/r02_fixed_chunks.txt)
        p.tune.fixedChunks = p.tuneConnect.fixedChunks = p.tune4.fixedChunks = 1;
    }
    if (k.tuneSet) p.tune = p.tuneConnect = p.tune4 = PersistTune{ k.tune[0], k.tune[1], k.tune[2], k.tune[3], 0 };
    p.tuneBlocks = k.tuneBlocks; p.connectBlocks = k.connectBlocks;
    if (k.fixedChunksSet) { p.tune.fixedChunks = p.tune4.fixedChunks = k.fixedChunks[0]; p.tuneConnect.fixedChunks = k.fixedChunks[1]; }
    if (k.tuneConnectSet) p.tuneConnect = PersistTune{ k.tuneConnect[0], k.tuneConnect[1], k.tuneConnect[2], k.tuneConnect[3], 0 };
    // RT355_TOP_LEVELS: levels of the BLAS that the event loops of k_trace_persist descend from a table in LDS when a lane takes a new ray
    // (rt355_kernels.h, top_descent), extend and connect.  0: the instantiation without the table.  Without the knob: the deepest table
    // up to kTopLevels* that leaves the stage's persistent grid as it is (rt355.hip, fit_top_tables)
    p.tune.topLevels = p.tuneConnect.topLevels = 0;
    if (p.trav == TRAV_BVH2) {
        p.tune.topLevels = kTopLevelsExtend; p.tuneConnect.topLevels = kTopLevelsConnect;
        p.topAuto = true;
        if (k.topLevelsSet) { p.tune.topLevels = k.topLevels[0]; p.tuneConnect.topLevels = k.topLevels[1]; p.topAuto = false; }
    }
    if (tlas_trav(p.trav)) {
        // Multi-BLAS scenes so far are open scenes whose rays take a dozen events (config 5: 1 TLAS visit, 1.5 instance entries, 7.7 box
        // pairs, 1.9 triangles per ray): extend runs the kernel's one-ray-per-lane branch over every queue (measured per bounce at 4K:
        // 522 / 446 / 198 us against 654 / 562 / 194 through the event loop and 730 / 643 / 237 through the nested loops at two
        // workgroups per CU), connect - unoccluded shadow rays cross the whole scene - the event loop (646 against 690 / 1,418 us).
        // RT355_TLAS_FLAT overrides (A/B runs).  profiles/r03_config5_per_bounce.txt
        // (k_trace_persist4_tlas takes its extend tune from tune4; the flat default was measured on BVH2 instances only)
        p.tune.flat = p.tune4.flat = 1; p.tuneConnect.flat = 0;
        if (k.flatSet) { p.tune.flat = p.tune4.flat = k.flat[0]; p.tuneConnect.flat = k.flat[1]; }
    }
    // sparse queues (the one-ray-per-lane branches) stay on as few XCDs as hold them at 1,024 rays each, so that their rays share an L2
    // (EXPERIMENTS.md (54): 16,384 before the thinning below made spreading the better default); contexts start on different XCDs
    p.tune.xcdRays = p.tuneConnect.xcdRays = p.tune4.xcdRays = k.xcdRaysSet ? k.xcdRays : 1024;
    p.tune.xcdFirst = p.tuneConnect.xcdFirst = p.tune4.xcdFirst = f.xcdFirst;
    // ... and on few lanes of every participating wave when they hold at most 16 rays per wave (sparse_map; RT355_THIN=0: off)
    p.tune.thin = p.tuneConnect.thin = p.tune4.thin = k.thinSet ? k.thin : 16;
    return p;
}

// The three knobs of k_shade's launch, read once per context (rt_create)
struct ShadeKnobs {
    bool tablesSet = false; int tables = 0;   // RT355_SHADE_TABLES; 0: k_shade reads lights and materials from global memory (A/B runs)
    int tile = 0;                             // RT355_SHADE_TILE: 256 or 512, else 0
    int perCU = 0;                            // RT355_SHADE_PER_CU: 1..16, else 0 (tuning / over-subscription tests)
};
static inline ShadeKnobs read_shade_knobs()
{
    ShadeKnobs k;
    if (const char* t = getenv("RT355_SHADE_TABLES")) { k.tables = atoi(t) != 0; k.tablesSet = true; }
    if (const char* t = getenv("RT355_SHADE_TILE")) { const int v = atoi(t); if (v == 256 || v == 512) k.tile = v; }
    if (const char* t = getenv("RT355_SHADE_PER_CU")) { const int v = atoi(t); if (v > 0 && v <= 16) k.perCU = v; }
    return k;
}

} // namespace rt355dev

// build_cores.h — the GPU BLAS builders as cores that work on device-resident arrays (sah.hip, lbvh.hip, sbvh.hip).  rt_build_bvh2_sah and
// rt_build_bvh2 wrap them (allocate, upload, core, download); rt_rebuild_scene (scene.hip) runs them BLAS by BLAS straight into a
// scene's device arrays.  The driver side the three files share (error reporting, the per-call session, the wrappers' common tail)
// is build_dev.h; the workgroup fold of the SAH and SBVH level kernels is fold_dev.h.
//
// A core builds the BLAS over dPrims[0, n) - the primitives [first, first + n) of the scene, `first` is added to the ids it writes to
// dIdx[0, n) - with its root at node id nodeBase and its leaves indexing primIdx from idxBase; dNodes[0, 2n - 1) receives the records
// (dNodes[0] is node nodeBase).  `work` holds work_bytes(n) bytes.  The caller has checked the arguments (check_args of the builder's
// *_common.h) and set the device; everything is queued on `stream`, which is idle when the core returns.  evBegin / evEnd (may be
// NULL) bracket the kernels.  `who` prefixes the messages of rt_last_error().  Returns RT_OK or RT_E_* (dNodes / dIdx may then hold
// partial results: they are the caller's scratch until a build has succeeded).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/rt355.h"
#include "lbvh_common.h"

struct Built {
    uint32_t nodes, leaves, depth;   // records written (2 * leaves - 1), leaves, height in edges (BVH2::Depth)
    uint32_t mortonBits, levels;     // linear builder: bits per axis; SAH: level passes
    float cost;                      // BVH2::TotalCost
    float ms[3];                     // SAH: wall-clock of the primitive pass, the level passes, numbering and emit
};

namespace sahdev {
using ::Built;
// the argument checks of rt_build_bvh2_sah for a build into arrays of 2 * count - 1 nodes and count indices (NULL: fine)
const char* check_args(int32_t nPrims, int32_t first, int32_t count, uint32_t nodeBase, uint32_t idxBase);
int work_bytes(const char* who, uint32_t n, hipStream_t stream, size_t* bytes);
int build(const char* who, hipStream_t stream, void* work, const RtPrimitive* dPrims, uint32_t n, uint32_t first, uint32_t nodeBase,
          uint32_t idxBase, RtBVHNode2* dNodes, uint32_t* dIdx, hipEvent_t evBegin, hipEvent_t evEnd, Built* out);
}
namespace lbvhdev {
using ::Built;
// the argument checks of rt_build_bvh2 likewise; P receives the options (opts NULL: the defaults)
const char* check_args(const RtBuildOptions* opts, int32_t nPrims, int32_t first, int32_t count, uint32_t nodeBase, uint32_t idxBase, lbvh::Params& P);
int work_bytes(const char* who, uint32_t n, hipStream_t stream, size_t* bytes);
int build(const char* who, hipStream_t stream, void* work, const lbvh::Params& P, const RtPrimitive* dPrims, uint32_t n, uint32_t first,
          uint32_t nodeBase, uint32_t idxBase, RtBVHNode2* dNodes, uint32_t* dIdx, hipEvent_t evBegin, hipEvent_t evEnd, Built* out);
}

// The SBVH builder (sbvh.hip, rules in sbvh_common.h).  A spatial split duplicates refs, so the size of the tree is known only after
// it is built: build() leaves the numbered tree on the device (its own allocations, grown level by level; RT_E_NOMEM when one fails)
// and reports the sizes, emit() then writes the records and primIdx into arrays of built.nodes / built.nIdx entries.  This is the
// shape an in-place rebuild with an SBVH builder needs (size, then place): rt_rebuild_scene builds, grows the scene's arrays to the
// sizes if it must, emits and destroys, BLAS by BLAS.  The caller has checked the arguments (sbvh::check_args) and set the device;
// *tree is set whenever build() got that far and is destroyed by the caller, after a failure too.  The stream is idle when either
// returns.  `pool` (may be NULL: hipMalloc / hipFree) keeps the device blocks of a build for the next one: a caller that builds the
// same sizes again allocates nothing; one pool serves one stream, and outlives every tree built from it.
struct SbvhBuilt {
    uint32_t nodes, leaves, nIdx, depth;                     // records, leaves, primIdx entries, BVH2::Depth
    uint32_t spatialSplits, primsClipped, forcedLeaves;      // as BVH2::stat_* count them
    uint32_t levels, peakRefs;                               // level passes; most refs alive in one level
    float cost;                                              // BVH2::TotalCost
    float ms[3];                                             // wall-clock of the primitive pass, the level passes, the numbering
};
namespace sbvhdev {
struct Tree;
struct Pool;
Pool* pool_create();
void pool_destroy(Pool* pool);
uint64_t pool_allocations(const Pool* pool);                 // hipMalloc calls so far
int build(const char* who, hipStream_t stream, float alpha, const RtPrimitive* dPrims, uint32_t n, uint32_t first, uint32_t nodeBase,
          uint32_t idxBase, hipEvent_t evBegin, hipEvent_t evEnd, Pool* pool, Tree** tree, SbvhBuilt* out);
int emit(const char* who, hipStream_t stream, Tree* tree, RtBVHNode2* dNodes, uint32_t* dIdx);
void destroy(Tree* tree);
}

// collapse_dev.h — the interface between the callers of the GPU BVH2 -> BVH4 collapse (rt_build_bvh4 in collapse.hip, scene.hip's upload
// and rebuild of a BVH4 copy) and collapse.hip's kernels.  Everything works on device arrays, on the caller's stream.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/rt355.h"
#include "collapse_common.h"

namespace collapsedev {

constexpr uint32_t kMaxLevels = collapse::kMaxLevels;
// the counter words (Work::ctr): frontier sizes and first live ids per level, then the status words the host reads together
constexpr uint32_t kCnt = 0, kBase = kMaxLevels + 2, kStatus = 2 * (kMaxLevels + 2);
constexpr uint32_t kWalkWord = kStatus, kLive = kStatus + 1, kLevels = kStatus + 2, kNeed = kStatus + 3, kLeaf = kStatus + 4, kLeafAny = kStatus + 5;
constexpr uint32_t kChanged = kStatus + 6;   // refit_records: live records whose slots differ from the bound ones (a count, not a position)
constexpr uint32_t kStatusWords = 7, kCtrWords = kStatus + kStatusWords;
constexpr uint32_t kWalk = 1;   // status bit: a frontier overflow, a child out of range, more live nodes than capacity

// Scratch of a collapse of trees with nNodes nodes in all whose largest BLAS has frontCap interior nodes (at least 1): frontA / frontB
// frontCap entries (node, stack base), flags / ranks / kids 4 * frontCap words, newId nNodes words, quadNode quadCap words (live id ->
// node; quadCap bounds the live nodes: interior nodes + BLAS), ctr kCtrWords words, scan: scan_bytes(4 * frontCap).
struct Work {
    uint2 *frontA, *frontB; uint32_t frontCap;
    uint32_t *flags, *ranks, *kids, *newId, *quadNode; uint32_t quadCap;
    uint32_t* ctr; void* scan; size_t scanBytes;
};

hipError_t scan_bytes(uint32_t items, hipStream_t s, size_t* bytes);
// zeroes the counters, then writes Convert's record of every BVH2 node into bvh4[0, nNodes)
hipError_t begin(hipStream_t s, const Work& w, const RtBVHNode2* nodes, uint32_t nNodes, RtBVHNode4* bvh4);
// collapses the BLAS at `root` (BVH2 height `height`, `interiors` interior nodes), live ids continuing where the last BLAS ended
hipError_t collapse_blas(hipStream_t s, const Work& w, const RtBVHNode2* nodes, uint32_t nNodes, uint32_t root, uint32_t interiors, uint32_t height,
                         RtBVHNode4* bvh4);
// The in-place collapse of a refit BVH2 (after begin): the final record of every one of the nLive live nodes of the bound collapse
// (quadNode: live id -> node) from the refit `nodes` into bvh4, and into the status words how many of them differ in a slot (first,
// count) from `bound4` (kChanged), the live count (kLive) and the largest live leaf (kLeaf).  kChanged == 0: bvh4 is the collapse of
// `nodes`, with the bound live ids, stack need and quadNode / newId tables; otherwise collapse_blas has to run (after begin again).
hipError_t refit_records(hipStream_t s, const Work& w, const RtBVHNode2* nodes, uint32_t nNodes, const RtBVHNode4* bound4, const uint32_t* quadNode,
                         uint32_t nLive, RtBVHNode4* bvh4);
// layout 1 (quads != NULL): the quad records of the live nodes and rootEntry[b] = the live id of roots[b * rootStride] (a uint32 array:
// stride 1; RtBVHInstance records: stride 17)
hipError_t finish(hipStream_t s, const Work& w, const RtBVHNode4* bvh4, uint32_t nNodes, uint32_t nIdx, const uint32_t* roots, uint32_t rootStride,
                  uint32_t nRoots, RtFloat4* quads, uint32_t* rootEntry);

} // namespace collapsedev

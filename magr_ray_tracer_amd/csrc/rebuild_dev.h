// rebuild_dev.h — the interface between scene.hip's rebuild_scene (rt_rebuild_scene) and rebuild.hip's kernels.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/rt355.h"

namespace rebuilddev {

constexpr uint32_t kMaxLevels = RT_BVH4_STACK;     // a BLAS deeper than the traversal stack is refused before it is numbered
// the counter words (Work::ctr): frontier sizes and first pair ids per level, then the status words the host reads
constexpr uint32_t kCnt = 0, kBase = kMaxLevels + 2, kStatus = 2 * (kMaxLevels + 2), kLargestLeaf = kStatus + 1, kCtrWords = kStatus + 2;
constexpr uint32_t kWalk = 1;                      // status bit: the walk did not end where the builder said (an inconsistent tree)

// scratch of the derivation, sized for trees of N nodes in all (scene.hip grows it with the trees): flags / ranks / newId N words,
// frontA / frontB frontCap (>= the interior nodes, N / 2) words, ctr kCtrWords words, scan: scan_bytes(N)
struct Work { uint32_t *flags, *ranks, *newId, *frontA, *frontB, *ctr; uint32_t frontCap; void* scan; size_t scanBytes; };

hipError_t scan_bytes(uint32_t items, hipStream_t s, size_t* bytes);
// zeroes the counters and clears the parent links of nodes [0, nNodes)
hipError_t begin(hipStream_t s, const Work& w, uint32_t* parent, uint32_t nNodes);
// numbers the interior nodes of the BLAS at `root` (height `depth`, `interiors` interior nodes) from pair id pairBase on: newId,
// pairNode, parent links
hipError_t number_blas(hipStream_t s, const Work& w, const RtBVHNode2* nodes, uint32_t nNodes, uint32_t root, uint32_t interiors, uint32_t depth,
                       uint32_t pairBase, uint32_t pairCap, uint32_t* pairNode, uint32_t* parent);
// the leaf list, and (pairs != NULL: layout 1) the pair records and the instances' root entries
hipError_t finish(hipStream_t s, const Work& w, const RtBVHNode2* nodes, uint32_t nNodes, uint32_t nPairs, uint32_t nLeaves, const RtBVHInstance* inst,
                  uint32_t nInst, const uint32_t* pairNode, RtFloat4* pairs, uint32_t* rootEntry, uint32_t* leaves);

// rt_resize_scene (rules: resize_common.h), over the nPrims new primitives already copied into a set that is not live:
// resize_check: k_resize_check writes per primitive the packed (objType, matIdx) pair the host keeps as its shadow and the light flag
//   (w.flags), puts the lowest index whose objType / matIdx is out of range into *bad (atomicMin: a value, never a position; kNoBad when
//   none), and the flags are ranked by an exclusive scan (w.ranks); w.flags / w.ranks must hold nPrims words
// light_emit: k_light_emit scatters lights[rank] = i and writes the complete 8-row light record at that rank; positions come from the
//   scan alone
hipError_t resize_check(hipStream_t s, const Work& w, const RtPrimitive* prims, uint32_t nPrims, const RtMaterial* mats, int32_t nMats, int2* packed,
                        uint32_t* bad);
hipError_t light_emit(hipStream_t s, const Work& w, const RtPrimitive* prims, uint32_t nPrims, const RtMaterial* mats, uint32_t nLights, uint32_t* lights,
                      RtFloat4* lightRecs);


// rt_update_materials (rules: resize_common.h), over the bound primitives.  assign (NULL: none) holds the new matIdx of primitives
// [first, first + count); every other primitive keeps its own (resize::new_mat: the one source of all three kernels).
// mat_flags: k_mat_flags writes per primitive the light flag under the table mats[nMats] (w.flags) and puts the lowest index whose matIdx
//   lies outside that table into *bad (atomicMin: a value, never a position; kNoBad when none); an exclusive scan ranks the flags (w.ranks)
// mat_emit: k_mat_emit scatters lights[rank] = i and writes the complete 8-row light record at that rank
// mat_assign (the commit, on live arrays): k_mat_assign writes prims[i].matIdx and shadeRecs[i] (refit::shade_rec of the patched record)
hipError_t mat_flags(hipStream_t s, const Work& w, const RtPrimitive* prims, uint32_t nPrims, const int32_t* assign, uint32_t first, uint32_t count,
                     const RtMaterial* mats, int32_t nMats, uint32_t* bad);
hipError_t mat_emit(hipStream_t s, const Work& w, const RtPrimitive* prims, uint32_t nPrims, const int32_t* assign, uint32_t first, uint32_t count,
                    const RtMaterial* mats, uint32_t nLights, uint32_t* lights, RtFloat4* lightRecs);
hipError_t mat_assign(hipStream_t s, RtPrimitive* prims, const int32_t* assign, uint32_t first, uint32_t count, RtFloat4* shadeRecs);

// rt_rebuild_ranges: one segment of kept nodes - src[0, nNodes) of the live array to dst[0, nNodes) of the set that is not live, every
// interior record's `first` moved by nodeDelta, every leaf's by idxDelta (rebuild::relocated_first; both modulo 2^32).  The caller merges
// adjacent kept BLAS with equal deltas into one segment and launches once per segment: after merging a plan has as many segments as
// runs of kept BLAS between built ones (one or two where one mesh moves beside a static one), so a launch each costs less than
// uploading a segment table and searching it in every thread, and the deltas stay wave-uniform kernel arguments.  Both deltas zero (the
// static mesh in front of the moving one): a plain device-to-device copy.
hipError_t relocate(hipStream_t s, const RtBVHNode2* src, RtBVHNode2* dst, uint32_t nNodes, uint32_t nodeDelta, uint32_t idxDelta);
// ... and what is derived from it.  relocate_pairs: the BLAS's run of nPairs pair records, src of the live array to dst of the set that is
// not live, the entries moved by rebuild::relocated_entry (both deltas zero: a plain copy).  relocate_ids: its parent links (nNodes
// words), its run of pair id -> node id (nPairs words; 0 in layout 0) and its run of leaves, every id + nodeDelta, kNone kept.
hipError_t relocate_pairs(hipStream_t s, const RtFloat4* src, RtFloat4* dst, uint32_t nPairs, uint32_t pairDelta, uint32_t idxDelta);
hipError_t relocate_ids(hipStream_t s, const uint32_t* parentSrc, uint32_t* parentDst, uint32_t nNodes, const uint32_t* pairNodeSrc, uint32_t* pairNodeDst,
                        uint32_t nPairs, const uint32_t* leavesSrc, uint32_t* leavesDst, uint32_t nLeaves, uint32_t nodeDelta);
// finish() for one built BLAS beside kept or refit ones: the leaves of the block [root, root + nBlasNodes) in node order into leafRun
// (its place in the leaf list), and (pairs != NULL) its `interiors` pair records from pair id pairBase on; number_blas has run for it
hipError_t finish_blas(hipStream_t s, const Work& w, const RtBVHNode2* nodes, uint32_t root, uint32_t nBlasNodes, uint32_t pairBase, uint32_t interiors,
                       const uint32_t* pairNode, RtFloat4* pairs, uint32_t* leafRun);

} // namespace rebuilddev

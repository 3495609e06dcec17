// rebuild.hip — what rt_upload_scene derives from a BVH2 on the host, derived on the device (rt_rebuild_scene, include/rt355.h;
// driven by rt355.hip).  The rules are rebuild_common.h's and refit_common.h's, which the upload path and the host restatement share.
//
// Pair ids are positions in a breadth-first walk, so they are produced level by level.  Per BLAS and level l (frontier: the interior
// nodes of that level, left to right; cnt[l] of them, the first has pair id base[l]):
//   k_rb_frontier   one thread per frontier node: its pair id (newId, pairNode), its children's parent links, and a flag per child
//                   that is an interior node; hipcub::DeviceScan ranks the flags
//   k_rb_next       writes the flagged children to the next frontier at their ranks; cnt[l + 1], base[l + 1]
// The host knows each tree's height and interior count from the builder, so it launches the levels without reading anything back;
// the last level checks that the walk ended where the builder said (status).  Every position comes from a scan: no atomic decides
// where anything is written, two runs give the same arrays.  Then, over all BLAS:
//   k_rb_pairs      one thread per pair id: the pair record (refit::pair_boxes + rebuild::pair_entries, what rebuild::pair_record packs)
//   k_rb_leaf_flag / k_rb_leaf_list   the leaves (refit topology) in node order, by a scan; the largest leaf (status)
//   k_rb_roots      one thread per instance: the packed entry of its BLAS root
// rt_resize_scene adds, over the new primitive array (rules: resize_common.h):
//   k_resize_check  one thread per primitive: objType / matIdx in range (the lowest refused index through atomicMin), the packed pair the
//                   host keeps as its shadow, the light flag; a scan ranks the flags
//   k_light_emit    one thread per primitive: a light writes its index and its complete light record at its rank
// rt_update_materials runs the same pipeline over the bound primitives under a new table and a new assignment of matIdx values:
//   k_mat_flags     one thread per primitive: its matIdx afterwards (resize::new_mat) in range of the new table (the lowest refused index
//                   through atomicMin), the light flag; a scan ranks the flags
//   k_mat_emit      k_light_emit with that matIdx
//   k_mat_assign    the commit, one thread per primitive of the range: matIdx and the shade record of the patched primitive
// rt_rebuild_ranges keeps the bound tree of a BLAS whose primitives did not change:
//   k_blas_relocate one thread per 16-byte vector of a kept block of nodes: copied to where the new scene numbers it, the `first` word
//                   of every record moved by the block's node or index offset (rebuild::relocated_first)
// ... and moves what is derived from it, so that nothing walks a kept or refit tree:
//   k_pairs_relocate one thread per 16-byte vector of the BLAS's run of pair records: the three box vectors copied, both entries of the
//                   fourth moved by the index or the pair-id offset (rebuild::relocated_entry)
//   k_ids_relocate  one thread per word of the BLAS's parent links, its run of pair id -> node id and its run of leaves: + the node
//                   offset (kNone, a root's parent, stays)
#include <algorithm>
#include <cstddef>
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>
#include "../../include/rt355.h"
#include "rebuild_common.h"
#include "rebuild_dev.h"
#include "resize_common.h"

namespace rebuilddev {

using namespace rebuild;

constexpr int kBlock = 256;

__global__ void __launch_bounds__(64) k_rb_begin(const RtBVHNode2* nodes, uint32_t root, uint32_t pairBase, uint32_t* front, uint32_t* ctr)
{
    if (threadIdx.x != 0) return;
    const bool interior = nodes[root].count == 0;
    front[0] = root;
    ctr[kCnt + 0] = interior ? 1u : 0u;
    ctr[kBase + 0] = pairBase;
}

__global__ void __launch_bounds__(kBlock) k_rb_frontier(const RtBVHNode2* nodes, uint32_t nNodes, const uint32_t* front, uint32_t ub, uint32_t level,
                                                        uint32_t pairCap, uint32_t* newId, uint32_t* pairNode, uint32_t* parent, uint32_t* flags,
                                                        uint32_t* ctr)
{
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= ub) return;
    uint32_t f0 = 0, f1 = 0;
    if (i < ctr[kCnt + level]) {
        const uint32_t node = front[i], id = ctr[kBase + level] + i;
        const uint32_t c = node < nNodes ? nodes[node].first : nNodes;   // (both tests below: c + 1 wraps for c = 0xffffffff)
        if (id >= pairCap || c >= nNodes || c + 1 >= nNodes) atomicOr(&ctr[kStatus], kWalk);
        else {
            newId[node] = id; pairNode[id] = node;
            parent[c] = node; parent[c + 1] = node;
            f0 = nodes[c].count == 0 ? 1u : 0u;
            f1 = nodes[c + 1].count == 0 ? 1u : 0u;
        }
    }
    flags[2 * i] = f0; flags[2 * i + 1] = f1;
}

// expectEnd != kNone: this is the tree's last level with interior nodes; the walk must end here, at that pair id
__global__ void __launch_bounds__(kBlock) k_rb_next(const RtBVHNode2* nodes, const uint32_t* front, uint32_t ub, uint32_t level, const uint32_t* flags,
                                                    const uint32_t* ranks, uint32_t* next, uint32_t nextCap, uint32_t expectEnd, uint32_t* ctr)
{
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= ub) return;
    const uint32_t cnt = ctr[kCnt + level];
    if (i == 0) {
        const uint32_t n = ranks[2 * ub - 1] + flags[2 * ub - 1], end = ctr[kBase + level] + cnt;
        ctr[kCnt + level + 1] = n; ctr[kBase + level + 1] = end;
        if (cnt > ub || n > nextCap) atomicOr(&ctr[kStatus], kWalk);
        if (expectEnd != kNone && (n != 0 || end != expectEnd)) atomicOr(&ctr[kStatus], kWalk);
    }
    if (i >= cnt) return;
    const uint32_t c = nodes[front[i]].first;
    for (uint32_t k = 0; k < 2; k++)
        if (flags[2 * i + k]) { const uint32_t r = ranks[2 * i + k]; if (r < nextCap) next[r] = c + k; }
}

__global__ void __launch_bounds__(kBlock) k_rb_pairs(const RtBVHNode2* nodes, const uint32_t* pairNode, const uint32_t* newId, uint32_t nPairs,
                                                     RtFloat4* pairs)
{
    const uint32_t k = blockIdx.x * kBlock + threadIdx.x;
    if (k >= nPairs) return;
    const uint32_t node = pairNode[k], c = nodes[node].first;
    RtFloat4 r[3];
    uint32_t e[2];
    refit::pair_boxes(nodes[c], nodes[c + 1], r);
    pair_entries(nodes, node, newId, e);
    for (int w = 0; w < 3; w++) pairs[(size_t)k * 4 + w] = r[w];
    *reinterpret_cast<uint4*>(&pairs[(size_t)k * 4 + 3]) = make_uint4(e[0], e[1], 0u, 0u);   // (pair_record's fourth word, as bits)
}

__global__ void __launch_bounds__(kBlock) k_rb_leaf_flag(const RtBVHNode2* nodes, uint32_t nNodes, uint32_t* flags, uint32_t* ctr)
{
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= nNodes) return;
    const uint32_t c = nodes[i].count;
    flags[i] = c > 0 ? 1u : 0u;
    if (c > kMaxPackedLeaf) atomicMax(&ctr[kLargestLeaf], c);   // a value, not a position
}
// (nodeBase: the id of node 0 of the nNodes flagged - 0 over a whole scene, a BLAS's root over its block)
__global__ void __launch_bounds__(kBlock) k_rb_leaf_list(const uint32_t* flags, const uint32_t* ranks, uint32_t nNodes, uint32_t nLeaves,
                                                         uint32_t nodeBase, uint32_t* leaves, uint32_t* ctr)
{
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= nNodes) return;
    if (i == nNodes - 1 && ranks[i] + flags[i] != nLeaves) atomicOr(&ctr[kStatus], kWalk);
    if (flags[i] && ranks[i] < nLeaves) leaves[ranks[i]] = nodeBase + i;
}

__global__ void __launch_bounds__(kBlock) k_rb_roots(const RtBVHNode2* nodes, const RtBVHInstance* inst, uint32_t nInst, const uint32_t* newId,
                                                     uint32_t* rootEntry)
{
    const uint32_t b = blockIdx.x * kBlock + threadIdx.x;
    if (b >= nInst) return;
    const uint32_t root = inst[b].bvhIdx;
    rootEntry[b] = child_entry(nodes[root], nodes[root].count > 0 ? 0u : newId[root]);
}

static dim3 grid(uint32_t n) { return dim3((unsigned)((n + kBlock - 1) / kBlock)); }

hipError_t scan_bytes(uint32_t items, hipStream_t s, size_t* bytes)
{
    *bytes = 0;
    return hipcub::DeviceScan::ExclusiveSum(nullptr, *bytes, (uint32_t*)nullptr, (uint32_t*)nullptr, (int)items, s);
}

hipError_t begin(hipStream_t s, const Work& w, uint32_t* parent, uint32_t nNodes)
{
    hipError_t e = hipMemsetAsync(w.ctr, 0, sizeof(uint32_t) * kCtrWords, s);
    if (e != hipSuccess) return e;
    return hipMemsetAsync(parent, 0xff, sizeof(uint32_t) * nNodes, s);   // roots keep kNone
}

hipError_t number_blas(hipStream_t s, const Work& w, const RtBVHNode2* nodes, uint32_t nNodes, uint32_t root, uint32_t interiors, uint32_t depth,
                       uint32_t pairBase, uint32_t pairCap, uint32_t* pairNode, uint32_t* parent)
{
    if (depth > kMaxLevels) return hipErrorInvalidValue;
    uint32_t *front = w.frontA, *next = w.frontB;
    size_t scanBytes = w.scanBytes;
    if (depth > 0 && interiors == 0) return hipErrorInvalidValue;   // (the caller has checked the builder's result)
    hipLaunchKernelGGL(k_rb_begin, dim3(1), dim3(64), 0, s, nodes, root, pairBase, front, w.ctr);
    for (uint32_t l = 0; l < depth; l++) {
        const uint64_t full = l < 31 ? (1ull << l) : (1ull << 31);
        const uint32_t ub = (uint32_t)(full < interiors ? full : interiors);
        hipLaunchKernelGGL(k_rb_frontier, grid(ub), dim3(kBlock), 0, s, nodes, nNodes, front, ub, l, pairCap, w.newId, pairNode, parent, w.flags, w.ctr);
        hipError_t e = hipcub::DeviceScan::ExclusiveSum(w.scan, scanBytes, w.flags, w.ranks, (int)(2 * ub), s);
        if (e != hipSuccess) return e;
        hipLaunchKernelGGL(k_rb_next, grid(ub), dim3(kBlock), 0, s, nodes, front, ub, l, w.flags, w.ranks, next, w.frontCap,
                           l + 1 == depth ? pairBase + interiors : kNone, w.ctr);
        uint32_t* t = front; front = next; next = t;
    }
    return hipGetLastError();
}

hipError_t finish(hipStream_t s, const Work& w, const RtBVHNode2* nodes, uint32_t nNodes, uint32_t nPairs, uint32_t nLeaves, const RtBVHInstance* inst,
                  uint32_t nInst, const uint32_t* pairNode, RtFloat4* pairs, uint32_t* rootEntry, uint32_t* leaves)
{
    hipLaunchKernelGGL(k_rb_leaf_flag, grid(nNodes), dim3(kBlock), 0, s, nodes, nNodes, w.flags, w.ctr);
    size_t scanBytes = w.scanBytes;
    hipError_t e = hipcub::DeviceScan::ExclusiveSum(w.scan, scanBytes, w.flags, w.ranks, (int)nNodes, s);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_rb_leaf_list, grid(nNodes), dim3(kBlock), 0, s, w.flags, w.ranks, nNodes, nLeaves, 0u, leaves, w.ctr);
    if (pairs) {
        if (nPairs) hipLaunchKernelGGL(k_rb_pairs, grid(nPairs), dim3(kBlock), 0, s, nodes, pairNode, w.newId, nPairs, pairs);
        hipLaunchKernelGGL(k_rb_roots, grid(nInst), dim3(kBlock), 0, s, nodes, inst, nInst, w.newId, rootEntry);
    }
    return hipGetLastError();
}

// One built BLAS among kept or refit ones: its leaves (node order) at their place in the leaf list, its pair records at its run of pair ids
hipError_t finish_blas(hipStream_t s, const Work& w, const RtBVHNode2* nodes, uint32_t root, uint32_t nBlasNodes, uint32_t pairBase, uint32_t interiors,
                       const uint32_t* pairNode, RtFloat4* pairs, uint32_t* leafRun)
{
    const uint32_t nLeaves = nBlasNodes - interiors;
    hipLaunchKernelGGL(k_rb_leaf_flag, grid(nBlasNodes), dim3(kBlock), 0, s, nodes + root, nBlasNodes, w.flags, w.ctr);
    size_t scanBytes = w.scanBytes;
    hipError_t e = hipcub::DeviceScan::ExclusiveSum(w.scan, scanBytes, w.flags, w.ranks, (int)nBlasNodes, s);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_rb_leaf_list, grid(nBlasNodes), dim3(kBlock), 0, s, w.flags, w.ranks, nBlasNodes, nLeaves, root, leafRun, w.ctr);
    if (pairs && interiors)
        hipLaunchKernelGGL(k_rb_pairs, grid(interiors), dim3(kBlock), 0, s, nodes, pairNode + pairBase, w.newId, interiors, pairs + (size_t)pairBase * 4);
    return hipGetLastError();
}

// ---- rt_resize_scene: the new primitives' checks, the light list and the light records (rules: resize_common.h) -------------------------
__global__ void __launch_bounds__(kBlock) k_resize_check(const RtPrimitive* prims, uint32_t nPrims, const RtMaterial* mats, int32_t nMats, int2* packed,
                                                         uint32_t* flags, uint32_t* bad)
{
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= nPrims) return;
    const int32_t type = prims[i].objType, mat = prims[i].matIdx;
    const bool ok = resize::prim_ok(type, mat, nMats);
    packed[i] = make_int2(type, mat);
    flags[i] = ok ? resize::light_flag(mats, mat) : 0u;   // (a refused record's material is never read)
    if (!ok) atomicMin(bad, i);   // a value, not a position
}
__global__ void __launch_bounds__(kBlock) k_light_emit(const RtPrimitive* prims, uint32_t nPrims, const RtMaterial* mats, const uint32_t* flags,
                                                       const uint32_t* ranks, uint32_t nLights, uint32_t* lights, RtFloat4* lightRecs)
{
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= nPrims || !flags[i]) return;
    const uint32_t r = ranks[i];
    if (r >= nLights) return;   // (the host sized both arrays from this scan: never taken)
    lights[r] = i;
    resize::light_record(prims[i], mats, lightRecs + (size_t)r * 8);   // (straight into the record: no private copy of 128 bytes)
}

hipError_t resize_check(hipStream_t s, const Work& w, const RtPrimitive* prims, uint32_t nPrims, const RtMaterial* mats, int32_t nMats, int2* packed,
                        uint32_t* bad)
{
    hipError_t e = hipMemsetAsync(bad, 0xff, sizeof(uint32_t), s);   // resize::kNoBad
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_resize_check, grid(nPrims), dim3(kBlock), 0, s, prims, nPrims, mats, nMats, packed, w.flags, bad);
    size_t scanBytes = w.scanBytes;
    e = hipcub::DeviceScan::ExclusiveSum(w.scan, scanBytes, w.flags, w.ranks, (int)nPrims, s);
    return e != hipSuccess ? e : hipGetLastError();
}
hipError_t light_emit(hipStream_t s, const Work& w, const RtPrimitive* prims, uint32_t nPrims, const RtMaterial* mats, uint32_t nLights, uint32_t* lights,
                      RtFloat4* lightRecs)
{
    if (nLights == 0) return hipMemsetAsync(lightRecs, 0, sizeof(RtFloat4) * 8, s);   // one zero record, as at upload
    hipLaunchKernelGGL(k_light_emit, grid(nPrims), dim3(kBlock), 0, s, prims, nPrims, mats, w.flags, w.ranks, nLights, lights, lightRecs);
    return hipGetLastError();
}

// ---- rt_update_materials: the light flags, the light list and the light records under a new table and a new assignment; the commit's
// patch of the live primitives (rules: resize_common.h) -------------------------------------------------------------------------------
__global__ void __launch_bounds__(kBlock) k_mat_flags(const RtPrimitive* prims, uint32_t nPrims, const int32_t* assign, uint32_t first, uint32_t count,
                                                      const RtMaterial* mats, int32_t nMats, uint32_t* flags, uint32_t* bad)
{
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= nPrims) return;
    const int32_t mat = resize::new_mat(prims, i, assign, first, count);
    const bool ok = mat >= 0 && mat < nMats;
    flags[i] = ok ? resize::light_flag(mats, mat) : 0u;   // (a refused value's material is never read)
    if (!ok) atomicMin(bad, i);   // a value, not a position
}
__global__ void __launch_bounds__(kBlock) k_mat_emit(const RtPrimitive* prims, uint32_t nPrims, const int32_t* assign, uint32_t first, uint32_t count,
                                                     const RtMaterial* mats, const uint32_t* flags, const uint32_t* ranks, uint32_t nLights,
                                                     uint32_t* lights, RtFloat4* lightRecs)
{
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= nPrims || !flags[i]) return;   // (a flag is set only where the matIdx passed k_mat_flags' check)
    const uint32_t r = ranks[i];
    if (r >= nLights) return;   // (the host sized both arrays from this scan: never taken)
    lights[r] = i;
    resize::light_record_as(prims[i], resize::new_mat(prims, i, assign, first, count), mats, lightRecs + (size_t)r * 8);
}
__global__ void __launch_bounds__(kBlock) k_mat_assign(RtPrimitive* prims, const int32_t* assign, uint32_t first, uint32_t count, RtFloat4* shadeRecs)
{
    const uint32_t k = blockIdx.x * kBlock + threadIdx.x;
    if (k >= count) return;
    RtPrimitive& p = prims[first + k];
    p.matIdx = assign[k];
    shadeRecs[first + k] = refit::shade_rec(p);   // the one rule, of the patched record
}

hipError_t mat_flags(hipStream_t s, const Work& w, const RtPrimitive* prims, uint32_t nPrims, const int32_t* assign, uint32_t first, uint32_t count,
                     const RtMaterial* mats, int32_t nMats, uint32_t* bad)
{
    hipError_t e = hipMemsetAsync(bad, 0xff, sizeof(uint32_t), s);   // resize::kNoBad
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_mat_flags, grid(nPrims), dim3(kBlock), 0, s, prims, nPrims, assign, first, count, mats, nMats, w.flags, bad);
    size_t scanBytes = w.scanBytes;
    e = hipcub::DeviceScan::ExclusiveSum(w.scan, scanBytes, w.flags, w.ranks, (int)nPrims, s);
    return e != hipSuccess ? e : hipGetLastError();
}
hipError_t mat_emit(hipStream_t s, const Work& w, const RtPrimitive* prims, uint32_t nPrims, const int32_t* assign, uint32_t first, uint32_t count,
                    const RtMaterial* mats, uint32_t nLights, uint32_t* lights, RtFloat4* lightRecs)
{
    if (nLights == 0) return hipMemsetAsync(lightRecs, 0, sizeof(RtFloat4) * 8, s);   // one zero record, as at upload
    hipLaunchKernelGGL(k_mat_emit, grid(nPrims), dim3(kBlock), 0, s, prims, nPrims, assign, first, count, mats, w.flags, w.ranks, nLights, lights, lightRecs);
    return hipGetLastError();
}
hipError_t mat_assign(hipStream_t s, RtPrimitive* prims, const int32_t* assign, uint32_t first, uint32_t count, RtFloat4* shadeRecs)
{
    if (count == 0) return hipSuccess;
    hipLaunchKernelGGL(k_mat_assign, grid(count), dim3(kBlock), 0, s, prims, assign, first, count, shadeRecs);
    return hipGetLastError();
}

// ---- rt_rebuild_ranges: a kept BLAS moves as a block (rule: rebuild::relocated_first) ---------------------------------------------------
// An RtBVHNode2 is 48 bytes, three 16-byte vectors: two of box, then {first, count, pad, pad}.  One thread per VECTOR, grid-stride: lane l
// of a wave reads and writes the 16 bytes right behind lane l - 1's, so every load and every store of a wave covers 1 KiB of consecutive
// memory (a thread per node would stride its three accesses by 48 bytes).  Every third vector gets the add to its first word; nothing
// else is computed, no LDS, no atomics.  src is the live array, dst the set that is not live: they never alias.
constexpr uint32_t kRelocateMaxBlocks = 2048;   // 256 CUs x 8 workgroups of 256 threads fill the device; larger blocks loop
__global__ void __launch_bounds__(kBlock) k_blas_relocate(const uint4* __restrict__ src, uint4* __restrict__ dst, uint32_t nVec, uint32_t nodeDelta,
                                                          uint32_t idxDelta)
{
    const uint32_t stride = gridDim.x * kBlock;
    for (uint32_t v = blockIdx.x * kBlock + threadIdx.x; v < nVec; v += stride) {
        uint4 q = src[v];
        if (v % 3u == 2u) q.x = relocated_first(q.x, q.y, nodeDelta, idxDelta);
        dst[v] = q;
    }
}
hipError_t relocate(hipStream_t s, const RtBVHNode2* src, RtBVHNode2* dst, uint32_t nNodes, uint32_t nodeDelta, uint32_t idxDelta)
{
    static_assert(sizeof(RtBVHNode2) == 48 && offsetof(RtBVHNode2, first) == 32 && offsetof(RtBVHNode2, count) == 36, "k_blas_relocate's vectors");
    if (nNodes == 0) return hipSuccess;
    if (nNodes > 0x7fffffffu / 3u) return hipErrorInvalidValue;   // (3 * nNodes vectors are counted in 32 bits: 715 million nodes, 34 GB)
    if (nodeDelta == 0 && idxDelta == 0) return hipMemcpyAsync(dst, src, sizeof(RtBVHNode2) * (size_t)nNodes, hipMemcpyDeviceToDevice, s);
    const uint32_t nVec = 3u * nNodes;
    const uint32_t blocks = std::min<uint32_t>((nVec + kBlock - 1) / kBlock, kRelocateMaxBlocks);
    hipLaunchKernelGGL(k_blas_relocate, dim3(blocks), dim3(kBlock), 0, s, reinterpret_cast<const uint4*>(src), reinterpret_cast<uint4*>(dst), nVec, nodeDelta, idxDelta);
    return hipGetLastError();
}

// ---- ... and so does what is derived from it (rules: rebuild::relocated_entry; ids move by the node offset) ---------------------------------
// A pair record is 64 bytes, four 16-byte vectors: three of boxes, then {entry, entry, 0, 0}.  One thread per VECTOR, grid-stride, as
// k_blas_relocate: every load and every store of a wave covers 1 KiB of consecutive memory.  Every fourth vector gets both entries
// patched; no LDS, no atomics.  src is the live array, dst the set that is not live: they never alias.
__global__ void __launch_bounds__(kBlock) k_pairs_relocate(const uint4* __restrict__ src, uint4* __restrict__ dst, uint32_t nVec, uint32_t pairDelta,
                                                           uint32_t idxDelta)
{
    const uint32_t stride = gridDim.x * kBlock;
    for (uint32_t v = blockIdx.x * kBlock + threadIdx.x; v < nVec; v += stride) {
        uint4 q = src[v];
        if ((v & 3u) == 3u) { q.x = relocated_entry(q.x, pairDelta, idxDelta); q.y = relocated_entry(q.y, pairDelta, idxDelta); }
        dst[v] = q;
    }
}
hipError_t relocate_pairs(hipStream_t s, const RtFloat4* src, RtFloat4* dst, uint32_t nPairs, uint32_t pairDelta, uint32_t idxDelta)
{
    static_assert(sizeof(RtFloat4) == 16, "k_pairs_relocate's vectors");
    if (nPairs == 0) return hipSuccess;
    if (nPairs > 0x7fffffffu / 4u) return hipErrorInvalidValue;   // (4 * nPairs vectors are counted in 32 bits)
    if (pairDelta == 0 && idxDelta == 0) return hipMemcpyAsync(dst, src, sizeof(RtFloat4) * 4 * (size_t)nPairs, hipMemcpyDeviceToDevice, s);
    const uint32_t nVec = 4u * nPairs;
    const uint32_t blocks = std::min<uint32_t>((nVec + kBlock - 1) / kBlock, kRelocateMaxBlocks);
    hipLaunchKernelGGL(k_pairs_relocate, dim3(blocks), dim3(kBlock), 0, s, reinterpret_cast<const uint4*>(src), reinterpret_cast<uint4*>(dst), nVec, pairDelta, idxDelta);
    return hipGetLastError();
}
// The three runs of node ids a BLAS owns, in one launch: thread i takes word i of the runs laid end to end (the run is wave-uniform
// but for the two waves that straddle a boundary)
struct IdRuns { const uint32_t* src[3]; uint32_t* dst[3]; uint32_t end[3]; };   // end: the running sum of the lengths
__global__ void __launch_bounds__(kBlock) k_ids_relocate(IdRuns r, uint32_t nodeDelta)
{
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= r.end[2]) return;
    const int run = i < r.end[0] ? 0 : i < r.end[1] ? 1 : 2;
    const uint32_t at = i - (run == 0 ? 0u : r.end[run - 1]);
    const uint32_t v = r.src[run][at];
    r.dst[run][at] = v == kNone ? kNone : v + nodeDelta;
}
hipError_t relocate_ids(hipStream_t s, const uint32_t* parentSrc, uint32_t* parentDst, uint32_t nNodes, const uint32_t* pairNodeSrc, uint32_t* pairNodeDst,
                        uint32_t nPairs, const uint32_t* leavesSrc, uint32_t* leavesDst, uint32_t nLeaves, uint32_t nodeDelta)
{
    if ((uint64_t)nNodes + nPairs + nLeaves > 0x7fffffffull) return hipErrorInvalidValue;
    IdRuns r{ { parentSrc, pairNodeSrc, leavesSrc }, { parentDst, pairNodeDst, leavesDst }, { nNodes, nNodes + nPairs, nNodes + nPairs + nLeaves } };
    if (r.end[2] == 0) return hipSuccess;
    hipLaunchKernelGGL(k_ids_relocate, grid(r.end[2]), dim3(kBlock), 0, s, r, nodeDelta);
    return hipGetLastError();
}

} // namespace rebuilddev

// refit.hip — the kernels of an in-place scene update (rt_update_scene, include/rt355.h; driven by rt355.hip).  Every value they
// write comes from a rule of refit_common.h, which the upload path and the host restatement (host/refit_host.cpp) share.
//
//   k_refit_nodes   one thread per reachable BLAS leaf: the leaf's box from its primitives, then it climbs towards the root while it
//                   is the second to arrive at a node (agent-scope release / acquire ticket per node, as k_lbvh_bottomup: nobody
//                   waits) and writes union(left, right).  Tickets are zeroed by a memset before each launch.
//   k_tlas_build    one workgroup runs TLAS::Build: instance boxes, then the agglomerative clustering with FindBestMatch as an LDS
//                   argmin keyed on (area, index); writes the TLAS nodes, both pair-record encodings, the instance records and the
//                   depth.  Every loop is bounded; nothing spins.
//   k_pair_boxes, k_tri_recs, k_shade_recs, k_light_recs   the derived records of rt_upload_scene, one thread per record.
#include <hip/hip_runtime.h>
#include "../../include/rt355.h"
#include "refit_common.h"

namespace refitdev {

using namespace refit;

constexpr int kBlock = 256;
constexpr int kMaxTreeHeight = 128;   // a climb never takes more steps (rt_validate_scene: BLAS trees are <= 64 deep)
static_assert(kMaxInstances == kBlock, "k_tlas_build: one instance per thread");

__global__ void __launch_bounds__(kBlock) k_refit_nodes(RtBVHNode2* nodes, const RtPrimitive* prims, const uint32_t* primIdx,
                                                       const uint32_t* leaves, uint32_t nLeaves, const uint32_t* parent, uint32_t* tickets)
{
    const uint32_t k = blockIdx.x * kBlock + threadIdx.x;
    if (k >= nLeaves) return;
    uint32_t node = leaves[k];
    set_box(nodes[node], leaf_box(prims, primIdx, nodes[node].first, nodes[node].count));
    uint32_t p = parent[node];
    for (int step = 0; p != kNone && step < kMaxTreeHeight; step++, p = parent[p]) {
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        if (__hip_atomic_fetch_add(&tickets[p], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == 0) return;
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
        const uint32_t c = nodes[p].first;
        set_box(nodes[p], lbvh::box_union(node_box(nodes[c]), node_box(nodes[c + 1])));
    }
}

struct Best { float area; int idx; };   // idx < 0: no candidate

// FindBestMatch(slot, N, A) of TLAS::Build over the LDS nodes: the smallest union area below RT_REALLYFAR (strict <, so NaN never
// wins), the lowest index among equal areas.  Called by the whole workgroup with uniform arguments; returns the same to every thread.
__device__ int best_match(const RtTLASNode* nd, const int* slot, int N, int A, Best* red)
{
    const int t = threadIdx.x;
    float area = 0.0f; int idx = -1;
    if (t < N && t != A) {
        const RtTLASNode& a = nd[slot[A]]; const RtTLASNode& b = nd[slot[t]];
        const float amn[3] = { a.aabbMin.x, a.aabbMin.y, a.aabbMin.z }, amx[3] = { a.aabbMax.x, a.aabbMax.y, a.aabbMax.z };
        const float bmn[3] = { b.aabbMin.x, b.aabbMin.y, b.aabbMin.z }, bmx[3] = { b.aabbMax.x, b.aabbMax.y, b.aabbMax.z };
        area = tlas_pair_area(amn, amx, bmn, bmx);
        if (area < RT_REALLYFAR) idx = t;
    }
    for (int off = warpSize / 2; off > 0; off >>= 1) {
        const float oa = __shfl_xor(area, off);
        const int oi = __shfl_xor(idx, off);
        if (oi >= 0 && (idx < 0 || oa < area || (!(area < oa) && oi < idx))) { area = oa; idx = oi; }
    }
    const int waves = kBlock / warpSize;
    if ((t % warpSize) == 0) red[t / warpSize] = Best{ area, idx };
    __syncthreads();
    Best r = red[0];
    for (int w = 1; w < waves; w++) {
        const Best o = red[w];
        if (o.idx >= 0 && (r.idx < 0 || o.area < r.area || (!(r.area < o.area) && o.idx < r.idx))) r = o;
    }
    __syncthreads();   // red[] is rewritten by the next call
    return r.idx;
}

// status[0]: 0 ok, 1 a singular transform, 2 the clustering found no partner; status[1]: the TLAS depth (node 0 at depth 0)
__global__ void __launch_bounds__(kBlock) k_tlas_build(const RtBVHNode2* nodes, const RtBVHInstance* inst, int n, const uint32_t* rootEntry,
                                                      RtTLASNode* tlas, RtFloat4* tp, RtFloat4* tpP, RtFloat4* ir, int32_t* status)
{
    __shared__ RtTLASNode nd[2 * kMaxInstances];
    __shared__ uint32_t height[2 * kMaxInstances];
    __shared__ int slot[kMaxInstances];
    __shared__ Best red[kBlock / 64];
    __shared__ int bad;
    const int t = threadIdx.x, nNodes = 2 * n;
    if (t == 0) bad = 0;
    for (int i = t; i < nNodes; i += kBlock) { nd[i] = RtTLASNode{}; height[i] = 0; }
    __syncthreads();
    if (t < n) {
        const RtBVHNode2& root = nodes[inst[t].bvhIdx];
        RtTLASNode& leaf = nd[1 + t];
        if (is_identity(inst[t].invT)) { leaf.aabbMin = root.aabbMin; leaf.aabbMax = root.aabbMax; }   // bit for bit
        else if (!instance_world_box(inst[t].invT, root.aabbMin, root.aabbMax, leaf.aabbMin, leaf.aabbMax)) bad = 1;
        leaf.BLASidx = (uint32_t)t; leaf.leftRight = 0;
        slot[t] = 1 + t;
    }
    __syncthreads();
    if (bad) { if (t == 0) { status[0] = 1; status[1] = 0; } return; }
    int live = n, used = n + 1, A = 0;
    int B = best_match(nd, slot, live, A, red);
    // the clustering merges one pair per join; between joins the nearest-neighbour chain only moves on (at most `live` steps)
    const int bound = 2 * kMaxInstances * kMaxInstances;
    for (int it = 0; live > 1; it++) {
        if (B < 0 || it >= bound) { if (t == 0) { status[0] = 2; status[1] = 0; } return; }
        const int C = best_match(nd, slot, live, B, red);
        if (A == C) {
            const int ia = slot[A], ib = slot[B];
            __syncthreads();   // every thread has read slot[] before thread 0 rewrites it
            if (t == 0) {
                const RtTLASNode& na = nd[ia]; const RtTLASNode& nb = nd[ib];
                RtTLASNode j{};
                j.leftRight = (uint32_t)ia + ((uint32_t)ib << 16);
                j.aabbMin = f4(tlas_min(na.aabbMin.x, nb.aabbMin.x), tlas_min(na.aabbMin.y, nb.aabbMin.y), tlas_min(na.aabbMin.z, nb.aabbMin.z), tlas_min(na.aabbMin.w, nb.aabbMin.w));
                j.aabbMax = f4(tlas_max(na.aabbMax.x, nb.aabbMax.x), tlas_max(na.aabbMax.y, nb.aabbMax.y), tlas_max(na.aabbMax.z, nb.aabbMax.z), tlas_max(na.aabbMax.w, nb.aabbMax.w));
                nd[used] = j;
                height[used] = 1 + (height[ia] > height[ib] ? height[ia] : height[ib]);
                slot[A] = used;
                slot[B] = slot[live - 1];
            }
            used++; live--;
            __syncthreads();
            B = best_match(nd, slot, live, A, red);
        } else { A = B; B = C; }
    }
    if (t == 0) { nd[0] = nd[slot[A]]; height[0] = height[slot[A]]; }
    __syncthreads();
    for (int i = t; i < nNodes; i += kBlock) {
        tlas[i] = nd[i];
        RtFloat4 r[4];
        tlas_pair(nd, (uint32_t)i, false, r);
        for (int k = 0; k < 4; k++) tp[(size_t)i * 4 + k] = r[k];
        tlas_pair(nd, (uint32_t)i, true, r);
        for (int k = 0; k < 4; k++) tpP[(size_t)i * 4 + k] = r[k];
    }
    if (t < n) {
        RtFloat4 r[4];
        inst_rec(inst[t], rootEntry ? rootEntry[t] : 0u, r);
        for (int k = 0; k < 4; k++) ir[(size_t)t * 4 + k] = r[k];
    }
    if (t == 0) { status[0] = 0; status[1] = (int32_t)height[0]; }
}

__global__ void __launch_bounds__(kBlock) k_pair_boxes(const RtBVHNode2* nodes, const uint32_t* pairNode, uint32_t nPairs, RtFloat4* pairs)
{
    const uint32_t k = blockIdx.x * kBlock + threadIdx.x;
    if (k >= nPairs) return;
    const uint32_t c = nodes[pairNode[k]].first;
    RtFloat4 r[3];
    pair_boxes(nodes[c], nodes[c + 1], r);
    for (int w = 0; w < 3; w++) pairs[(size_t)k * 4 + w] = r[w];
}
__global__ void __launch_bounds__(kBlock) k_tri_recs(const RtPrimitive* prims, const uint32_t* primIdx, uint32_t nIdx, RtFloat4* recs)
{
    const uint32_t s = blockIdx.x * kBlock + threadIdx.x;
    if (s >= nIdx) return;
    RtFloat4 r[3];
    tri_rec(prims[primIdx[s]], primIdx[s], r);
    for (int w = 0; w < 3; w++) recs[(size_t)s * 3 + w] = r[w];
}
__global__ void __launch_bounds__(kBlock) k_shade_recs(const RtPrimitive* prims, uint32_t first, uint32_t count, RtFloat4* recs)
{
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    if (i < count) recs[first + i] = shade_rec(prims[first + i]);
}
__global__ void __launch_bounds__(kBlock) k_light_recs(const RtPrimitive* prims, const uint32_t* lights, uint32_t nLights, RtFloat4* recs)
{
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= nLights) return;
    RtFloat4 r[5];
    light_rec(prims[lights[i]], r);
    for (int w = 0; w < 5; w++) recs[(size_t)i * 8 + w] = r[w];
}

static dim3 grid(uint32_t n) { return dim3((unsigned)((n + kBlock - 1) / kBlock)); }

hipError_t launch_refit(hipStream_t s, RtBVHNode2* nodes, uint32_t nNodes, const RtPrimitive* prims, const uint32_t* primIdx,
                        const uint32_t* leaves, uint32_t nLeaves, const uint32_t* parent, uint32_t* tickets)
{
    hipError_t e = hipMemsetAsync(tickets, 0, sizeof(uint32_t) * nNodes, s);
    if (e != hipSuccess || nLeaves == 0) return e;
    hipLaunchKernelGGL(k_refit_nodes, grid(nLeaves), dim3(kBlock), 0, s, nodes, prims, primIdx, leaves, nLeaves, parent, tickets);
    return hipGetLastError();
}
// One BLAS of a scene (RT_REBUILD_REFIT_RANGE): the tickets of its block [root, root + nBlasNodes) alone are zeroed, the kernel starts
// from its own run of leaves and climbs until parent == kNone, which is its root's
hipError_t launch_refit_blas(hipStream_t s, RtBVHNode2* nodes, uint32_t root, uint32_t nBlasNodes, const RtPrimitive* prims, const uint32_t* primIdx,
                             const uint32_t* leafRun, uint32_t nLeaves, const uint32_t* parent, uint32_t* tickets)
{
    hipError_t e = hipMemsetAsync(tickets + root, 0, sizeof(uint32_t) * nBlasNodes, s);
    if (e != hipSuccess || nLeaves == 0) return e;
    hipLaunchKernelGGL(k_refit_nodes, grid(nLeaves), dim3(kBlock), 0, s, nodes, prims, primIdx, leafRun, nLeaves, parent, tickets);
    return hipGetLastError();
}
// ... then the boxes of its run of pair records (pairNode / pairs: at the run's start) and the triangle records of its slot run
// (primIdx / triRecs: at the run's start); either may be NULL
hipError_t launch_blas_records(hipStream_t s, const RtPrimitive* prims, const RtBVHNode2* nodes, const uint32_t* pairNode, uint32_t nPairs, RtFloat4* pairs,
                               const uint32_t* primIdx, uint32_t nSlots, RtFloat4* triRecs)
{
    if (pairs && nPairs) hipLaunchKernelGGL(k_pair_boxes, grid(nPairs), dim3(kBlock), 0, s, nodes, pairNode, nPairs, pairs);
    if (triRecs && nSlots) hipLaunchKernelGGL(k_tri_recs, grid(nSlots), dim3(kBlock), 0, s, prims, primIdx, nSlots, triRecs);
    return hipGetLastError();
}
hipError_t launch_tlas(hipStream_t s, const RtBVHNode2* nodes, const RtBVHInstance* inst, int n, const uint32_t* rootEntry,
                       RtTLASNode* tlas, RtFloat4* tp, RtFloat4* tpP, RtFloat4* ir, int32_t* status)
{
    if (n < 1 || n > kMaxInstances) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_tlas_build, dim3(1), dim3(kBlock), 0, s, nodes, inst, n, rootEntry, tlas, tp, tpP, ir, status);
    return hipGetLastError();
}
hipError_t launch_records(hipStream_t s, const RtPrimitive* prims, const RtBVHNode2* nodes, const uint32_t* primIdx, uint32_t nIdx,
                          const uint32_t* lights, uint32_t nLights, uint32_t first, uint32_t count, const uint32_t* pairNode,
                          uint32_t nPairs, RtFloat4* pairs, RtFloat4* triRecs, RtFloat4* shadeRecs, RtFloat4* lightRecs)
{
    if (pairs && nPairs) hipLaunchKernelGGL(k_pair_boxes, grid(nPairs), dim3(kBlock), 0, s, nodes, pairNode, nPairs, pairs);
    if (count) {
        if (triRecs && nIdx) hipLaunchKernelGGL(k_tri_recs, grid(nIdx), dim3(kBlock), 0, s, prims, primIdx, nIdx, triRecs);
        hipLaunchKernelGGL(k_shade_recs, grid(count), dim3(kBlock), 0, s, prims, first, count, shadeRecs);
        if (nLights) hipLaunchKernelGGL(k_light_recs, grid(nLights), dim3(kBlock), 0, s, prims, lights, nLights, lightRecs);
    }
    return hipGetLastError();
}

} // namespace refitdev

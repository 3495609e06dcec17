// lbvh.hip — rt_build_bvh2 (include/rt355.h): the linear BVH builder on the GPU.  The algorithm and every value it computes are
// defined in lbvh_common.h; this file only distributes that work over kernels.  host/lbvh_host.cpp runs the same rules in sequence
// (rth_build_bvh2_lbvh) and must produce identical arrays (tests/test_gpu_lbvh.py).
//
//   k_lbvh_boxes     primitive boxes + centroid key bounds (workgroup reduction in LDS, then one atomicMin / atomicMax per workgroup)
//   k_lbvh_keys      Morton key | local index, value = local index
//   radix sort       hipcub::DeviceRadixSort::SortPairs over the L = 3k + b significant bits
//   k_lbvh_karras    internal nodes: children, sorted range, parent links
//   k_lbvh_bottomup  one thread per leaf climbs while it is the second to reach a node (atomic ticket per node, no waiting)
//   k_lbvh_survive   internal nodes emitted as interior nodes; exclusive scan (hipcub::DeviceScan) gives their pair slots
//   k_lbvh_emit      RtBVHNode2 records and primIdx
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>
#include "../../include/rt355.h"
#include "lbvh_common.h"
#include "build_dev.h"

using namespace lbvh;
using builddev::align_up;
using builddev::build_fail;
using builddev::grid;

namespace {

constexpr int kBlock = 256;

__global__ void __launch_bounds__(kBlock) k_lbvh_boxes(const RtPrimitive* prims, uint32_t n, Box* boxes, uint32_t* cb)
{
    __shared__ uint32_t s[6];
    if (threadIdx.x < 6) s[threadIdx.x] = threadIdx.x < 3 ? kKeyMinInit : kKeyMaxInit;
    __syncthreads();
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    if (i < n) {
        const Box b = prim_box(prims[i]);
        boxes[i] = b;
        for (int a = 0; a < 3; a++) {
            const float c = centroid(b, a);
            if (finite_(c)) { atomicMin(&s[a], order_key(c)); atomicMax(&s[3 + a], order_key(c)); }
        }
    }
    __syncthreads();
    if (threadIdx.x < 3) atomicMin(&cb[threadIdx.x], s[threadIdx.x]);
    else if (threadIdx.x < 6) atomicMax(&cb[threadIdx.x], s[threadIdx.x]);
}

__global__ void __launch_bounds__(kBlock) k_lbvh_keys(const Box* boxes, uint32_t n, const uint32_t* cb, int k, int bIdx,
                                                      uint64_t* keys, uint32_t* vals)
{
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    float clo[3], scale[3];
    quantizer(cb, cb + 3, k, clo, scale);
    keys[i] = make_key(boxes[i], clo, scale, k, bIdx, i);
    vals[i] = i;
}

struct Kids { uint32_t left, right, first; };

__global__ void __launch_bounds__(kBlock) k_lbvh_karras(const uint64_t* keys, uint32_t n, Kids* kids, uint32_t* parent)
{
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    if (i + 1 >= n) return;
    Kids c; uint32_t last;
    karras_node(keys, n, i, c.left, c.right, c.first, last);
    kids[i] = c;
    parent[c.left] = i;
    parent[c.right] = i;
}

// Records cross workgroups here: a node's two children are written by whichever threads climbed to them, anywhere on the chip.  Each
// hand-off is the agent-scope release / acquire of the ticket (cdna_hip_programming §6 Guideline 16): the writer stores its record
// with plain stores, releases at agent scope and drains its stores before it draws the ticket; the thread that draws the second
// ticket acquires at agent scope before it loads the sibling's record.  Nobody waits: the first visitor just stops.  The record
// array is read through plain (not const / restrict) pointers so that the loads stay on the vector path behind the acquire.
__global__ void __launch_bounds__(kBlock) k_lbvh_bottomup(const Box* boxes, const uint32_t* vals, uint32_t n, NodeRec* rec,
                                                          const uint32_t* parent, const Kids* kids, uint32_t* tickets, Params P)
{
    const uint32_t k = blockIdx.x * kBlock + threadIdx.x;
    if (k >= n) return;
    uint32_t node = n - 1 + k;
    rec[node] = leaf_rec(boxes[vals[k]], k, P);
    for (uint32_t p = parent[node]; p != kNone; p = parent[p]) {
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        if (__hip_atomic_fetch_add(&tickets[p], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == 0) return;
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
        const Kids c = kids[p];
        const NodeRec L = rec[c.left], R = rec[c.right];
        rec[p] = combine(L, R, c.first, P);
    }
}

__global__ void __launch_bounds__(kBlock) k_lbvh_survive(const NodeRec* rec, const uint32_t* parent, uint32_t nInternal,
                                                         uint32_t maxLeaf, uint32_t* flags)
{
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    if (i < nInternal) flags[i] = survives(rec, parent, i, maxLeaf);
}

__global__ void __launch_bounds__(kBlock) k_lbvh_emit(const NodeRec* rec, const Kids* kids, const uint32_t* flags, const uint32_t* rank,
                                                      const uint32_t* vals, uint32_t n, uint32_t first, uint32_t nodeBase,
                                                      uint32_t idxBase, RtBVHNode2* nodes, uint32_t* primIdx)
{
    const uint32_t t = blockIdx.x * kBlock + threadIdx.x;
    if (t >= n) return;
    const uint32_t nInternal = n - 1;
    primIdx[t] = first + vals[t];
    if (t == 0) nodes[0] = emit(rec[0], 0, nInternal, rank, nodeBase, idxBase);
    if (t < nInternal && flags[t]) {
        const uint32_t slot = 1 + 2 * rank[t];
        nodes[slot] = emit(rec[kids[t].left], kids[t].left, nInternal, rank, nodeBase, idxBase);
        nodes[slot + 1] = emit(rec[kids[t].right], kids[t].right, nInternal, rank, nodeBase, idxBase);
    }
}

// The carved workspace of one build of n primitives (everything but the primitives and the output arrays):
// [cb | tickets | parent] first (the words the memsets initialise), then the rest
struct Carve { size_t oCb, oTick, oPar, oBox, oK0, oK1, oV0, oV1, oKids, oRec, oFlag, oRank, oSort, oScan, sortBytes, scanBytes, total; };
hipError_t carve_work(uint32_t n, hipStream_t s, Carve& c)
{
    const uint32_t nInt = n - 1, nTree = 2 * n - 1;
    const int keyBits = 3 * axis_bits(n) + index_bits(n);
    c.sortBytes = c.scanBytes = 0;
    hipError_t e = hipcub::DeviceRadixSort::SortPairs(nullptr, c.sortBytes, (uint64_t*)nullptr, (uint64_t*)nullptr, (uint32_t*)nullptr,
                                                      (uint32_t*)nullptr, (int)n, 0, keyBits, s);
    if (e != hipSuccess) return e;
    if (nInt > 0) e = hipcub::DeviceScan::ExclusiveSum(nullptr, c.scanBytes, (uint32_t*)nullptr, (uint32_t*)nullptr, (int)nInt, s);
    if (e != hipSuccess) return e;
    const size_t nI = nInt > 0 ? nInt : 1;
    size_t off = 0;
    auto carve = [&](size_t bytes) { const size_t o = off; off += align_up(bytes); return o; };
    c.oCb = carve(6 * sizeof(uint32_t)); c.oTick = carve(nI * sizeof(uint32_t)); c.oPar = carve(nTree * sizeof(uint32_t));
    c.oBox = carve(n * sizeof(Box)); c.oK0 = carve(n * 8ull); c.oK1 = carve(n * 8ull);
    c.oV0 = carve(n * 4ull); c.oV1 = carve(n * 4ull); c.oKids = carve(nI * sizeof(Kids)); c.oRec = carve(nTree * sizeof(NodeRec));
    c.oFlag = carve(nI * 4ull); c.oRank = carve(nI * 4ull);
    c.oSort = carve(c.sortBytes); c.oScan = carve(c.scanBytes);
    c.total = off;
    return hipSuccess;
}

} // namespace

namespace lbvhdev {

const char* check_args(const RtBuildOptions* opts, int32_t nPrims, int32_t first, int32_t count, uint32_t nodeBase, uint32_t idxBase, Params& P)
{
    static const RtPrimitive prim{}; static const RtBVHNode2 node{}; static const int32_t n = 0; static const uint32_t idx = 0;   // (only their presence is checked)
    return lbvh::check_args(opts, &prim, nPrims, first, count, nodeBase, idxBase, &node, count > 0 ? 2 * count - 1 : 0, &n, &idx, P);
}

int work_bytes(const char* who, uint32_t n, hipStream_t s, size_t* bytes)
{
    Carve c;
    BUILD_CHK(carve_work(n, s, c));
    *bytes = c.total;
    return RT_OK;
}

// The build proper (build_cores.h): everything stays on the device; the host reads the root's record.
int build(const char* who, hipStream_t stream, void* work, const Params& P, const RtPrimitive* dPrims, uint32_t n, uint32_t first,
          uint32_t nodeBase, uint32_t idxBase, RtBVHNode2* dNodes, uint32_t* dIdx, hipEvent_t evBegin, hipEvent_t evEnd, Built* out)
{
    const uint32_t nInt = n - 1, nTree = 2 * n - 1;
    const int bIdx = index_bits(n), k = axis_bits(n), keyBits = 3 * k + bIdx;
    const size_t nI = nInt > 0 ? nInt : 1;
    Carve c;
    BUILD_CHK(carve_work(n, stream, c));
    char* base = (char*)work;
    auto at = [&](size_t o) { return (void*)(base + o); };
    uint32_t* cb = (uint32_t*)at(c.oCb);
    uint32_t* tickets = (uint32_t*)at(c.oTick);
    uint32_t* parent = (uint32_t*)at(c.oPar);
    Box* boxes = (Box*)at(c.oBox);
    uint64_t *k0 = (uint64_t*)at(c.oK0), *k1 = (uint64_t*)at(c.oK1);
    uint32_t *v0 = (uint32_t*)at(c.oV0), *v1 = (uint32_t*)at(c.oV1);
    Kids* kids = (Kids*)at(c.oKids);
    NodeRec* rec = (NodeRec*)at(c.oRec);
    uint32_t *flags = (uint32_t*)at(c.oFlag), *rank = (uint32_t*)at(c.oRank);

    const uint32_t cbInit[6] = { kKeyMinInit, kKeyMinInit, kKeyMinInit, kKeyMaxInit, kKeyMaxInit, kKeyMaxInit };
    BUILD_CHK(hipMemcpyAsync(cb, cbInit, sizeof cbInit, hipMemcpyHostToDevice, stream));
    BUILD_CHK(hipMemsetAsync(tickets, 0, nI * sizeof(uint32_t), stream));
    BUILD_CHK(hipMemsetAsync(parent, 0xff, nTree * sizeof(uint32_t), stream));
    BUILD_CHK(hipStreamSynchronize(stream));   // (rt_build_bvh2: nothing of the caller's host arrays is read after this point)

    const dim3 blk(kBlock), gN = grid(n, kBlock), gI = grid((uint32_t)nI, kBlock);
    if (evBegin) BUILD_CHK(hipEventRecord(evBegin, stream));
    hipLaunchKernelGGL(k_lbvh_boxes, gN, blk, 0, stream, dPrims, n, boxes, cb);
    hipLaunchKernelGGL(k_lbvh_keys, gN, blk, 0, stream, boxes, n, cb, k, bIdx, k0, v0);
    BUILD_CHK(hipcub::DeviceRadixSort::SortPairs(at(c.oSort), c.sortBytes, k0, k1, v0, v1, (int)n, 0, keyBits, stream));
    if (nInt > 0) hipLaunchKernelGGL(k_lbvh_karras, gI, blk, 0, stream, k1, n, kids, parent);
    hipLaunchKernelGGL(k_lbvh_bottomup, gN, blk, 0, stream, boxes, v1, n, rec, parent, kids, tickets, P);
    if (nInt > 0) {
        hipLaunchKernelGGL(k_lbvh_survive, gI, blk, 0, stream, rec, parent, nInt, P.maxLeaf, flags);
        BUILD_CHK(hipcub::DeviceScan::ExclusiveSum(at(c.oScan), c.scanBytes, flags, rank, (int)nInt, stream));
    }
    hipLaunchKernelGGL(k_lbvh_emit, gN, blk, 0, stream, rec, kids, flags, rank, v1, n, first, nodeBase, idxBase, dNodes, dIdx);
    BUILD_CHK(hipGetLastError());
    if (evEnd) BUILD_CHK(hipEventRecord(evEnd, stream));

    NodeRec root;
    BUILD_CHK(hipMemcpyAsync(&root, rec, sizeof root, hipMemcpyDeviceToHost, stream));
    BUILD_CHK(hipStreamSynchronize(stream));
    const uint32_t outNodes = 2 * root.leaves - 1;
    if (root.leaves < 1 || outNodes > nTree) return build_fail(RT_E_DEVICE, "%s: inconsistent device result (%u leaves)", who, root.leaves);
    *out = Built{};
    out->nodes = outNodes; out->leaves = root.leaves; out->depth = root.height; out->mortonBits = (uint32_t)k; out->cost = root.total;
    return RT_OK;
}

} // namespace lbvhdev

// The C-ABI entry: a session on the device, then builddev::build_flat around lbvhdev::build.
extern "C" int rt_build_bvh2(int32_t device, const RtBuildOptions* opt, const RtPrimitive* prims, int32_t nPrims, int32_t first,
                             int32_t count, uint32_t nodeBase, uint32_t idxBase, RtBVHNode2* nodes, int32_t nodeCap, int32_t* nNodes,
                             uint32_t* primIdx, RtBuildStats* stats)
{
    const char* who = "rt_build_bvh2";
    const auto t0 = builddev::Clock::now();
    Params P;
    if (const char* msg = check_args(opt, prims, nPrims, first, count, nodeBase, idxBase, nodes, nodeCap, nNodes, primIdx, P))
        return build_fail(RT_E_INVALID, "rt_build_bvh2: %s", msg);
    builddev::Session w;
    if (const int rc = builddev::open_session(who, device, w)) return rc;
    const uint32_t n = (uint32_t)count;
    return builddev::build_flat(who, w, t0, lbvhdev::work_bytes, prims, first, n, nodes, nNodes, primIdx, stats,
        [&](void* work, const RtPrimitive* dPrims, RtBVHNode2* dNodes, uint32_t* dIdx, Built* b) {
            return lbvhdev::build(who, w.stream, work, P, dPrims, n, (uint32_t)first, nodeBase, idxBase, dNodes, dIdx, w.ev[0], w.ev[1], b);
        });
}

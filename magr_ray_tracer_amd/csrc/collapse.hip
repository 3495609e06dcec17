// collapse.hip — the BVH2 -> BVH4 collapse on the device (rt_build_bvh4, include/rt355.h; scene.hip drives the same kernels for a BVH4
// copy that was bound with its BVH2, rt_upload_scene_bvh2, and for its in-place rebuilds).  The rules are collapse_common.h's, which the
// host restatement (host/collapse_host.cpp) shares.
//
//   k_c4_convert    one thread per BVH2 record: Convert's record (zero for a leaf) into bvh4[i].  Absorbed and unreachable nodes keep it.
// Per BLAS, in the order in which the instances first name their roots, and level l (frontier: the surviving nodes of that level with
// the stack entries below each; cnt[l] of them, the first has live id base[l]):
//   k_c4_frontier   one thread per frontier node: the greedy loop over the BVH2 (never over bvh4: nothing depends on what another
//                   thread has written), the final record, newId / quadNode, a flag and the node id per slot that is a child; folds
//                   the stack need and the largest leaf into status words (values, not positions); hipcub::DeviceScan ranks the flags
//   k_c4_next       writes the flagged children and their stack bases to the next frontier at their ranks; cnt[l + 1], base[l + 1]
// A BVH4 level descends at least one BVH2 level, so the host launches as many levels as the BVH2 is high (one for a leaf root) with
// frontiers bounded by min(4^l, interior nodes), and reads nothing back; empty levels do nothing.  Every position comes from a scan: no
// atomic decides where anything is written, two runs give the same bytes.  Then, over all BLAS:
//   k_c4_refit      (a refit BVH2 under a bound collapse, RT_REBUILD_REFIT) one thread per bound live id: the final record from the refit
//                   BVH2, and a count of the records whose slots differ from the bound ones; zero: the bound live ids still hold and
//                   the level loop above is skipped
//   k_c4_quads      one thread per live id: the quad record (collapse::quad_record)
//   k_c4_roots      one thread per instance: rootEntry[b] = newId[root of b]
// Flat kernels of 256 threads; nothing here depends on the wave size.
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>
#include <climits>
#include <string>
#include <vector>
#include "../../include/rt355.h"
#include "collapse_common.h"
#include "collapse_dev.h"
#include "build_dev.h"

namespace collapsedev {

using namespace collapse;

constexpr int kBlock = 256;

__global__ void __launch_bounds__(kBlock) k_c4_convert(const RtBVHNode2* nodes, uint32_t nNodes, RtBVHNode4* bvh4, uint32_t* ctr)
{
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= nNodes) return;
    RtBVHNode4 q;
    if (nodes[i].count == 0 && !children_inside(nodes, nNodes, i)) { zero_record(q); atomicOr(&ctr[kWalkWord], kWalk); }   // (the host has checked)
    else converted(nodes, i, q);
    bvh4[i] = q;
    const uint32_t leaf = nodes[i].count;   // every leaf a record can name, live or not: the upload's layout rule looks at all records
    if (leaf > rebuild::kMaxPackedLeaf) atomicMax(&ctr[kLeafAny], leaf);
}

__global__ void __launch_bounds__(64) k_c4_begin(uint32_t root, uint2* front, uint32_t* ctr)
{
    if (threadIdx.x != 0) return;
    front[0] = make_uint2(root, 0u);
    ctr[kCnt + 0] = 1u;
    ctr[kBase + 0] = ctr[kLive];
}

__global__ void __launch_bounds__(kBlock) k_c4_frontier(const RtBVHNode2* nodes, uint32_t nNodes, const uint2* front, uint32_t ub, uint32_t level,
                                                        uint32_t quadCap, RtBVHNode4* bvh4, uint32_t* newId, uint32_t* quadNode, uint32_t* flags,
                                                        uint32_t* kids, uint32_t* ctr)
{
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= ub) return;
    uint32_t f[4] = { 0, 0, 0, 0 }, c[4] = { 0, 0, 0, 0 };
    if (i < ctr[kCnt + level]) {
        const uint32_t node = front[i].x, base = front[i].y, id = ctr[kBase + level] + i;
        RtBVHNode4 rec;
        if (id >= quadCap || !final_record(nodes, nNodes, node, rec)) atomicOr(&ctr[kWalkWord], kWalk);
        else {
            bvh4[node] = rec;
            newId[node] = id; quadNode[id] = node;
            uint32_t n = 0;
            for (int k = 0; k < 4; k++) if (is_child(rec, k)) { f[k] = 1u; c[k] = (uint32_t)rec.first[k]; n++; }
            atomicMax(&ctr[kNeed], base + n);
            const uint32_t leaf = largest_leaf(rec);
            if (leaf) atomicMax(&ctr[kLeaf], leaf);
        }
    }
    *reinterpret_cast<uint4*>(&flags[4 * (size_t)i]) = make_uint4(f[0], f[1], f[2], f[3]);
    *reinterpret_cast<uint4*>(&kids[4 * (size_t)i]) = make_uint4(c[0], c[1], c[2], c[3]);
}

// last: this is the last level the host launches for the BLAS; the walk must have ended
__global__ void __launch_bounds__(kBlock) k_c4_next(const uint2* front, uint32_t ub, uint32_t level, const uint32_t* flags, const uint32_t* ranks,
                                                    const uint32_t* kids, uint2* next, uint32_t nextCap, uint32_t last, uint32_t* ctr)
{
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= ub) return;
    const uint32_t cnt = ctr[kCnt + level];
    if (i == 0) {
        const uint32_t n = ranks[4 * (size_t)ub - 1] + flags[4 * (size_t)ub - 1], end = ctr[kBase + level] + (cnt < ub ? cnt : ub);
        ctr[kCnt + level + 1] = n; ctr[kBase + level + 1] = end;
        ctr[kLive] = end;
        if (cnt > 0) atomicMax(&ctr[kLevels], level + 1);
        if (cnt > ub || n > nextCap || (last && n != 0)) atomicOr(&ctr[kWalkWord], kWalk);
    }
    if (i >= cnt) return;
    const uint32_t base = front[i].y;
    uint32_t j = 0;
    for (uint32_t k = 0; k < 4; k++)
        if (flags[4 * (size_t)i + k]) {
            const uint32_t r = ranks[4 * (size_t)i + k];
            if (r < nextCap) next[r] = make_uint2(kids[4 * (size_t)i + k], base + j);
            j++;
        }
}

// One thread per live id of the bound collapse.  Reads the BVH2 and the bound records only: nothing another thread writes.
__global__ void __launch_bounds__(kBlock) k_c4_refit(const RtBVHNode2* nodes, uint32_t nNodes, const RtBVHNode4* bound4, const uint32_t* quadNode,
                                                     uint32_t nLive, RtBVHNode4* bvh4, uint32_t* ctr)
{
    const uint32_t q = blockIdx.x * kBlock + threadIdx.x;
    if (q >= nLive) return;
    if (q == 0) ctr[kLive] = nLive;
    const uint32_t node = quadNode[q];
    RtBVHNode4 rec;
    if (!final_record(nodes, nNodes, node, rec)) { atomicOr(&ctr[kWalkWord], kWalk); return; }   // (node < nNodes: final_record's first check)
    bvh4[node] = rec;
    const RtBVHNode4& old = bound4[node];
    bool same = true;
    for (int k = 0; k < 4; k++) same = same && rec.first[k] == old.first[k] && rec.count[k] == old.count[k];
    if (!same) atomicAdd(&ctr[kChanged], 1u);
    const uint32_t leaf = largest_leaf(rec);
    if (leaf) atomicMax(&ctr[kLeaf], leaf);
}

__global__ void __launch_bounds__(kBlock) k_c4_quads(const RtBVHNode4* bvh4, uint32_t nNodes, uint32_t nIdx, const uint32_t* quadNode, const uint32_t* newId,
                                                     uint32_t quadCap, const uint32_t* ctr, RtFloat4* quads)
{
    const uint32_t q = blockIdx.x * kBlock + threadIdx.x;
    if (q >= quadCap || q >= ctr[kLive]) return;
    const uint32_t node = quadNode[q];
    if (node >= nNodes) return;   // (only after a failed walk, which the host reports)
    RtFloat4 r[8];
    quad_record(bvh4[node], (int32_t)nNodes, (int32_t)nIdx, newId, r);
    for (int w = 0; w < 8; w++) quads[(size_t)q * 8 + w] = r[w];
}

__global__ void __launch_bounds__(kBlock) k_c4_roots(const uint32_t* roots, uint32_t rootStride, uint32_t nRoots, const uint32_t* newId, uint32_t* rootEntry)
{
    const uint32_t b = blockIdx.x * kBlock + threadIdx.x;
    if (b >= nRoots) return;
    rootEntry[b] = newId[roots[(size_t)b * rootStride]];
}

static dim3 grid(uint32_t n) { return dim3((unsigned)((n + kBlock - 1) / kBlock)); }

hipError_t scan_bytes(uint32_t items, hipStream_t s, size_t* bytes)
{
    *bytes = 0;
    return hipcub::DeviceScan::ExclusiveSum(nullptr, *bytes, (uint32_t*)nullptr, (uint32_t*)nullptr, (int)items, s);
}

hipError_t begin(hipStream_t s, const Work& w, const RtBVHNode2* nodes, uint32_t nNodes, RtBVHNode4* bvh4)
{
    const hipError_t e = hipMemsetAsync(w.ctr, 0, sizeof(uint32_t) * kCtrWords, s);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_c4_convert, grid(nNodes), dim3(kBlock), 0, s, nodes, nNodes, bvh4, w.ctr);
    return hipGetLastError();
}

hipError_t collapse_blas(hipStream_t s, const Work& w, const RtBVHNode2* nodes, uint32_t nNodes, uint32_t root, uint32_t interiors, uint32_t height,
                         RtBVHNode4* bvh4)
{
    if (height > kMaxLevels || (height > 0 && interiors == 0) || root >= nNodes) return hipErrorInvalidValue;
    if (level_bound(kMaxLevels, interiors) > w.frontCap || 4ull * w.frontCap > (uint64_t)INT_MAX) return hipErrorInvalidValue;
    uint2 *front = w.frontA, *next = w.frontB;
    size_t scanBytes = w.scanBytes;
    hipLaunchKernelGGL(k_c4_begin, dim3(1), dim3(64), 0, s, root, front, w.ctr);
    const uint32_t levels = height > 0 ? height : 1;
    for (uint32_t l = 0; l < levels; l++) {
        const uint32_t ub = level_bound(l, interiors);
        hipLaunchKernelGGL(k_c4_frontier, grid(ub), dim3(kBlock), 0, s, nodes, nNodes, front, ub, l, w.quadCap, bvh4, w.newId, w.quadNode, w.flags, w.kids, w.ctr);
        const hipError_t e = hipcub::DeviceScan::ExclusiveSum(w.scan, scanBytes, w.flags, w.ranks, (int)(4 * ub), s);
        if (e != hipSuccess) return e;
        hipLaunchKernelGGL(k_c4_next, grid(ub), dim3(kBlock), 0, s, front, ub, l, w.flags, w.ranks, w.kids, next, w.frontCap, l + 1 == levels ? 1u : 0u, w.ctr);
        uint2* t = front; front = next; next = t;
    }
    return hipGetLastError();
}

hipError_t refit_records(hipStream_t s, const Work& w, const RtBVHNode2* nodes, uint32_t nNodes, const RtBVHNode4* bound4, const uint32_t* quadNode,
                         uint32_t nLive, RtBVHNode4* bvh4)
{
    if (nLive == 0 || nLive > w.quadCap) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_c4_refit, grid(nLive), dim3(kBlock), 0, s, nodes, nNodes, bound4, quadNode, nLive, bvh4, w.ctr);
    return hipGetLastError();
}

hipError_t finish(hipStream_t s, const Work& w, const RtBVHNode4* bvh4, uint32_t nNodes, uint32_t nIdx, const uint32_t* roots, uint32_t rootStride,
                  uint32_t nRoots, RtFloat4* quads, uint32_t* rootEntry)
{
    if (quads) {
        hipLaunchKernelGGL(k_c4_quads, grid(w.quadCap), dim3(kBlock), 0, s, bvh4, nNodes, nIdx, w.quadNode, w.newId, w.quadCap, w.ctr, quads);
        hipLaunchKernelGGL(k_c4_roots, grid(nRoots), dim3(kBlock), 0, s, roots, rootStride, nRoots, w.newId, rootEntry);
    }
    return hipGetLastError();
}

} // namespace collapsedev

// The C-ABI entry: the checks, a session on the device, one allocation, the kernels, the status words, then the download.
extern "C" int rt_build_bvh4(int32_t device, const RtBVHNode2* nodes2, int32_t nNodes, int32_t nIdx, const uint32_t* roots, int32_t nRoots,
                             RtBVHNode4* out4, RtBvh4Stats* stats)
{
    using namespace collapsedev;
    using builddev::build_fail;
    using builddev::align_up;
    const char* who = "rt_build_bvh4";
    const auto t0 = builddev::Clock::now();
    std::vector<collapse::Blas> blas;
    std::string why;
    if (const int rc = collapse::check_args(nodes2, nNodes, nIdx, roots, nRoots, blas, why)) return build_fail(rc, "%s: %s", who, why.c_str());
    if (!out4) return build_fail(RT_E_INVALID, "%s: missing array (out4)", who);
    size_t frontCap = 1, quadCap = 0;
    for (const collapse::Blas& b : blas) { frontCap = std::max<size_t>(frontCap, b.interiors); quadCap += b.interiors > 0 ? b.interiors : 1; }
    if (4 * frontCap > (size_t)INT_MAX) return build_fail(RT_E_UNSUPPORTED, "%s: a BLAS of %zu interior nodes (at most 2^29 - 1)", who, frontCap);
    builddev::Session s;
    if (const int rc = builddev::open_session(who, device, s)) return rc;
    size_t scanBytes = 0;
    BUILD_CHK(scan_bytes((uint32_t)(4 * frontCap), s.stream, &scanBytes));
    const size_t n = (size_t)nNodes;
    size_t off = 0;
    auto take = [&off](size_t bytes) { const size_t o = off; off += align_up(bytes); return o; };
    const size_t oN2 = take(n * sizeof(RtBVHNode2)), oN4 = take(n * sizeof(RtBVHNode4)), oRoots = take((size_t)nRoots * 4), oFA = take(frontCap * 8),
                 oFB = take(frontCap * 8), oFlags = take(frontCap * 16), oRanks = take(frontCap * 16), oKids = take(frontCap * 16), oNew = take(n * 4),
                 oQn = take(quadCap * 4), oCtr = take(kCtrWords * 4), oScan = take(std::max<size_t>(scanBytes, 256));
    if (hipMalloc(&s.mem[0], off) != hipSuccess) { s.mem[0] = nullptr; return build_fail(RT_E_NOMEM, "%s: %zu bytes of device memory", who, off); }
    char* base = (char*)s.mem[0];
    const RtBVHNode2* dN2 = (const RtBVHNode2*)(base + oN2);
    RtBVHNode4* dN4 = (RtBVHNode4*)(base + oN4);
    const Work w{ (uint2*)(base + oFA), (uint2*)(base + oFB), (uint32_t)frontCap, (uint32_t*)(base + oFlags), (uint32_t*)(base + oRanks), (uint32_t*)(base + oKids),
                  (uint32_t*)(base + oNew), (uint32_t*)(base + oQn), (uint32_t)quadCap, (uint32_t*)(base + oCtr), base + oScan, std::max<size_t>(scanBytes, 256) };
    BUILD_CHK(hipMemcpyAsync(base + oN2, nodes2, n * sizeof(RtBVHNode2), hipMemcpyHostToDevice, s.stream));
    BUILD_CHK(hipMemcpyAsync(base + oRoots, roots, (size_t)nRoots * 4, hipMemcpyHostToDevice, s.stream));
    BUILD_CHK(hipEventRecord(s.ev[0], s.stream));
    BUILD_CHK(begin(s.stream, w, dN2, (uint32_t)nNodes, dN4));
    for (const collapse::Blas& b : blas) BUILD_CHK(collapse_blas(s.stream, w, dN2, (uint32_t)nNodes, b.root, b.interiors, b.height, dN4));
    BUILD_CHK(hipEventRecord(s.ev[1], s.stream));
    uint32_t st[kStatusWords] = { 0 };
    BUILD_CHK(hipMemcpyAsync(st, w.ctr + kStatus, sizeof st, hipMemcpyDeviceToHost, s.stream));
    BUILD_CHK(hipStreamSynchronize(s.stream));
    if (st[kWalkWord - kStatus]) return build_fail(RT_E_DEVICE, "%s: the level walk does not match the tree (inconsistent device result)", who);
    BUILD_CHK(hipMemcpyAsync(out4, dN4, n * sizeof(RtBVHNode4), hipMemcpyDeviceToHost, s.stream));
    BUILD_CHK(hipStreamSynchronize(s.stream));
    if (stats) {
        float ms = 0;
        BUILD_CHK(hipEventElapsedTime(&ms, s.ev[0], s.ev[1]));
        stats->live_nodes = (int32_t)st[kLive - kStatus]; stats->levels = (int32_t)st[kLevels - kStatus]; stats->stack_need = (int32_t)st[kNeed - kStatus];
        stats->largest_leaf = (int32_t)st[kLeaf - kStatus];
        stats->device_ms = ms;
        stats->wall_ms = std::chrono::duration<float, std::milli>(builddev::Clock::now() - t0).count();
    }
    return RT_OK;
}

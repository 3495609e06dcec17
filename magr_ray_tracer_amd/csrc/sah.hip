// sah.hip — rt_build_bvh2_sah (include/rt355.h): the default SAH BLAS (BVH2::BuildBLAS with alpha = 1) built on the GPU.  The
// formulation and every value it computes are defined in sah_common.h; this file only distributes that work over kernels.
// host/sah_host.cpp runs the same steps in sequence (rth_build_bvh2_sah); both equal BuildBLAS's arrays byte for byte.
//
// Per level (the open nodes are the build ids [lb, le); a position p of the ref arrays belongs to node nid[p] or to none):
//   k_sah_reduce    node-bounds and centroid-bounds keys of the open nodes (LDS slots per workgroup, then 64-bit atomicMin / Max)
//   k_sah_bins      bin counts and bin-box keys per (open node, axis, bin), the same way; flags a NaN / infinite bin index
//   k_sah_decide    one thread per open node: the sweep and the decision
//   k_sah_small     one thread per small node: its whole subtree (build_small)
//   k_sah_flag      partition flags; hipcub::DeviceScan gives each ref its rank among the refs going left
//   k_sah_count     forced leaves, the children's contribution to the scan that places them; k_sah_children writes them
//   k_sah_scatter   the stable partition of every split segment into the other ref array (other positions are copied)
// The host reads back three words per level (splits, open children, status).  Then, with kernel boundaries between levels:
//   k_sah_up        interior counts, heights and TotalCost bottom-up; k_sah_down: pop ranks, ref offsets, output ids top-down
//   k_sah_emit      RtBVHNode2 records (level part and small subtrees); k_sah_emit_refs: primIdx
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>
#include <utility>
#include <vector>
#include "../../include/rt355.h"
#include "sah_common.h"
#include "build_dev.h"
#include "fold_dev.h"

using namespace sah;
using namespace fold;
using builddev::align_up;
using builddev::build_fail;
using builddev::grid;
using builddev::ms_since;

namespace {

constexpr int kBlock = 256;
constexpr int kSlots = 16;   // open nodes a workgroup's positions can meet: each holds > kSmall refs
static_assert(kBlock / (kSmall + 1) + 2 <= kSlots, "a workgroup's kBlock positions meet at most kSlots open nodes");
constexpr int kCnt = 3 * kBins;                     // bin counts per open node
constexpr int kKeys = 6 + kBinKeys;                 // 64-bit keys per open node and fold direction

// phases of the last build, for rt_debug_sah_phases: upload, level passes, numbering + emit, download (ms), levels
float g_phases[5] = { 0, 0, 0, 0, 0 };

__global__ void __launch_bounds__(kBlock) k_sah_prims(const RtPrimitive* prims, uint32_t n, Prim* P, uint32_t* cur, uint32_t* nid,
                                                      uint32_t* owner, uint32_t* status)
{
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    const Prim d = prim_data(prims[i]);
    P[i] = d;
    cur[i] = i; nid[i] = 0; owner[i] = kNone;
    if (!prim_finite(d)) atomicOr(status, kBadInput);
}

// rank among the level's open nodes of the node that holds position p, or kNone
__device__ inline uint32_t open_rank(const uint32_t* nid, const BNode* bn, uint32_t p, uint32_t n)
{
    if (p >= n) return kNone;
    const uint32_t id = nid[p];
    if (id == kNone) return kNone;
    return bn[id].kind == kOpen ? bn[id].big : kNone;
}

__global__ void __launch_bounds__(kBlock) k_sah_reduce(const Prim* P, const uint32_t* cur, const uint32_t* nid, const BNode* bn, uint32_t n,
                                                       uint64_t* kmin, uint64_t* kmax, uint32_t* status)
{
    __shared__ uint64_t smin[kSlots * 6], smax[kSlots * 6];
    __shared__ uint32_t sfirst;
    init_keys<kBlock, kSlots * 6>(smin, smax);
    init_first(&sfirst);
    __syncthreads();
    const uint32_t p = blockIdx.x * kBlock + threadIdx.x;
    const uint32_t br = open_rank(nid, bn, p, n);
    if (br != kNone) atomicMin(&sfirst, br);
    __syncthreads();
    if (br != kNone) {
        const uint32_t slot = br - sfirst;
        if (slot >= (uint32_t)kSlots) atomicOr(status, kInternal);
        else {
            const uint32_t i = cur[p];
            uint64_t km[6], kx[6];
            node_keys(P[i], i, km, kx);
            for (int j = 0; j < 6; j++) { lds_min(&smin[slot * 6 + j], km[j]); lds_max(&smax[slot * 6 + j], kx[j]); }
        }
    }
    __syncthreads();
    if (sfirst == kNone) return;
    flush_keys<kBlock, kSlots * 6>(smin, smax, kmin + sfirst * 6, kmax + sfirst * 6);   // their ranks are < the level's open nodes
}

__global__ void __launch_bounds__(kBlock) k_sah_bins(const Prim* P, const uint32_t* cur, const uint32_t* nid, const BNode* bn, uint32_t n,
                                                     const uint64_t* kmin, const uint64_t* kmax, uint64_t* bkmin, uint64_t* bkmax,
                                                     uint32_t* bcnt, uint32_t* status)
{
    __shared__ uint64_t smin[kSlots * kBinKeys], smax[kSlots * kBinKeys];
    __shared__ uint32_t scnt[kSlots * kCnt];
    __shared__ uint32_t sfirst;
    init_keys<kBlock, kSlots * kBinKeys>(smin, smax);
    init_counts<kBlock, kSlots * kCnt>(scnt);
    init_first(&sfirst);
    __syncthreads();
    const uint32_t p = blockIdx.x * kBlock + threadIdx.x;
    const uint32_t br = open_rank(nid, bn, p, n);
    if (br != kNone) atomicMin(&sfirst, br);
    __syncthreads();
    if (br != kNone) {
        const uint32_t slot = br - sfirst;
        if (slot >= (uint32_t)kSlots) atomicOr(status, kInternal);
        else {
            const uint32_t i = cur[p];
            const Prim d = P[i];
            float mn[3], mx[3], cmin[3], cmax[3];
            node_from_keys(kmin + br * 6, kmax + br * 6, mn, mx, cmin, cmax);
            for (int a = 0; a < 3; a++) {
                if (cmin[a] == cmax[a]) continue;
                int b;
                if (!bin_of(d.c[a], cmin[a], cmax[a], b)) { atomicOr(status, kBadBin); continue; }
                const int s = a * kBins + b;
                atomicAdd(&scnt[slot * kCnt + s], 1u);
                for (int k = 0; k < 3; k++) {
                    lds_min(&smin[slot * kBinKeys + s * 3 + k], key_min(d.mn[k], i));
                    lds_max(&smax[slot * kBinKeys + s * 3 + k], key_max(d.mx[k], i));
                }
            }
        }
    }
    __syncthreads();
    if (sfirst == kNone) return;
    flush_keys<kBlock, kSlots * kBinKeys>(smin, smax, bkmin + sfirst * kBinKeys, bkmax + sfirst * kBinKeys);
    flush_counts<kBlock, kSlots * kCnt>(scnt, bcnt + sfirst * kCnt);
}

__global__ void __launch_bounds__(kBlock) k_sah_decide(BNode* bn, uint32_t lb, uint32_t le, const uint64_t* kmin, const uint64_t* kmax,
                                                       const uint64_t* bkmin, const uint64_t* bkmax, const uint32_t* bcnt, uint32_t* status)
{
    const uint32_t id = lb + blockIdx.x * kBlock + threadIdx.x;
    if (id >= le) return;
    BNode N = bn[id];
    if (N.kind != kOpen) return;
    float cmin[3], cmax[3];
    node_from_keys(kmin + N.big * 6, kmax + N.big * 6, N.mn, N.mx, cmin, cmax);
    Bins B;
    bins_from_keys(bkmin + (size_t)N.big * kBinKeys, bkmax + (size_t)N.big * kBinKeys, bcnt + (size_t)N.big * kCnt, B);
    Decision d;
    if (!decide(N.cnt, N.mn, N.mx, cmin, cmax, B, d)) { atomicOr(status, kNoDecision); return; }
    apply_decision(N, d);
    bn[id] = N;
}

__global__ void __launch_bounds__(kBlock) k_sah_small(const Prim* P, const uint32_t* cur, BNode* bn, uint32_t lb, uint32_t le, uint32_t* sA,
                                                      uint32_t* sB, uint32_t* sout, LNode* snodes, uint32_t* status)
{
    const uint32_t id = lb + blockIdx.x * kBlock + threadIdx.x;
    if (id >= le) return;
    BNode& N = bn[id];
    if (N.kind != kSmallRoot) return;
    const uint32_t h = N.home;
    for (uint32_t j = 0; j < N.cnt; j++) sA[h + j] = cur[h + j];
    SubResult r;
    const int rc = build_small(P, sA + h, sB + h, N.cnt, sout + h, snodes + 2 * (size_t)h, r);
    if (rc) { atomicOr(status, rc == kErrBin ? kBadBin : kNoDecision); return; }
    apply_small(N, snodes[2 * (size_t)h], r);
}

__global__ void __launch_bounds__(kBlock) k_sah_flag(const Prim* P, const uint32_t* cur, const uint32_t* nid, const BNode* bn, uint32_t n,
                                                     uint32_t* f)
{
    const uint32_t p = blockIdx.x * kBlock + threadIdx.x;
    if (p > n) return;
    uint32_t v = 0;
    if (p < n && nid[p] != kNone) {
        const BNode& N = bn[nid[p]];
        if (N.kind == kSplit) v = goes_left(P[cur[p]], N.axis, N.pos) ? 1 : 0;
    }
    f[p] = v;
}

__global__ void __launch_bounds__(kBlock) k_sah_count(BNode* bn, uint32_t lb, uint32_t le, const uint32_t* F, uint64_t* v)
{
    const uint32_t t = blockIdx.x * kBlock + threadIdx.x;
    if (lb + t >= le) return;
    BNode& N = bn[lb + t];
    v[t] = N.kind == kSplit ? count_split(N, F[N.home + N.cnt] - F[N.home]) : 0;
}

__global__ void __launch_bounds__(kBlock) k_sah_children(BNode* bn, uint32_t lb, uint32_t le, uint32_t cap, const uint64_t* v,
                                                         const uint64_t* V, uint32_t* summary)
{
    const uint32_t t = blockIdx.x * kBlock + threadIdx.x;
    if (lb + t >= le) return;
    if (lb + t == le - 1) { const uint64_t all = V[t] + v[t]; summary[0] = (uint32_t)all; summary[1] = (uint32_t)(all >> 32); }
    BNode& N = bn[lb + t];
    if (N.kind != kSplit) return;
    BNode L, R;
    make_children(N, V[t], le, L, R);
    if (N.left + 1 >= cap) { atomicOr(&summary[2], kInternal); return; }
    bn[N.left] = L;
    bn[N.left + 1] = R;
}

__global__ void __launch_bounds__(kBlock) k_sah_scatter(const uint32_t* cur, const uint32_t* nid, const BNode* bn, uint32_t n,
                                                        const uint32_t* f, const uint32_t* F, uint32_t* nxt, uint32_t* nidN, uint32_t* owner)
{
    const uint32_t p = blockIdx.x * kBlock + threadIdx.x;
    if (p >= n) return;
    const uint32_t id = nid[p];
    if (id == kNone) { nxt[p] = cur[p]; nidN[p] = kNone; return; }
    const BNode& N = bn[id];
    if (N.kind == kSplit) {
        const bool left = f[p] != 0;
        const uint32_t dst = scatter_dst(N, p, F[p] - F[N.home], left);   // inside [home, home + cnt): a permutation of it
        nxt[dst] = cur[p];
        nidN[dst] = left ? N.left : N.left + 1;
    } else {
        nxt[p] = cur[p]; nidN[p] = kNone; owner[p] = id;
    }
}

__global__ void __launch_bounds__(kBlock) k_sah_up(BNode* bn, uint32_t lb, uint32_t le)
{
    const uint32_t id = lb + blockIdx.x * kBlock + threadIdx.x;
    if (id >= le || bn[id].kind != kSplit) return;
    const uint32_t l = bn[id].left;
    up(bn[id], bn[l], bn[l + 1]);
}

__global__ void __launch_bounds__(kBlock) k_sah_down(BNode* bn, uint32_t lb, uint32_t le)
{
    const uint32_t id = lb + blockIdx.x * kBlock + threadIdx.x;
    if (id >= le || bn[id].kind != kSplit) return;
    const uint32_t l = bn[id].left;
    down(bn[id], bn[l], bn[l + 1]);
}

__global__ void __launch_bounds__(kBlock) k_sah_emit(const BNode* bn, uint32_t total, const LNode* snodes, uint32_t nodeBase,
                                                     uint32_t idxBase, RtBVHNode2* nodes, uint32_t outCap, uint32_t* status)
{
    const uint32_t id = blockIdx.x * kBlock + threadIdx.x;
    if (id >= total) return;
    const BNode& N = bn[id];
    if (N.kind != kSmallRoot) {
        if (N.gid >= outCap) { atomicOr(status, kInternal); return; }
        nodes[N.gid] = emit_level(N, nodeBase, idxBase);
        return;
    }
    for (uint32_t j = 0; j < 2 * N.interiors + 1; j++) {
        const uint32_t o = small_index(N, j);
        if (o >= outCap || j >= 2 * N.cnt - 1) { atomicOr(status, kInternal); return; }
        nodes[o] = emit_small(N, snodes[2 * (size_t)N.home + j], nodeBase, idxBase);
    }
}

__global__ void __launch_bounds__(kBlock) k_sah_emit_refs(const BNode* bn, const uint32_t* owner, const uint32_t* cur, const uint32_t* sout,
                                                          uint32_t n, uint32_t first, uint32_t* primIdx, uint32_t* status)
{
    const uint32_t p = blockIdx.x * kBlock + threadIdx.x;
    if (p >= n) return;
    const uint32_t o = owner[p];
    if (o == kNone) { atomicOr(status, kInternal); return; }
    const BNode& N = bn[o];
    const uint32_t dst = N.offset + (p - N.home);
    if (dst >= n) { atomicOr(status, kInternal); return; }
    primIdx[dst] = first + (N.kind == kSmallRoot ? sout[p] : cur[p]);
}

// The carved workspace of one build of n primitives (everything but the primitives and the output arrays)
struct Carve {
    size_t oSum, oP, oCur, oNxt, oNid, oNidN, oOwn, of, oF, oSA, oSB, oSout, oSn, oBn, ov, oV, oKA, oKB, oScan, scanBytes, total;
};
hipError_t carve_work(uint32_t n, hipStream_t s, Carve& c)
{
    const uint32_t cap = 2 * n - 1, bigMax = n / (kSmall + 1) + 1;
    size_t scan32 = 0, scan64 = 0;
    hipError_t e = hipcub::DeviceScan::ExclusiveSum(nullptr, scan32, (uint32_t*)nullptr, (uint32_t*)nullptr, (int)(n + 1), s);
    if (e != hipSuccess) return e;
    e = hipcub::DeviceScan::ExclusiveSum(nullptr, scan64, (uint64_t*)nullptr, (uint64_t*)nullptr, (int)cap, s);
    if (e != hipSuccess) return e;
    c.scanBytes = scan32 > scan64 ? scan32 : scan64;
    size_t off = 0;
    auto carve = [&](size_t bytes) { const size_t o = off; off += align_up(bytes); return o; };
    c.oSum = carve(4 * sizeof(uint32_t)); c.oP = carve(n * sizeof(Prim));
    c.oCur = carve(n * 4ull); c.oNxt = carve(n * 4ull); c.oNid = carve(n * 4ull); c.oNidN = carve(n * 4ull); c.oOwn = carve(n * 4ull);
    c.of = carve((n + 1) * 4ull); c.oF = carve((n + 1) * 4ull); c.oSA = carve(n * 4ull); c.oSB = carve(n * 4ull); c.oSout = carve(n * 4ull);
    c.oSn = carve(2ull * n * sizeof(LNode)); c.oBn = carve((size_t)cap * sizeof(BNode)); c.ov = carve(cap * 8ull); c.oV = carve(cap * 8ull);
    c.oKA = carve((size_t)bigMax * kKeys * 8); c.oKB = carve((size_t)bigMax * (kKeys * 8 + kCnt * 4));
    c.oScan = carve(c.scanBytes);
    c.total = off;
    return hipSuccess;
}

} // namespace

extern "C" int rt_debug_sah_phases(float* out)
{
    if (!out) return RT_E_INVALID;
    for (int i = 0; i < 5; i++) out[i] = g_phases[i];
    return RT_OK;
}

namespace sahdev {

const char* check_args(int32_t nPrims, int32_t first, int32_t count, uint32_t nodeBase, uint32_t idxBase)
{
    static const RtPrimitive prim{}; static const RtBVHNode2 node{}; static const int32_t n = 0; static const uint32_t idx = 0;   // (only their presence is checked)
    return sah::check_args(&prim, nPrims, first, count, nodeBase, idxBase, &node, count > 0 ? 2 * count - 1 : 0, &n, &idx);
}

int work_bytes(const char* who, uint32_t n, hipStream_t s, size_t* bytes)
{
    Carve c;
    BUILD_CHK(carve_work(n, s, c));
    *bytes = c.total;
    return RT_OK;
}

// The build proper (build_cores.h): everything stays on the device; the host reads three words per level, then the root's record.
int build(const char* who, hipStream_t stream, void* work, const RtPrimitive* dPrims, uint32_t n, uint32_t first, uint32_t nodeBase,
          uint32_t idxBase, RtBVHNode2* dNodes, uint32_t* dIdx, hipEvent_t evBegin, hipEvent_t evEnd, Built* out)
{
    const auto t0 = builddev::Clock::now();
    const uint32_t cap = 2 * n - 1, bigMax = n / (kSmall + 1) + 1;
    Carve c;
    BUILD_CHK(carve_work(n, stream, c));
    char* base = (char*)work;
    auto at = [&](size_t o) { return (void*)(base + o); };
    uint32_t* summary = (uint32_t*)at(c.oSum);
    Prim* P = (Prim*)at(c.oP);
    uint32_t *cur = (uint32_t*)at(c.oCur), *nxt = (uint32_t*)at(c.oNxt), *nid = (uint32_t*)at(c.oNid), *nidN = (uint32_t*)at(c.oNidN);
    uint32_t *owner = (uint32_t*)at(c.oOwn), *f = (uint32_t*)at(c.of), *F = (uint32_t*)at(c.oF);
    uint32_t *sA = (uint32_t*)at(c.oSA), *sB = (uint32_t*)at(c.oSB), *sout = (uint32_t*)at(c.oSout);
    LNode* snodes = (LNode*)at(c.oSn);
    BNode* bn = (BNode*)at(c.oBn);
    uint64_t *v = (uint64_t*)at(c.ov), *V = (uint64_t*)at(c.oV), *keysA = (uint64_t*)at(c.oKA), *keysB = (uint64_t*)at(c.oKB);
    size_t scanBytes = c.scanBytes;

    const BNode root = open_node(0, n, 0);
    BUILD_CHK(hipMemcpyAsync(bn, &root, sizeof root, hipMemcpyHostToDevice, stream));
    BUILD_CHK(hipMemsetAsync(summary, 0, 4 * sizeof(uint32_t), stream));
    if (evBegin) BUILD_CHK(hipEventRecord(evBegin, stream));
    hipLaunchKernelGGL(k_sah_prims, grid(n, kBlock), dim3(kBlock), 0, stream, dPrims, n, P, cur, nid, owner, summary + 2);
    BUILD_CHK(hipGetLastError());
    uint32_t hs[4] = { 0, 0, 0, 0 };
    BUILD_CHK(hipMemcpyAsync(hs, summary, sizeof hs, hipMemcpyDeviceToHost, stream));
    BUILD_CHK(hipStreamSynchronize(stream));   // (rt_build_bvh2_sah: nothing of the caller's host arrays is read after this point)
    if (hs[2]) return build_fail(RT_E_UNSUPPORTED, "%s: %s", who, status_text(hs[2]));
    const double tPrims = ms_since(t0);

    // level passes
    std::vector<std::pair<uint32_t, uint32_t>> levels;
    uint32_t lb = 0, le = 1, nBig = n > kSmall ? 1 : 0;
    for (;;) {
        levels.emplace_back(lb, le);
        const uint32_t K = le - lb;
        uint64_t *kmin = keysA, *bkmin = keysA + (size_t)nBig * 6, *kmax = keysB, *bkmax = keysB + (size_t)nBig * 6;
        uint32_t* bcnt = (uint32_t*)(keysB + (size_t)nBig * kKeys);
        if (nBig) {
            BUILD_CHK(hipMemsetAsync(keysA, 0xff, (size_t)nBig * kKeys * 8, stream));
            BUILD_CHK(hipMemsetAsync(keysB, 0, (size_t)nBig * (kKeys * 8 + kCnt * 4), stream));
            hipLaunchKernelGGL(k_sah_reduce, grid(n, kBlock), dim3(kBlock), 0, stream, P, cur, nid, bn, n, kmin, kmax, summary + 2);
            hipLaunchKernelGGL(k_sah_bins, grid(n, kBlock), dim3(kBlock), 0, stream, P, cur, nid, bn, n, kmin, kmax, bkmin, bkmax, bcnt, summary + 2);
        }
        hipLaunchKernelGGL(k_sah_decide, grid(K, kBlock), dim3(kBlock), 0, stream, bn, lb, le, kmin, kmax, bkmin, bkmax, bcnt, summary + 2);
        hipLaunchKernelGGL(k_sah_small, grid(K, kBlock), dim3(kBlock), 0, stream, P, cur, bn, lb, le, sA, sB, sout, snodes, summary + 2);
        hipLaunchKernelGGL(k_sah_flag, grid(n + 1, kBlock), dim3(kBlock), 0, stream, P, cur, nid, bn, n, f);
        BUILD_CHK(hipcub::DeviceScan::ExclusiveSum(at(c.oScan), scanBytes, f, F, (int)(n + 1), stream));
        hipLaunchKernelGGL(k_sah_count, grid(K, kBlock), dim3(kBlock), 0, stream, bn, lb, le, F, v);
        BUILD_CHK(hipcub::DeviceScan::ExclusiveSum(at(c.oScan), scanBytes, v, V, (int)K, stream));
        hipLaunchKernelGGL(k_sah_children, grid(K, kBlock), dim3(kBlock), 0, stream, bn, lb, le, cap, v, V, summary);
        hipLaunchKernelGGL(k_sah_scatter, grid(n, kBlock), dim3(kBlock), 0, stream, cur, nid, bn, n, f, F, nxt, nidN, owner);
        BUILD_CHK(hipGetLastError());
        std::swap(cur, nxt);
        std::swap(nid, nidN);
        BUILD_CHK(hipMemcpyAsync(hs, summary, sizeof hs, hipMemcpyDeviceToHost, stream));
        BUILD_CHK(hipStreamSynchronize(stream));
        if (hs[2]) return build_fail(RT_E_UNSUPPORTED, "%s: %s", who, status_text(hs[2]));
        if (hs[0] == 0) break;
        if ((uint64_t)le + 2ull * hs[0] > cap || hs[1] > bigMax)
            return build_fail(RT_E_DEVICE, "%s: inconsistent device result (%u splits, %u open nodes)", who, hs[0], hs[1]);
        lb = le; le += 2 * hs[0]; nBig = hs[1];
    }
    const double tLevels = ms_since(t0) - tPrims;

    // numbering and emit
    for (size_t l = levels.size(); l-- > 0;)
        hipLaunchKernelGGL(k_sah_up, grid(levels[l].second - levels[l].first, kBlock), dim3(kBlock), 0, stream, bn, levels[l].first, levels[l].second);
    for (const auto& L : levels)
        hipLaunchKernelGGL(k_sah_down, grid(L.second - L.first, kBlock), dim3(kBlock), 0, stream, bn, L.first, L.second);
    const uint32_t total = levels.back().second;
    hipLaunchKernelGGL(k_sah_emit, grid(total, kBlock), dim3(kBlock), 0, stream, bn, total, snodes, nodeBase, idxBase, dNodes, cap, summary + 2);
    hipLaunchKernelGGL(k_sah_emit_refs, grid(n, kBlock), dim3(kBlock), 0, stream, bn, owner, cur, sout, n, first, dIdx, summary + 2);
    BUILD_CHK(hipGetLastError());
    if (evEnd) BUILD_CHK(hipEventRecord(evEnd, stream));
    BNode top;
    BUILD_CHK(hipMemcpyAsync(&top, bn, sizeof top, hipMemcpyDeviceToHost, stream));
    BUILD_CHK(hipMemcpyAsync(hs, summary, sizeof hs, hipMemcpyDeviceToHost, stream));
    BUILD_CHK(hipStreamSynchronize(stream));
    const uint32_t outNodes = 2 * top.interiors + 1;
    if (hs[2] || outNodes > cap)
        return build_fail(RT_E_DEVICE, "%s: inconsistent device result (%s, %u nodes)", who, status_text(hs[2]), outNodes);
    out->nodes = outNodes; out->leaves = top.interiors + 1; out->depth = top.depth; out->cost = top.cost; out->mortonBits = 0;
    out->levels = (uint32_t)levels.size();
    out->ms[0] = (float)tPrims; out->ms[1] = (float)tLevels; out->ms[2] = (float)(ms_since(t0) - tPrims - tLevels);
    return RT_OK;
}

} // namespace sahdev

// The C-ABI entry: a session on the device, then builddev::build_flat around sahdev::build.
extern "C" int rt_build_bvh2_sah(int32_t device, const RtPrimitive* prims, int32_t nPrims, int32_t first, int32_t count, uint32_t nodeBase,
                                 uint32_t idxBase, RtBVHNode2* nodes, int32_t nodeCap, int32_t* nNodes, uint32_t* primIdx, RtBuildStats* stats)
{
    const char* who = "rt_build_bvh2_sah";
    const auto t0 = builddev::Clock::now();
    if (const char* msg = check_args(prims, nPrims, first, count, nodeBase, idxBase, nodes, nodeCap, nNodes, primIdx))
        return build_fail(RT_E_INVALID, "rt_build_bvh2_sah: %s", msg);
    builddev::Session w;
    if (const int rc = builddev::open_session(who, device, w)) return rc;
    const uint32_t n = (uint32_t)count;
    Built b{};
    builddev::FlatTimes t{};
    const int rc = builddev::build_flat(who, w, t0, sahdev::work_bytes, prims, first, n, nodes, nNodes, primIdx, stats,
        [&](void* work, const RtPrimitive* dPrims, RtBVHNode2* dNodes, uint32_t* dIdx, Built* out) {
            return sahdev::build(who, w.stream, work, dPrims, n, (uint32_t)first, nodeBase, idxBase, dNodes, dIdx, w.ev[0], w.ev[1], out);
        }, &b, &t);
    if (rc != RT_OK) return rc;
    g_phases[0] = (float)t.alloc + b.ms[0]; g_phases[1] = b.ms[1]; g_phases[2] = b.ms[2]; g_phases[3] = (float)(t.done - t.built);
    g_phases[4] = (float)b.levels;
    return RT_OK;
}

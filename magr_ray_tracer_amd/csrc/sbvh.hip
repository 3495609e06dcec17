// sbvh.hip — rt_build_bvh2_sbvh (include/rt355.h): BVH2::BuildBLAS for any alpha in [0, 1], spatial splits included, built on the GPU.
// The formulation and every value it computes are defined in sbvh_common.h; this file only distributes that work over kernels.
// host/sbvh_host.cpp runs the same steps in sequence (rth_build_bvh2_sbvh); both equal BuildBLAS's arrays byte for byte.
//
// Per level (its nodes are the build ids [lb, le), all open; position p of the level's ref array belongs to node nid[p]):
//   k_sbvh_reduce    padded-bounds, centroid and exact-bounds keys of the nodes (LDS slots per workgroup, then 64-bit atomicMin / Max;
//                    a workgroup that meets more than kSlots nodes sends the rest straight to the global keys)
//   k_sbvh_obins     object-bin counts and bin-box keys per (node, axis, bin), the same way
//   k_sbvh_decide1   one thread per node: the object sweep with the winning plane's overlap, the test overlap / rootArea > alpha
//   k_sbvh_sbins     one thread per ref of the nodes that ask for a spatial search: bin range, one clip per spanned slab, entries /
//                    exits and bin-box keys, the same way; flags an undefined bin index
//   k_sbvh_decide2   the spatial sweep and the decision
//   k_sbvh_flag      0, 1 or 2 fragments per ref; hipcub::DeviceScan places them
//   k_sbvh_count     the termination guard, statistics, the children's contribution to the scan that places them and their segments;
//   k_sbvh_children  writes them.  The host reads the summary (splits, refs of the next level, status), grows the arrays, then
//   k_sbvh_scatter   the stable scatter of the fragments (box, primitive, clipped flag, node) into the next level's arrays
// The refs of leaves stay behind: the per-level (node, primitive) arrays are kept until k_sbvh_emit_refs writes primIdx.  Then, with
// kernel boundaries between levels: k_sbvh_up, k_sbvh_down (sah_common.h's numbering), k_sbvh_emit.
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>
#include <algorithm>
#include <cstdlib>
#include <utility>
#include <vector>
#include "../../include/rt355.h"
#include "sbvh_common.h"
#include "build_dev.h"
#include "fold_dev.h"

using namespace sbvh;
using namespace fold;
using builddev::align_up;
using builddev::build_fail;
using builddev::grid;
using builddev::ms_since;

// Device blocks that outlive a build (build_cores.h): a caller that builds again and again (rt_rebuild_scene, every frame) hands the
// same pool to every build, and the builds take their arrays from it.  Requests are rounded up to size classes (2^k and 3 * 2^(k-1)
// bytes) and a request only ever takes a free block of its own class, so a build that asks for the same sizes in the same order as
// an earlier one finds every block it needs: no hipMalloc, and no hipFree (which waits for the whole device) between frames.
// Blocks are reused in stream order only (one stream per pool).
namespace sbvhdev {
struct Pool {
    struct Block { void* p; size_t cap; bool used; };
    std::vector<Block> blocks;
    uint64_t allocations = 0;
    ~Pool() { for (Block& b : blocks) (void)hipFree(b.p); }
};
Pool* pool_create() { return new Pool(); }
void pool_destroy(Pool* p) { delete p; }
uint64_t pool_allocations(const Pool* p) { return p ? p->allocations : 0; }
}

namespace {

size_t size_class(size_t bytes)
{
    size_t c = 256;
    while (c < bytes) {
        if (c + c / 2 >= bytes) return c + c / 2;
        c *= 2;
    }
    return c;
}
// *bytes in: what is needed; out: what the block holds
hipError_t pool_alloc(sbvhdev::Pool* pool, void** out, size_t* bytes)
{
    if (!pool) return hipMalloc(out, *bytes);
    const size_t c = size_class(*bytes);
    *bytes = c;
    for (sbvhdev::Pool::Block& b : pool->blocks) if (!b.used && b.cap == c) { b.used = true; *out = b.p; return hipSuccess; }
    const hipError_t e = hipMalloc(out, c);
    if (e != hipSuccess) return e;
    pool->blocks.push_back({ *out, c, true });
    pool->allocations++;
    return hipSuccess;
}
void pool_free(sbvhdev::Pool* pool, void* p)
{
    if (!pool) { (void)hipFree(p); return; }
    for (sbvhdev::Pool::Block& b : pool->blocks) if (b.p == p) { b.used = false; return; }
}

constexpr int kBlock = 256;
constexpr int kSlots = 16;                          // nodes per workgroup that are folded in LDS; further ones go to global memory
constexpr int kCnt = 3 * kBins;
// summary words: splits, refs of the next level, status, spatial splits, clipped primitives, forced leaves
constexpr int kSumWords = 8, kSumStatus = 2, kSumSpatial = 3, kSumClipped = 4, kSumForced = 5;

float g_phases[8] = { 0, 0, 0, 0, 0, 0, 0, 0 };   // rt_debug_sbvh_phases

__global__ void __launch_bounds__(kBlock) k_sbvh_prims(const RtPrimitive* prims, uint32_t n, Ref* refs, uint32_t* nid, uint32_t* prim,
                                                       uint32_t* status)
{
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    const Prim d = prim_data(prims[i]);
    refs[i] = ref_of(d, i);
    nid[i] = 0; prim[i] = i;
    if (!prim_finite(d)) atomicOr(status, kBadInput);
}

// m refs of the level [lb, lb + K); kmin / kmax: K * kNodeKeys keys
__global__ void __launch_bounds__(kBlock) k_sbvh_reduce(const Ref* refs, const uint32_t* nid, uint32_t m, uint32_t lb, uint32_t K,
                                                        uint64_t* kmin, uint64_t* kmax, uint32_t* status)
{
    __shared__ uint64_t smin[kSlots * kNodeKeys], smax[kSlots * kNodeKeys];
    __shared__ uint32_t sfirst;
    init_keys<kBlock, kSlots * kNodeKeys>(smin, smax);
    init_first(&sfirst);
    __syncthreads();
    const uint32_t p = blockIdx.x * kBlock + threadIdx.x;
    uint32_t t = kNone;
    if (p < m) {
        t = nid[p] - lb;
        if (t >= K) { atomicOr(status, kInternal); t = kNone; }
    }
    if (t != kNone) atomicMin(&sfirst, t);
    __syncthreads();
    if (t != kNone) {
        uint64_t km[kNodeKeys], kx[kNodeKeys];
        ref_keys(refs[p], km, kx);
        const uint32_t slot = t - sfirst;
        if (slot < (uint32_t)kSlots)
            for (int j = 0; j < kNodeKeys; j++) { lds_min(&smin[slot * kNodeKeys + j], km[j]); lds_max(&smax[slot * kNodeKeys + j], kx[j]); }
        else
            for (int j = 0; j < kNodeKeys; j++) { glb_min(&kmin[(size_t)t * kNodeKeys + j], km[j]); glb_max(&kmax[(size_t)t * kNodeKeys + j], kx[j]); }
    }
    __syncthreads();
    if (sfirst == kNone) return;
    flush_keys<kBlock, kSlots * kNodeKeys>(smin, smax, kmin + (size_t)sfirst * kNodeKeys, kmax + (size_t)sfirst * kNodeKeys);   // their nodes are < K
}

__global__ void __launch_bounds__(kBlock) k_sbvh_obins(const Ref* refs, const uint32_t* nid, uint32_t m, uint32_t lb, uint32_t K,
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
    uint32_t t = kNone;
    if (p < m) { t = nid[p] - lb; if (t >= K) t = kNone; }
    if (t != kNone) atomicMin(&sfirst, t);
    __syncthreads();
    if (t != kNone) {
        const Ref r = refs[p];
        const uint32_t slot = t - sfirst;
        const bool local = slot < (uint32_t)kSlots;
        float mn[3], mx[3], cmin[3], cmax[3];
        node_from_keys(kmin + (size_t)t * kNodeKeys, kmax + (size_t)t * kNodeKeys, mn, mx, cmin, cmax);
        for (int a = 0; a < 3; a++) {
            if (cmin[a] == cmax[a]) continue;
            int b;
            if (!bin_of(center(r, a), cmin[a], cmax[a], b)) { atomicOr(status, kBadBin); continue; }
            const int s = a * kBins + b;
            if (local) {
                atomicAdd(&scnt[slot * kCnt + s], 1u);
                for (int k = 0; k < 3; k++) {
                    lds_min(&smin[slot * kBinKeys + s * 3 + k], key_min(r.mn[k], r.prim));
                    lds_max(&smax[slot * kBinKeys + s * 3 + k], key_max(r.mx[k], r.prim));
                }
            } else {
                atomicAdd(&bcnt[(size_t)t * kCnt + s], 1u);
                for (int k = 0; k < 3; k++) {
                    glb_min(&bkmin[(size_t)t * kBinKeys + s * 3 + k], key_min(r.mn[k], r.prim));
                    glb_max(&bkmax[(size_t)t * kBinKeys + s * 3 + k], key_max(r.mx[k], r.prim));
                }
            }
        }
    }
    __syncthreads();
    if (sfirst == kNone) return;
    flush_keys<kBlock, kSlots * kBinKeys>(smin, smax, bkmin + (size_t)sfirst * kBinKeys, bkmax + (size_t)sfirst * kBinKeys);
    flush_counts<kBlock, kSlots * kCnt>(scnt, bcnt + (size_t)sfirst * kCnt);
}

__global__ void __launch_bounds__(kBlock) k_sbvh_decide1(SNode* bn, uint32_t lb, uint32_t le, float alpha, const uint64_t* kmin,
                                                         const uint64_t* kmax, const uint64_t* bkmin, const uint64_t* bkmax,
                                                         const uint32_t* bcnt)
{
    const uint32_t t = blockIdx.x * kBlock + threadIdx.x;
    if (lb + t >= le) return;
    SNode N = bn[lb + t];
    float cmin[3], cmax[3];
    node_from_keys(kmin + (size_t)t * kNodeKeys, kmax + (size_t)t * kNodeKeys, N.b.mn, N.b.mx, cmin, cmax);
    Bins B;
    bins_from_keys(bkmin + (size_t)t * kBinKeys, bkmax + (size_t)t * kBinKeys, bcnt + (size_t)t * kCnt, B);
    // the BLAS root's area: the root's bounds are final after level 0 (at level 0 this thread is the root)
    const float rootArea = lb == 0 ? area(N.b.mn, N.b.mx) : area(bn[0].b.mn, bn[0].b.mx);
    decide_object(N, cmin, cmax, B, rootArea, alpha);
    bn[lb + t] = N;
}

__global__ void __launch_bounds__(kBlock) k_sbvh_sbins(const Ref* refs, const uint32_t* nid, const RtPrimitive* prims, const SNode* bn,
                                                       uint32_t m, uint32_t lb, uint32_t K, const uint64_t* kmin, const uint64_t* kmax,
                                                       uint64_t* skmin, uint64_t* skmax, uint32_t* sent, uint32_t* sext, uint32_t* status)
{
    __shared__ uint64_t smin[kSlots * kBinKeys], smax[kSlots * kBinKeys];
    __shared__ uint32_t sen[kSlots * kSpCnt], sex[kSlots * kSpCnt];
    __shared__ uint32_t sfirst;
    init_keys<kBlock, kSlots * kBinKeys>(smin, smax);
    init_counts<kBlock, kSlots * kSpCnt>(sen);
    init_counts<kBlock, kSlots * kSpCnt>(sex);
    init_first(&sfirst);
    __syncthreads();
    const uint32_t p = blockIdx.x * kBlock + threadIdx.x;
    uint32_t t = kNone;
    if (p < m) {
        t = nid[p] - lb;
        if (t >= K || !(bn[lb + t].flags & kWantSpatial)) t = kNone;
    }
    if (t != kNone) atomicMin(&sfirst, t);
    __syncthreads();
    if (t != kNone) {
        const Ref r = refs[p];
        const RtPrimitive& prim = prims[r.prim];
        const uint32_t slot = t - sfirst;
        const bool local = slot < (uint32_t)kSlots;
        float emn[3], emx[3];
        exact_from_keys(kmin + (size_t)t * kNodeKeys, kmax + (size_t)t * kNodeKeys, emn, emx);
        for (int a = 0; a < 3; a++) {
            if (emn[a] == emx[a]) continue;
            int f, l;
            const uint32_t st = spatial_ref(r, prim, a, emn[a], emx[a], f, l, [&](int b, const float* mn, const float* mx) {
                const int s = a * kBins + b;
                for (int k = 0; k < 3; k++) {
                    if (local) {
                        lds_min(&smin[slot * kBinKeys + s * 3 + k], key_min(mn[k], r.prim));
                        lds_max(&smax[slot * kBinKeys + s * 3 + k], key_max(mx[k], r.prim));
                    } else {
                        glb_min(&skmin[(size_t)t * kBinKeys + s * 3 + k], key_min(mn[k], r.prim));
                        glb_max(&skmax[(size_t)t * kBinKeys + s * 3 + k], key_max(mx[k], r.prim));
                    }
                }
            });
            if (st) { atomicOr(status, st); continue; }
            if (f >= 0) {
                if (local) { atomicAdd(&sen[slot * kSpCnt + a * kBins + f], 1u); atomicAdd(&sex[slot * kSpCnt + a * kBins + l], 1u); }
                else { atomicAdd(&sent[(size_t)t * kSpCnt + a * kBins + f], 1u); atomicAdd(&sext[(size_t)t * kSpCnt + a * kBins + l], 1u); }
            }
        }
    }
    __syncthreads();
    if (sfirst == kNone) return;
    flush_keys<kBlock, kSlots * kBinKeys>(smin, smax, skmin + (size_t)sfirst * kBinKeys, skmax + (size_t)sfirst * kBinKeys);
    flush_counts<kBlock, kSlots * kSpCnt>(sen, sent + (size_t)sfirst * kSpCnt);
    flush_counts<kBlock, kSlots * kSpCnt>(sex, sext + (size_t)sfirst * kSpCnt);
}

__global__ void __launch_bounds__(kBlock) k_sbvh_decide2(SNode* bn, uint32_t lb, uint32_t le, const uint64_t* kmin, const uint64_t* kmax,
                                                         const uint64_t* skmin, const uint64_t* skmax, const uint32_t* sent,
                                                         const uint32_t* sext, uint32_t* status)
{
    const uint32_t t = blockIdx.x * kBlock + threadIdx.x;
    if (lb + t >= le) return;
    SNode N = bn[lb + t];
    float emn[3], emx[3];
    exact_from_keys(kmin + (size_t)t * kNodeKeys, kmax + (size_t)t * kNodeKeys, emn, emx);
    SBins S;
    if (N.flags & kWantSpatial)
        sbins_from_keys(skmin + (size_t)t * kBinKeys, skmax + (size_t)t * kBinKeys, sent + (size_t)t * kSpCnt, sext + (size_t)t * kSpCnt, S);
    if (!decide_final(N, emn, emx, &S)) { atomicOr(status, kNoDecision); return; }
    bn[lb + t] = N;
}

// f[p] = fragments going left | fragments going right << 32 of ref p (0 for the refs of leaves and for p == m)
__global__ void __launch_bounds__(kBlock) k_sbvh_flag(const Ref* refs, const uint32_t* nid, const RtPrimitive* prims, const SNode* bn,
                                                      uint32_t m, uint64_t* f, uint32_t* summary)
{
    const uint32_t p = blockIdx.x * kBlock + threadIdx.x;
    if (p > m) return;
    uint64_t v = 0;
    if (p < m) {
        const SNode& N = bn[nid[p]];
        if (N.b.kind == kSplit) {
            const Ref r = refs[p];
            Ref L, R;
            bool overflow = false;
            const uint32_t e = split_ref(N, r, prims[r.prim], L, R, overflow);
            if (overflow) atomicOr(&summary[kSumStatus], kInternal);
            if (e & kStraddle) atomicAdd(&summary[kSumClipped], 1u);
            v = (uint64_t)((e & kEmitL) ? 1 : 0) | ((uint64_t)((e & kEmitR) ? 1 : 0) << 32);
        }
    }
    f[p] = v;
}

__global__ void __launch_bounds__(kBlock) k_sbvh_count(SNode* bn, uint32_t lb, uint32_t le, const uint64_t* F, uint64_t* v, uint32_t* summary)
{
    const uint32_t t = blockIdx.x * kBlock + threadIdx.x;
    if (lb + t >= le) return;
    SNode& N = bn[lb + t];
    const uint64_t d = F[N.b.home + N.b.cnt] - F[N.b.home];
    uint32_t sp, fo;
    v[t] = count_node(N, (uint32_t)d, (uint32_t)(d >> 32), sp, fo);
    if (sp) atomicAdd(&summary[kSumSpatial], 1u);
    if (fo) atomicAdd(&summary[kSumForced], 1u);
}

__global__ void __launch_bounds__(kBlock) k_sbvh_children(SNode* bn, uint32_t lb, uint32_t le, uint32_t cap, const uint64_t* v,
                                                          const uint64_t* V, uint32_t* summary)
{
    const uint32_t t = blockIdx.x * kBlock + threadIdx.x;
    if (lb + t >= le) return;
    if (lb + t == le - 1) { const uint64_t all = V[t] + v[t]; summary[0] = (uint32_t)all; summary[1] = (uint32_t)(all >> 32); }
    SNode& N = bn[lb + t];
    if (N.b.kind != kSplit) return;
    SNode L, R;
    make_schildren(N, V[t], le, L, R);
    if ((uint64_t)N.b.left + 1 >= cap) { atomicOr(&summary[kSumStatus], kInternal); return; }
    bn[N.b.left] = L;
    bn[N.b.left + 1] = R;
}

__global__ void __launch_bounds__(kBlock) k_sbvh_scatter(const Ref* refs, const uint32_t* nid, const RtPrimitive* prims, const SNode* bn,
                                                         uint32_t m, uint32_t bnCap, const uint64_t* F, Ref* refsN, uint32_t* nidN,
                                                         uint32_t* primN, uint32_t mNext, uint32_t* status)
{
    const uint32_t p = blockIdx.x * kBlock + threadIdx.x;
    if (p >= m) return;
    const SNode& N = bn[nid[p]];
    if (N.b.kind != kSplit) return;
    if ((uint64_t)N.b.left + 1 >= bnCap) { atomicOr(status, kInternal); return; }
    const Ref r = refs[p];
    Ref L, R;
    bool overflow = false;
    const uint32_t e = split_ref(N, r, prims[r.prim], L, R, overflow);
    const uint64_t d = F[p] - F[N.b.home];
    if (e & kEmitL) {
        const uint32_t dst = bn[N.b.left].b.home + (uint32_t)d;
        if (dst >= mNext) atomicOr(status, kInternal);
        else { refsN[dst] = L; nidN[dst] = N.b.left; primN[dst] = L.prim; }
    }
    if (e & kEmitR) {
        const uint32_t dst = bn[N.b.left + 1].b.home + (uint32_t)(d >> 32);
        if (dst >= mNext) atomicOr(status, kInternal);
        else { refsN[dst] = R; nidN[dst] = N.b.left + 1; primN[dst] = R.prim; }
    }
}

__global__ void __launch_bounds__(kBlock) k_sbvh_up(SNode* bn, uint32_t lb, uint32_t le)
{
    const uint32_t id = lb + blockIdx.x * kBlock + threadIdx.x;
    if (id >= le || bn[id].b.kind != kSplit) return;
    const uint32_t l = bn[id].b.left;
    sup(bn[id], bn[l], bn[l + 1]);
}

__global__ void __launch_bounds__(kBlock) k_sbvh_down(SNode* bn, uint32_t lb, uint32_t le)
{
    const uint32_t id = lb + blockIdx.x * kBlock + threadIdx.x;
    if (id >= le || bn[id].b.kind != kSplit) return;
    const uint32_t l = bn[id].b.left;
    down(bn[id].b, bn[l].b, bn[l + 1].b);
}

__global__ void __launch_bounds__(kBlock) k_sbvh_emit(const SNode* bn, uint32_t total, uint32_t nodeBase, uint32_t idxBase, RtBVHNode2* nodes,
                                                      uint32_t outNodes, uint32_t* status)
{
    const uint32_t id = blockIdx.x * kBlock + threadIdx.x;
    if (id >= total) return;
    const BNode& N = bn[id].b;
    if (N.gid >= outNodes) { atomicOr(status, kInternal); return; }
    nodes[N.gid] = emit_level(N, nodeBase, idxBase);
}

__global__ void __launch_bounds__(kBlock) k_sbvh_emit_refs(const SNode* bn, uint32_t total, const uint32_t* nid, const uint32_t* prim, uint32_t m,
                                                           uint32_t first, uint32_t* primIdx, uint32_t outIdx, uint32_t* status)
{
    const uint32_t p = blockIdx.x * kBlock + threadIdx.x;
    if (p >= m) return;
    const uint32_t id = nid[p];
    if (id >= total) { atomicOr(status, kInternal); return; }
    const BNode& N = bn[id].b;
    if (N.kind != kLeaf) return;
    const uint64_t dst = (uint64_t)N.offset + (p - N.home);
    if (dst >= outIdx) { atomicOr(status, kInternal); return; }
    primIdx[dst] = first + prim[p];
}

// A device array that grows: ensure() keeps the first `keep` bytes when it has to move.  Its memory comes from the build's pool
// (sbvhdev::Pool, below) when there is one, from hipMalloc / hipFree otherwise.
struct DBuf {
    void* p = nullptr;
    size_t cap = 0;
    sbvhdev::Pool* pool = nullptr;
    explicit DBuf(sbvhdev::Pool* pl = nullptr) : pool(pl) {}
    DBuf(const DBuf&) = delete;
    DBuf& operator=(const DBuf&) = delete;
    ~DBuf() { if (p) pool_free(pool, p); }
    hipError_t ensure(size_t bytes, size_t keep, hipStream_t s)
    {
        if (bytes <= cap) return hipSuccess;
        size_t want = cap + cap / 2;
        if (want < bytes) want = bytes;
        void* q = nullptr;
        hipError_t e = pool_alloc(pool, &q, &want);
        if (e != hipSuccess) return e;
        if (keep && p) {
            e = hipMemcpyAsync(q, p, keep, hipMemcpyDeviceToDevice, s);
            if (e == hipSuccess) e = hipStreamSynchronize(s);
            if (e != hipSuccess) { pool_free(pool, q); return e; }
        }
        if (p) pool_free(pool, p);
        p = q; cap = want;
        return hipSuccess;
    }
};

// What one rt_build_bvh2_sbvh call owns on the device: the session's two allocations and the built tree, which goes while the stream
// still exists and is idle
struct SbvhSession : builddev::Session {
    void *&prims = mem[0], *&out = mem[1];   // the uploaded primitives; the emitted arrays
    sbvhdev::Tree* tree = nullptr;
    ~SbvhSession() { idle(); sbvhdev::destroy(tree); }
};

} // namespace

extern "C" int rt_debug_sbvh_phases(float* out)
{
    if (!out) return RT_E_INVALID;
    hipFuncAttributes a{};
    g_phases[5] = hipFuncGetAttributes(&a, (const void*)k_sbvh_sbins) == hipSuccess ? (float)a.localSizeBytes : -1.0f;
    g_phases[6] = hipFuncGetAttributes(&a, (const void*)k_sbvh_flag) == hipSuccess ? (float)a.localSizeBytes : -1.0f;
    g_phases[7] = hipFuncGetAttributes(&a, (const void*)k_sbvh_scatter) == hipSuccess ? (float)a.localSizeBytes : -1.0f;
    for (int i = 0; i < 8; i++) out[i] = g_phases[i];
    return RT_OK;
}

namespace sbvhdev {

// The device-side state of a finished build: the build nodes, numbered, and per level the (node, primitive) of every ref
struct Tree {
    Pool* pool;
    DBuf bn, summary;
    std::vector<void*> hist;                                  // per level: nid[m], then prim[m]
    std::vector<uint32_t> histN;
    std::vector<std::pair<uint32_t, uint32_t>> levels;
    uint32_t first = 0, nodeBase = 0, idxBase = 0, total = 0;
    SbvhBuilt built{};
    explicit Tree(Pool* pl) : pool(pl), bn(pl), summary(pl) {}
    ~Tree() { for (void* h : hist) if (h) pool_free(pool, h); }
};

void destroy(Tree* t) { delete t; }

int build(const char* who, hipStream_t stream, float alpha, const RtPrimitive* dPrims, uint32_t n, uint32_t first, uint32_t nodeBase,
          uint32_t idxBase, hipEvent_t evBegin, hipEvent_t evEnd, Pool* pool, Tree** treeOut, SbvhBuilt* out)
{
    const auto t0 = builddev::Clock::now();
    Tree* T = new Tree(pool);
    *treeOut = T;                                             // the caller destroys it, on failure too
    T->first = first; T->nodeBase = nodeBase; T->idxBase = idxBase;
    // the initial capacity of the ref arrays (they grow from the scan of every level)
    size_t refCap = (size_t)n + n / 2 + 1024;
    if (const char* env = getenv("RT355_SBVH_INITIAL_REFS")) {
        const long long k = atoll(env);
        if (k > 0) refCap = (size_t)k;
    }
    if (refCap < n) refCap = n;
    DBuf refsA(pool), refsB(pool), fbuf(pool), Fbuf(pool), scan(pool), lvl(pool);
    auto add_level = [&](uint32_t m) -> hipError_t {
        void* h = nullptr;
        size_t bytes = (size_t)(m ? m : 1) * 8;
        const hipError_t e = pool_alloc(pool, &h, &bytes);
        if (e != hipSuccess) return e;
        T->hist.push_back(h); T->histN.push_back(m);
        return hipSuccess;
    };
    BUILD_CHK(T->summary.ensure(kSumWords * sizeof(uint32_t), 0, stream));
    BUILD_CHK(T->bn.ensure(1024 * sizeof(SNode), 0, stream));
    BUILD_CHK(refsA.ensure(refCap * sizeof(Ref), 0, stream));
    BUILD_CHK(add_level(n));
    uint32_t* summary = (uint32_t*)T->summary.p;
    const SNode root = open_snode(0, n);
    BUILD_CHK(hipMemcpyAsync(T->bn.p, &root, sizeof root, hipMemcpyHostToDevice, stream));
    BUILD_CHK(hipMemsetAsync(summary, 0, kSumWords * sizeof(uint32_t), stream));
    if (evBegin) BUILD_CHK(hipEventRecord(evBegin, stream));
    hipLaunchKernelGGL(k_sbvh_prims, grid(n, kBlock), dim3(kBlock), 0, stream, dPrims, n, (Ref*)refsA.p, (uint32_t*)T->hist[0], (uint32_t*)T->hist[0] + n,
                       summary + kSumStatus);
    BUILD_CHK(hipGetLastError());
    uint32_t hs[kSumWords] = {};
    BUILD_CHK(hipMemcpyAsync(hs, summary, sizeof hs, hipMemcpyDeviceToHost, stream));
    BUILD_CHK(hipStreamSynchronize(stream));   // (rt_build_bvh2_sbvh: nothing of the caller's host arrays is read after this point)
    if (hs[kSumStatus]) return build_fail(RT_E_UNSUPPORTED, "%s: %s", who, sstatus_text(hs[kSumStatus]));
    const double tPrims = ms_since(t0);

    // level passes
    DBuf *cur = &refsA, *nxt = &refsB;
    uint32_t lb = 0, le = 1, m = n, peak = n;
    for (;;) {
        T->levels.emplace_back(lb, le);
        const uint32_t K = le - lb;
        // per-level arrays: keys (all bits set / zero are the empty min / max keys), counts, the node scan
        const size_t oKmin = 0, oBkmin = oKmin + (size_t)K * kNodeKeys * 8, oSkmin = oBkmin + (size_t)K * kBinKeys * 8;
        const size_t ffBytes = align_up(oSkmin + (size_t)K * kBinKeys * 8);
        const size_t oKmax = ffBytes, oBkmax = oKmax + (size_t)K * kNodeKeys * 8, oSkmax = oBkmax + (size_t)K * kBinKeys * 8;
        const size_t oBcnt = oSkmax + (size_t)K * kBinKeys * 8, oSent = oBcnt + (size_t)K * kCnt * 4, oSext = oSent + (size_t)K * kSpCnt * 4;
        const size_t zeroBytes = align_up(oSext + (size_t)K * kSpCnt * 4 - ffBytes);
        const size_t ov = ffBytes + zeroBytes, oV = ov + align_up((size_t)K * 8);
        BUILD_CHK(lvl.ensure(oV + align_up((size_t)K * 8), 0, stream));
        size_t scanA = 0, scanB = 0;
        BUILD_CHK(hipcub::DeviceScan::ExclusiveSum(nullptr, scanA, (uint64_t*)nullptr, (uint64_t*)nullptr, (int)(m + 1), stream));
        BUILD_CHK(hipcub::DeviceScan::ExclusiveSum(nullptr, scanB, (uint64_t*)nullptr, (uint64_t*)nullptr, (int)K, stream));
        size_t scanBytes = scanA > scanB ? scanA : scanB;
        BUILD_CHK(scan.ensure(scanBytes ? scanBytes : 256, 0, stream));
        BUILD_CHK(fbuf.ensure(((size_t)m + 1) * 8, 0, stream));
        BUILD_CHK(Fbuf.ensure(((size_t)m + 1) * 8, 0, stream));
        BUILD_CHK(T->bn.ensure(((size_t)le + 2 * (size_t)K) * sizeof(SNode), (size_t)le * sizeof(SNode), stream));
        const uint32_t bnCap = (uint32_t)std::min<size_t>(T->bn.cap / sizeof(SNode), 0xffffffffu);
        char* base = (char*)lvl.p;
        uint64_t *kmin = (uint64_t*)(base + oKmin), *bkmin = (uint64_t*)(base + oBkmin), *skmin = (uint64_t*)(base + oSkmin);
        uint64_t *kmax = (uint64_t*)(base + oKmax), *bkmax = (uint64_t*)(base + oBkmax), *skmax = (uint64_t*)(base + oSkmax);
        uint32_t *bcnt = (uint32_t*)(base + oBcnt), *sent = (uint32_t*)(base + oSent), *sext = (uint32_t*)(base + oSext);
        uint64_t *v = (uint64_t*)(base + ov), *V = (uint64_t*)(base + oV);
        uint64_t *f = (uint64_t*)fbuf.p, *F = (uint64_t*)Fbuf.p;
        SNode* bn = (SNode*)T->bn.p;
        const Ref* refs = (const Ref*)cur->p;
        const uint32_t* nid = (const uint32_t*)T->hist.back();
        BUILD_CHK(hipMemsetAsync(base, 0xff, ffBytes, stream));
        BUILD_CHK(hipMemsetAsync(base + ffBytes, 0, zeroBytes, stream));
        hipLaunchKernelGGL(k_sbvh_reduce, grid(m, kBlock), dim3(kBlock), 0, stream, refs, nid, m, lb, K, kmin, kmax, summary + kSumStatus);
        hipLaunchKernelGGL(k_sbvh_obins, grid(m, kBlock), dim3(kBlock), 0, stream, refs, nid, m, lb, K, kmin, kmax, bkmin, bkmax, bcnt, summary + kSumStatus);
        hipLaunchKernelGGL(k_sbvh_decide1, grid(K, kBlock), dim3(kBlock), 0, stream, bn, lb, le, alpha, kmin, kmax, bkmin, bkmax, bcnt);
        hipLaunchKernelGGL(k_sbvh_sbins, grid(m, kBlock), dim3(kBlock), 0, stream, refs, nid, dPrims, bn, m, lb, K, kmin, kmax, skmin, skmax, sent, sext,
                           summary + kSumStatus);
        hipLaunchKernelGGL(k_sbvh_decide2, grid(K, kBlock), dim3(kBlock), 0, stream, bn, lb, le, kmin, kmax, skmin, skmax, sent, sext, summary + kSumStatus);
        hipLaunchKernelGGL(k_sbvh_flag, grid(m + 1, kBlock), dim3(kBlock), 0, stream, refs, nid, dPrims, bn, m, f, summary);
        BUILD_CHK(hipcub::DeviceScan::ExclusiveSum(scan.p, scanBytes, f, F, (int)(m + 1), stream));
        hipLaunchKernelGGL(k_sbvh_count, grid(K, kBlock), dim3(kBlock), 0, stream, bn, lb, le, F, v, summary);
        BUILD_CHK(hipcub::DeviceScan::ExclusiveSum(scan.p, scanBytes, v, V, (int)K, stream));
        hipLaunchKernelGGL(k_sbvh_children, grid(K, kBlock), dim3(kBlock), 0, stream, bn, lb, le, bnCap, v, V, summary);
        BUILD_CHK(hipGetLastError());
        BUILD_CHK(hipMemcpyAsync(hs, summary, sizeof hs, hipMemcpyDeviceToHost, stream));
        BUILD_CHK(hipStreamSynchronize(stream));
        if (hs[kSumStatus] & kInternal) return build_fail(RT_E_DEVICE, "%s: %s", who, sstatus_text(hs[kSumStatus]));
        if (hs[kSumStatus]) return build_fail(RT_E_UNSUPPORTED, "%s: %s", who, sstatus_text(hs[kSumStatus]));
        const uint32_t splits = hs[0], mNext = hs[1];
        if (splits == 0) break;
        if (splits > K || (uint64_t)mNext > 2ull * m || mNext == 0)
            return build_fail(RT_E_DEVICE, "%s: inconsistent device result (%u splits of %u nodes, %u refs from %u)", who, splits, K, mNext, m);
        if (mNext > kMaxRefs - 1 || (uint64_t)le + 2ull * splits > kMaxRefs)
            return build_fail(RT_E_NOMEM, "%s: more than 2^31 refs or nodes", who);
        // the next level's arrays, sized from the scan
        if (nxt->ensure((size_t)mNext * sizeof(Ref), 0, stream) != hipSuccess || add_level(mNext) != hipSuccess)
            return build_fail(RT_E_NOMEM, "%s: device memory for %u refs", who, mNext);
        uint32_t* nidN = (uint32_t*)T->hist.back();
        hipLaunchKernelGGL(k_sbvh_scatter, grid(m, kBlock), dim3(kBlock), 0, stream, refs, nid, dPrims, bn, m, bnCap, F, (Ref*)nxt->p, nidN, nidN + mNext, mNext,
                           summary + kSumStatus);
        BUILD_CHK(hipGetLastError());
        std::swap(cur, nxt);
        m = mNext;
        if (m > peak) peak = m;
        lb = le; le += 2 * splits;
    }
    const double tLevels = ms_since(t0) - tPrims;

    // numbering
    SNode* bn = (SNode*)T->bn.p;
    for (size_t l = T->levels.size(); l-- > 0;)
        hipLaunchKernelGGL(k_sbvh_up, grid(T->levels[l].second - T->levels[l].first, kBlock), dim3(kBlock), 0, stream, bn, T->levels[l].first, T->levels[l].second);
    for (const auto& L : T->levels)
        hipLaunchKernelGGL(k_sbvh_down, grid(L.second - L.first, kBlock), dim3(kBlock), 0, stream, bn, L.first, L.second);
    BUILD_CHK(hipGetLastError());
    if (evEnd) BUILD_CHK(hipEventRecord(evEnd, stream));
    SNode top;
    BUILD_CHK(hipMemcpyAsync(&top, bn, sizeof top, hipMemcpyDeviceToHost, stream));
    BUILD_CHK(hipMemcpyAsync(hs, summary, sizeof hs, hipMemcpyDeviceToHost, stream));
    BUILD_CHK(hipStreamSynchronize(stream));
    T->total = T->levels.back().second;
    const uint64_t outNodes = 2ull * top.b.interiors + 1;
    if (hs[kSumStatus] || outNodes != T->total)
        return build_fail(RT_E_DEVICE, "%s: inconsistent device result (%s, %llu nodes of %u)", who, sstatus_text(hs[kSumStatus]), (unsigned long long)outNodes, T->total);
    SbvhBuilt& b = T->built;
    b.nodes = (uint32_t)outNodes; b.leaves = top.b.interiors + 1; b.nIdx = top.b.cnt; b.depth = top.b.depth; b.cost = top.b.cost;
    b.spatialSplits = hs[kSumSpatial]; b.primsClipped = hs[kSumClipped]; b.forcedLeaves = hs[kSumForced];
    b.levels = (uint32_t)T->levels.size(); b.peakRefs = peak;
    b.ms[0] = (float)tPrims; b.ms[1] = (float)tLevels; b.ms[2] = (float)(ms_since(t0) - tPrims - tLevels);
    *out = b;
    return RT_OK;
}

// The records and primIdx of a built tree into dNodes[0, built.nodes) and dIdx[0, built.nIdx)
int emit(const char* who, hipStream_t stream, Tree* T, RtBVHNode2* dNodes, uint32_t* dIdx)
{
    uint32_t* summary = (uint32_t*)T->summary.p;
    const SNode* bn = (const SNode*)T->bn.p;
    hipLaunchKernelGGL(k_sbvh_emit, grid(T->total, kBlock), dim3(kBlock), 0, stream, bn, T->total, T->nodeBase, T->idxBase, dNodes, T->built.nodes,
                       summary + kSumStatus);
    for (size_t l = 0; l < T->hist.size(); l++) {
        const uint32_t m = T->histN[l];
        const uint32_t* nid = (const uint32_t*)T->hist[l];
        hipLaunchKernelGGL(k_sbvh_emit_refs, grid(m, kBlock), dim3(kBlock), 0, stream, bn, T->total, nid, nid + m, m, T->first, dIdx, T->built.nIdx,
                           summary + kSumStatus);
    }
    BUILD_CHK(hipGetLastError());
    uint32_t st = 0;
    BUILD_CHK(hipMemcpyAsync(&st, summary + kSumStatus, sizeof st, hipMemcpyDeviceToHost, stream));
    BUILD_CHK(hipStreamSynchronize(stream));
    if (st) return build_fail(RT_E_DEVICE, "%s: inconsistent device result (%s)", who, sstatus_text(st));
    return RT_OK;
}

} // namespace sbvhdev

// The C-ABI entry: upload, build (sbvhdev::build), check the capacities, emit, download.
extern "C" int rt_build_bvh2_sbvh(int32_t device, float alpha, const RtPrimitive* prims, int32_t nPrims, int32_t first, int32_t count,
                                  uint32_t nodeBase, uint32_t idxBase, RtBVHNode2* nodes, int32_t nodeCap, int32_t* nNodes, uint32_t* primIdx,
                                  int32_t idxCap, int32_t* nIdx, RtSbvhStats* stats)
{
    const char* who = "rt_build_bvh2_sbvh";
    const auto t0 = builddev::Clock::now();
    if (const char* msg = check_args(alpha, prims, nPrims, first, count, nodes, nodeCap, nNodes, primIdx, idxCap, nIdx))
        return build_fail(RT_E_INVALID, "rt_build_bvh2_sbvh: %s", msg);
    SbvhSession w;
    if (const int rc = builddev::open_session(who, device, w)) return rc;
    const uint32_t n = (uint32_t)count;
    if (hipMalloc(&w.prims, n * sizeof(RtPrimitive)) != hipSuccess) { w.prims = nullptr; return build_fail(RT_E_NOMEM, "rt_build_bvh2_sbvh: device memory for %u primitives", n); }
    BUILD_CHK(hipMemcpyAsync(w.prims, prims + first, n * sizeof(RtPrimitive), hipMemcpyHostToDevice, w.stream));
    const double tAlloc = ms_since(t0);

    SbvhBuilt b{};
    if (const int rc = sbvhdev::build(who, w.stream, alpha, (const RtPrimitive*)w.prims, n, (uint32_t)first, nodeBase, idxBase, w.ev[0], nullptr, nullptr, &w.tree, &b))
        return rc;
    if ((uint64_t)nodeBase + b.nodes > 0xffffffffull || (uint64_t)idxBase + b.nIdx > 0xffffffffull)
        return build_fail(RT_E_INVALID, "rt_build_bvh2_sbvh: nodeBase / idxBase + the tree overflow 32-bit ids");
    *nNodes = (int32_t)b.nodes; *nIdx = (int32_t)b.nIdx;
    if ((uint32_t)nodeCap < b.nodes || (uint32_t)idxCap < b.nIdx)
        return build_fail(RT_E_INVALID, "rt_build_bvh2_sbvh: capacity: the tree has %u nodes and %u primIdx entries (nodeCap %d, idxCap %d)", b.nodes, b.nIdx,
                     nodeCap, idxCap);
    const double tEmit = ms_since(t0);
    const size_t oIdx = align_up((size_t)b.nodes * sizeof(RtBVHNode2));
    if (hipMalloc(&w.out, oIdx + align_up((size_t)b.nIdx * 4)) != hipSuccess) { w.out = nullptr; return build_fail(RT_E_NOMEM, "rt_build_bvh2_sbvh: device memory for the tree"); }
    RtBVHNode2* dNodes = (RtBVHNode2*)w.out;
    uint32_t* dIdx = (uint32_t*)((char*)w.out + oIdx);
    if (const int rc = sbvhdev::emit(who, w.stream, w.tree, dNodes, dIdx)) return rc;
    BUILD_CHK(hipEventRecord(w.ev[1], w.stream));
    const double tBuilt = ms_since(t0);
    BUILD_CHK(hipMemcpyAsync(nodes, dNodes, (size_t)b.nodes * sizeof(RtBVHNode2), hipMemcpyDeviceToHost, w.stream));
    BUILD_CHK(hipMemcpyAsync(primIdx, dIdx, (size_t)b.nIdx * sizeof(uint32_t), hipMemcpyDeviceToHost, w.stream));
    BUILD_CHK(hipStreamSynchronize(w.stream));
    g_phases[0] = (float)tAlloc + b.ms[0]; g_phases[1] = b.ms[1]; g_phases[2] = b.ms[2] + (float)(tBuilt - tEmit);
    g_phases[3] = (float)(ms_since(t0) - tBuilt); g_phases[4] = (float)b.levels;
    if (stats) {
        float ms = 0;
        BUILD_CHK(hipEventElapsedTime(&ms, w.ev[0], w.ev[1]));
        stats->nodes = (int32_t)b.nodes; stats->leaves = (int32_t)b.leaves; stats->n_idx = (int32_t)b.nIdx; stats->depth = (int32_t)b.depth;
        stats->spatial_splits = (int32_t)b.spatialSplits; stats->prims_clipped = (int32_t)b.primsClipped;
        stats->forced_leaves = (int32_t)b.forcedLeaves; stats->levels = (int32_t)b.levels;
        stats->sah_cost = b.cost; stats->device_ms = ms;
        stats->wall_ms = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count();
        stats->peak_refs = (int32_t)b.peakRefs;
    }
    return RT_OK;
}

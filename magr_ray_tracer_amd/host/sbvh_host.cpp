// sbvh_host.cpp — the sequential host restatement of the GPU SBVH build (rth_build_bvh2_sbvh) and its Scene path
// (BVH2::BuildBLASSBVHGPU, rth_build_blas_sbvh_gpu).  It runs the level-synchronous formulation of csrc/sbvh_common.h step by step as
// the kernels of csrc/sbvh.hip run it, with the same key folds, the same clipping and the same numbering: it is not a call into
// BVH2::BuildBVH.  Its arrays equal BuildBLAS's for every alpha in [0, 1] (tests/test_sbvh_gpu_cpu.py).
#include <algorithm>
#include <chrono>
#include <cstring>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>
#include "../../include/rt355.h"
#include "../../include/rt355_host.h"
#include "../csrc/sbvh_common.h"
#include "rt_host.h"

using namespace sbvh;

namespace rt355 {

// The build into vectors of the tree's own size (the arguments are checked by the callers)
int SbvhBuildVectors(float alpha, const RtPrimitive* prims, int32_t first, int32_t count, uint32_t nodeBase, uint32_t idxBase,
                            std::vector<RtBVHNode2>& nodes, std::vector<uint32_t>& primIdx, RtSbvhStats* stats, std::string& err)
{
    const std::string who = "rth_build_bvh2_sbvh: ";
    const auto t0 = std::chrono::steady_clock::now();
    try {
        const uint32_t n = (uint32_t)count;
        const RtPrimitive* P = prims + first;
        uint32_t status = 0;
        // level 0: one ref per primitive (k_sbvh_prims)
        std::vector<Ref> refs(n), refsN;
        std::vector<std::vector<uint32_t>> hNid(1), hPrim(1);     // per level: the node and the primitive of every ref
        hNid[0].assign(n, 0); hPrim[0].resize(n);
        for (uint32_t i = 0; i < n; i++) {
            const Prim d = prim_data(P[i]);
            if (!prim_finite(d)) status |= kBadInput;
            refs[i] = ref_of(d, i);
            hPrim[0][i] = i;
        }
        if (status) { err = who + sstatus_text(status); return RT_E_UNSUPPORTED; }
        std::vector<SNode> bn(1, open_snode(0, n));
        std::vector<std::pair<uint32_t, uint32_t>> levels;
        uint32_t lb = 0, le = 1, spatialSplits = 0, clipped = 0, forcedLeaves = 0, peak = n;
        for (;;) {
            levels.emplace_back(lb, le);
            const uint32_t K = le - lb, m = (uint32_t)refs.size();
            const std::vector<uint32_t>& nid = hNid.back();
            // keys of the nodes (k_sbvh_reduce), then their object bins (k_sbvh_obins)
            std::vector<uint64_t> kmin((size_t)K * kNodeKeys, kKeyMinEmpty), kmax((size_t)K * kNodeKeys, kKeyMaxEmpty);
            std::vector<uint64_t> bkmin((size_t)K * kBinKeys, kKeyMinEmpty), bkmax((size_t)K * kBinKeys, kKeyMaxEmpty);
            std::vector<uint32_t> bcnt((size_t)K * 3 * kBins, 0);
            for (uint32_t p = 0; p < m; p++) {
                const size_t t = nid[p] - lb;
                uint64_t km[kNodeKeys], kx[kNodeKeys];
                ref_keys(refs[p], km, kx);
                for (int j = 0; j < kNodeKeys; j++) {
                    kmin[t * kNodeKeys + j] = std::min(kmin[t * kNodeKeys + j], km[j]);
                    kmax[t * kNodeKeys + j] = std::max(kmax[t * kNodeKeys + j], kx[j]);
                }
            }
            for (uint32_t p = 0; p < m; p++) {
                const size_t t = nid[p] - lb;
                const Ref& r = refs[p];
                float mn[3], mx[3], cmin[3], cmax[3];
                node_from_keys(&kmin[t * kNodeKeys], &kmax[t * kNodeKeys], mn, mx, cmin, cmax);
                for (int a = 0; a < 3; a++) {
                    if (cmin[a] == cmax[a]) continue;
                    int k;
                    if (!bin_of(center(r, a), cmin[a], cmax[a], k)) { status |= kBadBin; continue; }
                    const size_t s = t * 3 * kBins + a * kBins + k;
                    bcnt[s]++;
                    for (int c = 0; c < 3; c++) {
                        bkmin[s * 3 + c] = std::min(bkmin[s * 3 + c], key_min(r.mn[c], r.prim));
                        bkmax[s * 3 + c] = std::max(bkmax[s * 3 + c], key_max(r.mx[c], r.prim));
                    }
                }
            }
            if (status) break;
            // first decision step (k_sbvh_decide1)
            bool anySpatial = false;
            for (uint32_t id = lb; id < le; id++) {
                SNode& N = bn[id];
                const size_t t = id - lb;
                float cmin[3], cmax[3];
                node_from_keys(&kmin[t * kNodeKeys], &kmax[t * kNodeKeys], N.b.mn, N.b.mx, cmin, cmax);
                Bins B;
                bins_from_keys(&bkmin[t * kBinKeys], &bkmax[t * kBinKeys], &bcnt[t * 3 * kBins], B);
                const float rootArea = area(bn[0].b.mn, bn[0].b.mx);
                decide_object(N, cmin, cmax, B, rootArea, alpha);
                anySpatial = anySpatial || (N.flags & kWantSpatial);
            }
            // spatial bins of the nodes that ask for them (k_sbvh_sbins)
            std::vector<uint64_t> skmin, skmax;
            std::vector<uint32_t> sent, sext;
            if (anySpatial) {
                skmin.assign((size_t)K * kBinKeys, kKeyMinEmpty); skmax.assign((size_t)K * kBinKeys, kKeyMaxEmpty);
                sent.assign((size_t)K * kSpCnt, 0); sext.assign((size_t)K * kSpCnt, 0);
                for (uint32_t p = 0; p < m; p++) {
                    const SNode& N = bn[nid[p]];
                    if (!(N.flags & kWantSpatial)) continue;
                    const size_t t = nid[p] - lb;
                    const Ref& r = refs[p];
                    float emn[3], emx[3];
                    exact_from_keys(&kmin[t * kNodeKeys], &kmax[t * kNodeKeys], emn, emx);
                    for (int a = 0; a < 3; a++) {
                        if (emn[a] == emx[a]) continue;
                        int f, l;
                        const size_t base = t * kSpCnt + a * kBins;
                        status |= spatial_ref(r, P[r.prim], a, emn[a], emx[a], f, l, [&](int b, const float* mn, const float* mx) {
                            for (int c = 0; c < 3; c++) {
                                skmin[(base + b) * 3 + c] = std::min(skmin[(base + b) * 3 + c], key_min(mn[c], r.prim));
                                skmax[(base + b) * 3 + c] = std::max(skmax[(base + b) * 3 + c], key_max(mx[c], r.prim));
                            }
                        });
                        if (f >= 0) { sent[base + f]++; sext[base + l]++; }
                    }
                }
                if (status) break;
            }
            // second decision step (k_sbvh_decide2)
            for (uint32_t id = lb; id < le; id++) {
                SNode& N = bn[id];
                const size_t t = id - lb;
                float emn[3], emx[3];
                exact_from_keys(&kmin[t * kNodeKeys], &kmax[t * kNodeKeys], emn, emx);
                SBins S;
                if (N.flags & kWantSpatial) sbins_from_keys(&skmin[t * kBinKeys], &skmax[t * kBinKeys], &sent[t * kSpCnt], &sext[t * kSpCnt], S);
                if (!decide_final(N, emn, emx, &S)) status |= kNoDecision;
            }
            if (status) break;
            // fragments per ref and their exclusive scan (k_sbvh_flag, hipcub::DeviceScan)
            std::vector<uint64_t> f(m + 1, 0), F(m + 1);
            for (uint32_t p = 0; p < m; p++) {
                const SNode& N = bn[nid[p]];
                if (N.b.kind != kSplit) continue;
                Ref L, R;
                bool overflow = false;
                const uint32_t e = split_ref(N, refs[p], P[refs[p].prim], L, R, overflow);
                if (overflow) status |= kInternal;
                if (e & kStraddle) clipped++;
                f[p] = (uint64_t)((e & kEmitL) ? 1 : 0) | ((uint64_t)((e & kEmitR) ? 1 : 0) << 32);
            }
            if (status) break;
            { uint64_t run = 0; for (uint32_t p = 0; p <= m; p++) { F[p] = run; run += f[p]; } }
            // forced leaves and the children's places (k_sbvh_count, scan, k_sbvh_children)
            std::vector<uint64_t> v(K), V(K);
            for (uint32_t id = lb; id < le; id++) {
                SNode& N = bn[id];
                const uint64_t d = F[N.b.home + N.b.cnt] - F[N.b.home];
                uint32_t sp, fo;
                v[id - lb] = count_node(N, (uint32_t)d, (uint32_t)(d >> 32), sp, fo);
                spatialSplits += sp; forcedLeaves += fo;
            }
            uint64_t run = 0;
            for (uint32_t t = 0; t < K; t++) { V[t] = run; run += v[t]; }
            const uint32_t splits = (uint32_t)run;
            const uint64_t mNext = run >> 32;
            if (splits == 0) break;
            if (mNext > kMaxRefs || (uint64_t)le + 2ull * splits > kMaxRefs) throw std::bad_alloc();
            bn.resize((size_t)le + 2 * splits);
            for (uint32_t id = lb; id < le; id++) {
                if (bn[id].b.kind != kSplit) continue;
                SNode L, R;
                make_schildren(bn[id], V[id - lb], le, L, R);
                bn[bn[id].b.left] = L;
                bn[bn[id].b.left + 1] = R;
            }
            // the stable scatter of the fragments into the next level's arrays (k_sbvh_scatter)
            refsN.assign((size_t)mNext, Ref{});
            std::vector<uint32_t> nidN((size_t)mNext), primN((size_t)mNext);
            for (uint32_t p = 0; p < m; p++) {
                const SNode& N = bn[nid[p]];
                if (N.b.kind != kSplit) continue;
                Ref L, R;
                bool overflow = false;
                const uint32_t e = split_ref(N, refs[p], P[refs[p].prim], L, R, overflow);
                const uint64_t d = F[p] - F[N.b.home];
                const SNode& CL = bn[N.b.left];
                const SNode& CR = bn[N.b.left + 1];
                if (e & kEmitL) { const uint32_t dst = CL.b.home + (uint32_t)d; refsN[dst] = L; nidN[dst] = N.b.left; primN[dst] = L.prim; }
                if (e & kEmitR) { const uint32_t dst = CR.b.home + (uint32_t)(d >> 32); refsN[dst] = R; nidN[dst] = N.b.left + 1; primN[dst] = R.prim; }
            }
            refs.swap(refsN);
            hNid.push_back(std::move(nidN)); hPrim.push_back(std::move(primN));
            if (mNext > peak) peak = (uint32_t)mNext;
            lb = le; le += 2 * splits;
        }
        if (status) { err = who + sstatus_text(status); return (status & kInternal) ? RT_E_DEVICE : RT_E_UNSUPPORTED; }
        // numbering: bottom-up, top-down (k_sbvh_up, k_sbvh_down)
        for (size_t l = levels.size(); l-- > 0;)
            for (uint32_t id = levels[l].first; id < levels[l].second; id++)
                if (bn[id].b.kind == kSplit) sup(bn[id], bn[bn[id].b.left], bn[bn[id].b.left + 1]);
        for (const auto& L : levels)
            for (uint32_t id = L.first; id < L.second; id++)
                if (bn[id].b.kind == kSplit) down(bn[id].b, bn[bn[id].b.left].b, bn[bn[id].b.left + 1].b);
        const uint64_t outNodes = 2ull * bn[0].b.interiors + 1, outIdx = bn[0].b.cnt;
        if (outNodes > kMaxRefs || (uint64_t)nodeBase + outNodes > 0xffffffffull || (uint64_t)idxBase + outIdx > 0xffffffffull) {
            err = who + "nodeBase / idxBase + the tree overflow 32-bit ids";
            return RT_E_INVALID;
        }
        nodes.resize((size_t)outNodes); primIdx.resize((size_t)outIdx);
        // emit (k_sbvh_emit, k_sbvh_emit_refs)
        for (const SNode& N : bn) nodes[N.b.gid] = emit_level(N.b, nodeBase, idxBase);
        for (size_t l = 0; l < levels.size(); l++)
            for (size_t p = 0; p < hNid[l].size(); p++) {
                const BNode& N = bn[hNid[l][p]].b;
                if (N.kind == kLeaf) primIdx[N.offset + ((uint32_t)p - N.home)] = (uint32_t)first + hPrim[l][p];
            }
        if (stats) {
            stats->nodes = (int32_t)outNodes; stats->leaves = (int32_t)bn[0].b.interiors + 1; stats->n_idx = (int32_t)outIdx;
            stats->depth = (int32_t)bn[0].b.depth; stats->spatial_splits = (int32_t)spatialSplits; stats->prims_clipped = (int32_t)clipped;
            stats->forced_leaves = (int32_t)forcedLeaves; stats->levels = (int32_t)levels.size();
            stats->sah_cost = bn[0].b.cost; stats->device_ms = 0;
            stats->wall_ms = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count();
            stats->peak_refs = (int32_t)peak;
        }
        return RT_OK;
    } catch (const std::exception& e) {
        err = who + e.what();
        return RT_E_NOMEM;
    }
}

int SbvhBuildHost(float alpha, const RtPrimitive* prims, int32_t nPrims, int32_t first, int32_t count, uint32_t nodeBase, uint32_t idxBase,
                  RtBVHNode2* nodes, int32_t nodeCap, int32_t* nNodes, uint32_t* primIdx, int32_t idxCap, int32_t* nIdx, RtSbvhStats* stats,
                  std::string& err)
{
    const std::string who = "rth_build_bvh2_sbvh: ";
    if (const char* msg = check_args(alpha, prims, nPrims, first, count, nodes, nodeCap, nNodes, primIdx, idxCap, nIdx)) {
        err = who + msg;
        return RT_E_INVALID;
    }
    std::vector<RtBVHNode2> vn;
    std::vector<uint32_t> vi;
    RtSbvhStats st{};
    const int rc = SbvhBuildVectors(alpha, prims, first, count, nodeBase, idxBase, vn, vi, &st, err);
    if (rc != RT_OK) return rc;
    *nNodes = (int32_t)vn.size(); *nIdx = (int32_t)vi.size();
    if ((size_t)nodeCap < vn.size() || (size_t)idxCap < vi.size()) {
        err = who + "capacity: the tree has " + std::to_string(vn.size()) + " nodes and " + std::to_string(vi.size()) +
              " primIdx entries (nodeCap " + std::to_string(nodeCap) + ", idxCap " + std::to_string(idxCap) + ")";
        return RT_E_INVALID;
    }
    memcpy(nodes, vn.data(), vn.size() * sizeof(RtBVHNode2));
    memcpy(primIdx, vi.data(), vi.size() * sizeof(uint32_t));
    if (stats) *stats = st;
    return RT_OK;
}

// The GPU SBVH build, appended as BuildBLAS appends (AppendBuiltBLAS).  The scene is left unchanged when the build is refused.
void BVH2::BuildBLASSBVHGPU(int startIdx, float a, int device)
{
    const int64_t n = (int64_t)primitives_.size() - startIdx;
    if (startIdx < 0 || n <= 0) throw LbvhError(RT_E_INVALID, "BuildBLASSBVHGPU: empty primitive range");
    if (n > (1 << 30)) throw LbvhError(RT_E_INVALID, "BuildBLASSBVHGPU: more than 2^30 primitives");
    const uint32_t nodeBase = (uint32_t)bvhNodes.size(), idxBase = (uint32_t)primIdx.size();
    std::vector<RtBVHNode2> nodes;
    std::vector<uint32_t> idx;
    RtSbvhStats st{};
    int32_t nN = 0, nI = 0;
    std::string err;
    int rc;
    if (device < 0) {
        if (!(a >= 0.0f && a <= 1.0f)) throw LbvhError(RT_E_INVALID, "BuildBLASSBVHGPU: alpha must lie in [0, 1]");
        rc = SbvhBuildVectors(a, primitives_.data(), startIdx, (int32_t)n, nodeBase, idxBase, nodes, idx, &st, err);
        nN = (int32_t)nodes.size(); nI = (int32_t)idx.size();
    } else {
        nodes.resize((size_t)(2 * n - 1)); idx.resize((size_t)n);
        auto call = [&]() {
            return rt_build_bvh2_sbvh(device, a, primitives_.data(), (int32_t)primitives_.size(), startIdx, (int32_t)n, nodeBase, idxBase,
                                      nodes.data(), (int32_t)nodes.size(), &nN, idx.data(), (int32_t)idx.size(), &nI, &st);
        };
        rc = call();
        if (rc == RT_E_INVALID && ((size_t)nN > nodes.size() || (size_t)nI > idx.size())) {   // the capacity protocol: once more with the sizes it reported
            nodes.resize((size_t)nN); idx.resize((size_t)nI);
            rc = call();
        }
    }
    if (rc != RT_OK) throw LbvhError(rc, device < 0 ? err : std::string(rt_last_error()));
    AppendBuiltBLAS(nodeBase, nodes.data(), (size_t)nN, idx.data(), (size_t)nI, st.wall_ms, st.depth, st.sah_cost);
    alpha = a;
    stat_spatial_splits += (uint32_t)st.spatial_splits;
    stat_prims_clipped += (uint32_t)st.prims_clipped;
    stat_forced_leaves += (uint32_t)st.forced_leaves;
}

} // namespace rt355

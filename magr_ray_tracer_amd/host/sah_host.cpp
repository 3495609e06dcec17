// sah_host.cpp — the sequential host restatement of the GPU SAH build (rth_build_bvh2_sah) and its Scene path
// (BVH2::BuildBLASSAHGPU, rth_build_blas_sah_gpu).  It runs the level-synchronous formulation of csrc/sah_common.h step by step as
// the kernels of csrc/sah.hip run it, with the same key folds, the same small-subtree builder and the same numbering formula: it
// is not a call into BVH2::BuildBVH.  Its arrays equal BuildBLAS's with alpha = 1 (tests/test_sah_gpu_cpu.py).
#include <algorithm>
#include <chrono>
#include <cstring>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>
#include "../../include/rt355.h"
#include "../../include/rt355_host.h"
#include "../csrc/sah_common.h"
#include "rt_host.h"

using namespace sah;

namespace rt355 {

int SahBuildHost(const RtPrimitive* prims, int32_t nPrims, int32_t first, int32_t count, uint32_t nodeBase, uint32_t idxBase,
                 RtBVHNode2* nodes, int32_t nodeCap, int32_t* nNodes, uint32_t* primIdx, RtBuildStats* stats, std::string& err)
{
    const auto t0 = std::chrono::steady_clock::now();
    if (const char* msg = check_args(prims, nPrims, first, count, nodeBase, idxBase, nodes, nodeCap, nNodes, primIdx)) {
        err = std::string("rth_build_bvh2_sah: ") + msg;
        return RT_E_INVALID;
    }
    try {
        const uint32_t n = (uint32_t)count;
        uint32_t status = 0;
        // primitive data (k_sah_prims)
        std::vector<Prim> P(n);
        std::vector<uint32_t> cur(n), nxt(n), nid(n, 0), nidN(n), owner(n, kNone), f(n + 1), F(n + 1);
        std::vector<uint32_t> sA(n), sB(n), sout(n);
        std::vector<LNode> snodes(2 * (size_t)n);
        for (uint32_t i = 0; i < n; i++) {
            P[i] = prim_data(prims[first + i]);
            if (!prim_finite(P[i])) status |= kBadInput;
            cur[i] = i;
        }
        if (status) { err = std::string("rth_build_bvh2_sah: ") + status_text(status); return RT_E_UNSUPPORTED; }
        std::vector<BNode> bn(2 * (size_t)n - 1);
        bn[0] = open_node(0, n, 0);
        std::vector<std::pair<uint32_t, uint32_t>> levels;
        uint32_t lb = 0, le = 1, nBig = n > kSmall ? 1 : 0;
        for (;;) {
            levels.emplace_back(lb, le);
            // keys of the open nodes (k_sah_reduce), then their bins (k_sah_bins)
            std::vector<uint64_t> kmin(nBig * 6, kKeyMinEmpty), kmax(nBig * 6, kKeyMaxEmpty);
            std::vector<uint64_t> bkmin(nBig * (size_t)kBinKeys, kKeyMinEmpty), bkmax(nBig * (size_t)kBinKeys, kKeyMaxEmpty);
            std::vector<uint32_t> bcnt(nBig * 3 * (size_t)kBins, 0);
            for (uint32_t p = 0; p < n; p++) {
                if (nid[p] == kNone || bn[nid[p]].kind != kOpen) continue;
                const uint32_t b = bn[nid[p]].big, i = cur[p];
                uint64_t km[6], kx[6];
                node_keys(P[i], i, km, kx);
                for (int j = 0; j < 6; j++) { kmin[b * 6 + j] = std::min(kmin[b * 6 + j], km[j]); kmax[b * 6 + j] = std::max(kmax[b * 6 + j], kx[j]); }
            }
            for (uint32_t p = 0; p < n; p++) {
                if (nid[p] == kNone || bn[nid[p]].kind != kOpen) continue;
                const uint32_t b = bn[nid[p]].big, i = cur[p];
                float mn[3], mx[3], cmin[3], cmax[3];
                node_from_keys(&kmin[b * 6], &kmax[b * 6], mn, mx, cmin, cmax);
                for (int a = 0; a < 3; a++) {
                    if (cmin[a] == cmax[a]) continue;
                    int k;
                    if (!bin_of(P[i].c[a], cmin[a], cmax[a], k)) { status |= kBadBin; continue; }
                    const size_t s = (size_t)b * 3 * kBins + a * kBins + k;
                    bcnt[s]++;
                    for (int c = 0; c < 3; c++) {
                        bkmin[s * 3 + c] = std::min(bkmin[s * 3 + c], key_min(P[i].mn[c], i));
                        bkmax[s * 3 + c] = std::max(bkmax[s * 3 + c], key_max(P[i].mx[c], i));
                    }
                }
            }
            // decisions of the open nodes (k_sah_decide) and the small subtrees (k_sah_small)
            for (uint32_t id = lb; id < le; id++) {
                BNode& N = bn[id];
                if (N.kind == kOpen) {
                    float cmin[3], cmax[3];
                    node_from_keys(&kmin[N.big * 6], &kmax[N.big * 6], N.mn, N.mx, cmin, cmax);
                    Bins B;
                    bins_from_keys(&bkmin[N.big * (size_t)kBinKeys], &bkmax[N.big * (size_t)kBinKeys], &bcnt[N.big * 3 * (size_t)kBins], B);
                    Decision d;
                    if (!decide(N.cnt, N.mn, N.mx, cmin, cmax, B, d)) { status |= kNoDecision; continue; }
                    apply_decision(N, d);
                } else if (N.kind == kSmallRoot) {
                    for (uint32_t j = 0; j < N.cnt; j++) sA[N.home + j] = cur[N.home + j];
                    SubResult r;
                    const int rc = build_small(P.data(), &sA[N.home], &sB[N.home], N.cnt, &sout[N.home], &snodes[2 * (size_t)N.home], r);
                    if (rc) { status |= rc == kErrBin ? kBadBin : kNoDecision; continue; }
                    apply_small(N, snodes[2 * (size_t)N.home], r);
                }
            }
            if (status) break;
            // partition flags and their exclusive scan (k_sah_flag, hipcub::DeviceScan)
            for (uint32_t p = 0; p <= n; p++) {
                const uint32_t id = p < n ? nid[p] : kNone;
                f[p] = id != kNone && bn[id].kind == kSplit && goes_left(P[cur[p]], bn[id].axis, bn[id].pos) ? 1 : 0;
            }
            for (uint32_t p = 0, run = 0; p <= n; p++) { F[p] = run; run += f[p]; }
            // forced leaves and the children's places (k_sah_count, scan, k_sah_children)
            std::vector<uint64_t> v(le - lb), V(le - lb);
            for (uint32_t id = lb; id < le; id++) {
                BNode& N = bn[id];
                v[id - lb] = N.kind == kSplit ? count_split(N, F[N.home + N.cnt] - F[N.home]) : 0;
            }
            uint64_t run = 0;
            for (uint32_t t = 0; t < le - lb; t++) { V[t] = run; run += v[t]; }
            const uint32_t splits = (uint32_t)run, bigs = (uint32_t)(run >> 32);
            for (uint32_t id = lb; id < le; id++) {
                if (bn[id].kind != kSplit) continue;
                BNode L, R;
                make_children(bn[id], V[id - lb], le, L, R);
                bn[bn[id].left] = L;
                bn[bn[id].left + 1] = R;
            }
            // the stable partition (k_sah_scatter)
            for (uint32_t p = 0; p < n; p++) {
                const uint32_t id = nid[p];
                if (id == kNone) { nxt[p] = cur[p]; nidN[p] = kNone; continue; }
                const BNode& N = bn[id];
                if (N.kind == kSplit) {
                    const bool left = f[p] != 0;
                    const uint32_t dst = scatter_dst(N, p, F[p] - F[N.home], left);
                    nxt[dst] = cur[p];
                    nidN[dst] = left ? N.left : N.left + 1;
                } else {
                    nxt[p] = cur[p]; nidN[p] = kNone; owner[p] = id;
                }
            }
            std::swap(cur, nxt);
            std::swap(nid, nidN);
            if (splits == 0) break;
            lb = le; le += 2 * splits; nBig = bigs;
        }
        if (status) { err = std::string("rth_build_bvh2_sah: ") + status_text(status); return RT_E_UNSUPPORTED; }
        // numbering: bottom-up (k_sah_up), top-down (k_sah_down), then emit
        for (size_t l = levels.size(); l-- > 0;)
            for (uint32_t id = levels[l].first; id < levels[l].second; id++)
                if (bn[id].kind == kSplit) up(bn[id], bn[bn[id].left], bn[bn[id].left + 1]);
        for (const auto& L : levels)
            for (uint32_t id = L.first; id < L.second; id++)
                if (bn[id].kind == kSplit) down(bn[id], bn[bn[id].left], bn[bn[id].left + 1]);
        const uint32_t outNodes = 2 * bn[0].interiors + 1, total = levels.back().second;
        for (uint32_t id = 0; id < total; id++) {
            const BNode& N = bn[id];
            if (N.kind != kSmallRoot) { nodes[N.gid] = emit_level(N, nodeBase, idxBase); continue; }
            for (uint32_t j = 0; j < 2 * N.interiors + 1; j++)
                nodes[small_index(N, j)] = emit_small(N, snodes[2 * (size_t)N.home + j], nodeBase, idxBase);
        }
        for (uint32_t p = 0; p < n; p++) {
            const BNode& N = bn[owner[p]];
            primIdx[N.offset + (p - N.home)] = (uint32_t)first + (N.kind == kSmallRoot ? sout[p] : cur[p]);
        }
        *nNodes = (int32_t)outNodes;
        if (stats) {
            stats->nodes = (int32_t)outNodes; stats->leaves = (int32_t)bn[0].interiors + 1; stats->depth = (int32_t)bn[0].depth;
            stats->morton_bits = 0; stats->sah_cost = bn[0].cost; stats->device_ms = 0;
            stats->wall_ms = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count();
            stats->_reserved = 0;
        }
        return RT_OK;
    } catch (const std::exception& e) {
        err = std::string("rth_build_bvh2_sah: ") + e.what();
        return RT_E_NOMEM;
    }
}

// The GPU SAH build, appended as BuildBLAS appends (AppendBuiltBLAS).  The scene is left unchanged when the build is refused.
void BVH2::BuildBLASSAHGPU(int startIdx, int device)
{
    const int64_t n = (int64_t)primitives_.size() - startIdx;
    if (startIdx < 0 || n <= 0) throw LbvhError(RT_E_INVALID, "BuildBLASSAHGPU: empty primitive range");
    if (n > (1 << 30)) throw LbvhError(RT_E_INVALID, "BuildBLASSAHGPU: more than 2^30 primitives");
    const uint32_t nodeBase = (uint32_t)bvhNodes.size(), idxBase = (uint32_t)primIdx.size();
    std::vector<RtBVHNode2> nodes((size_t)(2 * n - 1));
    std::vector<uint32_t> idx((size_t)n);
    RtBuildStats st{};
    int32_t written = 0;
    std::string err;
    const int rc = device < 0
        ? SahBuildHost(primitives_.data(), (int32_t)primitives_.size(), startIdx, (int32_t)n, nodeBase, idxBase, nodes.data(),
                       (int32_t)nodes.size(), &written, idx.data(), &st, err)
        : rt_build_bvh2_sah(device, primitives_.data(), (int32_t)primitives_.size(), startIdx, (int32_t)n, nodeBase, idxBase,
                            nodes.data(), (int32_t)nodes.size(), &written, idx.data(), &st);
    if (rc != RT_OK) throw LbvhError(rc, device < 0 ? err : std::string(rt_last_error()));
    AppendBuiltBLAS(nodeBase, nodes.data(), (size_t)written, idx.data(), idx.size(), st.wall_ms, st.depth, st.sah_cost);
}

} // namespace rt355

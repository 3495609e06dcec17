// records_main.cpp — the derived records' codecs on their own (csrc/refit_common.h, rebuild_common.h, collapse_common.h): the headers
// compile without HIP, and what every encoder writes is what its decoders read back, lane for lane and bit for bit, at the limits of
// every field, under the sanitizers.  (The kernels read the records through the same decoders: csrc/rt355_kernels.h.)
//   g++ -std=c++17 -Wall -Wextra -fsanitize=address,undefined -fno-sanitize-recover=all tools/records_main.cpp -o records_main && ./records_main
#include <cstdio>
#include <cstring>
#include "../magr_ray_tracer_amd/csrc/collapse_common.h"

using namespace refit;

static int g_bad = 0;
#define EXPECT(what, got, want) do { const unsigned long long g_ = (unsigned long long)(got), w_ = (unsigned long long)(want); \
    if (g_ != w_) { printf("FAIL %s: %s = 0x%llx, expected 0x%llx\n", what, #got, g_, w_); g_bad++; } } while (0)
// a decoded xyz vector against three floats, as bit patterns; its w lane is +0
static void expect_xyz(const char* what, const RtFloat4& v, float x, float y, float z)
{
    EXPECT(what, f2u(v.x), f2u(x)); EXPECT(what, f2u(v.y), f2u(y)); EXPECT(what, f2u(v.z), f2u(z)); EXPECT(what, f2u(v.w), 0u);
}

static void entries()
{
    const uint32_t maxFirst = (uint32_t)rebuild::kMaxPackedIdx - 1u, maxCount = rebuild::kMaxPackedLeaf;
    for (uint32_t count : { 1u, maxCount }) for (uint32_t first : { 0u, maxFirst }) {
        const uint32_t e = leaf_entry(first, count);
        EXPECT("leaf entry", e & kLeafBit, kLeafBit); EXPECT("leaf entry", leaf_first(e), first); EXPECT("leaf entry", leaf_count(e), count);
        EXPECT("child_entry of a leaf", rebuild::child_entry(first, count, 12345u), e);
    }
    EXPECT("child_entry of an interior node", rebuild::child_entry(7u, 0u, 12345u), 12345u);
    // the rest of a leaf, one primitive at a time, down to its last
    for (uint32_t first : { 0u, maxFirst - (maxCount - 1u) }) {
        uint32_t e = leaf_entry(first, maxCount);
        for (uint32_t k = 1; k < maxCount; k++) {
            e = leaf_rest(leaf_first(e), leaf_count(e));
            EXPECT("leaf_rest", e, leaf_entry(first + k, maxCount - k));
        }
        EXPECT("leaf_rest ends", leaf_count(e), 1u); EXPECT("leaf_rest ends", leaf_first(e), first + maxCount - 1u);
    }
    // the unused quad slot is no legal entry: not an interior id (the leaf bit), and as a leaf it would end past the last slot
    EXPECT("kNoChild", kNoChild & kLeafBit, kLeafBit);
    EXPECT("kNoChild", (unsigned long long)leaf_first(kNoChild) + leaf_count(kNoChild) > (unsigned long long)maxFirst, 1);
    for (uint32_t count = 1; count <= maxCount; count++) EXPECT("kNoChild", leaf_entry(maxFirst - count, count) != kNoChild, 1);   // the last legal leaf of each size
    // TLAS entries, plain and tagged: ids 0 and the largest legal one
    const uint32_t maxInst = (uint32_t)kMaxInstances - 1u, maxNode = 2u * (uint32_t)kMaxInstances - 2u;
    for (uint32_t id : { 0u, maxInst }) {
        const uint32_t p = tlas_leaf_entry(false, id), t = tlas_leaf_entry(true, id);
        EXPECT("plain leaf", plain_leaf(p) != 0u, 1); EXPECT("plain leaf", plain_inst(p), id);
        EXPECT("tagged leaf", t & kLeafBit, 0u); EXPECT("tagged leaf", tagged_tag(t), kTagInst); EXPECT("tagged leaf", tagged_id(t), id);
    }
    for (uint32_t id : { 0u, maxNode, kIdMask }) {   // (kIdMask: the largest id the tagged column can carry, trav_common.h's 2^29 limit)
        const uint32_t p = tlas_node_entry(false, id), t = tlas_node_entry(true, id);
        if (id <= maxNode) { EXPECT("plain node", plain_leaf(p), 0u); EXPECT("plain node", p, id); }
        EXPECT("tagged node", t & kLeafBit, 0u); EXPECT("tagged node", tagged_tag(t), kTagTlas); EXPECT("tagged node", tagged_tlas(t) != 0u, 1);
        EXPECT("tagged node", tagged_id(t), id);
        EXPECT("BLAS interior entry", tagged_tag(id) | tagged_tlas(id) | (id & kLeafBit), 0u);   // an id below 2^29 carries no tag
    }
    // the 16-bit TLAS stack: every value it can hold (bit 15 = leaf, 15 bits of id) comes back as the plain entry it stands for
    for (uint32_t v = 0; v < 0x10000u; v++) {
        const uint32_t id = v & 0x7fffu, e = (v & 0x8000u) ? tlas_leaf_entry(false, id) : tlas_node_entry(false, id);
        EXPECT("tlas_pack16", tlas_pack16(e), v); EXPECT("tlas_unpack16", tlas_unpack16(tlas_pack16(e)), e);
    }
}

// nodes whose twelve box coordinates are base + 1 .. base + 12 in the order min.xyz, max.xyz of child 1, then of child 2
template <class N> static void fill_boxes(N& a, N& b, float base)
{
    a.aabbMin = f4(base + 1, base + 2, base + 3, -1.0f); a.aabbMax = f4(base + 4, base + 5, base + 6, -2.0f);
    b.aabbMin = f4(base + 7, base + 8, base + 9, -3.0f); b.aabbMax = f4(base + 10, base + 11, base + 12, -4.0f);
}
static void expect_pair_boxes(const char* what, const RtFloat4 q[3], float base)
{
    expect_xyz(what, pair_min1(q[0], q[1], q[2]), base + 1, base + 2, base + 3); expect_xyz(what, pair_max1(q[0], q[1], q[2]), base + 4, base + 5, base + 6);
    expect_xyz(what, pair_min2(q[0], q[1], q[2]), base + 7, base + 8, base + 9); expect_xyz(what, pair_max2(q[0], q[1], q[2]), base + 10, base + 11, base + 12);
}

static void pair_records()
{
    // BLAS: node 0 with children 1 (a leaf of 127 from slot 5) and 2 (interior, pair id 9)
    RtBVHNode2 n[3]; memset(n, 0, sizeof n);
    n[0].first = 1; n[0].count = 0; fill_boxes(n[1], n[2], 0.0f);
    n[1].first = 5; n[1].count = 127; n[2].first = 40; n[2].count = 0;
    const uint32_t newId[3] = { 0u, 0xdeadu, 9u };
    RtFloat4 q[4];
    rebuild::pair_record(n, 0, newId, q);
    expect_pair_boxes("pair record", q, 0.0f);
    EXPECT("pair record", pair_entry1(q[3]), leaf_entry(5, 127)); EXPECT("pair record", pair_entry2(q[3]), 9u);
    EXPECT("pair record", f2u(q[3].z) | f2u(q[3].w), 0u);
    // TLAS: node 0 with children 1 (the leaf of instance 255) and 2 (interior), both encodings; a leaf's record is zero
    RtTLASNode t[3]; memset(t, 0, sizeof t);
    t[0].leftRight = 1u | (2u << 16); fill_boxes(t[1], t[2], 100.0f);
    t[1].leftRight = 0; t[1].BLASidx = 255; t[2].leftRight = 1u | (1u << 16);
    tlas_pair(t, 0, false, q);
    expect_pair_boxes("TLAS pair, plain", q, 100.0f);
    EXPECT("TLAS pair, plain", pair_entry1(q[3]), tlas_leaf_entry(false, 255)); EXPECT("TLAS pair, plain", pair_entry2(q[3]), 2u);
    tlas_pair(t, 0, true, q);
    expect_pair_boxes("TLAS pair, tagged", q, 100.0f);
    EXPECT("TLAS pair, tagged", tagged_tag(pair_entry1(q[3])), kTagInst); EXPECT("TLAS pair, tagged", tagged_id(pair_entry1(q[3])), 255u);
    EXPECT("TLAS pair, tagged", tagged_tag(pair_entry2(q[3])), kTagTlas); EXPECT("TLAS pair, tagged", tagged_id(pair_entry2(q[3])), 2u);
    tlas_pair(t, 1, true, q);
    for (int k = 0; k < 4; k++) EXPECT("TLAS leaf record", f2u(q[k].x) | f2u(q[k].y) | f2u(q[k].z) | f2u(q[k].w), 0u);
}

static void quad_records()
{
    // four slots whose 24 box coordinates are 1..24; slot 0 a leaf, slot 1 a child (live id 77), slot 2 a leaf at the limits, slot 3 unused
    RtBVHNode4 q4; memset(&q4, 0, sizeof q4);
    for (int k = 0; k < 4; k++) {
        const float b = 6.0f * (float)k;
        q4.aabbMin[k] = f4(b + 1, b + 2, b + 3, -1.0f); q4.aabbMax[k] = f4(b + 4, b + 5, b + 6, -2.0f);
    }
    const int32_t nNodes = 8, nIdx = rebuild::kMaxPackedIdx - 1;
    q4.first[0] = 3; q4.count[0] = 1;
    q4.first[1] = 5; q4.count[1] = 0;
    q4.first[2] = nIdx - 127; q4.count[2] = 127;
    q4.first[3] = RT_INVALID; q4.count[3] = RT_INVALID;
    uint32_t newId[8] = { 0 }; newId[5] = 77u;
    RtFloat4 q[8];
    collapse::quad_record(q4, nNodes, nIdx, newId, q);
    const RtFloat4 mn[4] = { collapse::quad_min<0>(q[0], q[1], q[2], q[3], q[4], q[5]), collapse::quad_min<1>(q[0], q[1], q[2], q[3], q[4], q[5]),
                             collapse::quad_min<2>(q[0], q[1], q[2], q[3], q[4], q[5]), collapse::quad_min<3>(q[0], q[1], q[2], q[3], q[4], q[5]) };
    const RtFloat4 mx[4] = { collapse::quad_max<0>(q[0], q[1], q[2], q[3], q[4], q[5]), collapse::quad_max<1>(q[0], q[1], q[2], q[3], q[4], q[5]),
                             collapse::quad_max<2>(q[0], q[1], q[2], q[3], q[4], q[5]), collapse::quad_max<3>(q[0], q[1], q[2], q[3], q[4], q[5]) };
    for (int k = 0; k < 4; k++) {
        const float b = 6.0f * (float)k;
        expect_xyz("quad record", mn[k], b + 1, b + 2, b + 3); expect_xyz("quad record", mx[k], b + 4, b + 5, b + 6);
    }
    EXPECT("quad record", collapse::quad_entry<0>(q[6]), leaf_entry(3, 1)); EXPECT("quad record", collapse::quad_entry<1>(q[6]), 77u);
    EXPECT("quad record", collapse::quad_entry<2>(q[6]), leaf_entry((uint32_t)nIdx - 127u, 127)); EXPECT("quad record", collapse::quad_entry<3>(q[6]), kNoChild);
    EXPECT("quad record", f2u(q[7].x) | f2u(q[7].y) | f2u(q[7].z) | f2u(q[7].w), 0u);
}

static void triangle_records()
{
    RtPrimitive p; memset(&p, 0, sizeof p);
    p.objType = RT_PRIM_TRIANGLE;
    p.obj.triangle.v0 = f4(1, 2, 3, 0); p.obj.triangle.v1 = f4(5, 7, 9, 0); p.obj.triangle.v2 = f4(12, 15, 18, 0);   // edges (4, 5, 6), (11, 13, 15)
    RtFloat4 t[3];
    tri_rec(p, 0xfedcba98u, t);
    expect_xyz("triangle record", tri_v0(t[0], t[1], t[2]), 1, 2, 3);
    expect_xyz("triangle record", tri_edge1(t[0], t[1], t[2]), 4, 5, 6); expect_xyz("triangle record", tri_edge2(t[0], t[1], t[2]), 11, 13, 15);
    EXPECT("triangle record", tri_prim(t[2]), 0xfedcba98u); EXPECT("triangle record", tri_not_plain(t[2]), 0u); EXPECT("triangle record", f2u(t[2].w), 0u);
    p.obj.triangle.v1.w = 1.0f;   // a vertex with a w lane: the reference-layout test
    tri_rec(p, 0u, t);
    EXPECT("triangle record, w lane", tri_not_plain(t[2]) != 0u, 1); EXPECT("triangle record, w lane", tri_prim(t[2]), 0u);
    p.obj.triangle.v1.w = 0.0f; p.objType = RT_PRIM_SPHERE;
    tri_rec(p, 3u, t);
    EXPECT("triangle record, sphere", tri_not_plain(t[2]) != 0u, 1); EXPECT("triangle record, sphere", tri_prim(t[2]), 3u);
}

static void instance_records()
{
    RtBVHInstance inst; memset(&inst, 0, sizeof inst);
    inst.bvhIdx = 0x89abcdefu;
    for (int k = 0; k < 16; k++) inst.invT[k] = (float)(k + 1);
    RtFloat4 t[4];
    inst_rec(inst, leaf_entry(0x00ffffffu, 127), t);
    for (int k = 0; k < 3; k++) {
        const float b = 4.0f * (float)k;
        expect_xyz("instance record", inst_axis(t[k]), b + 1, b + 2, b + 3); EXPECT("instance record", f2u(inst_shift(t[k])), f2u(b + 4));
    }
    EXPECT("instance record", inst_root(t[3]), leaf_entry(0x00ffffffu, 127)); EXPECT("instance record", inst_bvh(t[3]), 0x89abcdefu);
    EXPECT("instance record", f2u(t[3].z) | f2u(t[3].w), 0u);
}

// rebuild::relocated_entry (the derived pair records of a kept or refit BLAS): a leaf entry moves inside its slot field, up and down and
// to both ends of it, and keeps its count and leaf bit; an interior entry moves by the pair offset; the offsets are taken modulo 2^32.
// A plan with the per-range refit word passes check_plan's rules as a kept one does.
static void relocated_entries()
{
    const uint32_t maxFirst = (uint32_t)rebuild::kMaxPackedIdx - 1u, maxCount = rebuild::kMaxPackedLeaf;
    for (uint32_t count : { 1u, maxCount }) for (uint32_t from : { 0u, 5u, maxFirst }) for (uint32_t to : { 0u, 7u, maxFirst }) {
        const uint32_t idxDelta = to - from;   // (wraps when the block moves down)
        for (uint32_t pairDelta : { 0u, 3u, 0xfffffffdu })
            EXPECT("relocated leaf entry", rebuild::relocated_entry(leaf_entry(from, count), pairDelta, idxDelta), leaf_entry(to, count));
    }
    for (uint32_t id : { 3u, 1000u, kIdMask - 3u }) for (uint32_t idxDelta : { 0u, 9u, 0xfffffff7u }) {
        EXPECT("relocated interior entry", rebuild::relocated_entry(id, 3u, idxDelta), id + 3u);
        EXPECT("relocated interior entry", rebuild::relocated_entry(id, 0xfffffffdu, idxDelta), id - 3u);
    }
    EXPECT("relocated_first, interior", rebuild::relocated_first(10u, 0u, 0xfffffffeu, 5u), 8u);
    EXPECT("relocated_first, leaf", rebuild::relocated_first(10u, 2u, 0xfffffffeu, 5u), 15u);
    const std::vector<rebuild::BlasRange> ranges = { { 0u, 0u, 1u }, { 1u, 1u, 37u }, { 40u, 38u, 220u } };
    const rebuild::BlasBlock blocks[3] = { { 1u, 0u, 1u, 1, 0u }, { 39u, 1u, 37u, 0, 6u }, { 261u, 38u, 220u, 1, 9u } };
    std::string msg;
    const int32_t refit3[3] = { RT_REBUILD_KEEP, RT_REBUILD_SAH, RT_REBUILD_REFIT_RANGE }, notCompact[3] = { RT_REBUILD_KEEP, RT_REBUILD_REFIT_RANGE, RT_REBUILD_KEEP };
    const int32_t word3[3] = { RT_REBUILD_KEEP, RT_REBUILD_REFIT, RT_REBUILD_REFIT_RANGE };
    EXPECT("check_plan, a window in a refit range", rebuild::check_plan(refit3, 3, ranges, blocks, 1, 257, msg), RT_OK);
    EXPECT("check_plan, a window in a kept range", rebuild::check_plan(refit3, 3, ranges, blocks, 0, 5, msg), RT_E_INVALID);
    EXPECT("check_plan, a refit range that is not compact", rebuild::check_plan(notCompact, 3, ranges, blocks, 0, 0, msg), RT_E_UNSUPPORTED);
    EXPECT("check_plan names the range", msg.find("BLAS 1 (primitives [1, 38))") != std::string::npos, 1);
    EXPECT("check_plan, RT_REBUILD_REFIT", rebuild::check_plan(word3, 3, ranges, blocks, 0, 0, msg), RT_E_INVALID);
}

int main()
{
    entries();
    relocated_entries();
    pair_records();
    quad_records();
    triangle_records();
    instance_records();
    if (g_bad) { printf("%d checks failed\n", g_bad); return 1; }
    printf("records_main: ok\n");
    return 0;
}

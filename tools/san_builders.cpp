// san_builders — the host builders (binned SAH, SBVH with clipping, BVH4 collapse and its level-wise restatement, TLAS, parallel build)
// and the OBJ reader under AddressSanitizer/UBSan on the CPU build: random soups of every size class, degenerate input, hand-made node
// arrays, mutated OBJ text.
//   g++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=undefined tools/san_builders.cpp \
//       magr_ray_tracer_amd/host/{image_io,jpeg_io,scene_build,scene_io,accel_build,collapse_host}.cpp -lz -pthread -o /tmp/san_builders
#include <cmath>
#include <cstdio>
#include <cstring>
#include <exception>
#include <fstream>
#include <random>
#include <string>
#include "../include/rt355.h"
#include "../magr_ray_tracer_amd/host/rt_host.h"

using namespace rt355;

// rth_build_bvh4_levels' core on `n2` (roots `roots`): it must answer `expect`; with RT_OK and `want` given, the same bytes as `want`
static void levels(const std::vector<RtBVHNode2>& n2, int32_t nIdx, const std::vector<uint32_t>& roots, int expect, const std::vector<RtBVHNode4>* want,
                   const char* what)
{
    std::vector<RtBVHNode4> out(n2.size());
    std::vector<RtFloat4> quads(n2.size() * 8);
    std::vector<uint32_t> entry(roots.size()), qnode(n2.size());
    RtBvh4Stats st{};
    std::string err;
    const int rc = Bvh4LevelsHost(n2.data(), (int32_t)n2.size(), nIdx, roots.data(), (int32_t)roots.size(), out.data(), &st, quads.data(), entry.data(),
                                  qnode.data(), err);
    if (rc != expect) { printf("san_builders: %s: code %d, expected %d (%s)\n", what, rc, expect, err.c_str()); exit(1); }
    if (rc == 0 && want && memcmp(out.data(), want->data(), sizeof(RtBVHNode4) * out.size()) != 0) { printf("san_builders: %s: the level-wise collapse differs\n", what); exit(1); }
}
static RtBVHNode2 node2(float half, uint32_t first, uint32_t count)
{
    RtBVHNode2 n{};
    n.aabbMin = RtFloat4{ -half, -half, -half, 0 }; n.aabbMax = RtFloat4{ half, half, half, 0 };
    n.first = first; n.count = count;
    return n;
}
// a complete BVH2 of `lv` interior levels in pair order with one-primitive leaves; nanNode's box has a NaN extent
static std::vector<RtBVHNode2> complete(int lv, int nanNode)
{
    const uint32_t interiors = (1u << lv) - 1;
    std::vector<RtBVHNode2> n(2 * interiors + 1);
    for (uint32_t i = 0, slot = 0; i < n.size(); i++) {
        n[i] = i < interiors ? node2(1.0f, 2 * i + 1, 0) : node2(1.0f, slot++, 1);
        if ((int)i == nanNode) n[i].aabbMax.y = NAN;
    }
    return n;
}
// the hand-made arrays of tests/test_collapse_cpu.py, against BVH4::Convert (one BLAS rooted at node 0), and its refusals
static void hand_made()
{
    std::vector<RtPrimitive> prims; std::vector<RtBVHInstance> blas(1);
    memset(&blas[0], 0, sizeof blas[0]);
    auto reference = [&](const std::vector<RtBVHNode2>& n2) { BVH2 b2(prims, blas); b2.bvhNodes = n2; BVH4 b4(b2); return b4.Nodes(); };
    std::vector<RtBVHNode2> f(13);
    const int in[6][3] = { { 0, 1, 20 }, { 1, 3, 9 }, { 2, 5, 12 }, { 3, 7, 8 }, { 6, 9, 10 }, { 9, 11, 9 } };
    for (const auto& r : in) f[(size_t)r[0]] = node2((float)r[2], (uint32_t)r[1], 0);
    for (uint32_t k : { 4u, 5u, 7u, 8u, 10u, 11u }) f[k] = node2(0, k, k);
    f[12] = node2(0, 0, 12);
    std::vector<RtBVHNode4> want = reference(f);
    levels(f, 24, { 0 }, RT_OK, &want, "fixture13");
    for (int nanNode : { -1, 1 }) { const auto c = complete(5, nanNode); want = reference(c); levels(c, 32, { 0 }, RT_OK, &want, nanNode < 0 ? "lattice" : "nan child"); }
    std::vector<RtBVHNode2> u = f;                               // an unreachable interior record and its leaves
    u.push_back(node2(3, 14, 0)); u.push_back(node2(1, 1, 2)); u.push_back(node2(2, 3, 4));
    want = reference(u);
    levels(u, 24, { 0 }, RT_OK, &want, "unreachable");
    u[13].first = 15; levels(u, 24, { 0 }, RT_E_INVALID, nullptr, "unreachable record, child out of range");
    std::vector<RtBVHNode2> bad = f;
    bad[9].first = 0xffffffffu; levels(bad, 24, { 0 }, RT_E_INVALID, nullptr, "child index wraps");
    bad = f; bad[6].first = 7; levels(bad, 24, { 0 }, RT_E_INVALID, nullptr, "reachable twice");
    levels(f, 24, { 0, 1 }, RT_E_INVALID, nullptr, "a root inside another BLAS");
    levels(f, 24, { 0, 13 }, RT_E_INVALID, nullptr, "root out of range");
    levels(f, 21, { 0 }, RT_E_INVALID, nullptr, "leaf range");
    for (uint32_t h : { 64u, 65u }) {                            // a caterpillar on either side of the depth limit
        std::vector<RtBVHNode2> c(2 * h + 1);
        for (uint32_t k = 0; k < h; k++) { c[k == 0 ? 0 : 2 * k - 1] = node2(1.0f + (float)k, 2 * k + 1, 0); c[2 * k + 2] = node2(1, k, 1); }
        c[2 * h - 1] = node2(1, h, 1);
        if (h == 64) { want = reference(c); levels(c, (int32_t)h + 1, { 0 }, RT_OK, &want, "chain(64)"); }
        else levels(c, (int32_t)h + 1, { 0 }, RT_E_UNSUPPORTED, nullptr, "chain(65)");
    }
}

int main()
{
    hand_made();
    std::mt19937 rng(99);
    auto uni = [&](float a, float b) { return a + (b - a) * (float)(rng() & 0xffffff) / 16777216.0f; };
    int built = 0;
    for (int it = 0; it < 60; it++) {
        Scene s;
        s.AddMaterial("m");
        { RtMaterial& l = s.AddMaterial("light"); l.isLight = 1; }
        const int n = it < 6 ? it + 1 : (int)(rng() % 4000) + 2;
        for (int i = 0; i < n; i++) {
            const float3 c(uni(-5, 5), uni(-5, 5), uni(-5, 5));
            const float sz = (rng() % 10 == 0) ? 4.f : 0.5f;
            float3 a = c + float3(uni(-sz, sz), uni(-sz, sz), uni(-sz, sz)), b = c + float3(uni(-sz, sz), uni(-sz, sz), uni(-sz, sz)),
                   d = c + float3(uni(-sz, sz), uni(-sz, sz), uni(-sz, sz));
            if (rng() % 20 == 0) d = a;                         // degenerate
            if (rng() % 25 == 0) { a = c; b = c; d = c; }       // a point
            s.AddTriangle(a, b, d, { 0, 0 }, { 1, 0 }, { 0, 1 }, i % 50 == 0 ? "light" : "m");
        }
        static const float alphas[3] = { 1.f, 1e-5f, 0.f };
        s.bvh2->alpha = alphas[it % 3];
        s.bvh2->buildThreads = (it & 1) ? 8 : 1;
        s.bvh2->BuildBLAS(true, 0);
        if (it % 4 == 0) {                                       // a second BLAS over more triangles
            const int first = (int)s.primitives.size();
            for (int i = 0; i < 50; i++) s.AddTriangle(float3(uni(8, 9), uni(0, 1), uni(0, 1)), float3(uni(8, 9), uni(0, 1), uni(0, 1)), float3(uni(8, 9), uni(0, 1), uni(0, 1)), { 0, 0 }, { 0, 0 }, { 0, 0 }, "m");
            s.bvh2->BuildBLAS(true, first);
        }
        s.BuildBVH4();
        {   // the level-wise restatement gives the same array
            std::vector<uint32_t> roots;
            for (const RtBVHInstance& inst : s.blasNodes) roots.push_back(inst.bvhIdx);
            levels(s.bvh2->bvhNodes, (int32_t)s.bvh2->primIdx.size(), roots, RT_OK, &s.bvh4->Nodes(), "random soup");
        }
        if (it % 3 == 0 && s.blasNodes.size() > 1) {             // a moved instance: TLAS leaf bounds through inverse(invT)
            float* T = s.blasNodes[1].invT;
            const float a = uni(0, 6.28f), c = cosf(a), sn = sinf(a), sc = uni(0.5f, 2.f);
            const float m[16] = { c * sc, 0, sn * sc, uni(-3, 3), 0, sc, 0, uni(-3, 3), -sn * sc, 0, c * sc, uni(-3, 3), 0, 0, 0, 1 };
            for (int k = 0; k < 16; k++) T[k] = m[k];
        }
        TLAS t(*s.bvh2);
        t.Build();
        built++;
    }
    // OBJ reader on mutated text (the MTL names a texture that does not exist: LoadModel must report it, not crash)
    { std::ofstream m("/tmp/san_case.mtl"); m << "newmtl a\nmap_Kd missing_texture.png\nnewmtl b\nKd 1 0 0\n"; }
    const std::string obj = "mtllib san_case.mtl\nv 0 0 0\nv 1 0 0\nv 0 1 0\nv 1 1 0\nvt 0 0\nvt 1 0\nvt 0 1\nusemtl a\nf 1/1 2/2 3/3\nf -1/-1 -2/-2 -3/-3 -4\nf 1//1 2//2 4//4\n";
    int parsed = 0, rejected = 0;
    for (int it = 0; it < 3000; it++) {
        std::string b = obj;
        for (int k = 0; k < 1 + (int)(rng() % 6); k++) {
            const size_t p = rng() % b.size();
            switch (rng() % 4) { case 0: b[p] = (char)(32 + rng() % 90); break; case 1: b.erase(p, 1 + rng() % 5); break;
                                 case 2: b.insert(p, std::to_string((int)(rng() % 2000) - 1000)); break; default: b[p] = '/'; }
            if (b.empty()) b = "f";
        }
        { std::ofstream o("/tmp/san_case.obj"); o << b; }
        try { Scene s; s.AddMaterial("white"); s.LoadModel("/tmp/san_case.obj", "white"); parsed++; } catch (const std::exception&) { rejected++; }
    }
    // polygons (tinyobjloader's quad rule and ear clipping), number spellings and index forms, no texture to miss
    const std::string poly = "v 0 0 0\nv 2 0 0\nv 2 2 0\nv 1 .5 0\nv 0 2 0\nv 1e-3 -2.5E+2 .5\nv 3 3 3\nv -1 -1 2\nvt 0.5 0.25\nvt 1 1\n"
                             "f 1 2 3 4 5\nf 1/1 2/2 3/1 4/2\nf -1 -2 -3 -4 -5 -6 -7 -8\ng a\nf 1 2 3 4 5 6 7\no b\nf 8//1 7//1 6//1 5//1 4//1 3//1\nf 1 2\n";
    for (int it = 0; it < 3000; it++) {
        std::string b = poly;
        for (int k = 0; k < 1 + (int)(rng() % 5); k++) {
            const size_t p = rng() % b.size();
            switch (rng() % 4) { case 0: b[p] = (char)(32 + rng() % 90); break; case 1: b.erase(p, 1 + rng() % 5); break;
                                 case 2: b.insert(p, std::to_string((int)(rng() % 40) - 20)); break; default: b[p] = "/ .-e\n"[rng() % 6]; }
            if (b.empty()) b = "f";
        }
        { std::ofstream o("/tmp/san_case.obj"); o << b; }
        try { Scene s; s.AddMaterial("white"); s.LoadModel("/tmp/san_case.obj", "white"); parsed++; } catch (const std::exception&) { rejected++; }
    }
    printf("san_builders: %d scenes built, OBJ: %d parsed, %d rejected, no crash\n", built, parsed, rejected);
    return 0;
}

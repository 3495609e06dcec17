// trav_plan_main.cpp — csrc/trav_common.h on its own: the header compiles without HIP, and the boundaries of plan_traversal hold under
// the sanitizers.  Expected values are worked out by hand from the rules (tests/test_traversal_plan_cpu.py pins every field of the plan
// through the library; this program is for the compiler and the sanitizers).
//   g++ -std=c++17 -Wall -Wextra -fsanitize=address,undefined -fno-sanitize-recover=all tools/trav_plan_main.cpp -o trav_plan_main && ./trav_plan_main
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <initializer_list>
#include "../magr_ray_tracer_amd/csrc/trav_common.h"

using namespace rt355dev;

static const char* kKnobs[] = { "RT355_SPILL_CAP", "RT355_NO_SPILL", "RT355_COHERENT", "RT355_TUNE", "RT355_FIXED_CHUNKS", "RT355_TUNE_CONNECT",
                                "RT355_TOP_LEVELS", "RT355_TLAS_FLAT", "RT355_XCD_RAYS", "RT355_THIN", "RT355_CONNECT_BLOCKS" };
static int g_bad = 0;

// facts of a layout-1 scene with `stackEntries + tlasDepth + 1 = entries` column entries (tlasDepth 1 unless one BLAS)
static TravFacts facts(int accel, bool single, int entries, int variant = 0, int lds = 65536)
{
    TravFacts f;
    f.accel = accel; f.extend_variant = variant; f.layout = 1; f.singleBlas = single; f.tlasDepth = single ? 0 : 1;
    f.stackEntries = entries - f.tlasDepth - 1; f.nInterior = 1000; f.nQuads = 1000; f.sharedMemPerBlock = lds; f.xcdFirst = 3;
    return f;
}
static TravPlan plan(const TravFacts& f, std::initializer_list<const char*> env = {})
{
    for (const char* k : kKnobs) unsetenv(k);
    for (const char* kv : env) { const char* eq = strchr(kv, '='); char name[64] = {}; memcpy(name, kv, (size_t)(eq - kv)); setenv(name, eq + 1, 1); }
    return plan_traversal(f, read_trav_knobs());
}
#define EXPECT(what, got, want) do { const long g_ = (long)(got), w_ = (long)(want); if (g_ != w_) { printf("FAIL %s: %s = %ld, expected %ld\n", what, #got, g_, w_); g_bad++; } } while (0)

int main()
{
    const int B2 = RT_ACCEL_BVH2, B4 = RT_ACCEL_BVH4;
    TravFacts f;
    // one BLAS
    EXPECT("one BLAS, BVH2", plan(facts(B2, true, 20)).trav, TRAV_BVH2);
    EXPECT("one BLAS, BVH4", plan(facts(B4, true, 20)).trav, TRAV_BVH4);
    EXPECT("one BLAS, BVH4, variant 6", plan(facts(B4, true, 20, 6)).trav, TRAV_BVH4);
    EXPECT("variant 2", plan(facts(B2, true, 20, 2)).trav, TRAV_NESTED);
    f = facts(B2, true, 20); f.layout = 0;
    EXPECT("layout 0", plan(f).trav, TRAV_NESTED);
    // several BLAS, BVH2
    f = facts(B2, false, 20); f.stackEntries = 10; f.tlasDepth = 8; EXPECT("tlasDepth 8", plan(f).trav, TRAV_TLAS);   // 19, 20 entries
    f.tlasDepth = 9; EXPECT("tlasDepth 9", plan(f).trav, TRAV_NESTED);
    f = facts(B2, false, 20); f.nInterior = (1 << 29) - 1; EXPECT("2^29 - 1 pair records", plan(f).trav, TRAV_TLAS);
    f.nInterior = 1 << 29; EXPECT("2^29 pair records", plan(f).trav, TRAV_NESTED);
    EXPECT("variant 4", plan(facts(B2, false, 20, 4)).trav, TRAV_NESTED);
    // several BLAS, BVH4
    EXPECT("BVH4, variant 0", plan(facts(B4, false, 20, 0)).trav, TRAV_NESTED);
    EXPECT("BVH4, variant 6", plan(facts(B4, false, 20, 6)).trav, TRAV_BVH4_TLAS);
    f = facts(B4, false, 20, 6); f.nQuads = 1 << 29; EXPECT("2^29 quad records", plan(f).trav, TRAV_NESTED);
    f = facts(B4, false, 20, 6); f.tlasDepth = 9; EXPECT("BVH4, tlasDepth 9", plan(f).trav, TRAV_NESTED);
    // column depth
    EXPECT("22 entries", plan(facts(B2, false, 22)).trav, TRAV_TLAS);
    { const TravPlan p = plan(facts(B2, false, 23)); EXPECT("23 entries", p.trav, TRAV_TLAS_SPILL); EXPECT("23 entries", p.spillCap, 12); }
    EXPECT("23 entries, NO_SPILL", plan(facts(B2, false, 23), { "RT355_NO_SPILL=1" }).trav, TRAV_TLAS);
    EXPECT("73 entries, NO_SPILL", plan(facts(B2, false, 73), { "RT355_NO_SPILL=1" }).trav, TRAV_TLAS);
    { const TravPlan p = plan(facts(B2, false, 74), { "RT355_NO_SPILL=1" }); EXPECT("74 entries, NO_SPILL", p.trav, TRAV_NESTED); EXPECT("74 entries, NO_SPILL", p.tune.flat, 0); }
    // RT355_SPILL_CAP
    { const TravPlan p = plan(facts(B2, false, 10), { "RT355_SPILL_CAP=6" }); EXPECT("cap 6, 10 entries", p.trav, TRAV_TLAS_SPILL); EXPECT("cap 6, 10 entries", p.spillCap, 6); }
    EXPECT("cap 6, 6 entries", plan(facts(B2, false, 6), { "RT355_SPILL_CAP=6" }).trav, TRAV_TLAS);
    for (const char* kv : { "RT355_SPILL_CAP=5", "RT355_SPILL_CAP=65" }) {
        const TravPlan p = plan(facts(B2, false, 20), { kv });
        EXPECT(kv, p.trav, TRAV_TLAS); EXPECT(kv, p.spillCap, 12);
    }
    { const TravPlan p = plan(facts(B2, false, 65), { "RT355_SPILL_CAP=64" }); EXPECT("cap 64, 65 entries", p.trav, TRAV_TLAS_SPILL); EXPECT("cap 64, 65 entries", p.spillCap, 64); }
    // BVH4 TLAS against 64 KB and 160 KB of LDS
    EXPECT("BVH4 22 entries", plan(facts(B4, false, 22, 6)).trav, TRAV_BVH4_TLAS);
    EXPECT("BVH4 23 entries", plan(facts(B4, false, 23, 6)).trav, TRAV_BVH4_TLAS_SPILL);
    EXPECT("BVH4 54 entries, NO_SPILL", plan(facts(B4, false, 54, 6), { "RT355_NO_SPILL=1" }).trav, TRAV_BVH4_TLAS);
    EXPECT("BVH4 55 entries, NO_SPILL", plan(facts(B4, false, 55, 6), { "RT355_NO_SPILL=1" }).trav, TRAV_NESTED);
    EXPECT("BVH4 65 entries, cap 64", plan(facts(B4, false, 65, 6), { "RT355_SPILL_CAP=64" }).trav, TRAV_NESTED);
    EXPECT("BVH4 30 entries, cap 64", plan(facts(B4, false, 30, 6), { "RT355_SPILL_CAP=64" }).trav, TRAV_BVH4_TLAS);
    EXPECT("BVH4 55 entries, 160 KB", plan(facts(B4, false, 55, 6, 163840)).trav, TRAV_BVH4_TLAS_SPILL);
    EXPECT("BVH4 55 entries, 160 KB, NO_SPILL", plan(facts(B4, false, 55, 6, 163840), { "RT355_NO_SPILL=1" }).trav, TRAV_BVH4_TLAS);
    // the tunes' clamps and the knobs that are ignored
    {
        const TravPlan p = plan(facts(B2, true, 20), { "RT355_THIN=100", "RT355_XCD_RAYS=-3", "RT355_TOP_LEVELS=7", "RT355_TUNE=64,65,6,8", "RT355_CONNECT_BLOCKS=3" });
        EXPECT("clamps", p.tune.thin, 64); EXPECT("clamps", p.tuneConnect.xcdRays, 0); EXPECT("clamps", p.tune.topLevels, 6); EXPECT("clamps", p.topAuto, 1);
        EXPECT("clamps", p.tune.chunk, 112); EXPECT("clamps", p.connectBlocks, 3); EXPECT("clamps", p.tune4.xcdFirst, 3);
    }
    {
        f = facts(B2, true, 20); f.persist_blocks_per_cu = 2;
        EXPECT("shared", plan(f).tune.leafK, 16); EXPECT("shared", plan(f).tune.fixedChunks, 0);
        const TravPlan p = plan(f, { "RT355_TUNE=64,20,6,8,1", "RT355_TOP_LEVELS=2,5" });
        EXPECT("RT355_TUNE", p.tune.leafK, 8); EXPECT("RT355_TUNE", p.tuneBlocks, 1); EXPECT("RT355_TUNE", p.tuneConnect.chunk, 64);
        EXPECT("RT355_TOP_LEVELS", p.tune.topLevels, 2); EXPECT("RT355_TOP_LEVELS", p.tuneConnect.topLevels, 5); EXPECT("RT355_TOP_LEVELS", p.topAuto, 0);
    }
    EXPECT("column bytes", tlas_column_bytes(54), 65536); EXPECT("stack bytes", stack_bytes(22), 22528); EXPECT("top bytes", top_bytes(6), 63 * 64);
    (void)read_shade_knobs();
    if (g_bad) { printf("%d checks failed\n", g_bad); return 1; }
    printf("trav_plan_main: ok\n");
    return 0;
}

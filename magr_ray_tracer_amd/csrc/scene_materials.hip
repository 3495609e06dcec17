// scene_materials.hip — in-place material updates of a bound scene copy (rt_update_materials; kernels: rebuild.hip, rules:
// resize_common.h).  Host code only; what it shares with the upload and the rebuilds is scene_dev.h's.
#include <chrono>
#include "scene_dev.h"
#include "resize_common.h"

using namespace scenedev;

// validate_scene's checks of a material table against an atlas of nTexels texels, with its message; texPad receives the atlas pad
static int materials_check(const char* who, const RtMaterial* mats, int32_t nMats, int64_t nTexels, int64_t* texPad)
{
    if (!mats || nMats <= 0) return fail(RT_E_INVALID, "%s: a material table holds at least one material (nMats %d)", who, nMats);
    if (nTexels < 0) return fail(RT_E_INVALID, "%s: negative atlas length %lld", who, (long long)nTexels);
    if (const int32_t m = resize::check_materials(mats, nMats, nTexels, texPad); m >= 0)
        return fail(RT_E_INVALID, "material %d: texture window exceeds the atlas", m);
    return RT_OK;
}
extern "C" int rt_materials_check(const RtMaterial* mats, int32_t nMats, int32_t nTexels)
{
    return materials_check("rt_materials_check", mats, nMats, nTexels, nullptr);
}
int scenedev::update_materials(SceneBag& b, const RtMaterialUpdate& u, RtMaterialStats* stats)
{
    using clock = std::chrono::steady_clock;
    const char* who = "rt_update_materials";
    const auto t0 = clock::now();
    const SceneArrays& sc = b.sc;
    // ---- refusals that need no device work: counts and ranges, then the table that will be bound against the atlas that will be bound
    const bool newTable = u.mats != nullptr;
    if (newTable && u.nMats <= 0) return fail(RT_E_INVALID, "%s: a material table holds at least one material (nMats %d)", who, u.nMats);
    if (u.nTexels < -1) return fail(RT_E_INVALID, "%s: nTexels %d (the new atlas length, or -1 to keep the bound one)", who, u.nTexels);
    if (u.texFirst < 0 || u.texCount < 0) return fail(RT_E_INVALID, "%s: negative texel range (first %d, count %d)", who, u.texFirst, u.texCount);
    if (u.primFirst < 0 || u.primCount < 0) return fail(RT_E_INVALID, "%s: negative primitive range (first %d, count %d)", who, u.primFirst, u.primCount);
    if (u.texCount > 0 && !u.texels) return fail(RT_E_INVALID, "%s: texCount %d but texels == NULL", who, u.texCount);
    if (u.primCount > 0 && !u.primMat) return fail(RT_E_INVALID, "%s: primCount %d but primMat == NULL", who, u.primCount);
    const int32_t oldTex = sc.nTex, nTex = u.nTexels < 0 ? sc.nTex : u.nTexels;
    if (u.texels && (int64_t)u.texFirst + u.texCount > (int64_t)nTex)
        return fail(RT_E_INVALID, "%s: texel range [%d, %lld) outside the new atlas of %d texels", who, u.texFirst, (long long)u.texFirst + u.texCount, nTex);
    if (u.primMat && (int64_t)u.primFirst + u.primCount > (int64_t)sc.nPrims)
        return fail(RT_E_INVALID, "%s: primitive range [%d, %lld) outside the %d bound", who, u.primFirst, (long long)u.primFirst + u.primCount, sc.nPrims);
    const bool writeTex = u.texels && u.texCount > 0, assign = u.primMat && u.primCount > 0;
    const int32_t nMats = newTable ? u.nMats : sc.nMats;
    int64_t texPad = b.texPad;
    if (newTable || nTex != oldTex)   // (mats NULL: the bound table, from its host shadow, against a new atlas length)
        if (const int rc = materials_check(who, newTable ? u.mats : b.hMats.data(), nMats, nTex, &texPad)) return rc;
    const bool lightsChange = newTable || assign, padChange = nTex != oldTex || texPad != b.texPad;
    if (stats) { *stats = RtMaterialStats{}; stats->lights = sc.nLights; }
    if (!lightsChange && !writeTex && !padChange) return RT_OK;   // nothing to do: nothing is touched
    HIPCHK(hipSetDevice(b.device));
    if (const int rc = scene_stream(b, b.rev)) return rc;
    hipStream_t s = b.stream;
    // ---- device memory: everything is made before anything is written (a call that ran out of memory is taken up where it stopped)
    SceneBag::Grown<RtMaterial>& M = b.mmats[b.mmatsNext];
    SceneBag::LightSet& L = b.mlights[b.mlightsNext];
    SceneBag::Grown<RtFloat4>& T = b.mtex[b.mtexNext];
    const size_t texNeed = (size_t)nTex + (size_t)texPad;
    const bool moveTex = texNeed > b.texCap;
    if (lightsChange) {
        if (!b.rStatus) { if (const int rc = dalloc(b.allocs, &b.rStatus, 2)) return rc; b.rallocs++; }
        if (const int rc = rebuild_scratch(b, (size_t)sc.nPrims)) return rc;   // (flags and ranks: a word per primitive)
        if (newTable) if (const int rc = rebuild_fit(b, M, (size_t)nMats, "the material table")) return rc;
        if (assign) if (const int rc = rebuild_fit(b, b.mAssign, (size_t)u.primCount, "the new matIdx values")) return rc;
    }
    if (moveTex) if (const int rc = rebuild_fit(b, T, texNeed, "the texture atlas")) return rc;
    // ---- stage, in memory no holder reads: the table, the new assignment (one path for host and device input), the light list and the
    // complete light records under both; an atlas that has to move, whole
    HIPCHK(hipEventRecord(b.rev[0], s));
    int32_t nLights = sc.nLights;
    const int32_t* dAssign = nullptr;
    if (lightsChange) {
        const RtMaterial* dMats = sc.mats;
        if (newTable) { HIPCHK(hipMemcpyAsync(M.p, u.mats, sizeof(RtMaterial) * (size_t)nMats, hipMemcpyHostToDevice, s)); dMats = M.p; }
        if (assign) { HIPCHK(hipMemcpyAsync(b.mAssign.p, u.primMat, sizeof(int32_t) * (size_t)u.primCount, hipMemcpyDefault, s)); dAssign = b.mAssign.p; }
        uint32_t* bad = (uint32_t*)b.rStatus;
        const uint32_t first = (uint32_t)u.primFirst, count = assign ? (uint32_t)u.primCount : 0u;
        HIPCHK(rebuilddev::mat_flags(s, b.dw, sc.prims, (uint32_t)sc.nPrims, dAssign, first, count, dMats, nMats, bad));
        uint32_t firstBad = resize::kNoBad;
        if (const int rc = flag_scan_result(b, sc.nPrims, &firstBad, &nLights)) return rc;
        if (firstBad != resize::kNoBad) {   // a new value out of range, or a bound primitive the new, shorter table no longer serves
            int32_t mat = 0;
            const bool inRange = dAssign && firstBad - first < count;
            HIPCHK(hipMemcpy(&mat, inRange ? (const void*)(dAssign + (firstBad - first)) : (const void*)&sc.prims[firstBad].matIdx, sizeof mat, hipMemcpyDeviceToHost));
            return fail(RT_E_INVALID, "%s: primitive %u: matIdx %d outside the new table (nMats %d); the scene is unchanged", who, firstBad, mat, nMats);
        }
        int rc = rebuild_fit(b, L.lights, (size_t)nLights, "the light list");
        if (rc == RT_OK) rc = rebuild_fit(b, L.lightRecs, std::max<size_t>((size_t)nLights, 1) * 8, "light records");
        if (rc != RT_OK) return rc;
        HIPCHK(rebuilddev::mat_emit(s, b.dw, sc.prims, (uint32_t)sc.nPrims, dAssign, first, count, dMats, (uint32_t)nLights, L.lights.p, L.lightRecs.p));
    }
    if (moveTex) {   // the kept part device to device, the rest and the pad zero, then the range
        const size_t keep = (size_t)std::min(oldTex, nTex);
        if (keep) HIPCHK(hipMemcpyAsync(T.p, sc.tex, sizeof(RtFloat4) * keep, hipMemcpyDeviceToDevice, s));
        HIPCHK(hipMemsetAsync(T.p + keep, 0, sizeof(RtFloat4) * (texNeed - keep), s));
        if (writeTex) HIPCHK(hipMemcpyAsync(T.p + u.texFirst, u.texels, sizeof(RtFloat4) * (size_t)u.texCount, hipMemcpyDefault, s));
    }
    HIPCHK(hipEventRecord(b.rev[1], s));
    HIPCHK(hipStreamSynchronize(s));
    // ---- commit: no kernel of a holder may read the arrays while they are patched; then the swap
    if (const int rc = b.wait_holders()) return rc;
    HIPCHK(hipEventRecord(b.rev[2], s));
    if (assign) HIPCHK(rebuilddev::mat_assign(s, sc.prims, dAssign, (uint32_t)u.primFirst, (uint32_t)u.primCount, sc.shadeRecs));
    if (!moveTex) {   // the live atlas has the room: what an in-place growth uncovers is zeroed, then the range, then the pad
        if (nTex > oldTex) HIPCHK(hipMemsetAsync(sc.tex + oldTex, 0, sizeof(RtFloat4) * (size_t)(nTex - oldTex), s));
        if (writeTex) HIPCHK(hipMemcpyAsync(sc.tex + u.texFirst, u.texels, sizeof(RtFloat4) * (size_t)u.texCount, hipMemcpyDefault, s));
        if (padChange) HIPCHK(hipMemsetAsync(sc.tex + nTex, 0, sizeof(RtFloat4) * (size_t)texPad, s));
    }
    HIPCHK(hipEventRecord(b.rev[3], s));
    HIPCHK(hipStreamSynchronize(s));
    SceneArrays n = b.sc;
    if (newTable) { n.mats = M.p; n.nMats = nMats; b.mmatsNext ^= 1; b.hMats.assign(u.mats, u.mats + nMats); }
    if (lightsChange) {
        n.lights = L.lights.p; n.lightRecs = L.lightRecs.p; n.nLights = nLights; b.mlightsNext ^= 1;
        b.lightsInSet = true;   // later rebuilds carry the list from set to set, as after a resize
    }
    if (moveTex) { n.tex = T.p; b.texCap = T.cap; b.mtexNext ^= 1; }
    n.nTex = nTex; b.texPad = texPad;
    if (assign && !b.primMat.empty())   // the host shadow of matIdx: the range's values, the only per-primitive data that comes back
        HIPCHK(hipMemcpy(b.primMat.data() + u.primFirst, dAssign, sizeof(int32_t) * (size_t)u.primCount, hipMemcpyDeviceToHost));
    const bool rebind = n.mats != sc.mats || n.lights != sc.lights || n.lightRecs != sc.lightRecs || n.tex != sc.tex || n.nMats != sc.nMats ||
                        n.nLights != sc.nLights || n.nTex != sc.nTex;
    b.sc = n;
    if (rebind) b.generation++;   // every holder takes the new arrays and counts before its next launch
    if (stats) {
        float ms = 0, ms2 = 0;   // GPU time of both phases (not the wait for the holders in between)
        (void)hipEventElapsedTime(&ms, b.rev[0], b.rev[1]); (void)hipEventElapsedTime(&ms2, b.rev[2], b.rev[3]);
        stats->gpu_ms = ms + ms2; stats->wall_ms = ms_between(t0, clock::now());
        stats->mats = newTable ? nMats : 0; stats->texels = writeTex ? u.texCount : 0; stats->prims = assign ? u.primCount : 0;
        stats->lights = nLights; stats->atlas_reallocated = moveTex ? 1 : 0;
    }
    return RT_OK;
}

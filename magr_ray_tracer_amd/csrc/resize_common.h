// resize_common.h — the rules of rt_resize_scene (include/rt355.h) that its kernels in rebuild.hip, the argument checks of scene.hip and the
// host restatement (host/host_capi.cpp, rth_light_list) share: which primitive records a resize takes, which primitives are lights, and
// what a caller's shape (ranges, instance map, transforms) must look like.
#pragma once
#include <string>
#include <vector>
#include "refit_common.h"

namespace resize {

constexpr uint32_t kNoBad = 0xffffffffu;   // the status word of k_resize_check while no primitive has been refused

// validate_scene's rule for one primitive: objType is one of RT_PRIM_*, matIdx names a bound material
LB_HD bool prim_ok(int32_t objType, int32_t matIdx, int32_t nMats)
{
    return objType >= RT_PRIM_SPHERE && objType <= RT_PRIM_TRIANGLE && matIdx >= 0 && matIdx < nMats;
}
// Scene's rule for the light list (host/scene_build.cpp): a primitive is a light iff its material is one; the list holds their indices
// in increasing order, so a light's position is the number of lights before it
LB_HD uint32_t light_flag(const RtMaterial* mats, int32_t matIdx) { return mats[matIdx].isLight != 0 ? 1u : 0u; }
// the complete light record of primitive p (8 rows): refit::light_rec's words 0..4, the material's emittance, zeros
LB_HD void light_record(const RtPrimitive& p, const RtMaterial* mats, RtFloat4* r)
{
    refit::light_rec(p, r);
    r[5] = mats[p.matIdx].emittance;
    r[6] = r[7] = refit::f4(0, 0, 0, 0);
}
// ... of a primitive that rt_update_materials is about to give the material matIdx (its own matIdx is stale until the commit)
LB_HD void light_record_as(const RtPrimitive& p, int32_t matIdx, const RtMaterial* mats, RtFloat4* r)
{
    refit::light_rec(p, r);
    r[5] = mats[matIdx].emittance;
    r[6] = r[7] = refit::f4(0, 0, 0, 0);
}
// rt_update_materials: the matIdx primitive i has after the call - assign[i - first] inside [first, first + count), the bound one outside
LB_HD int32_t new_mat(const RtPrimitive* prims, uint32_t i, const int32_t* assign, uint32_t first, uint32_t count)
{
    return assign && i - first < count ? assign[i - first] : prims[i].matIdx;   // (i < first wraps past count)
}
// validate_scene's rule for a material table against an atlas of nTexels texels: -1, or the first material whose texture window is not
// inside it; texPad receives the atlas pad (max(2, texW + 2) over the textured materials)
inline int32_t check_materials(const RtMaterial* mats, int32_t nMats, int64_t nTexels, int64_t* texPad)
{
    int64_t pad = 2;   // the reference's lookup can land one row + one texel past a texture (uv == 1)
    for (int32_t i = 0; i < nMats; i++) if (mats[i].texIdx != -1) {
        if (mats[i].texIdx < 0 || mats[i].texW <= 0 || mats[i].texH <= 0 || (int64_t)mats[i].texIdx + (int64_t)mats[i].texW * mats[i].texH > nTexels) return i;
        pad = pad > (int64_t)mats[i].texW + 2 ? pad : (int64_t)mats[i].texW + 2;
    }
    if (texPad) *texPad = pad;
    return -1;
}

// ---- host only ----
// The light list of prims[nPrims] on the host (every record must have passed prim_ok)
inline void light_list(const RtPrimitive* prims, int32_t nPrims, const RtMaterial* mats, std::vector<uint32_t>& lights)
{
    lights.clear();
    for (int32_t i = 0; i < nPrims; i++) if (light_flag(mats, prims[i].matIdx)) lights.push_back((uint32_t)i);
}
// The shape of a resize, checked before any device work: NULL, or what is wrong with it.  nRanges BLAS cover the new primitive array
// back to back (rangeCount), nBlas instances name them (instRange), invT (NULL: identity) must be regular.
inline const char* check_shape(int32_t nPrims, int32_t nRanges, const int32_t* rangeCount, int32_t nBlas, const int32_t* instRange,
                               const RtBVHInstance* blas, std::string& msg)
{
    if (nPrims <= 0) { msg = "nPrims must be positive (" + std::to_string(nPrims) + " given)"; return msg.c_str(); }
    if (nRanges < 1 || !rangeCount) { msg = "at least one BLAS range is required (nRanges " + std::to_string(nRanges) + ")"; return msg.c_str(); }
    if (nBlas < 1 || nBlas > refit::kMaxInstances) { msg = std::to_string(nBlas) + " instances: 1.." + std::to_string(refit::kMaxInstances) + " are supported"; return msg.c_str(); }
    if (!instRange) { msg = "instRange is NULL"; return msg.c_str(); }
    int64_t sum = 0;
    for (int32_t k = 0; k < nRanges; k++) {
        if (rangeCount[k] < 1) { msg = "range " + std::to_string(k) + " holds " + std::to_string(rangeCount[k]) + " primitives: every BLAS needs at least one"; return msg.c_str(); }
        sum += rangeCount[k];
    }
    if (sum != nPrims) { msg = "the ranges hold " + std::to_string(sum) + " primitives in all, nPrims is " + std::to_string(nPrims); return msg.c_str(); }
    std::vector<uint8_t> named((size_t)nRanges, 0);
    for (int32_t i = 0; i < nBlas; i++) {
        if (instRange[i] < 0 || instRange[i] >= nRanges) { msg = "instance " + std::to_string(i) + ": instRange " + std::to_string(instRange[i]) + " outside [0, " + std::to_string(nRanges) + ")"; return msg.c_str(); }
        named[(size_t)instRange[i]] = 1;
    }
    for (int32_t k = 0; k < nRanges; k++) if (!named[(size_t)k]) { msg = "range " + std::to_string(k) + " is named by no instance"; return msg.c_str(); }
    if (blas) for (int32_t i = 0; i < nBlas; i++) if (refit::singular(blas[i].invT)) { msg = "instance " + std::to_string(i) + ": the transform is singular"; return msg.c_str(); }
    return nullptr;
}

} // namespace resize

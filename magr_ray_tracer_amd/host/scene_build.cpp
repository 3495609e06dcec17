// scene_build.cpp — Scene primitive/material factory and CameraManager maths.
// Mirrors reference src/scene.cpp:84-176 (AddMaterial, AddSphere, AddPlane, AddQuad,
// AddTriangle: geometric normal, centroid, Heron area, light list) and
// src/camera.h:24-121 (Fov, UpdateCamVec).  File IO (LoadModel, LoadTexture) lives in
// scene_io.cpp / image_io.cpp; AddTexture takes texels that are already in memory.
#include <cmath>
#include <cstring>
#include <iterator>
#include "../../include/rt355.h"
#include "../csrc/resize_common.h"
#include "rt_host.h"

namespace rt355 {

Scene::Scene() { bvh2 = new BVH2(primitives, blasNodes); }
Scene::~Scene() { delete bvh4; delete bvh2; }

RtMaterial& Scene::AddMaterial(const std::string& name) // scene.cpp:84-100
{
    RtMaterial m;
    memset(&m, 0, sizeof m);
    m.texIdx = -1;
    materials.push_back(m);
    matMap_[name] = matIdx_++;
    return materials.back();
}
int Scene::MaterialIndex(const std::string& name) { return matMap_[name]; } // unknown names fall back to 0 like matMap_[name]

int Scene::AddTexture(const RtFloat4* texels, int width, int height, const std::string& name) // scene.cpp:244-256
{
    int texIdx = (int)textures.size();
    textures.insert(textures.end(), texels, texels + (size_t)width * height);
    RtMaterial& m = AddMaterial(name);
    m.texIdx = texIdx; m.isDielectric = 0; m.texW = width; m.texH = height;
    return matIdx_ - 1;
}

void Scene::AddSphere(float3 pos, float radius, const std::string& material) // scene.cpp:125-138
{
    RtPrimitive p;
    memset(&p, 0, sizeof p);
    p.objType = RT_PRIM_SPHERE;
    p.obj.sphere.pos = to4(pos);
    p.obj.sphere.r = radius; p.obj.sphere.r2 = radius * radius; p.obj.sphere.invr = 1 / radius;
    p.matIdx = matMap_[material];
    p.area = 4 * 3.14159265358979323846264f * p.obj.sphere.r2;
    primitives.push_back(p);
    if (materials[p.matIdx].isLight) lights.push_back((uint32_t)primitives.size() - 1);
}
void Scene::AddPlane(float3 N, float d, const std::string& material) // scene.cpp:140-150
{
    RtPrimitive p;
    memset(&p, 0, sizeof p);
    p.objType = RT_PRIM_PLANE;
    p.obj.plane.N = to4(N); p.obj.plane.d = d;
    p.matIdx = matMap_[material];
    primitives.push_back(p);
    if (materials[p.matIdx].isLight) lights.push_back((uint32_t)primitives.size() - 1);
}
void Scene::AddQuad(float3 v0, float3 v1, float3 v2, float3 v3, const std::string& material, bool flip,
                    float2 uv0, float2 uv1, float2 uv2, float2 uv3) // scene.cpp:152-156
{
    AddTriangle(v0, v1, v2, uv0, uv1, uv2, material, flip);
    AddTriangle(v2, v3, v0, uv2, uv3, uv1, material, flip);
}
void Scene::AddTriangle(float3 v0, float3 v1, float3 v2, float2 uv0, float2 uv1, float2 uv2,
                        const std::string& material, bool flip) // scene.cpp:158-176
{
    RtPrimitive p;
    memset(&p, 0, sizeof p);
    p.objType = RT_PRIM_TRIANGLE;
    RtTriangle& t = p.obj.triangle;
    t.v0 = to4(v0); t.v1 = to4(v1); t.v2 = to4(v2);
    t.uv0 = RtFloat2{ uv0.x, uv0.y }; t.uv1 = RtFloat2{ uv1.x, uv1.y }; t.uv2 = RtFloat2{ uv2.x, uv2.y };
    t.N = to4(normalize(cross(v1 - v0, v2 - v0)));
    if (flip) { t.N.x *= -1; t.N.y *= -1; t.N.z *= -1; t.N.w *= -1; }
    t.centroid = to4((v0 + v1 + v2) * (1 / 3.f));
    p.matIdx = matMap_[material];
    float a = length(v1 - v0), b = length(v1 - v2), c = length(v2 - v0); // Heron, scene.cpp:107-123
    float s = 0.5f * (a + b + c);
    p.area = sqrtf(s * (s - a) * (s - b) * (s - c));
    primitives.push_back(p);
    if (materials[p.matIdx].isLight) lights.push_back((uint32_t)primitives.size() - 1);
}
void Scene::BuildBVH4() { delete bvh4; bvh4 = new BVH4(*bvh2); } // scene.cpp:71

// ---- the host restatement of rt_update_materials: the checks of csrc/resize_common.h, the Scene rule for the light list ---------------
int Scene::SetMaterials(const RtMaterial* mats, int32_t nMats, std::string& err)
{
    if (!mats || nMats <= 0) { err = "rth_set_materials: a material table holds at least one material (nMats " + std::to_string(nMats) + ")"; return RT_E_INVALID; }
    if (const int32_t m = resize::check_materials(mats, nMats, (int64_t)textures.size(), nullptr); m >= 0) {
        err = "material " + std::to_string(m) + ": texture window exceeds the atlas"; return RT_E_INVALID;
    }
    for (size_t i = 0; i < primitives.size(); i++) if (primitives[i].matIdx < 0 || primitives[i].matIdx >= nMats) {
        err = "rth_set_materials: primitive " + std::to_string(i) + ": matIdx " + std::to_string(primitives[i].matIdx) + " outside the new table (nMats " +
              std::to_string(nMats) + "); the scene is unchanged";
        return RT_E_INVALID;
    }
    materials.assign(mats, mats + nMats);
    for (auto it = matMap_.begin(); it != matMap_.end();) it = it->second >= nMats ? matMap_.erase(it) : std::next(it);
    matIdx_ = nMats;
    resize::light_list(primitives.data(), (int32_t)primitives.size(), materials.data(), lights);
    return RT_OK;
}
int Scene::SetTexels(const RtFloat4* texels, int32_t first, int32_t count, int32_t nTexels, std::string& err)
{
    if (nTexels < -1) { err = "rth_set_texels: nTexels " + std::to_string(nTexels) + " (the new atlas length, or -1 to keep it)"; return RT_E_INVALID; }
    if (first < 0 || count < 0 || (count > 0 && !texels)) { err = "rth_set_texels: bad texel range / NULL texels"; return RT_E_INVALID; }
    const int64_t n = nTexels < 0 ? (int64_t)textures.size() : (int64_t)nTexels;
    if (texels && (int64_t)first + count > n) {
        err = "rth_set_texels: texel range [" + std::to_string(first) + ", " + std::to_string((int64_t)first + count) + ") outside the new atlas of " + std::to_string(n) + " texels";
        return RT_E_INVALID;
    }
    if (const int32_t m = resize::check_materials(materials.data(), (int32_t)materials.size(), n, nullptr); m >= 0) {
        err = "material " + std::to_string(m) + ": texture window exceeds the atlas"; return RT_E_INVALID;
    }
    textures.resize((size_t)n, RtFloat4{ 0, 0, 0, 0 });   // kept texels stay, new ones are zero
    if (texels && count) memcpy(textures.data() + first, texels, sizeof(RtFloat4) * (size_t)count);
    return RT_OK;
}
int Scene::SetPrimMaterials(int32_t first, int32_t count, const int32_t* matIdx, std::string& err)
{
    if (first < 0 || count < 0 || (count > 0 && !matIdx)) { err = "rth_set_prim_materials: bad primitive range / NULL values"; return RT_E_INVALID; }
    if (matIdx && (int64_t)first + count > (int64_t)primitives.size()) {
        err = "rth_set_prim_materials: primitive range [" + std::to_string(first) + ", " + std::to_string((int64_t)first + count) + ") outside the " +
              std::to_string(primitives.size()) + " primitives";
        return RT_E_INVALID;
    }
    for (int32_t k = 0; k < count; k++) if (matIdx[k] < 0 || matIdx[k] >= (int32_t)materials.size()) {
        err = "rth_set_prim_materials: primitive " + std::to_string(first + k) + ": matIdx " + std::to_string(matIdx[k]) + " outside the table (nMats " +
              std::to_string(materials.size()) + "); the scene is unchanged";
        return RT_E_INVALID;
    }
    for (int32_t k = 0; k < count; k++) primitives[(size_t)first + (size_t)k].matIdx = matIdx[k];
    resize::light_list(primitives.data(), (int32_t)primitives.size(), materials.data(), lights);
    return RT_OK;
}

// ------------------------------------------------------------------ camera
CameraManager::CameraManager(int width, int height, float vfov, int type) // camera.h:24-34
{
    memset(&cam, 0, sizeof cam);
    aspect = (float)width / (float)height;
    cam.type = type;
    cam.origin = RtFloat4{ -10, 10, 15, 0 };
    cam.forward = RtFloat4{ 0, 0, 1, 0 };
    cam.right = RtFloat4{ 1, 0, 0, 0 };
    cam.up = RtFloat4{ 0, 1, 0, 0 };
    cam.aperture = 0.1f;
    cam.focalLength = 1;
    Fov(vfov);
}
void CameraManager::Fov(float vfov) // camera.h:101-109 (theta is a double there: float*PI / 180.0)
{
    cam.fov = vfov;
    double theta = (double)(cam.fov * 3.14159265358979323846264f) / 180.0;
    double h = tan(theta / 2);
    viewportHeight = (float)(2 * h);
    viewportWidth = aspect * viewportHeight;
}
void CameraManager::Move(int camdir, float) // camera.h:47-73 (velocity = speed, deltaTime unused there too)
{
    moved = true;
    const float v = speed;
    auto axpy = [&](const RtFloat4& d, float s) { cam.origin.x += d.x * s; cam.origin.y += d.y * s; cam.origin.z += d.z * s; cam.origin.w += d.w * s; };
    switch (camdir) {
    case 0: axpy(cam.forward, -v); break;   // Forward: the camera looks along -forward
    case 1: axpy(cam.forward, v); break;
    case 2: axpy(cam.right, -v); break;
    case 3: axpy(cam.right, v); break;
    case 4: axpy(cam.up, v); break;
    case 5: axpy(cam.up, -v); break;
    }
}
void CameraManager::MouseMove(float xOffset, float yOffset) // camera.h:75-93
{
    moved = true;
    xOffset *= mouseSensivity; yOffset *= mouseSensivity;
    yaw_ = fmodf(yaw_ + xOffset, 360.f);
    pitch_ += yOffset;
    pitch_ = pitch_ < -89.f ? -89.f : (pitch_ > 89.f ? 89.f : pitch_);
    const double yaw = (double)(yaw_ * 3.14159265358979323846264f) / 180.0, pitch = (double)(pitch_ * 3.14159265358979323846264f) / 180.0;
    float3 f((float)(cos(yaw) * cos(pitch)), (float)sin(pitch), (float)(sin(yaw) * cos(pitch)));
    cam.forward = to4(normalize(f));
}
void CameraManager::Zoom(float offset) { moved = true; Fov(cam.fov + offset); } // camera.h:95-99

void CameraManager::UpdateCamVec() // camera.h:111-121
{
    Fov(cam.fov);
    const float3 worldUp(0, 1, 0);
    float3 fwd(cam.forward);
    float3 right = normalize(cross(worldUp, fwd));
    float3 up = normalize(cross(right, fwd));
    cam.right = to4(right); cam.up = to4(up);
    cam.horizontal = to4(viewportWidth * right);
    cam.vertical = to4(viewportHeight * up);
    RtFloat4 o = cam.origin, hz = cam.horizontal, vt = cam.vertical, f = cam.forward;
    cam.topLeft = RtFloat4{ o.x - hz.x / 2 - vt.x / 2 - f.x, o.y - hz.y / 2 - vt.y / 2 - f.y,
                            o.z - hz.z / 2 - vt.z / 2 - f.z, o.w - hz.w / 2 - vt.w / 2 - f.w };
}

} // namespace rt355

// rt_host.h — host-side mirror of the reference's Scene / BVH2 / BVH4 / TLAS /
// CameraManager / Renderer surface (reference: src/scene.h, src/bvh.h, src/tlas.h,
// src/camera.h, src/renderer.h).  Same class and method names, same argument meaning;
// the arrays these classes produce use the wire format of include/rt355_types.h and
// are handed to the device path through the C-ABI of include/rt355.h.
//
// All arithmetic is strict binary32 in source order (build with -ffp-contract=off):
// the reference's own host build used MSVC /fp:fast and is not reproducible
// (SURVEY.md Appendix B #13).
#pragma once
#include <cstdint>
#include <map>
#include <stdexcept>
#include <string>
#include <vector>
#include "../../include/rt355_types.h"

struct RtCtx;
struct RtGroup;

namespace rt355 {

struct float2 { float x = 0, y = 0; };
struct float3 {
    float x = 0, y = 0, z = 0;
    float3() = default;
    float3(float a, float b, float c) : x(a), y(b), z(c) {}
    explicit float3(float a) : x(a), y(a), z(a) {}
    explicit float3(const RtFloat4& v) : x(v.x), y(v.y), z(v.z) {}
    float  operator[](int i) const { return i == 0 ? x : (i == 1 ? y : z); }
    float& operator[](int i) { return i == 0 ? x : (i == 1 ? y : z); }
};
inline float3 operator+(const float3& a, const float3& b) { return { a.x + b.x, a.y + b.y, a.z + b.z }; }
inline float3 operator-(const float3& a, const float3& b) { return { a.x - b.x, a.y - b.y, a.z - b.z }; }
inline float3 operator*(const float3& a, float s) { return { a.x * s, a.y * s, a.z * s }; }
inline float3 operator*(float s, const float3& a) { return { s * a.x, s * a.y, s * a.z }; }
inline float3 operator+(const float3& a, float s) { return { a.x + s, a.y + s, a.z + s }; }
inline float3 operator-(const float3& a, float s) { return { a.x - s, a.y - s, a.z - s }; }
inline RtFloat4 to4(const float3& v, float w = 0.0f) { return RtFloat4{ v.x, v.y, v.z, w }; }
float  dot(const float3& a, const float3& b);
float3 cross(const float3& a, const float3& b);
float3 normalize(const float3& v);
float  length(const float3& v);

// Axis-aligned box with the min/max semantics of the template's SSE aabb
// (reference: template/precomp.h:889-941): 4 lanes, w held at 0, empty = (+1e34, -1e34).
struct Aabb {
    float bmin[4] = { 1e34f, 1e34f, 1e34f, 0 };
    float bmax[4] = { -1e34f, -1e34f, -1e34f, 0 };
    void  Grow(const float3& p);
    void  Grow(const RtFloat4& p);
    void  Grow(const Aabb& b);
    Aabb  Union(const Aabb& b) const;
    Aabb  Intersection(const Aabb& b) const;
    float Area() const;
    float Center(int axis) const { return (bmin[axis] + bmax[axis]) * 0.5f; }
};

struct BVHPrimData { Aabb box; uint32_t idx = 0; bool clipped = false; };   // clipped: a fragment of a spatial split (see RefBounds)

// reference: src/bvh.h:4-40
class BVH2 {
public:
    BVH2(std::vector<RtPrimitive>& prims, std::vector<RtBVHInstance>& blasNodes);
    void     BuildBLAS(bool statistics, int startIdx);
    // The linear BVH builder (csrc/lbvh_common.h) over primitives [startIdx, end): appends a BLAS exactly as BuildBLAS does (instance
    // record, nodes, primIdx, statistics).  device >= 0: rt_build_bvh2 on that GPU; -1: the host restatement.  Throws LbvhError and
    // leaves everything unchanged when the build is refused.
    void     BuildBLASLBVH(int startIdx, int device, const RtBuildOptions* opt);
    RtBuildStats lastLbvh{};     // statistics of the last BuildBLASLBVH
    // The GPU build of BuildBLAS with alpha = 1 (csrc/sah_common.h) over primitives [startIdx, end): appends exactly what
    // BuildBLAS(alpha = 1) appends.  device >= 0: rt_build_bvh2_sah on that GPU; -1: the host restatement.  Throws LbvhError and
    // leaves everything unchanged when the build is refused.
    void     BuildBLASSAHGPU(int startIdx, int device);
    // The GPU build of BuildBLAS for any alpha in [0, 1], spatial splits included (csrc/sbvh_common.h): appends exactly what BuildBLAS
    // appends with bvh2->alpha = alpha, statistics included.  device >= 0: rt_build_bvh2_sbvh on that GPU; -1: the host restatement.
    // Throws LbvhError and leaves everything unchanged when the build is refused.
    void     BuildBLASSBVHGPU(int startIdx, float alpha, int device);
    // Discards the trees and builds every BLAS again over the primitive range it covers, in increasing order of the ranges, with the
    // host restatement of rt_rebuild_scene's builder (RT_REBUILD_SAH / RT_REBUILD_LBVH / RT_REBUILD_SBVH, opt as there); instance transforms stay,
    // bvhIdx follows.  Throws LbvhError and leaves everything unchanged when refused (rebuild_host.cpp).
    void     Rebuild(int builder, const RtBuildOptions* opt);
    // The same under a plan (rt_rebuild_ranges): plan[nRanges], one RT_REBUILD_SAH / LBVH / SBVH / KEEP / REFIT_RANGE per distinct BLAS in increasing
    // order of the ranges; a kept BLAS is appended as its bound block of nodes, relocated (csrc/rebuild_common.h, relocated_first).
    void     RebuildRanges(const int32_t* plan, int nRanges, const RtBuildOptions* opt);
    int      buildThreads = 1;   // > 1: subtrees are built by parallel tasks, then numbered in the reference's LIFO order (same arrays)
    uint32_t Depth(uint32_t nodeIdx) const;
    uint32_t Count(uint32_t nodeIdx) const;
    float    TotalCost(uint32_t nodeIdx) const;
    std::vector<RtBVHNode2> bvhNodes;
    std::vector<uint32_t>   primIdx;
    float    alpha = 1.f;
    uint32_t stat_depth = 0, stat_node_count = 0, stat_spatial_splits = 0, stat_prims_clipped = 0, stat_prim_count = 0, stat_forced_leaves = 0;
    float    stat_sah_cost = 0, stat_build_time = 0;
    std::vector<RtBVHInstance>& blasNodes;
private:
    using Refs = std::vector<BVHPrimData>;
    void  BuildBLASUnguarded(bool statistics, int startIdx);
    void  RebuildPlan(const char* who, const int32_t* plan, int nRanges, const RtBuildOptions* opt);   // Rebuild's and RebuildRanges' loop (nRanges < 0: every range plan[0])
    // what BuildBLASLBVH / BuildBLASSAHGPU / BuildBLASSBVHGPU do once their build has succeeded (lbvh_host.cpp)
    void  AppendBuiltBLAS(uint32_t nodeBase, const RtBVHNode2* nodes, size_t nN, const uint32_t* idx, size_t nI, float wall_ms, int32_t depth,
                          float cost);
    void  BuildBVH(uint32_t root, Refs data);
    struct TNode;                                       // temporary pointer tree of the parallel build
    TNode* BuildSubtree(Refs refs, float rootArea, int depth, int& budget);
    void  FlattenLIFO(uint32_t root, TNode* tree);
    void  UpdateNodeBounds(uint32_t nodeIdx, const Refs& prims);
    Refs  CreateBVHPrimData(int startIdx) const;
    float CalculateNodeCost(const RtBVHNode2& node, uint32_t count) const;
    float FindBestObjectSplitPlane(int& axis, float& splitPos, float& overlap, const Refs& prims) const;
    void  ObjectSplit(int axis, float splitPos, const Refs& prims, Refs& left, Refs& right) const;
    float FindBestSpatialSplitPlane(int& axis, float& splitPos, const Refs& prims) const;
    void  SpatialSplit(int axis, float splitPos, const Refs& prims, Refs& left, Refs& right, uint32_t& clippedCount) const;
    bool  ClipTriangleToAABB(const Aabb& bounds, float3 v0, float3 v1, float3 v2, Aabb& out) const;
    bool  ClipSphereToAABB(const Aabb& bounds, float3 pos, float r, Aabb& out) const;
    std::vector<RtPrimitive>& primitives_;
    uint32_t rootNodeIdx_ = 0, nodesUsed_ = 0;
};

struct LbvhError : std::runtime_error { int code; LbvhError(int c, const std::string& m) : std::runtime_error(m), code(c) {} };
// The linear builder's sequential host restatement (rth_build_bvh2_lbvh); err receives the message of a refused call.
int LbvhBuildHost(const RtBuildOptions* opt, const RtPrimitive* prims, int32_t nPrims, int32_t first, int32_t count, uint32_t nodeBase,
                  uint32_t idxBase, RtBVHNode2* nodes, int32_t nodeCap, int32_t* nNodes, uint32_t* primIdx, RtBuildStats* stats,
                  std::string& err);

// The GPU SAH build's sequential host restatement (rth_build_bvh2_sah); err receives the message of a refused call.
int SahBuildHost(const RtPrimitive* prims, int32_t nPrims, int32_t first, int32_t count, uint32_t nodeBase, uint32_t idxBase,
                 RtBVHNode2* nodes, int32_t nodeCap, int32_t* nNodes, uint32_t* primIdx, RtBuildStats* stats, std::string& err);

// The GPU SBVH build's sequential host restatement (rth_build_bvh2_sbvh); err receives the message of a refused call.
// the same build into vectors of the tree's own size, for callers that have checked the arguments (BVH2::Rebuild)
int SbvhBuildVectors(float alpha, const RtPrimitive* prims, int32_t first, int32_t count, uint32_t nodeBase, uint32_t idxBase,
                     std::vector<RtBVHNode2>& nodes, std::vector<uint32_t>& primIdx, RtSbvhStats* stats, std::string& err);
int SbvhBuildHost(float alpha, const RtPrimitive* prims, int32_t nPrims, int32_t first, int32_t count, uint32_t nodeBase, uint32_t idxBase,
                  RtBVHNode2* nodes, int32_t nodeCap, int32_t* nNodes, uint32_t* primIdx, int32_t idxCap, int32_t* nIdx, RtSbvhStats* stats,
                  std::string& err);

// The GPU BVH2 -> BVH4 collapse's sequential host restatement (rth_build_bvh4_levels, collapse_host.cpp); err receives the message of a
// refused call, which writes nothing.
int Bvh4LevelsHost(const RtBVHNode2* nodes2, int32_t nNodes, int32_t nIdx, const uint32_t* roots, int32_t nRoots, RtBVHNode4* out4, RtBvh4Stats* stats,
                   RtFloat4* quads, uint32_t* rootEntry, uint32_t* quadNode, std::string& err);
// rth_bvh4_refit: the collapse of a refit BVH2 under the live ids of the collapse in inout4 (collapse_host.cpp)
int Bvh4RefitHost(const RtBVHNode2* refit2, int32_t nNodes, int32_t nIdx, const uint32_t* roots, int32_t nRoots, RtBVHNode4* inout4, const uint32_t* quadNode,
                  int32_t nLive, int32_t* changedNodes, std::string& err);

// In-place updates (refit_host.cpp, the host restatement of rt_update_scene): replace primitives keeping objType / matIdx, then refit
// every BLAS by the rules of csrc/refit_common.h; err receives why a call is refused (RT_E_* returned, nothing changed).
int SetPrimitivesHost(std::vector<RtPrimitive>& prims, int32_t first, int32_t count, const RtPrimitive* in, std::string& err);
int RefitHost(std::vector<RtBVHNode2>& nodes, const std::vector<uint32_t>& primIdx, const std::vector<RtPrimitive>& prims,
              const std::vector<RtBVHInstance>& inst, std::string& err);

// reference: src/bvh.h:41-56
class BVH4 {
public:
    explicit BVH4(BVH2& bvh2);
    BVH4(BVH2& bvh2, std::vector<RtBVHNode4>&& collapsed) : bvh2(bvh2), bvhNodes(std::move(collapsed)) {}   // nodes collapsed elsewhere (rt_build_bvh4)
    std::vector<RtBVHNode4>& Nodes() { return bvhNodes; }
    std::vector<uint32_t>&   Idx() { return bvh2.primIdx; }
    uint32_t Depth(uint32_t nodeIdx) const;
    uint32_t Count(uint32_t nodeIdx) const;
private:
    BVH2& bvh2;
    std::vector<RtBVHNode4> bvhNodes;
    void Convert();
    void Collapse(int index);
    int  GetChildCount(const RtBVHNode4& node) const;
};

// reference: src/tlas.h:2-12
class TLAS {
public:
    explicit TLAS(BVH2& bvh2);
    void Build();
    std::vector<RtTLASNode> tlasNodes;
private:
    int FindBestMatch(const int* list, int N, int A) const;
    BVH2& bvh2_;
    uint32_t nodesUsed_ = 0;
};

// reference: src/scene.h:5-34 (LoadModel / LoadTexture file IO: scene_io.cpp, image_io.cpp)
class Scene {
public:
    Scene();
    ~Scene();
    RtMaterial& AddMaterial(const std::string& name);
    void AddSphere(float3 pos, float radius, const std::string& material);
    void AddPlane(float3 N, float d, const std::string& material);
    void AddQuad(float3 v0, float3 v1, float3 v2, float3 v3, const std::string& material, bool flipNormal = false,
                 float2 uv0 = { 0, 0 }, float2 uv1 = { 1, 0 }, float2 uv2 = { 0, 1 }, float2 uv3 = { 1, 1 });
    void AddTriangle(float3 v0, float3 v1, float3 v2, float2 uv0, float2 uv1, float2 uv2, const std::string& material,
                     bool flipNormal = false);
    int  AddTexture(const RtFloat4* texels, int width, int height, const std::string& name); // LoadTexture minus the file read
    // reference: Scene::LoadTexture (scene.cpp:244-256); PNG, JPEG, TGA and Radiance HDR files (image_io.cpp, jpeg_io.cpp); returns the material index
    int  LoadTexture(const std::string& filename, const std::string& name);
    int  MaterialIndex(const std::string& name);
    // The host restatement of rt_update_materials (include/rt355_host.h): each checks first, changes nothing when it refuses (the reason
    // goes to err, the return value is RT_E_INVALID), and leaves `lights` as the Scene rule gives it for the new state
    int  SetMaterials(const RtMaterial* mats, int32_t nMats, std::string& err);   // the whole table; names of dropped indices are forgotten
    int  SetTexels(const RtFloat4* texels, int32_t first, int32_t count, int32_t nTexels, std::string& err);
    int  SetPrimMaterials(int32_t first, int32_t count, const int32_t* matIdx, std::string& err);
    bool HasMaterial(const std::string& name) const { return matMap_.count(name) != 0; }
    // reference: Scene::LoadModel (scene.cpp:178-243), OBJ + MTL diffuse-texture names; returns the triangles added
    int  LoadModel(const std::string& filename, const std::string& defaultMaterial, float3 pos = float3(0, 0, 0), bool forceDefaultMat = false);
    void BuildBVH4();
    std::vector<RtPrimitive>   primitives;
    std::vector<RtMaterial>    materials;
    std::vector<uint32_t>      lights;
    std::vector<RtFloat4>      textures;
    std::vector<RtBVHInstance> blasNodes;
    BVH2* bvh2 = nullptr;
    BVH4* bvh4 = nullptr;
private:
    std::map<std::string, int> matMap_;
    int matIdx_ = 0;
};

// reference: SaveImageF (template/template.cpp:1629-1644) behind Renderer::SaveFrame (renderer.cpp:303-308)
void SavePNG(const std::string& file, int w, int h, const RtFloat4* data);
// LoadImageF (template/template.cpp:1613-1627): w*h RGB float triples, top row first (image_io.cpp)
constexpr int64_t kMaxTexturePixels = int64_t(1) << 26;   // larger headers are treated as corrupt files, not as allocation requests
std::vector<float> LoadImageF(const std::string& file, int& w, int& h);
// ITU-T T.81 baseline / progressive Huffman JPEG -> 8-bit RGB, top row first (jpeg_io.cpp)
void DecodeJpeg(const std::vector<uint8_t>& bytes, const std::string& file, int& w, int& h, std::vector<uint8_t>& rgb);

// reference: src/camera.h:7-122 (aspect = width/height is a run-time value here)
class CameraManager {
public:
    CameraManager(int width, int height, float vfov = 110, int type = RT_CAM_PROJECTION);
    RtCamera cam;
    float viewportHeight = 0, viewportWidth = 0, aspect = 1;
    bool  moved = true;
    void Fov(float vfov);
    void UpdateCamVec();
    // controller (camera.h:47-99): dir 0..5 = Forward, Backwards, Left, Right, Up, Down
    void Move(int camdir, float deltaTime);
    void MouseMove(float xOffset, float yOffset);
    void Zoom(float offset);
    float mouseSensivity = 0.5f, speed = 1.f;
private:
    float yaw_ = 0, pitch_ = 0;   // uninitialised in the reference (camera.h:20-21); zero here
};

// reference: src/renderer.h:23-26,36 (ImGuiData kernel variants)
struct RenderOptions {
    int  shading = 1;          // 0 SHADING_SIMPLE, 1 SHADING_NEE
    int  sampling = 1;         // 0 SAMPLING_HEMISPHERE, 1 SAMPLING_COSINE
    int  bvh = 0;              // 0 USE_BVH2, 1 USE_BVH4
    bool use_russian_roulette = true;
    bool filter_fireflies = true;
    bool reset_every_frame = false;
};

// reference: src/renderer.h:44-120, src/renderer.cpp:6-94,126-140,289-301.
// Owns the Scene, camera, TLAS and Settings like the reference's Renderer and drives
// the device path exclusively through the C-ABI (rt_create / rt_upload_scene /
// rt_render / ...).  Resolution and row band are run-time values.
class Renderer {
public:
    Renderer(int width, int height, int device = 0, int y0 = 0, int y1 = -1);
    ~Renderer();
    void Init();                       // renderer.cpp:6-21
    void Tick(float deltaTime);        // renderer.cpp:26-63 (one accumulated frame)
    void RayTrace();                   // renderer.cpp:64-94
    void ComputeEnergy();              // renderer.cpp:126-140
    void FocusCamera(int x, int y);    // renderer.cpp:289-301
    void ReadAccum(RtFloat4* out);     // accumBuffer->CopyFromDevice()
    void SaveFrame(const char* file);  // renderer.cpp:303-308 (PostProc chain + saveImage + SaveImageF)
    float vignet_strength = 0, chromatic_strength = 0, gamma_strength = .9f;   // renderer.h:28-30
    Scene          scene;
    CameraManager  camera;
    RtSettings*    settings = nullptr;
    TLAS*          tlas = nullptr;
    RenderOptions  imgui;
    float          energy_total = 0;
    RtGroup*       group = nullptr;    // the lanes behind this Renderer (include/rt355.h, rt_group_*)
    RtCtx*         ctx = nullptr;      // lane 0 (focus pick, counters, stage-level debugging)
    int            lanes = 1;          // set before Init(): sample streams whose frames overlap on the GPU; Tick() = `lanes` frames
    int            builtins = 0;       // set before Init(): RtConfig.builtins of the lanes (RT_BUILTINS_DEFAULT / _IEEE / _REFERENCE, include/rt355.h)
    int            extend_variant = 0; // set before Init(): RtConfig.extend_variant of the lanes (0 = best available; 6 also takes k_trace_persist4_tlas, include/rt355.h)
    int width, height, device, y0, y1;
};

} // namespace rt355
